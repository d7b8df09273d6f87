"""The stored-header decoder (k_decode.hip) against the oracle (oracle/cbor_header.py) on the
cases of tests/decode_cases.py: every head's first byte, every head width, the integer and
length edges, every span length at every alignment, and the era selection; in all three
modes of the kernel (Praos, TPraos, either era) and through every call that launches it
(DESIGN.md section 26).

Every comparison is of whole output arrays with arrays built from the oracle's result, which
are zero wherever the oracle has nothing: the rows of a header that does not decode, and a
signed row from its signed length to the stride.  So "holds no stale bytes" is part of every
equality here, and test_no_stale_rows_* runs it over rows that just held valid headers."""
import functools
import random

import numpy as np
import pytest

import block_corpus as bc
import block_integrity as bi
import cbor_header as ch
import decode_cases as dc

pytestmark = pytest.mark.gpu
SPKP = 129600
ERAS = (False, True)
INTS = (("block_no", "block_no"), ("slot", "slot"), ("body_size", "body_size"), ("ocert_n", "n"), ("ocert_c0", "c0"),
        ("prot_major", "prot_major"), ("prot_minor", "prot_minor"))
BYTES = ("cold_vk", "vrf_vk", "vrf_out", "vrf_proof", "body_hash", "hot_vk", "ocert_sig", "kes_sig")


@functools.lru_cache(maxsize=None)
def _cases(kind, *args):
    arena, off, ln, names = getattr(dc, kind)(*args)
    return np.frombuffer(arena, np.uint8).copy(), np.array(off, np.uint64), np.array(ln, np.uint32), names, arena


@functools.lru_cache(maxsize=None)
def _want(kind, args, mode):
    """The decoded arrays the oracle gives for a corpus in a mode (False Praos, 2 TPraos), as
    the calls return them; computed once and shared (read-only)."""
    from praos_hip import abi
    _, off, ln, _, raw = _cases(kind, *args)
    n = len(off)
    stride = abi.TP_SIGNED_STRIDE if mode else abi.SIGNED_STRIDE
    E = {name: np.zeros((n,) + (shp if name != "signed_body" else (stride,)), dt)
         for name, dt, shp in abi.DECODED_FIELDS}
    if mode:
        E["leader_out"], E["leader_proof"] = np.zeros((n, 64), np.uint8), np.zeros((n, 80), np.uint8)
    for i in range(n):
        r = ch.decode_header(raw, int(off[i]), int(ln[i]), allow_tpraos=mode)
        E["status"][i] = r["status"]
        E["header_hash"][i] = np.frombuffer(r["header_hash"], np.uint8)
        f = r["fields"]
        if f is None:
            E["signed_len"][i] = 0xFFFFFFFF
            continue
        for k, fk in INTS:
            E[k][i] = f[fk]
        for k in BYTES:
            E[k][i] = np.frombuffer(f[k], np.uint8)
        E["prev_is_genesis"][i] = f["prev_hash"] is None
        E["prev_hash"][i] = np.frombuffer(f["prev_hash"] or bytes(32), np.uint8)
        E["signed_len"][i] = len(r["signed"])
        E["signed_body"][i][:len(r["signed"])] = np.frombuffer(r["signed"], np.uint8)
        if r["tpraos"]:
            E["leader_out"][i] = np.frombuffer(f["leader_out"], np.uint8)
            E["leader_proof"][i] = np.frombuffer(f["leader_proof"], np.uint8)
    for v in E.values():
        v.setflags(write=False)
    return E


def _same(D, E, names):
    """Every output array bit for bit, leader_out / leader_proof included where returned."""
    assert set(D) == set(E)
    for k in E:
        assert D[k].shape == E[k].shape and D[k].dtype == E[k].dtype, k
        bad = np.nonzero((D[k] != E[k]).reshape(len(names), -1).any(axis=1))[0]
        assert bad.size == 0, (k, len(bad), [names[i] for i in bad[:5]], D[k][bad[0]], E[k][bad[0]])


def _epoch(ctx):
    from praos_hip import abi
    ctx.set_epoch(None, [], abi.params(slots_per_kes_period=SPKP, max_kes_evo=62))


def _decode(ctx, kind, args, tp):
    """One corpus through the era's call; every output against the oracle."""
    from praos_hip import abi
    arena, off, ln, names, _ = _cases(kind, *args)
    E = _want(kind, args, 2 if tp else False)
    if tp:
        o, D = ctx.verify_tpraos_header_bytes(arena, off, ln, decoded=True)
        failed = (E["status"] & ch.DEC_FAIL) != 0
        assert ((o["bits"][failed] & abi.BIT_INPUT) != 0).all()      # a header that does not decode is flagged
    else:
        D = ctx.decode_headers(arena, off, ln)
    _same(D, E, names)
    return E


CORPORA = [("first_bytes", (False,)), ("first_bytes", (True,)), ("widths", (False,)), ("widths", (True,)),
           ("values", ()), ("lengths", ())]


@pytest.mark.parametrize("tp", ERAS, ids=("praos", "tpraos"))
@pytest.mark.parametrize("kind,args", CORPORA, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_oracle_equality(ctx, kind, args, tp):
    _epoch(ctx)
    E = _decode(ctx, kind, args + (tp,), tp)
    names = _cases(kind, *args, tp)[3]
    for i, nm in enumerate(names):                        # the generator's claims, on the kernel's own output
        assert dc.claim(nm) in (None, int(E["status"][i])), nm
    assert len(names) == {"first_bytes": (5397, 5654), "values": (243, 245), "lengths": (15324, 17762),
                          "widths": ((96, 99), (84, 87))[bool(args and args[0])]}[kind][tp]


def test_era_selection_three_modes(ctx):
    """Arities 9, 10, 11, 14, 15, 16 over both layouts: Praos mode, TPraos mode, and (block
    batches) either era, where the body's arity picks the layout."""
    _epoch(ctx)
    for tp in ERAS:
        E = _decode(ctx, "eras", (), tp)
        assert int((E["status"] == 0).sum()) == 1
    _blocks(ctx, "eras", (), range(12))


# ---- every route to the kernel ----
@pytest.mark.parametrize("multi", (False, True), ids=("onebyte", "multibyte"))
def test_every_route_equals_decode_headers(ctx, multi):
    """verify_header_bytes, upload_bytes / run / download_decoded and submit_header_bytes /
    drain launch the kernel over sub-ranges [i0, n) of the batch (3 chunks of unequal size
    here): the decoded arrays of each, row for row those of decode_headers and the oracle."""
    from praos_hip import abi
    arena, off, ln, names, _ = _cases("first_bytes", multi, False)
    E = _want("first_bytes", (multi, False), False)
    n = len(off)
    failed = (E["status"] & ch.DEC_FAIL) != 0
    _epoch(ctx)
    D0 = ctx.decode_headers(arena, off, ln)
    _same(D0, E, names)
    try:
        for chunks in (0, 3):
            ctx.set_option(abi.OPT_PIPELINE, chunks)
            o, D = ctx.verify_header_bytes(arena, off, ln, decoded=True)
            _same(D, D0, names)
            assert ((o["bits"][failed] & abi.BIT_INPUT) != 0).all() and ((o["bits"][~failed] & abi.BIT_INPUT) == 0).all()
        outs = [(ctx.alloc_out(n), ctx.alloc_decoded(n)) for _ in range(2)]
        for out, d in outs:
            ctx.submit_header_bytes(arena, off, ln, out=out, decoded=d)
        ctx.drain()
        for out, d in outs:
            _same(d[0], D0, names)
            assert np.array_equal(out["bits"], o["bits"])
    finally:
        ctx.drain()
        ctx.set_option(abi.OPT_PIPELINE, 0)
    b = ctx.upload_bytes(arena, off, ln)
    try:
        for _ in range(2):                                # the second run decodes over the first one's rows
            ctx.run(b)
            ctx.sync()
        D = ctx.download_decoded(b, n)
        ob = ctx.download(b, n)
    finally:
        ctx.free(b)
    _same(D, D0, names)
    assert np.array_equal(ob["bits"], o["bits"])


# ---- re-encoded bytes are what gets verified ----
@pytest.mark.parametrize("tp", ERAS, ids=("praos", "tpraos"))
def test_reencoded_body_is_the_kes_message(ctx, tp):
    """Headers signed (genuine Sum6 KES signature) over the canonical body, stored with each
    wider form of each body head: every one decodes NONCANONICAL, is re-encoded to the signed
    bytes, and verifies -- all KES bits clear, every bit as the canonical header's."""
    from praos_hip import abi
    arena, off, ln, names = dc.genuine_wide(tp, SPKP)
    assert len(names) == (57, 59)[tp]
    _epoch(ctx)
    if tp:
        o, D = ctx.verify_tpraos_header_bytes(arena, off, ln, decoded=True)
    else:
        o, D = ctx.verify_header_bytes(arena, off, ln, decoded=True)
    kes = abi.BIT_KES_BEFORE_START | abi.BIT_KES_AFTER_END | abi.BIT_KES_MERKLE | abi.BIT_KES_LEAF | abi.BIT_INPUT
    assert [int(s) for s in D["status"]] == [dc.claim(nm) for nm in names]
    assert ((o["bits"] & kes) == 0).all(), [names[i] for i in np.nonzero(o["bits"] & kes)[0]]
    assert (o["bits"] == o["bits"][0]).all()
    assert (D["signed_len"] == D["signed_len"][0]).all() and (D["signed_body"] == D["signed_body"][0]).all()
    # and one changed payload byte of a wide body is a KES failure (the check can fail)
    bad = bytearray(arena)
    for i in range(len(off)):
        bad[off[i] + 60 + i % 200] ^= 0x04
    ob = (ctx.verify_tpraos_header_bytes if tp else ctx.verify_header_bytes)(bytes(bad), off, ln)
    assert ((ob["bits"] & kes) != 0).all()


@pytest.mark.parametrize("era", (5, 6), ids=("alonzo", "babbage"))
def test_reencoded_body_in_blocks(ctx, era):
    """The same through verify_block_integrity: blocks whose stored header body has one wider
    head each (make_block's `wide`): 0 for the intact block, BLK_KES with one byte of the wide
    body's payload changed; both as the oracle says."""
    slot = 1 << 30
    c0 = slot // SPKP - 3
    _, f, _ = bc.make_block(random.Random(era), SPKP, era=era, slot=slot, c0=c0)
    its = dc.items(dict(f, kes_sig=bytes(448)), era == 5)
    wides = [{name: ai} for name, _, val, _ in its if name not in dc.OUTSIDE_BODY for ai in dc.forms_for(val)[1:]]
    wides.append({name: 27 for name, _, _, _ in its if name not in dc.OUTSIDE_BODY})
    assert len(wides) > 45
    blocks, want = [], []
    for j, w in enumerate(wides):
        blk, g, _ = bc.make_block(random.Random(era), SPKP, era=era, slot=slot, c0=c0, wide=w)
        assert g == f
        i = blk.index(f["vrf_out"]) + j % 64
        blocks += [blk, blk[:i] + bytes([blk[i] ^ 0x20]) + blk[i + 1:]]
        want += [0, bi.BLK_KES]
    arena, off, ln = b"".join(blocks), [], []
    for blk in blocks:
        off.append(sum(ln))
        ln.append(len(blk))
    res, bh = ctx.verify_block_integrity(arena, off, ln, SPKP)
    assert [int(x) for x in res] == want
    for i in range(len(blocks)):
        bits, h = bi.verify_block_integrity(arena, off[i], ln[i], SPKP)
        assert (bits, h) == (want[i], bytes(bh[i])), i


SEGS = b"\x80\x80\xa0\x80"                   # four one-byte segments


def _blocks(ctx, kind, args, rows):
    """Headers `rows` of a corpus wrapped as Alonzo (TPraos), Babbage (Praos) and bare blocks:
    the verdicts and body hashes of verify_block_integrity against the oracle's."""
    _, off, ln, names, raw = _cases(kind, *args)
    blocks = []
    for i in rows:
        h = raw[int(off[i]):int(off[i]) + int(ln[i])]
        inner = b"\x85" + h + SEGS
        blocks += [b"\x82\x05" + inner, b"\x82\x06" + inner, inner]
    arena, boff, bln = b"".join(blocks), [], []
    for blk in blocks:
        boff.append(sum(bln))
        bln.append(len(blk))
    res, bh = ctx.verify_block_integrity(arena, boff, bln, SPKP)
    want = [bi.verify_block_integrity(arena, boff[j], bln[j], SPKP) for j in range(len(blocks))]
    for j, (bits, h) in enumerate(want):
        assert (int(res[j]), bytes(bh[j])) == (bits, h), (names[list(rows)[j // 3]], j % 3, int(res[j]), bits)
    return [w[0] for w in want]


@pytest.mark.parametrize("tp", ERAS, ids=("praos", "tpraos"))
def test_block_verdicts_of_first_bytes(ctx, tp):
    """The 15-field and 10-field branches of block batches with failing and non-canonical
    headers: every 16th first-byte case plus every case the oracle accepts."""
    E = _want("first_bytes", (True, tp), 2 if tp else False)
    rows = sorted(set(range(0, len(E["status"]), 16)) | set(np.nonzero((E["status"] & ch.DEC_FAIL) == 0)[0].tolist()))
    bits = _blocks(ctx, "first_bytes", (True, tp), rows)
    # headers that decode reach the KES and body-hash checks (random signature, no body hash), the others stop at decode
    assert bits.count(bi.BLK_KES | bi.BLK_BODY_HASH) >= 22 and bits.count(bi.BLK_DECODE) > 600
    assert set(bits) == {bi.BLK_DECODE, bi.BLK_KES | bi.BLK_BODY_HASH}


# ---- no stale bytes ----
def _valid(n, tp):
    """n valid headers (the canonical multi-byte header)."""
    h = dc.header(dc.base_fields(True, tp), tp)
    return (np.frombuffer(h * n, np.uint8).copy(), np.arange(n, dtype=np.uint64) * len(h),
            np.full(n, len(h), np.uint32))


@pytest.mark.parametrize("tp", ERAS, ids=("stride448", "stride640"))
@pytest.mark.parametrize("kind", ("first_bytes", "lengths"))
def test_no_stale_rows_after_valid_batch(ctx, kind, tp):
    """A batch of n valid headers, then n cases at the same rows in the same context (Praos:
    the pipelined call keeps its device batch between calls): every failed row zero in every
    field, leader certificate and whole signed row included, every passing row zero from its
    signed length to the stride -- the oracle arrays hold zeros there."""
    from praos_hip import abi
    args = ((True, tp) if kind == "first_bytes" else (tp,))
    arena, off, ln, names, _ = _cases(kind, *args)
    E = _want(kind, args, 2 if tp else False)
    va, vo, vl = _valid(len(off), tp)
    _epoch(ctx)
    if tp:
        _, V = ctx.verify_tpraos_header_bytes(va, vo, vl, decoded=True)
        _, D = ctx.verify_tpraos_header_bytes(arena, off, ln, decoded=True)
    else:
        try:
            ctx.set_option(abi.OPT_PIPELINE, 2)
            _, V = ctx.verify_header_bytes(va, vo, vl, decoded=True)
            _, D = ctx.verify_header_bytes(arena, off, ln, decoded=True)
        finally:
            ctx.set_option(abi.OPT_PIPELINE, 0)
    assert (V["status"] == 0).all() and V["kes_sig"].any(axis=1).all() and (V["signed_len"] > 400).all()
    _same(D, E, names)
    failed = (E["status"] & ch.DEC_FAIL) != 0
    assert failed.sum() > len(names) // 2
    for k in D:                                            # said once more, on the device's arrays alone
        if k not in ("status", "header_hash", "signed_len"):
            assert not D[k][failed].any(), k
    sl = D["signed_len"][~failed].astype(np.int64)
    cols = np.arange(D["signed_body"].shape[1])
    assert not (D["signed_body"][~failed] * (cols[None, :] >= sl[:, None])).any()


def test_no_stale_rows_in_reused_upload_batch(ctx):
    """upload_bytes batch run twice (decode over its own earlier rows), after a freed batch of
    valid headers of the same size."""
    arena, off, ln, names, _ = _cases("lengths", False)
    E = _want("lengths", (False,), False)
    _epoch(ctx)
    v = ctx.upload_bytes(*_valid(len(off), False))
    try:
        ctx.run(v)
        ctx.sync()
    finally:
        ctx.free(v)
    b = ctx.upload_bytes(arena, off, ln)
    try:
        for _ in range(2):
            ctx.run(b)
            ctx.sync()
            _same(ctx.download_decoded(b, len(off)), E, names)
    finally:
        ctx.free(b)
