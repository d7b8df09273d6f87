"""GPU: Byron header validation (k_pbft.hip through praos_verify_pbft_headers, the fold, the
directory walk and the harness phase) against tests/pbft_model.py, case by case."""
import copy
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import byron_corpus as bc
import byron_model as bm
import pbft_corpus as pc
import pbft_model as pm
from helpers import L as ORDER_L
from helpers import P as FIELD_P
from helpers import rbytes, rng
from praos_hip import abi, immutable

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ES, PMAG = pc.EPOCH_SLOTS, pc.PM
K, THR = 10, 4
COLS = [name for name, _, _ in abi.PBFT_OUT_FIELDS]
GOLD = json.load(open(os.path.join(HERE, "golden", "pbft_golden.json")))
BLOCKS = json.load(open(os.path.join(HERE, "golden", "byron_blocks.json")))


def params(pmagic=PMAG, es=ES, k=K, thr=THR):
    return abi.Context.pbft_params(k, thr, es, pmagic)


def same(H, rows, where=""):
    want = pc.rows_to_columns(rows)
    for c in COLS:
        bad = np.nonzero((np.asarray(H[c]).reshape(len(rows), -1) != want[c].reshape(len(rows), -1)).any(axis=1))[0]
        assert len(bad) == 0, (where, c, bad[:5], H[c][bad[:2]], want[c][bad[:2]])


def run(ctx, blocks, delegs, is_ebb=None, pmagic=PMAG):
    arena, off, ln, ebb = pc.columns(blocks)
    return ctx.verify_pbft_headers(arena, off, ln, ebb if is_ebb is None else is_ebb, params(pmagic), delegs,
                                   delegate_hash=True)


class Hdr:
    """header bytes standing in for a block in pc.columns / pc.model_rows"""

    def __init__(self, header, kind):
        self.header, self.kind = bytes(header), kind


@pytest.fixture(scope="module")
def forged(oracle):
    """300 headers: 3 epochs x (EBB + 99 main headers) at 40 slots per epoch, 5 delegates: three in
    the map and used many times, one in the map used once, one not in the map.  Five headers have
    signed-message lengths on the SHA-512 stream's padding and block boundaries."""
    r = rng(0x0b51)
    D = [bc.Delegate(r) for _ in range(5)]

    def pick(k):
        return D[3] if k == 150 else D[4] if k % 50 == 7 else D[k % 3]
    fit = {10: 0, 11: 1, 12: 111, 13: 112, 14: 127}
    blocks = pc.make_chain(r, 99, pick, epochs=3, fit=fit)
    delegs = pc.delegation(r, D[:4])
    return {"blocks": blocks, "delegs": delegs, "rows": pc.model_rows(blocks, delegs), "D": D, "fit": fit}


def test_key_hash_against_hashlib(ctx):
    r = rng(77)
    for n in (1, 64, 65, 300):
        keys = [rbytes(r, 64) for _ in range(n)]
        got = ctx.byron_key_hash(b"".join(keys))
        assert [bytes(g) for g in got] == [pm.key_hash(k) for k in keys], n
    assert bytes(ctx.byron_key_hash(bytes.fromhex(GOLD["issuer_pk"]))[0]) == bytes.fromhex(GOLD["genesis_key_hash"])


def _golden_headers():
    out = []
    for name in ("ebb", "main"):
        blk = bytes.fromhex(BLOCKS[name])
        d = bm.parse_block(blk, 0, len(blk))
        out.append((Hdr(blk[d["hoff"]:d["hoff"] + d["hlen"]], d["kind"]), d, blk))
    return out


def test_golden_headers(ctx, oracle):
    (ebb, _, _), (main, d, blk) = _golden_headers()
    magic = BLOCKS["protocol_magic"]
    assert magic == 55550001
    xpub = blk[d["delegate"]:d["delegate"] + 64]
    delegs = [(pm.key_hash(blk[d["issuer"]:d["issuer"] + 64]), pm.key_hash(xpub))]
    for pmagic, bits in ((magic, 0), (magic + 1, pm.BIT_SIG)):
        rows = pc.model_rows([ebb, main], delegs, ES, pmagic)
        H = run(ctx, [ebb, main], delegs, pmagic=pmagic)
        same(H, rows, pmagic)
        assert list(H["bits"]) == [0, bits] and list(H["gk_idx"]) == [-1, 0]
    # both header hashes are the reference's: HeaderHash is the main block's (5820 || hash), and the
    # main block's prevHash is the EBB's
    assert bytes(H["header_hash"][1]) == bytes.fromhex(BLOCKS["header_hash"])[2:]
    assert bytes(H["header_hash"][0]) == bytes(H["prev_hash"][1]) == d["prev_hash"]
    assert H["prev_is_genesis"][0] == 1 and H["block_no"][1] == 1
    # without the delegate in the map: PBftNotGenesisDelegate, the signature still verifies
    H = run(ctx, [ebb, main], [(bytes(28), bytes(28))], pmagic=magic)
    assert list(H["bits"]) == [0, pm.BIT_NOT_DELEGATE] and bytes(H["delegate_hash"][1]) == pm.key_hash(xpub)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300])
def test_forged_chain(ctx, forged, n):
    lo = 1 if n == 1 else 0                       # a batch of one: a main header
    blocks, rows = forged["blocks"][lo:lo + n], forged["rows"][lo:lo + n]
    H = run(ctx, blocks, forged["delegs"])
    same(H, rows, n)
    if n == 300:
        bits = [r["bits"] for r in rows]
        gk = [r["gk_idx"] for r in rows]
        assert bits.count(pm.BIT_NOT_DELEGATE) == 6 and bits.count(0) == 294 and gk.count(3) == 1
        assert sum(b.kind == 0 for b in blocks) == 3 and {0, 1, 2} <= set(gk)
        # the fold over the device's columns equals the fold over the model's (the chain's slots run
        # past its 40-slot epochs, so it also has envelope failures)
        ebb = [int(b.kind == 0) for b in blocks]
        want = pm.fold(rows, ebb, K, THR, ES, forged["delegs"])
        v, aux, stop, tip, st = ctx.pbft_update_chain_dep_state(H, ebb, params(), forged["delegs"])
        assert (list(v), [int(a) for a in aux], stop, tip, st) == tuple(want)


def test_signed_message_lengths(ctx, forged):
    mains = [b for b in forged["blocks"] if b.kind == 1]
    picked = [mains[k] for k in sorted(forged["fit"])]
    assert [(64 + len(b.message)) % 128 for b in picked] == [0, 1, 111, 112, 127]
    H = run(ctx, picked, forged["delegs"])
    same(H, pc.model_rows(picked, forged["delegs"]))
    assert not H["bits"].any()


@pytest.fixture(scope="module")
def residues(oracle):
    """one epoch of 128 main headers, three delegates in turn: the SHA-512 stream's input (64 +
    signed message) takes every length modulo 128"""
    r = rng(0x0128)
    D = [bc.Delegate(r) for _ in range(3)]
    mains = pc.make_chain(r, 128, lambda k: D[k % 3], epochs=1, fit={k: k for k in range(128)})[1:]
    delegs = pc.delegation(r, D)
    return mains, delegs, pc.model_rows(mains, delegs)


@pytest.mark.parametrize("shift", range(8))
def test_every_message_residue_at_every_offset(ctx, residues, shift):
    """the 128 residues with every header at arena offset `shift` + its own place, between
    non-zero bytes: over the eight shifts every header sits at every offset 0..7"""
    mains, delegs, rows = residues
    assert [(64 + len(b.message)) % 128 for b in mains] == list(range(128))
    fill = np.random.default_rng(shift).integers(1, 256, 16, dtype=np.uint8).tobytes()
    arena, off = bytearray(fill[:8 + shift]), []
    for i, b in enumerate(mains):
        arena += fill[:i % 3]
        off.append(len(arena))
        arena += b.header
    H = ctx.verify_pbft_headers(np.frombuffer(bytes(arena), np.uint8).copy(), np.array(off, np.uint64),
                                np.array([len(b.header) for b in mains], np.uint32), np.zeros(128, np.uint8), params(),
                                delegs, delegate_hash=True)
    same(H, rows, shift)
    assert not H["bits"].any()


def _mutations(forged):
    base = forged["blocks"][6]                    # a main header of delegate D[2] (in the map)
    ebb = forged["blocks"][0]
    assert base.kind == 1 and base.dlg is forged["D"][2]
    hdr = base.header
    d = pm.decode_header(hdr, 0, ES)
    at = lambda key, k=0: (d[key][0] if isinstance(d[key], tuple) else d[key]) - 3 + k

    def flip(pos, mask=0x01):
        b = bytearray(hdr)
        b[pos] ^= mask
        return bytes(b)
    tag = d["diff_span"][1] - 3                   # consensus: ..., [difficulty], [2, [cert, sig]]
    assert hdr[tag:tag + 2] == b"\x82\x02" and hdr[0] == 0x85
    m = {
        "clean": (hdr, 0, PMAG, 0),
        "sig-R": (flip(at("sig", 3)), 0, PMAG, pm.BIT_SIG),
        "sig-S": (flip(at("sig", 40)), 0, PMAG, pm.BIT_SIG),
        "configured-pm": (hdr, 0, PMAG + 1, pm.BIT_SIG),
        "header-pm": (flip(3), 0, PMAG, 0),                               # not part of the signed message
        "prev": (flip(at("prev_span", 7)), 0, PMAG, pm.BIT_SIG),
        "proof": (flip(at("proof_span", 12)), 0, PMAG, pm.BIT_SIG),
        "slot-id": (flip(d["slotid_span"][1] - 4), 0, PMAG, pm.BIT_SIG),
        "difficulty": (flip(d["diff_span"][1] - 4), 0, PMAG, pm.BIT_SIG),
        "extra": (flip(d["extra_span"][1] - 4), 0, PMAG, pm.BIT_SIG),
        "issuer-key": (flip(at("issuer", 9)), 0, PMAG, pm.BIT_SIG),
        "delegate-key": (flip(at("delegate", 5)), 0, PMAG, None),         # the hash and the verdict
        "delegate-chain-code": (flip(at("delegate", 45)), 0, PMAG, pm.BIT_NOT_DELEGATE),
        "truncated": (hdr[:-1], 0, PMAG, pm.BIT_DECODE),
        "list-length": (b"\x84" + hdr[1:], 0, PMAG, pm.BIT_DECODE),
        "sig-tag": (hdr[:tag + 1] + b"\x03" + hdr[tag + 2:], 0, PMAG, pm.BIT_DECODE),
        "trailing": (hdr + b"\x00", 0, PMAG, pm.BIT_DECODE),
        "main-as-ebb": (hdr, 1, PMAG, pm.BIT_DECODE),
        "ebb-as-main": (ebb.header, 0, PMAG, pm.BIT_DECODE),
        "ebb": (ebb.header, 1, PMAG, 0),
        "ebb-trailing": (ebb.header + b"\x00", 1, PMAG, pm.BIT_DECODE),
        "empty": (b"", 0, PMAG, pm.BIT_DECODE),
    }
    return m


def test_mutations_one_at_a_time(ctx, forged):
    muts = _mutations(forged)
    for pmagic in (PMAG, PMAG + 1):
        names = [k for k, v in muts.items() if v[2] == pmagic]
        hs = [Hdr(muts[k][0], 0 if muts[k][1] else 1) for k in names]
        ebb = [muts[k][1] for k in names]
        rows = pc.model_rows(hs, forged["delegs"], ES, pmagic, is_ebb=ebb)
        H = run(ctx, hs, forged["delegs"], is_ebb=np.array(ebb, np.uint8), pmagic=pmagic)
        same(H, rows, names)
        for k, r in zip(names, rows):
            if muts[k][3] is not None:
                assert r["bits"] == muts[k][3], k
            else:
                assert r["bits"] & pm.BIT_NOT_DELEGATE and r["bits"] & pm.BIT_SIG, k
    # what the mutations of the unsigned parts change
    rows = {k: pm.verify_header(muts[k][0], muts[k][1], ES, muts[k][2], forged["delegs"]) for k in muts}
    assert rows["header-pm"]["header_hash"] != rows["clean"]["header_hash"]
    assert rows["delegate-chain-code"]["delegate_hash"] != rows["clean"]["delegate_hash"]
    assert rows["clean"]["gk_idx"] == 2 and rows["delegate-chain-code"]["gk_idx"] == -1


class BadKey:
    """a delegate whose Ed25519 key is a given 32-byte encoding (it cannot sign: the header carries
    another key's signature)"""

    def __init__(self, r, key32):
        d = bc.Delegate(r)
        self.seed, self.issuer = d.seed, d.issuer
        self.xpub = bytes(key32) + d.xpub[32:]
        H = bc.H
        self.cert = H(4, 4) + H(0, 0) + H(2, 64) + self.issuer + H(2, 64) + self.xpub + H(2, 64) + rbytes(r, 64)


EDGE_KEYS = {
    "identity": (1).to_bytes(32, "little"),
    "order-4": bytes(32),
    "order-2": (FIELD_P - 1).to_bytes(32, "little"),
    "order-8": bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05"),
    "noncanonical-p+1": (FIELD_P + 1).to_bytes(32, "little"),
    "noncanonical-p+3": (FIELD_P + 3).to_bytes(32, "little"),
    "noncanonical-all-ones": b"\xff" * 32,
}


@pytest.fixture(scope="module")
def edge(forged):
    """per multiplicity (1, 3): the forged chain's first 70 headers plus headers under small-order
    and non-canonical delegate keys and with S >= L, each such key used that many times"""
    r = rng(0xed9e)
    out = {}
    prev = forged["blocks"][-1].header_hash
    for uses in (1, 3):
        extra, dl = [], []
        for name, key in EDGE_KEYS.items():
            d = BadKey(r, key)
            dl.append(d)
            extra += [bc.Main(r, d, prev, 5, j, 400 + j) for j in range(uses)]
        d = bc.Delegate(r)                        # a sound key, S + L in place of S
        dl.append(d)
        for j in range(uses):
            b = bc.Main(r, d, prev, 6, j, 500 + j)
            s = int.from_bytes(b.sig[32:], "little") + ORDER_L
            extra.append(b.sign(sig=b.sig[:32] + s.to_bytes(32, "little")))
        blocks = forged["blocks"][:70] + extra
        delegs = forged["delegs"] + pc.delegation(r, dl)
        out[uses] = (blocks, delegs, pc.model_rows(blocks, delegs), len(extra))
    return out


FORCED = {   # name: (PRAOS_PBFT_CK_MIN, key cache option)
    "cached": ("1", None),                 # hits k_pbft_sig_ck, misses k_pbft_sig
    "uncached": (str(1 << 40), None),      # every verify k_pbft_sig
    "off": ("1", 0),                       # PRAOS_OPT_KEYCACHE = 0 on the cached side of the cut-over
}


@pytest.fixture(scope="module")
def forced():
    """contexts forced to either side of the cut-over (read when a context opens), and the cache
    switched off; run_forced checks through praos_pbft_stats that each ran what it says"""
    made = {}
    names = ("PRAOS_PBFT_CK_MIN",)
    old = {k: os.environ.get(k) for k in names}
    try:
        for name, (ck, opt) in FORCED.items():
            os.environ["PRAOS_PBFT_CK_MIN"] = ck
            made[name] = abi.Context(0)
            if opt is not None:
                made[name].set_option(abi.OPT_KEYCACHE, opt)
    finally:
        for k in names:
            if old[k] is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = old[k]
    yield made
    for c in made.values():
        c.close()


def run_forced(forced, blocks, delegs, rows, keys_cached, cached_verifies, is_ebb=None, pmagic=PMAG):
    """the batch through every forced context: equal to the model, equal to each other bit for
    bit, and each context ran the kernels its name says (praos_pbft_stats)"""
    verifies = sum(1 for r in rows if not r["bits"] & pm.BIT_DECODE and r["delegate_hash"] != bytes(28))
    got = {}
    for name, c in forced.items():
        got[name] = run(c, blocks, delegs, is_ebb=is_ebb, pmagic=pmagic)
        same(got[name], rows, name)
        st = c.pbft_stats()
        want_cache = name.startswith("cached")
        assert st["cache"] == want_cache, (name, st)
        if want_cache:
            assert (st["keys_cached"], st["cached_verifies"]) == (keys_cached, cached_verifies), (name, st)
            assert st["uncached_verifies"] == verifies - cached_verifies, (name, st)
        else:
            assert (st["keys_cached"], st["cached_verifies"], st["uncached_verifies"]) == (0, 0, verifies), (name, st)
    for name, H in got.items():
        for c in COLS:
            assert (H[c] == got["uncached"][c]).all(), (name, c)
    return got


@pytest.mark.parametrize("uses", [1, 3])
def test_cached_equals_uncached(forced, edge, uses):
    blocks, delegs, rows, n_extra = edge[uses]
    # the chain's first 70 headers: D[0..2] many times and D[4] twice (main headers 7 and 57), all
    # cached; the 8 edge keys are cached when used three times and missed when used once
    base_keys = 4
    base_hits = sum(1 for b in blocks[:70] if b.kind == 1)
    extra_keys, extra_hits = (8, n_extra) if uses == 3 else (0, 0)
    run_forced(forced, blocks, delegs, rows, base_keys + extra_keys, base_hits + extra_hits)
    tail = [r["bits"] for r in rows[-n_extra:]]
    assert all(b & pm.BIT_SIG for b in tail) and not any(b & pm.BIT_DECODE for b in tail)
    assert [r["bits"] for r in rows[:70]].count(0) >= 60


def test_forged_chain_forced(forced, forged):
    """the whole chain on both sides of the cut-over: three keys hit the cache (290 headers), the key used once and the absent delegate's
    six headers (one key, six uses: cached too) go where their counts send them"""
    mains = [b for b in forged["blocks"] if b.kind == 1]
    assert len(mains) == 297
    run_forced(forced, forged["blocks"], forged["delegs"], forged["rows"], 4, 296)


def test_mutations_forced(forced, forged):
    """the mutated headers (bad R, S, fields, keys, shapes) through every forced context: the
    cached path and k_pbft_sig give the same rejections"""
    muts = _mutations(forged)
    names = [k for k, v in muts.items() if v[2] == PMAG]
    # each twice, so that a mutated header's key is used often enough to be cached
    hs = [Hdr(muts[k][0], 0 if muts[k][1] else 1) for k in names] * 2
    ebb = [muts[k][1] for k in names] * 2
    rows = pc.model_rows(hs, forged["delegs"], ES, PMAG, is_ebb=ebb)
    verifying = [r for r in rows if not r["bits"] & pm.BIT_DECODE and r["delegate_hash"] != bytes(28)]
    keys = {}
    for h, r in zip(hs, rows):
        if not r["bits"] & pm.BIT_DECODE and r["delegate_hash"] != bytes(28):
            d = pm.decode_header(h.header, 0, ES)
            k32 = d["blk"][d["delegate"]:d["delegate"] + 32]
            keys[k32] = keys.get(k32, 0) + 1
    assert len(verifying) == sum(keys.values()) and all(v >= 2 for v in keys.values())
    got = run_forced(forced, hs, forged["delegs"], rows, len(keys), len(verifying), is_ebb=np.array(ebb, np.uint8))
    bits = dict(zip(names, got["uncached"]["bits"][:len(names)]))
    assert bits["clean"] == 0 and bits["sig-R"] == bits["sig-S"] == pm.BIT_SIG


@pytest.fixture(scope="module")
def healthy(oracle):
    """three epochs of an EBB and 12 main headers, three delegates in turn: valid from Origin"""
    r = rng(0x4ea1)
    D = [bc.Delegate(r) for _ in range(3)]
    blocks = pc.make_chain(r, 12, lambda k: D[k % 3], epochs=3)
    return blocks, pc.delegation(r, D), D


def _entries(blocks):
    """the secondary index of a chunk of these blocks (Secondary.hs:93-128), whatever they hold"""
    out, pos = b"", 0
    for b in blocks:
        slot = b.epoch if b.kind == 0 else b.epoch * ES + b.sie
        out += (pos.to_bytes(8, "big") + (3).to_bytes(2, "big") + len(b.header).to_bytes(2, "big") +
                zlib.crc32(b.bytes).to_bytes(4, "big") + b.header_hash + slot.to_bytes(8, "big"))
        pos += len(b.bytes)
    return out


def _write_dir(path, blocks, per_chunk=13):
    for k in range(0, len(blocks), per_chunk):
        part = blocks[k:k + per_chunk]
        c = k // per_chunk
        (path / f"{c:05d}.chunk").write_bytes(b"".join(b.bytes for b in part))
        (path / f"{c:05d}.secondary").write_bytes(_entries(part))


def test_three_chunk_directory(ctx, healthy, tmp_path):
    blocks, delegs, D = healthy
    good, bad = tmp_path / "good", tmp_path / "bad"
    good.mkdir()
    bad.mkdir()
    _write_dir(good, blocks)
    ebb = [int(b.kind == 0) for b in blocks]
    rows = pc.model_rows(blocks, delegs)
    want = pm.fold(rows, ebb, K, THR, ES, delegs)
    assert want[2] == len(blocks) == 39
    res = immutable.validate_byron_headers(ctx, str(good), params(), delegs)
    assert res["stop"] is None and res["headers"] == 39 and (res["tip"], res["state"]) == (want[3], want[4])
    assert [(r["chunk"], r["headers"], r["chain_stop"]) for r in res["rows"]] == [(0, 13, 13), (1, 13, 13), (2, 13, 13)]
    # one bad signature in the second chunk: the walk stops there, state and tip are those before it
    j = 13 + 5
    broken = copy.copy(blocks[j])
    broken.sign(sig=broken.sig[:40] + bytes([broken.sig[40] ^ 0x01]) + broken.sig[41:])
    mixed = blocks[:j] + [broken] + blocks[j + 1:]
    _write_dir(bad, mixed)
    want = pm.fold(pc.model_rows(mixed, delegs), ebb, K, THR, ES, delegs)
    assert want[2] == j and want[0][j] == pm.V_INVALID_SIG
    res = immutable.validate_byron_headers(ctx, str(bad), params(), delegs)
    assert res["stop"] == (1, 5, pm.V_INVALID_SIG, 0) and res["headers"] == j and len(res["rows"]) == 2
    assert (res["tip"], res["state"]) == (want[3], want[4]) and res["tip"][2] == blocks[j - 1].header_hash
    # carried state: the second and third chunk's headers after the first's equal the one walk
    first = pm.fold(rows[:13], ebb[:13], K, THR, ES, delegs)
    arena, off, ln, e = pc.columns(blocks[13:])
    _, v, _, stop, tip, st = ctx.validate_pbft_headers(arena, off, ln, e, params(), delegs, first[3], first[4])
    full = pm.fold(rows, ebb, K, THR, ES, delegs)
    assert stop == 26 and not v.any() and (tip, st) == (full[3], full[4])


def _harness(path, delegs, k, thr, es, pmagic, tmp_path):
    harness = os.path.join(os.path.dirname(HERE), "integration", "c", "ffi_harness")
    assert os.path.exists(harness), "build it: make -C integration/c (done by __graft_entry__.build())"
    df = tmp_path / "delegs.txt"
    df.write_text("".join(f"{bytes(g).hex()} {bytes(d).hex()}\n" for g, d in delegs))
    out = subprocess.run([harness, "--pbft-headers", str(path), str(k), str(thr), str(es), str(pmagic), str(df)],
                         check=True, capture_output=True, text=True, timeout=120).stdout
    return json.loads(out.strip().splitlines()[-1])


def test_harness_phase(ctx, healthy, tmp_path):
    """ffi_harness --pbft-headers (the foreign-call sequence of Batch.hs validatePBftHeaderBatch)
    prints what the binding returns: over the golden pair and over the forged directory."""
    (ebb, _, eblk), (main, d, blk) = _golden_headers()
    magic = BLOCKS["protocol_magic"]
    gdir = tmp_path / "golden"
    gdir.mkdir()
    data = eblk + blk
    (gdir / "00000.chunk").write_bytes(data)
    (gdir / "00000.secondary").write_bytes(bm.parse_chunk(data, None, (10, magic))["entries"])
    delegs = [(pm.key_hash(blk[d["issuer"]:d["issuer"] + 64]), pm.key_hash(blk[d["delegate"]:d["delegate"] + 64]))]
    rows = pc.model_rows([ebb, main], delegs, 10, magic)
    want = pm.fold(rows, [1, 0], K, THR, 10, delegs)
    assert want[2] == 2
    got = _harness(gdir, delegs, K, THR, 10, magic, tmp_path)
    assert (got["phase"], got["headers"], got["valid"], got["stop_chunk"]) == ("pbft_headers", 2, 2, -1)
    assert got["tip_hash"] == rows[1]["header_hash"].hex() and got["state"] == pm.state_encode(want[4]).hex()
    assert got["signers"] == 1 and got["tip_block_no"] == 1
    got = _harness(gdir, delegs, K, THR, 10, magic + 1, tmp_path)
    assert (got["valid"], got["stop_chunk"], got["stop_index"], got["stop_verdict"], got["stop_bits"]) == \
        (1, 0, 1, pm.V_INVALID_SIG, pm.BIT_SIG)
    # the forged chain, three chunks
    blocks, fdelegs, _ = healthy
    fdir = tmp_path / "forged"
    fdir.mkdir()
    _write_dir(fdir, blocks)
    want = pm.fold(pc.model_rows(blocks, fdelegs), [int(b.kind == 0) for b in blocks], K, THR, ES, fdelegs)
    got = _harness(fdir, fdelegs, K, THR, ES, PMAG, tmp_path)
    assert (got["headers"], got["valid"], got["stop_chunk"]) == (39, 39, -1)
    assert got["state"] == pm.state_encode(want[4]).hex() and got["tip_hash"] == want[3][2].hex()
    assert (got["tip_slot"], got["tip_block_no"], got["tip_is_ebb"], got["signers"]) == (want[3][0], want[3][1], 0, K)
