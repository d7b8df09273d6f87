"""GPU: Byron blocks and EBBs through praos_validate_chunk_cfg / praos_verify_byron_integrity
(csrc/k_byron.hip), compared field by field with tests/byron_model.py.

The reference's golden EBB and main block are a two-block chunk; a forged chain (byron_corpus)
covers the Merkle shapes, the Blake2b and SHA-512 block edges and the CRC tile; every other case
is one mutation of that chain.  UNSUPPORTED may come back only where the test names it: every
parse goes through check(), which refuses it elsewhere."""
import json
import os
import zlib

import numpy as np
import pytest

import byron_corpus as bc
import byron_model as bm
import chunk_corpus as cc
from helpers import rng
from praos_hip import abi, immutable

pytestmark = pytest.mark.gpu
SPKP = 129600
BYRON = (bc.EPOCH_SLOTS, bc.PM)
HERE = os.path.dirname(os.path.abspath(__file__))
assert hasattr(abi.load(), "praos_validate_chunk_cfg")      # without the feature: fails at import

# 3 epochs, 23 blocks: transaction counts 0 1 2 3 4 5 7 8 9 (every Merkle shape around a power of
# two), transaction sizes 1..300 (Blake2b's 128-byte blocks), SHA-512 input lengths (64 + message)
# and message lengths at 111 112 127 128 129 mod 128, one EBB body above the 16,384-byte CRC tile,
# definite and indefinite txPayload lists
PLAN = [
    [{"tx_sizes": ()}, {"tx_sizes": (1,), "indef": True}, {"tx_sizes": (2, 300)}, {"tx_sizes": (24, 25, 26)},
     {"tx_sizes": (127, 128, 129, 130)}, {"tx_sizes": (10,), "fit": (111, 64)}, {"tx_sizes": (11,), "fit": (112, 64)},
     {"tx_sizes": (12,), "fit": (127, 64)}],
    [{"tx_sizes": (3, 255, 256, 257, 200), "indef": True, "ebb_ids": 600}, {"tx_sizes": (5, 6, 7, 8, 9, 100, 23)},
     {"tx_sizes": (13,), "fit": (0, 64)}, {"tx_sizes": (14,), "fit": (1, 64), "indef": True},
     {"tx_sizes": (15,), "fit": (111, 0)}, {"tx_sizes": (), "fit": (112, 0), "indef": True}],
    [{"tx_sizes": (40, 41, 42, 43, 44, 45, 46, 47)}, {"tx_sizes": (1, 2, 3, 4, 5, 6, 7, 8, 290), "indef": True},
     {"tx_sizes": (16,), "fit": (127, 0)}, {"tx_sizes": (17,), "fit": (0, 0)}, {"tx_sizes": (18,), "fit": (1, 0)},
     {"tx_sizes": (64,)}],
]
T = 6          # the mutated block: one transaction, definite lists, in the middle of epoch 0
N3 = 4         # a block with three transactions


class Chain:
    def __init__(self):
        r = rng(2024)
        self.dlg = bc.Delegate(r)
        self.blocks = bc.make_chain(r, PLAN, self.dlg)
        self.blobs = [b.bytes for b in self.blocks]
        self.data, self.off, self.crc = cc.layout(self.blobs)

    def with_block(self, i, blob, trust=False):
        blobs = list(self.blobs)
        blobs[i] = blob
        data, off, crc = cc.layout(blobs)
        return data, off, (crc if trust else self.crc)

    def resigned(self, i, **fields):
        """Block i rebuilt and signed again with other fields; the chain's own block is restored."""
        b = self.blocks[i]
        old = {k: getattr(b, k) for k in fields}
        for k, v in fields.items():
            setattr(b, k, v)
        blob = b.sign().bytes
        for k, v in old.items():
            setattr(b, k, v)
        b.sign()
        assert b.bytes == self.blobs[i]
        return blob


@pytest.fixture(scope="module")
def chain(oracle):
    c = Chain()
    assert len(c.blocks) == 23 and sorted({len(b.txs) for b in c.blocks if b.kind}) == [0, 1, 2, 3, 4, 5, 7, 8, 9]
    sha = {(64 + len(b.message)) % 128 for b in c.blocks if b.kind}
    msg = {len(b.message) % 128 for b in c.blocks if b.kind}
    assert {111, 112, 127, 0, 1} <= sha and {111, 112, 127, 0, 1} <= msg
    assert max(len(b.bytes) for b in c.blocks if not b.kind) > 16384
    assert len(c.blocks[T].txs) == 1 and not c.blocks[T].indef and len(c.blocks[N3].txs) == 3
    return c


def same(got, want, skip=()):
    for k, w in want.items():
        if k in skip:
            continue
        g = got[k]
        if isinstance(w, np.ndarray):
            assert g.shape == w.shape and (g == w).all(), k
        else:
            assert g == w, (k, g, w)
    assert set(got) == set(want)


def check(ctx, data, crc, off, byron=BYRON, unsupported=False, skip=()):
    """One parse, compared with the model in every field; UNSUPPORTED only where the caller names it."""
    got = ctx.validate_chunk(data, crc, off, SPKP, byron=byron)
    want = bm.parse_chunk(data, crc, byron, SPKP, off)
    same(got, want, skip)
    assert (got["outcome"] == abi.CHUNK_UNSUPPORTED) == unsupported
    return got


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(os.path.join(HERE, "golden", "byron_blocks.json")))
    return bytes.fromhex(g["ebb"]), bytes.fromhex(g["main"]), g["protocol_magic"]


@pytest.mark.parametrize("hints", [False, True])
def test_golden_pair(ctx, golden, hints):
    ebb, main, pm = golden
    data = ebb + main
    crc = [zlib.crc32(ebb), zlib.crc32(main)]
    got = check(ctx, data, crc if hints else None, [0, 87] if hints else None, byron=(10, pm))
    assert (got["outcome"], got["blocks"], got["checked"]) == (abi.CHUNK_OK, 2, 0 if hints else 2)
    e = got["entries"]
    h0 = "88900fba40903da0b4a38d06a3d2bdadff6d49a8a6b804efe1b4522890e3b82c"
    h1 = "93e9c624e615f90e7a78fb8eb12c4520befc1a3379ad98b8218833cc77b9c26f"
    ent = lambda o, ho, hl, c, h, s: (o.to_bytes(8, "big") + ho.to_bytes(2, "big") + hl.to_bytes(2, "big") +
                                      c.to_bytes(4, "big") + bytes.fromhex(h) + s.to_bytes(8, "big"))
    assert e == ent(0, 3, 80, crc[0], h0, 0) + ent(87, 3, 606, crc[1], h1, 1)
    assert list(got["is_ebb"]) == [1, 0] and list(got["prev_is_genesis"]) == [1, 0] and list(got["block_no"]) == [0, 1]
    assert list(got["integrity"]) == ([-1, -1] if hints else [0, 0])
    # a stale index: both blocks take verifyBlockIntegrity and pass
    stale = check(ctx, data, [1, 2], [0, 87], byron=(10, pm))
    assert (stale["outcome"], stale["checked"], list(stale["integrity"])) == (abi.CHUNK_OK, 2, [0, 0])
    # another protocol magic: PM only
    other = check(ctx, data, None, None, byron=(10, pm + 1))
    assert (other["outcome"], other["integrity_bits"], other["blocks"], other["truncate_at"], other["err_slot"]) == \
        (abi.CHUNK_ERR_CORRUPT, abi.BLK_PM, 1, 87, 1)


def test_golden_pair_without_byron_is_unsupported_as_before(ctx, golden):
    ebb, main, _ = golden
    old = ctx.validate_chunk(ebb + main, None, None, SPKP)
    assert (old["outcome"], old["truncate_at"], old["blocks"]) == (abi.CHUNK_UNSUPPORTED, 0, 0) and "is_ebb" not in old
    same(old, bm.parse_chunk(ebb + main, None, None, SPKP))
    # byron_epoch_slots = 0 through the new entry: the same bytes out
    lib = ctx.L
    import ctypes
    data = np.frombuffer(ebb + main, np.uint8)
    outs = []
    for new in (False, True):
        ch, res, out = abi.Chunk(), abi.ChunkResult(), abi.ChunkOut()
        ch.bytes, ch.bytes_len = abi.ptr(data), len(data)
        bufs = [np.zeros(8 * 56, np.uint8), np.zeros(8, np.uint64), np.zeros((8, 32), np.uint8), np.zeros(8, np.uint8),
                np.zeros(8, np.int8)]
        out.cap, out.entries, out.block_no, out.prev_hash = 8, abi.ptr(bufs[0]), abi.ptr(bufs[1], abi.u64p), abi.ptr(bufs[2])
        out.prev_is_genesis, out.integrity = abi.ptr(bufs[3]), abi.ptr(bufs[4], ctypes.POINTER(ctypes.c_int8))
        if new:
            cfg = abi.ChunkCfg(SPKP, 0, 55550001, 0)
            rc = lib.praos_validate_chunk_cfg(ctx.h, ctypes.byref(ch), ctypes.byref(cfg), ctypes.byref(res),
                                              ctypes.byref(out), None)
        else:
            rc = lib.praos_validate_chunk(ctx.h, ctypes.byref(ch), SPKP, ctypes.byref(res), ctypes.byref(out))
        assert rc == 0
        outs.append(bytes(res) + b"".join(b.tobytes() for b in bufs))
    assert outs[0] == outs[1]


def test_forged_chain_all_untrusted(ctx, chain):
    got = check(ctx, chain.data, None, None)
    n = len(chain.blocks)
    assert (got["outcome"], got["blocks"], got["checked"], got["truncate_at"]) == (abi.CHUNK_OK, n, n, len(chain.data))
    assert list(got["is_ebb"]) == [1 - b.kind for b in chain.blocks]
    assert list(got["block_no"]) == [b.difficulty for b in chain.blocks]
    slots = [int.from_bytes(got["entries"][56 * i + 48:56 * i + 56], "big") for i in range(n)]
    assert slots == [b.epoch if not b.kind else b.epoch * bc.EPOCH_SLOTS + b.sie for b in chain.blocks]
    # a stale index with the right offsets: still every block checked, candidates confirmed on the device
    stale = check(ctx, chain.data, [c ^ 1 for c in chain.crc], chain.off)
    assert (stale["outcome"], stale["checked"], stale["rescanned_from"]) == (abi.CHUNK_OK, n, len(chain.data))


def test_forged_chain_trusted(ctx, chain):
    got = check(ctx, chain.data, chain.crc, chain.off)
    assert (got["outcome"], got["blocks"], got["checked"]) == (abi.CHUNK_OK, len(chain.blocks), 0)


def _flip(blob, at, mask=0x01):
    return blob[:at] + bytes([blob[at] ^ mask]) + blob[at + 1:]


def _mutations(chain):
    """name -> (blob for block T, outcome, bits or None where the model alone decides)"""
    b = chain.blocks[T]
    blob = b.bytes
    d = bm.parse_block(blob, 0, len(blob))
    SIG, BODY = abi.BLK_PBFT_SIG, abi.BLK_BODY_HASH
    tx, wit = d["pairs"][0]
    tag = blob.index(b"\x82\x02\x82\x84") + 1
    other = chain.blocks[T - 2].header_hash
    return {
        "prev": (_flip(blob, d["prev_span"][0] + 9), abi.CHUNK_ERR_CORRUPT, SIG),
        "proof": (_flip(blob, d["proof_span"][1] - 40), abi.CHUNK_ERR_CORRUPT, None),
        "ssc_proof": (_flip(blob, blob.index(b.ssc_proof) + 10), abi.CHUNK_ERR_CORRUPT, SIG),
        "slot_id": (_flip(blob, d["slotid_span"][1] - 1), abi.CHUNK_ERR_CORRUPT, SIG),
        "difficulty": (_flip(blob, d["diff_span"][1] - 1), abi.CHUNK_ERR_CORRUPT, SIG),
        "extra": (_flip(blob, d["extra_span"][1] - 5), abi.CHUNK_ERR_CORRUPT, SIG),
        "sig": (_flip(blob, d["sig"] + 40, 0x20), abi.CHUNK_ERR_CORRUPT, SIG),
        "sig_r": (_flip(blob, d["sig"] + 3), abi.CHUNK_ERR_CORRUPT, SIG),
        "wrong_pm": (chain.resigned(T, pm=bc.PM + 1), abi.CHUNK_ERR_CORRUPT, abi.BLK_PM),
        "dlg_payload": (_flip(blob, d["dlg_span"][0], 0x20), abi.CHUNK_ERR_CORRUPT, BODY),
        "upd_payload": (_flip(blob, d["upd_span"][1] - 1, 0x20), abi.CHUNK_ERR_CORRUPT, BODY),
        "transaction": (_flip(blob, tx[1] - 1), abi.CHUNK_ERR_CORRUPT, BODY),
        "witness": (_flip(blob, wit[1] - 1), abi.CHUNK_ERR_CORRUPT, BODY),
        "ntx": (_flip(blob, d["proof_span"][0] + 2), abi.CHUNK_ERR_CORRUPT, SIG | BODY),
        "sig_tag_0": (_flip(blob, tag, 0x02), abi.CHUNK_ERR_READ, 0),
        "prev_31_bytes": (chain.resigned(T, prev=b.prev[:31]), abi.CHUNK_ERR_READ, 0),
        "broken_link": (chain.resigned(T, prev=other), abi.CHUNK_ERR_HASH_MISMATCH, 0),
    }


CASES = ["prev", "proof", "ssc_proof", "slot_id", "difficulty", "extra", "sig", "sig_r", "wrong_pm", "dlg_payload",
         "upd_payload", "transaction", "witness", "ntx", "sig_tag_0", "prev_31_bytes", "broken_link"]


@pytest.fixture(scope="module")
def mutations(chain):
    m = _mutations(chain)
    assert list(m) == CASES
    return m


@pytest.mark.parametrize("case", CASES)
def test_one_mutation(ctx, chain, mutations, case):
    blob, outcome, bits = mutations[case]
    assert blob != chain.blobs[T]
    data, off, crc = chain.with_block(T, blob)
    # a later block's link is broken too: the earlier error is the one reported
    later = chain.resigned(T + 3, prev=chain.blocks[0].header_hash)
    data = data[:off[T + 3]] + later + data[off[T + 3] + len(chain.blobs[T + 3]):]
    assert len(later) == len(chain.blobs[T + 3])
    for c, o in ((None, None), (crc, off)):
        got = check(ctx, data, c, o)
        assert (got["outcome"], got["blocks"], got["truncate_at"]) == (outcome, T, off[T])
        if bits is not None:
            assert got["integrity_bits"] == bits
        assert got["entries"] == check(ctx, chain.data, chain.crc, chain.off)["entries"][:56 * T]   # the prefix
        if outcome == abi.CHUNK_ERR_CORRUPT:
            assert got["err_slot"] == bc.EPOCH_SLOTS * chain.blocks[T].epoch + (
                chain.blocks[T].sie ^ 1 if case == "slot_id" else chain.blocks[T].sie)
        if case == "broken_link":
            assert got["expected_prev"] == chain.blocks[T - 1].header_hash
            assert got["actual_prev"] == chain.blocks[T - 2].header_hash


@pytest.mark.parametrize("case", ["dlg_payload", "upd_payload", "transaction", "witness", "sig", "ntx"])
def test_mutation_under_a_matching_crc_is_trusted(ctx, chain, mutations, case):
    """The index's checksum recomputed over the damaged block: checkEntries trusts it.  Damage in
    the body changes nothing; damage in the header changes only the header hash, so the next
    block no longer lines up -- never ERR_CORRUPT."""
    data, off, crc = chain.with_block(T, mutations[case][0], trust=True)
    got = check(ctx, data, crc, off)
    assert got["checked"] == 0
    if case in ("sig", "ntx"):
        assert (got["outcome"], got["blocks"]) == (abi.CHUNK_ERR_HASH_MISMATCH, T + 1)
    else:
        assert (got["outcome"], got["blocks"]) == (abi.CHUNK_OK, len(chain.blocks))
        assert got["entries"][:56 * T] == check(ctx, chain.data, chain.crc, chain.off)["entries"][:56 * T]


def test_epoch0_ebb_after_the_first_block_is_a_mismatch(ctx, chain):
    k = 5
    stray = bc.EBB(rng(3), chain.blocks[k - 1].header_hash, 0, chain.blocks[k - 1].difficulty)
    blobs = chain.blobs[:k] + [stray.bytes] + chain.blobs[k:]
    data, off, _ = cc.layout(blobs)
    got = check(ctx, data, None, None)
    assert (got["outcome"], got["blocks"], got["truncate_at"]) == (abi.CHUNK_ERR_HASH_MISMATCH, k, off[k])
    assert got["actual_prev_is_genesis"] == 1 and got["actual_prev"] == bytes(32)
    assert got["expected_prev"] == chain.blocks[k - 1].header_hash and got["err_hash"] == stray.header_hash
    # the same EBB with epoch 1 is BlockHash prev and lines up (the block after it then does not)
    ok = bc.EBB(rng(3), chain.blocks[k - 1].header_hash, 1, chain.blocks[k - 1].difficulty)
    data, off, _ = cc.layout(chain.blobs[:k] + [ok.bytes] + chain.blobs[k:])
    got = check(ctx, data, None, None)
    assert (got["outcome"], got["blocks"]) == (abi.CHUNK_ERR_HASH_MISMATCH, k + 1)


def test_unsupported_only_for_an_unpinned_root(ctx, chain):
    """A txRoot that is not the body's, everything else (signature included) right: with n = 3 no
    reference file pins the rule that failed, so the reference decides; with n = 1 the root is
    the leaf hash the golden block pins, and the block is corrupt."""
    bad3 = chain.resigned(N3, bad_root=True)
    data, off, crc = chain.with_block(N3, bad3)
    for c, o in ((None, None), (crc, off)):
        got = check(ctx, data, c, o, unsupported=True)
        assert (got["outcome"], got["blocks"], got["truncate_at"]) == (abi.CHUNK_UNSUPPORTED, N3, off[N3])
        assert got["entries"] == check(ctx, chain.data, chain.crc, chain.off)["entries"][:56 * N3]
    bad1 = chain.resigned(T, bad_root=True)
    data, off, crc = chain.with_block(T, bad1)
    got = check(ctx, data, crc, off)
    assert (got["outcome"], got["integrity_bits"], got["blocks"], got["truncate_at"]) == \
        (abi.CHUNK_ERR_CORRUPT, abi.BLK_BODY_HASH, T, off[T])
    # under a matching CRC the block is not looked at (its header hash differs, so the next one does not line up)
    data, off, crc = chain.with_block(N3, bad3, trust=True)
    got = check(ctx, data, crc, off)
    assert (got["outcome"], got["blocks"], got["checked"]) == (abi.CHUNK_ERR_HASH_MISMATCH, N3 + 1, 0)


def test_mixed_chunk(ctx, chain):
    """Byron blocks, then two Babbage blocks: the first one's prevHash is a Byron header hash."""
    r = rng(77)
    last = chain.blocks[7]
    s1 = cc.Block(r, SPKP, 6, 5000, last.difficulty + 1, last.header_hash)
    s2 = cc.Block(r, SPKP, 6, 5020, last.difficulty + 2, s1.header_hash)
    blobs = chain.blobs[:8] + [s1.bytes, s2.bytes]
    data, off, crc = cc.layout(blobs)
    for c, o in ((None, None), (crc, off), ([x ^ 1 for x in crc], off)):
        got = check(ctx, data, c, o)
        assert (got["outcome"], got["blocks"]) == (abi.CHUNK_OK, 10)
        assert list(got["is_ebb"]) == [1] + [0] * 9
    # that one link broken
    s1.f["prev_hash"] = chain.blocks[6].header_hash
    s1.sign()
    s2.f["prev_hash"] = s1.header_hash
    s2.sign()
    data, off, crc = cc.layout(chain.blobs[:8] + [s1.bytes, s2.bytes])
    got = check(ctx, data, None, None)
    assert (got["outcome"], got["blocks"], got["truncate_at"]) == (abi.CHUNK_ERR_HASH_MISMATCH, 8, off[8])
    assert got["expected_prev"] == last.header_hash and got["actual_prev"] == chain.blocks[6].header_hash
    # without Byron the same file stops at its first item, as it always did
    old = check(ctx, data, None, None, byron=None, unsupported=True)
    assert (old["outcome"], old["truncate_at"]) == (abi.CHUNK_UNSUPPORTED, 0)


def test_three_chunk_directory(ctx, chain, tmp_path):
    cuts = [0, 9, 16, len(chain.blocks)]       # one chunk per epoch
    for k in range(3):
        blobs = chain.blobs[cuts[k]:cuts[k + 1]]
        data, _, _ = cc.layout(blobs)
        (tmp_path / f"{k:05d}.chunk").write_bytes(data)
        (tmp_path / f"{k:05d}.secondary").write_bytes(bm.parse_chunk(data, None, BYRON)["entries"])
    rows = immutable.validate_immutable(ctx, str(tmp_path), SPKP, byron=BYRON)
    assert len(rows) == 3
    for k, row in enumerate(rows):
        assert (row["outcome"], row["blocks"], row["checked"]) == (abi.CHUNK_OK, cuts[k + 1] - cuts[k], 0)
        assert row["entries_match"] and row["fits"]
    rows = immutable.validate_immutable(ctx, str(tmp_path), SPKP)
    assert len(rows) == 1 and rows[0]["outcome"] == abi.CHUNK_UNSUPPORTED and rows[0]["blocks"] == 0


def test_direct_entry_equals_the_model(ctx, chain, mutations, golden):
    r = rng(9)
    shelley = cc.Block(r, SPKP, 6, 7000, 1, bytes(32)).bytes
    blobs = (chain.blobs + [m[0] for m in mutations.values()] +
             [chain.resigned(N3, bad_root=True), chain.resigned(T, bad_root=True), shelley, b"\x82\x01\x83\x00\x00\x00",
              b"\x82\x00", golden[0], golden[1]])
    data, off, _ = cc.layout(blobs)
    res, which = ctx.verify_byron_integrity(data, off, [len(b) for b in blobs], bc.EPOCH_SLOTS, bc.PM)
    want = [bm.integrity(b, bc.PM) for b in blobs]
    assert [(int(a), int(b)) for a, b in zip(res, which)] == want
    n = len(chain.blobs)
    assert not res[:n].any() and not which[:n].any()
    assert want[-1] == (abi.BLK_PM, 0) and want[-2] == (0, 0) and want[-3][0] == want[-4][0] == want[-5][0] == 1
    seen = {w for _, w in want}
    assert {abi.BYRON_W_DLG, abi.BYRON_W_UPD, abi.BYRON_W_NTX, abi.BYRON_W_WIT, abi.BYRON_W_ROOT} <= seen


@pytest.fixture(scope="module")
def residues(oracle):
    """An EBB and 128 main blocks: the SHA-512 stream's input (64 + signed message) takes every
    length modulo 128, the witness stream 2 + 12 n bytes for n = 0..12 transactions."""
    plan = [[{"tx_sizes": tuple(5 + j for j in range(k % 13)), "fit": (k, 64), "indef": k % 2 == 1}
             for k in range(128)]]
    blocks = bc.make_chain(rng(0x0128), plan)
    assert [(64 + len(b.message)) % 128 for b in blocks[1:]] == list(range(128))
    want = [bm.integrity(b.bytes, bc.PM) for b in blocks]
    assert want == [(0, 0)] * 129
    return blocks, want


@pytest.mark.parametrize("shift", range(8))
def test_every_message_residue_at_every_offset(ctx, residues, shift):
    """Those blocks with every one at arena offset `shift` + its own place, between non-zero
    bytes: over the eight shifts every block sits at every offset 0..7."""
    blocks, want = residues
    fill = np.random.default_rng(shift).integers(1, 256, 16, dtype=np.uint8).tobytes()
    arena, off = bytearray(fill[:shift]), []
    for i, b in enumerate(blocks):
        arena += fill[:i % 3]
        off.append(len(arena))
        arena += b.bytes
    res, which = ctx.verify_byron_integrity(bytes(arena), off, [len(b.bytes) for b in blocks], bc.EPOCH_SLOTS, bc.PM)
    assert [(int(a), int(b)) for a, b in zip(res, which)] == want


def test_harness_phase_over_the_golden_pair(ctx, golden, tmp_path):
    """ffi_harness --validate-chunk-byron (the foreign-call sequence of Batch.hs validateChunkBatch
    with the Byron parameters) prints what the binding returns."""
    import subprocess
    harness = os.path.join(os.path.dirname(HERE), "integration", "c", "ffi_harness")
    assert os.path.exists(harness), "build it: make -C integration/c (done by __graft_entry__.build())"
    ebb, main, pm = golden
    data = ebb + main
    want = check(ctx, data, None, None, byron=(10, pm))
    (tmp_path / "00000.chunk").write_bytes(data)
    for sec in (None, want["entries"]):
        if sec is not None:
            (tmp_path / "00000.secondary").write_bytes(sec)
        out = subprocess.run([harness, "--validate-chunk-byron", str(tmp_path), "0", str(SPKP), "10", str(pm)],
                             check=True, capture_output=True, text=True, timeout=120).stdout
        got = json.loads(out.strip().splitlines()[-1])
        assert (got["phase"], got["outcome"], got["blocks"]) == ("validate_chunk_byron", "OK", 2)
        assert got["entries"] == want["entries"].hex() and got["is_ebb"] == [1, 0] and got["block_no"] == [0, 1]
        assert got["checked"] == (2 if sec is None else 0) and got["entries_match"] == (sec is not None)
    # the old phase on the same directory: UNSUPPORTED at 0, as before
    out = subprocess.run([harness, "--validate-chunk", str(tmp_path), "0", str(SPKP)], check=True, capture_output=True,
                         text=True, timeout=120).stdout
    got = json.loads(out.strip().splitlines()[-1])
    assert (got["phase"], got["outcome"], got["blocks"], got["truncate_at"]) == ("validate_chunk", "UNSUPPORTED", 0, 0)
