"""CPU: the Byron rules of tests/byron_model.py against the reference's golden blocks
(tests/golden/byron_blocks.json), and the forger of tests/byron_corpus.py against the model."""
import json
import os

import pytest

import byron_corpus as bc
import byron_model as bm
from helpers import rng

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(os.path.join(HERE, "golden", "byron_blocks.json")))
    return {"ebb": bytes.fromhex(g["ebb"]), "main": bytes.fromhex(g["main"]),
            "header_hash": bytes.fromhex(g["header_hash"]), "pm": g["protocol_magic"]}


def test_golden_sizes_and_header_hashes(golden):
    assert (len(golden["ebb"]), len(golden["main"]), len(golden["header_hash"])) == (87, 862, 34)
    e = bm.parse_block(golden["ebb"], 0, 87)
    m = bm.parse_block(golden["main"], 0, 862)
    assert (e["hoff"], e["hlen"], m["hoff"], m["hlen"]) == (3, 80, 3, 606)
    assert m["header_hash"].hex().startswith("93e9c624") and m["header_hash"].hex().endswith("c26f")
    assert golden["header_hash"] == b"\x58\x20" + m["header_hash"]           # disk/HeaderHash
    assert e["header_hash"].hex().startswith("88900fba") and e["header_hash"].hex().endswith("b82c")
    assert m["prev_hash"] == e["header_hash"]                                # the pair lines up
    assert (m["pm"], m["epoch"], m["slot_in_epoch"], m["block_no"]) == (55550001, 0, 1, 1)
    assert (e["pm"], e["epoch"], e["block_no"], e["prev_hash"]) == (55550001, 0, 0, None)   # GenesisHash


def test_golden_signature_and_body_proof(golden, oracle):
    blk = golden["main"]
    d = bm.parse_block(blk, 0, len(blk))
    msg = bm.signed_message(blk, d)
    assert msg[:2] == b"01" and msg[66:73] == b"\x09\x1a" + (55550001).to_bytes(4, "big") + b"\x85"
    assert oracle.ed25519_verify(blk[d["delegate"]:d["delegate"] + 32], msg, blk[d["sig"]:d["sig"] + 64])
    assert d["ntx"] == len(d["pairs"]) == 1
    assert bm.body_which(blk, d) == 0                                        # all five comparisons hold
    assert bm.integrity(blk, golden["pm"]) == (0, 0)
    assert bm.integrity(blk, 764824073) == (bm.BLK_PM, 0)
    assert bm.integrity(golden["ebb"], 1) == (0, 0)                          # an EBB always passes
    bad = bytearray(blk)
    bad[d["sig"] + 5] ^= 1
    assert bm.integrity(bad, golden["pm"]) == (bm.BLK_PBFT_SIG, 0)


def test_golden_pair_is_a_chunk(golden):
    data = golden["ebb"] + golden["main"]
    res = bm.parse_chunk(data, None, (10, golden["pm"]))
    assert (res["outcome"], res["blocks"], res["checked"], res["truncate_at"]) == (bm.OK, 2, 2, 949)
    assert list(res["is_ebb"]) == [1, 0] and list(res["prev_is_genesis"]) == [1, 0] and list(res["block_no"]) == [0, 1]
    e = res["entries"]
    assert int.from_bytes(e[56:64], "big") == 87 and e[64:68] == (3).to_bytes(2, "big") + (606).to_bytes(2, "big")
    assert int.from_bytes(e[48:56], "big") == 0 and int.from_bytes(e[104:112], "big") == 1
    off = bm.parse_chunk(data, None, None)
    assert (off["outcome"], off["truncate_at"], off["blocks"]) == (bm.UNSUPPORTED, 0, 0)


def test_merkle_root_is_the_binary_counter_tree():
    """The recursive split at the largest power of two below n equals the stack form the kernel uses."""
    r = rng(5)
    leaves = [bytes(r.getrandbits(8) for _ in range(32)) for _ in range(21)]
    for n in range(1, 22):
        stack = []
        for i, leaf in enumerate(leaves[:n], 1):
            h = leaf
            while i % 2 == 0:
                h = bm.b2b(b"\x01" + stack.pop() + h)
                i //= 2
            stack.append(h)
        acc = stack.pop()
        while stack:
            acc = bm.b2b(b"\x01" + stack.pop() + acc)
        assert acc == bm.merkle_root(leaves[:n]), n


def test_forged_blocks_pass_the_model(oracle):
    r = rng(11)
    plan = [[{"tx_sizes": ()}, {"tx_sizes": (1,), "indef": True}, {"tx_sizes": (25, 300, 129), "attr_len": 40}],
            [{"tx_sizes": (2, 128, 127, 24, 26), "fit": (111, 64)}]]
    chain = bc.make_chain(r, plan)
    assert [b.kind for b in chain] == [0, 1, 1, 1, 0, 1]
    assert [b.difficulty for b in chain] == [0, 1, 2, 3, 3, 4]
    for b in chain:
        d = bm.parse_block(b.bytes, 0, len(b.bytes))
        assert d["header_hash"] == b.header_hash and d["block_no"] == b.difficulty
        assert bm.integrity(b.bytes, bc.PM) == (0, 0)
        if b.kind:
            assert bm.signed_message(b.bytes, d) == b.message and len(d["pairs"]) == len(b.txs)
    assert (64 + len(chain[-1].message)) % 128 == 111
    data = b"".join(b.bytes for b in chain)
    res = bm.parse_chunk(data, None, (bc.EPOCH_SLOTS, bc.PM))
    assert (res["outcome"], res["blocks"]) == (bm.OK, 6)
    slots = [int.from_bytes(res["entries"][56 * i + 48:56 * i + 56], "big") for i in range(6)]
    assert slots == [0, 0, 1, 2, 1, bc.EPOCH_SLOTS]                # an EBB's entry carries its epoch
    # a root that is not the body's, signed: UNSUPPORTED for n = 3 at that block, ERR_CORRUPT for n = 1
    for idx, want in ((3, bm.UNSUPPORTED), (2, bm.ERR_CORRUPT)):
        b = chain[idx]
        b.bad_root = True
        bad = b.sign().bytes
        b.bad_root = False
        b.sign()
        assert bm.integrity(bad, bc.PM) == (bm.BLK_BODY_HASH, bm.W_ROOT)
        blobs = [c.bytes for c in chain]
        blobs[idx] = bad
        out = bm.parse_chunk(b"".join(blobs), None, (bc.EPOCH_SLOTS, bc.PM))
        assert (out["outcome"], out["blocks"], out["truncate_at"]) == (want, idx, sum(map(len, blobs[:idx])))
