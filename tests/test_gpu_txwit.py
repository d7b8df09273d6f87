"""GPU: the key-witness check (k_txwit.hip through praos_verify_tx_witnesses /
praos_block_batch_tx_witnesses) against the sequential model (tx_witness_model.py).

Every array of the call -- per block, per transaction, per witness -- equals the model's, bit for
bit: on the reference's golden blocks (whose 9 witnesses verify), on the whole corpus
(txwit_corpus.py) in one call, on the corpus reversed, with slices of 64 and of 100 witnesses,
and over a resident batch before and after its integrity run, whose results and a following
index stay as they were.  Also: capacities one short are PRAOS_E_ARG with the counts needed and
the per-block arrays filled, a call without row arrays fills the per-block arrays, with Byron off
the Byron blocks have no rows, and the empty call."""
import json
import os

import numpy as np
import pytest

import tx_index_model as tm
import tx_witness_model as wm
import txwit_corpus as wc
from praos_hip import abi
from test_tx_index_model import ERAS, stored_block

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def corp():
    cases = wc.corpus()
    arena, off, ln = wc.layout(cases)
    return cases, arena, off, ln, wm.verify_blocks(arena, off, ln, byron=True)


def same_blocks(B, mB):
    assert set(B) == set(wm.BLOCKS)
    for k in wm.BLOCKS:
        assert B[k].tolist() == mB[k], k


def same(got, want):
    B, T, W = got[:3]
    mB, mT, mW = want
    same_blocks(B, mB)
    assert set(T) == set(wm.TXS) and set(W) == set(wm.WITS)
    for k in wm.TXS:
        assert ([bytes(x) for x in T[k]] if k == "tx_id" else T[k].tolist()) == mT[k], k
    for k in wm.WITS:
        assert ([bytes(x) for x in W[k]] if k == "key_hash" else W[k].tolist()) == mW[k], k
    assert got[3] == (len(mT["block"]), len(mW["tx"]))


def test_golden_blocks(ctx):
    with open(os.path.join(HERE, "golden", "tx_golden.json")) as f:
        g = json.load(f)
    blobs = [stored_block(g["eras"][e]["block"]) for e in ERAS]
    blobs += [stored_block(g["byron"]["main"]), stored_block(g["byron"]["ebb"])]
    arena, off, ln = wc.layout([wc.Case("", b, (), None) for b in blobs])
    got = ctx.verify_tx_witnesses(arena, off, ln, byron=True)
    same(got, wm.verify_blocks(arena, off, ln, byron=True))
    B, T, W, _ = got
    assert B["n_wit"].tolist() == [2, 2, 2, 1, 1, 1, 0, 0] and B["n_bad"].tolist() == [0] * 8
    assert W["ok"].tolist() == [1] * 9 and T["status"].tolist() == [0] * 6 + [abi.TXW_SKIPPED]
    for k, e in enumerate(ERAS):
        assert bytes(T["tx_id"][k]) == bytes.fromhex(g["eras"][e]["gen_tx_id"])[4:]


def test_whole_corpus(ctx, corp):
    _, arena, off, ln, want = corp
    same(ctx.verify_tx_witnesses(arena, off, ln, byron=True), want)
    assert wm.SHAPE in want[1]["status"] and 0 in want[2]["ok"] and len(want[2]["tx"]) > 1000


def test_corpus_reversed(ctx, corp):
    _, arena, off, ln, _ = corp
    off, ln = off[::-1], ln[::-1]
    same(ctx.verify_tx_witnesses(arena, off, ln, byron=True), wm.verify_blocks(arena, off, ln, byron=True))


@pytest.mark.parametrize("lanes", (64, 100))
def test_slices_do_not_change_the_outputs(ctx, corp, lanes):
    _, arena, off, ln, want = corp
    same(ctx.verify_tx_witnesses(arena, off, ln, byron=True, max_lanes=lanes), want)


def test_resident_batch_around_the_integrity_run(ctx, corp):
    _, arena, off, ln, want = corp
    n = len(off)
    b = ctx.upload_blocks(arena, off, ln)
    try:
        same(ctx.tx_witnesses_blocks(b, n, byron=True), want)           # before the integrity run
        ctx.run_blocks(b, 129600)
        res0, hash0 = ctx.download_blocks(b, n)
        idx0 = ctx.tx_index_blocks(b, n, byron=True)
        same(ctx.tx_witnesses_blocks(b, n, byron=True), want)           # after it
        res1, hash1 = ctx.download_blocks(b, n)
        assert res0.tolist() == res1.tolist() and hash0.tobytes() == hash1.tobytes()
        idx1 = ctx.tx_index_blocks(b, n, byron=True)
        for d0, d1 in zip(idx0, idx1):
            assert set(d0) == set(d1) and all(d0[k].tobytes() == d1[k].tobytes() for k in d0)
        mst, mrw = tm.index_blocks(arena, off, ln, byron=True)
        assert idx1[0]["n_tx"].tolist() == mst["n_tx"] and idx1[1]["wit_off"].tolist() == mrw["wit_off"]
        ctx.run_blocks(b, 129600)
        res2, hash2 = ctx.download_blocks(b, n)
        assert res0.tolist() == res2.tolist() and hash0.tobytes() == hash2.tobytes()
    finally:
        ctx.free(b)


def test_caps_one_short(ctx, corp):
    _, arena, off, ln, want = corp
    nt, nw = len(want[1]["block"]), len(want[2]["tx"])
    for cap in ((nt, nw - 1), (nt - 1, nw)):
        with pytest.raises(abi.PraosError) as e:
            ctx.verify_tx_witnesses(arena, off, ln, byron=True, cap=cap)
        assert "rc=-2" in str(e.value) and e.value.needed == (nt, nw)
        same_blocks(e.value.blocks, want[0])
    same(ctx.verify_tx_witnesses(arena, off, ln, byron=True, cap=(nt, nw)), want)


def test_no_row_arrays_still_fills_the_blocks(ctx, corp):
    _, arena, off, ln, want = corp
    B, T, W, counts = ctx.verify_tx_witnesses(arena, off, ln, byron=True, rows=False)
    assert T == {} and W == {} and counts == (len(want[1]["block"]), len(want[2]["tx"]))
    same_blocks(B, want[0])


def test_byron_off(ctx, corp):
    cases, arena, off, ln, _ = corp
    got = ctx.verify_tx_witnesses(arena, off, ln, byron=False)
    same(got, wm.verify_blocks(arena, off, ln, byron=False))
    byr = [i for i, c in enumerate(cases) if "byron" in c.tags]
    assert len(byr) == 3 and all(got[0]["status"][i] == abi.TXI_DECODE and got[0]["n_tx"][i] == 0 for i in byr)
    assert abi.TXW_SKIPPED not in got[1]["status"].tolist()


def test_the_empty_call_and_blocks_without_transactions(ctx):
    B, T, W, counts = ctx.verify_tx_witnesses(np.zeros(16, np.uint8), [], [])
    assert counts == (0, 0) and B["tx_first"].tolist() == [0] and T["wit_first"].tolist() == [0]
    assert len(T["block"]) == 0 and len(W["tx"]) == 0
    # blocks that hold no transaction at all, and transactions that hold no witness
    cases = [c for c in wc.corpus() if c.name in ("byron_ebb", "txi_decode", "txi_shape")]
    arena, off, ln = wc.layout(cases)
    same(ctx.verify_tx_witnesses(arena, off, ln, byron=True), wm.verify_blocks(arena, off, ln, byron=True))
    cases = [c for c in wc.corpus() if c.name == "byron_main_3"]
    arena, off, ln = wc.layout(cases)
    same(ctx.verify_tx_witnesses(arena, off, ln, byron=True), wm.verify_blocks(arena, off, ln, byron=True))
