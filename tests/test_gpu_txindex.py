"""GPU: the transaction index (k_txindex.hip through praos_index_block_txs /
praos_block_batch_tx_index) against the sequential model (tx_index_model.py).

Every array of the call -- the per-block statistics and every row field -- equals the model's,
exactly: on the reference's golden blocks, on the whole corpus (tx_corpus.py) in one call, on
the corpus with the block order reversed (row placement through tx_first), and over a resident batch after its integrity run, whose results stay as they were.  Also: a
row capacity one short is PRAOS_E_ARG with the count needed and the statistics filled, a call
without row arrays still fills the statistics, and with Byron off the Byron items are DECODE."""
import json
import os

import numpy as np
import pytest

import tx_corpus as tc
import tx_index_model as tm
from praos_hip import abi
from test_tx_index_model import ERAS, stored_block

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def corp():
    cases = tc.corpus()
    arena, off, ln = tc.layout(cases)
    return cases, arena, off, ln, tm.index_blocks(arena, off, ln, byron=True)


def same(got, want):
    st, rw = got
    mst, mrw = want
    assert set(st) == set(tm.STATS) and set(rw) == set(tm.ROWS)
    for k in tm.STATS:
        assert st[k].tolist() == mst[k], k
    for k in tm.ROWS:
        if k == "tx_id":
            assert [bytes(x) for x in rw[k]] == mrw[k]
        else:
            assert rw[k].tolist() == mrw[k], k


def test_golden_blocks(ctx):
    with open(os.path.join(HERE, "golden", "tx_golden.json")) as f:
        g = json.load(f)
    blobs = [stored_block(g["eras"][e]["block"]) for e in ERAS]
    blobs += [stored_block(g["byron"]["main"]), stored_block(g["byron"]["ebb"])]
    arena, off, ln = tc.layout([tc.Case("", b, ()) for b in blobs])
    st, rw = ctx.index_block_txs(arena, off, ln, byron=True)
    same((st, rw), tm.index_blocks(arena, off, ln, byron=True))
    assert st["n_tx"].tolist() == [1] * 7 + [0] and st["status"].tolist() == [0] * 8
    for k, e in enumerate(ERAS):
        assert bytes(rw["tx_id"][k]) == bytes.fromhex(g["eras"][e]["gen_tx_id"])[4:]
    assert rw["size"].tolist() == [680, 792, 887, 864, 967, 889, 236]


def test_whole_corpus(ctx, corp):
    _, arena, off, ln, want = corp
    same(ctx.index_block_txs(arena, off, ln, byron=True), want)
    assert tm.SHAPE in want[0]["status"] and tm.DECODE in want[0]["status"] and len(want[1]["block"]) > 1000


def test_corpus_reversed(ctx, corp):
    _, arena, off, ln, _ = corp
    off, ln = off[::-1], ln[::-1]
    same(ctx.index_block_txs(arena, off, ln, byron=True), tm.index_blocks(arena, off, ln, byron=True))


def test_resident_batch_after_the_integrity_run(ctx, corp):
    _, arena, off, ln, want = corp
    b = ctx.upload_blocks(arena, off, ln)
    try:
        ctx.run_blocks(b, 129600)
        res0, hash0 = ctx.download_blocks(b, len(off))
        same(ctx.tx_index_blocks(b, len(off), byron=True), want)
        res1, hash1 = ctx.download_blocks(b, len(off))
        assert res0.tolist() == res1.tolist() and hash0.tobytes() == hash1.tobytes()
        ctx.run_blocks(b, 129600)                # and the run after the index gives the same again
        res2, hash2 = ctx.download_blocks(b, len(off))
        assert res0.tolist() == res2.tolist() and hash0.tobytes() == hash2.tobytes()
        same(ctx.tx_index_blocks(b, len(off), byron=True), want)
    finally:
        ctx.free(b)


def test_cap_one_short(ctx, corp):
    _, arena, off, ln, (mst, mrw) = corp
    need = len(mrw["block"])
    with pytest.raises(abi.PraosError) as e:
        ctx.index_block_txs(arena, off, ln, byron=True, cap=need - 1)
    assert "rc=-2" in str(e.value) and e.value.needed == need
    for k in tm.STATS:
        assert e.value.stats[k].tolist() == mst[k], k
    st, rw = ctx.index_block_txs(arena, off, ln, byron=True, cap=need)
    same((st, rw), (mst, mrw))


def test_no_row_arrays_still_fills_stats(ctx, corp):
    _, arena, off, ln, (mst, mrw) = corp
    st, rw = ctx.index_block_txs(arena, off, ln, byron=True, rows=False, cap=0)
    assert rw == {}
    for k in tm.STATS:
        assert st[k].tolist() == mst[k], k
    # a selection of the row arrays
    st, rw = ctx.index_block_txs(arena, off, ln, byron=True, rows=("tx_id", "n_out"))
    assert set(rw) == {"tx_id", "n_out"} and rw["n_out"].tolist() == mrw["n_out"]
    assert [bytes(x) for x in rw["tx_id"]] == mrw["tx_id"]


def test_byron_off_marks_byron_items_decode(ctx, corp):
    cases, arena, off, ln, _ = corp
    want = tm.index_blocks(arena, off, ln, byron=False)
    got = ctx.index_block_txs(arena, off, ln, byron=False)
    same(got, want)
    byr = [i for i, c in enumerate(cases) if c.name.startswith("byron_")]
    assert len(byr) >= 8 and all(got[0]["status"][i] == abi.TXI_DECODE and got[0]["n_tx"][i] == 0 for i in byr)


def test_spans_outside_the_arena_and_the_empty_call(ctx):
    cases = tc.corpus()[:3]
    arena, off, ln = tc.layout(cases)
    off2, ln2 = off + [len(arena) - 2, len(arena) + 5], ln + [10, 1]
    same(ctx.index_block_txs(arena, off2, ln2), tm.index_blocks(arena, off2, ln2))
    st, rw = ctx.index_block_txs(arena, [], [])
    assert st["tx_first"].tolist() == [0] and len(rw["block"]) == 0
