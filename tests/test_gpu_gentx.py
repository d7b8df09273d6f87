"""GPU: wire transactions (k_gentx.hip and k_txwit.hip's passes through praos_verify_gen_txs)
against the sequential model (gentx_model.py).

Every array of the call -- per item, per distinct transaction, per witness -- equals the model's,
bit for bit: on the reference's six golden GenTxs, on the whole corpus (gentx_corpus.py) in one
call, on the corpus reversed (rows follow first appearance, so the hash set's representatives must
not depend on the order the lanes arrive in), on its first 0, 1, 63, 64, 65 and 257 items, with
slices of 64 and of 100 witnesses, and without dedup.  Capacities one short are PRAOS_E_ARG with
the counts needed and the per-item arrays filled; a call without row arrays fills the per-item
arrays.  The distinct transactions agree with praos_index_block_txs / praos_verify_tx_witnesses
over the blocks they were taken from, and K copies of the corpus have the rows of one."""
import numpy as np
import pytest

import gentx_corpus as gc
import gentx_model as gm
import txwit_corpus as wc
from praos_hip import abi
from test_gentx_model import SIZE, golden_items, layout
from test_tx_index_model import ERAS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corp():
    items = gc.corpus()
    arena, off, ln = gc.layout(items)
    return items, arena, off, ln, gm.verify(arena, off.tolist(), ln.tolist())


def same_items(I, mI):
    assert set(I) == set(gm.ITEMS)
    for k in gm.ITEMS:
        assert I[k].tolist() == mI[k], k


def same(got, want):
    I, T, W = got[:3]
    mI, mT, mW = want
    same_items(I, mI)
    assert set(T) == set(gm.TXS) and set(W) == set(gm.WITS)
    for k in gm.TXS:
        assert ([bytes(x) for x in T[k]] if k == "tx_id" else T[k].tolist()) == mT[k], k
    for k in gm.WITS:
        assert ([bytes(x) for x in W[k]] if k == "key_hash" else W[k].tolist()) == mW[k], k
    assert got[3] == (len(mT["item"]), len(mW["tx"]))


def test_golden_gen_txs(ctx):
    items, g = golden_items()
    items.append(bytes.fromhex(g["byron"]["gen_tx"]))
    arena, off, ln = layout(items)
    got = ctx.verify_gen_txs(arena, off, ln)
    same(got, gm.verify(arena, off, ln))
    I, T, W, _ = got
    assert I["status"].tolist() == [0] * 6 + [abi.GTX_BYRON] and I["payload_len"][6] == 236
    assert T["size"].tolist() == [SIZE[e] for e in ERAS] and W["ok"].tolist() == [1] * 9
    assert T["ex_mem"].tolist() == [0, 0, 0, 5000, 5000, 5000] == T["ex_steps"].tolist()
    for k, e in enumerate(ERAS):
        assert bytes(T["tx_id"][k]) == bytes.fromhex(g["eras"][e]["gen_tx_id"])[4:]


def test_whole_corpus(ctx, corp):
    _, arena, off, ln, want = corp
    same(ctx.verify_gen_txs(arena, off, ln), want)
    assert len(want[2]["tx"]) > 1000 and 0 in want[2]["ok"] and set(want[0]["status"]) == set(range(7))


def test_corpus_reversed(ctx, corp):
    _, arena, off, ln, _ = corp
    off, ln = off[::-1].copy(), ln[::-1].copy()
    same(ctx.verify_gen_txs(arena, off, ln), gm.verify(arena, off.tolist(), ln.tolist()))


@pytest.mark.parametrize("n", gc.COUNTS)
def test_item_counts_at_the_wave_and_workgroup_edges(ctx, corp, n):
    _, arena, off, ln, _ = corp
    same(ctx.verify_gen_txs(arena, off[:n], ln[:n]), gm.verify(arena, off[:n].tolist(), ln[:n].tolist()))


@pytest.mark.parametrize("lanes", (64, 100))
def test_slices_do_not_change_the_outputs(ctx, corp, lanes):
    _, arena, off, ln, want = corp
    same(ctx.verify_gen_txs(arena, off, ln, max_lanes=lanes), want)


def test_dedup_off(ctx, corp):
    items, arena, off, ln, _ = corp
    got = ctx.verify_gen_txs(arena, off, ln, dedup=False)
    same(got, gm.verify(arena, off.tolist(), ln.tolist(), dedup=False))
    assert got[3][0] == sum(s == 0 for s in got[0]["status"].tolist())


def test_caps_one_short(ctx, corp):
    _, arena, off, ln, want = corp
    nt, nw = len(want[1]["item"]), len(want[2]["tx"])
    for cap in ((nt, nw - 1), (nt - 1, nw)):
        with pytest.raises(abi.PraosError) as e:
            ctx.verify_gen_txs(arena, off, ln, cap=cap)
        assert "rc=-2" in str(e.value) and e.value.needed == (nt, nw)
        same_items(e.value.items, want[0])
    same(ctx.verify_gen_txs(arena, off, ln, cap=(nt, nw)), want)


def test_no_row_arrays_still_fills_the_items(ctx, corp):
    _, arena, off, ln, want = corp
    I, T, W, counts = ctx.verify_gen_txs(arena, off, ln, rows=False)
    assert T == {} and W == {} and counts == (len(want[1]["item"]), len(want[2]["tx"]))
    same_items(I, want[0])


def test_the_callers_buffers_are_written_again_in_place(ctx, corp):
    items, arena, off, ln, want = corp
    nt, nw = len(want[1]["item"]), len(want[2]["tx"])
    buf = ctx.gen_tx_buffers(len(items), nt + 3, nw + 5)
    ctx.verify_gen_txs(arena, off[::-1].copy(), ln[::-1].copy(), out=buf)     # what a call before left behind
    got = ctx.verify_gen_txs(arena, off, ln, out=buf)
    same(got, want)
    assert got[1]["tx_id"].base is buf[1]["tx_id"] and got[0]["row"] is buf[0]["row"]
    buf0 = ctx.gen_tx_buffers(len(items), 0, 0, rows=False)
    I, T, W, counts = ctx.verify_gen_txs(arena, off, ln, rows=False, out=buf0)
    assert T == {} and W == {} and counts == (nt, nw)
    same_items(I, want[0])


def test_the_empty_call(ctx):
    I, T, W, counts = ctx.verify_gen_txs(np.zeros(16, np.uint8), [], [])
    assert counts == (0, 0) and T["wit_first"].tolist() == [0] and len(I["status"]) == 0
    assert len(T["item"]) == 0 and len(W["tx"]) == 0
    # items none of which has a row
    items = [it for it in gc.corpus() if it.want is None]
    arena, off, ln = gc.layout(items)
    got = ctx.verify_gen_txs(arena, off, ln)
    same(got, gm.verify(arena, off.tolist(), ln.tolist()))
    assert got[3] == (0, 0)


def test_the_transactions_agree_with_the_blocks_they_came_from(ctx):
    blocks = gc.source_blocks()
    items = gc.from_blocks()
    arena, off, ln = gc.layout(items)
    I, T, W, (nt, nw) = ctx.verify_gen_txs(arena, off, ln, dedup=False)
    barena, boff, bln = wc.layout(blocks)
    _, R = ctx.index_block_txs(barena, boff, bln)
    B, bT, bW, (bnt, bnw) = ctx.verify_tx_witnesses(barena, boff, bln)
    assert nt == bnt == len(items) and nw == bnw and I["row"].tolist() == list(range(nt))
    assert T["tx_id"].tobytes() == bT["tx_id"].tobytes() == R["tx_id"].tobytes()
    for k in ("size", "aux_len", "ex_steps", "is_valid", "body_len", "wit_len"):
        assert T[k].tolist() == R[k].tolist(), k
    assert T["wstatus"].tolist() == bT["status"].tolist()
    for k in ("n_vkey", "n_boot", "n_bad", "wit_first"):
        assert T[k].tolist() == bT[k].tolist(), k
    for k in ("tx", "kind", "ok"):
        assert W[k].tolist() == bW[k].tolist(), k
    assert W["key_hash"].tobytes() == bW["key_hash"].tobytes()
    assert T["in_block_size"].tolist() == [s + 4 for s in R["size"].tolist()]


def test_k_copies_have_the_rows_of_one(ctx, corp):
    items, arena, off, ln, want = corp
    K, n = 3, len(items)
    got = ctx.verify_gen_txs(arena, np.tile(off, K), np.tile(ln, K))
    I, T, W, _ = got
    for k in ("item",) + gm.TXS[1:]:
        assert ([bytes(x) for x in T[k]] if k == "tx_id" else T[k].tolist()) == want[1][k], k
    for k in gm.WITS:
        assert ([bytes(x) for x in W[k]] if k == "key_hash" else W[k].tolist()) == want[2][k], k
    assert I["row"].tolist() == want[0]["row"] * K and I["status"].tolist() == want[0]["status"] * K
