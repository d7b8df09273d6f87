"""GPU: wire blocks (k_blockfetch.hip with the stored-block kernels through
praos_verify_fetched_blocks) against the sequential model (blockfetch_model.py).

Every array of the call -- per item, per range, per distinct block, and the witness call's per
block, per transaction and per witness -- equals the model's, bit for bit: on the reference's
eight golden wire blocks, on the whole corpus (blockfetch_corpus.py) in one call, with its ranges
reversed (rows follow first appearance, so the representatives must not depend on the order the
lanes arrive in), on its first 0, 1, 63, 64, 65 and 257 items, with slices of 64 and of 100
witnesses, without dedup, without witnesses and with Byron off.  Capacities one short are
PRAOS_E_ARG with the counts needed and the per-item and per-range arrays filled; a call without
row arrays fills them too.  Three copies of the corpus in three ranges have the rows of one (and
one more for each deviant of the later copies, which has a row of its own every time); the
rows' body check is praos_verify_block_integrity's and their transactions and witnesses are
praos_verify_tx_witnesses' over the same inner bytes."""
import numpy as np
import pytest

import blockfetch_corpus as fc
import blockfetch_model as fm
import tx_witness_model as wm
from praos_hip import abi
from test_blockfetch_model import EPOCH_SLOTS, golden_items

pytestmark = pytest.mark.gpu
ES = fc.EPOCH_SLOTS
HASHES = ("header_hash", "prev_hash", "body_hash", "tx_id", "key_hash")


@pytest.fixture(scope="module")
def corp():
    L = fc.layout(fc.corpus())
    return L, fm.verify(*L[:7], byron_epoch_slots=ES)


def call(ctx, L, **kw):
    arena, off, ln, ifirst, efirst, es, eh = L[:7]
    eh = np.frombuffer(b"".join(eh), np.uint8).reshape(-1, 32)
    kw.setdefault("byron_epoch_slots", ES)
    return ctx.verify_fetched_blocks(np.frombuffer(arena, np.uint8), off, ln, ifirst, efirst, es, eh, **kw)


def lists(d, names):
    assert set(d) == set(names)
    return {k: ([bytes(x) for x in d[k]] if k in HASHES else d[k].tolist()) for k in names}


def same_items(I, G, want):
    assert lists(I, fm.ITEMS) == want[0]
    assert lists(G, fm.RANGES) == want[1]


def same(got, want, witnesses=True):
    I, G, R, B, T, W, counts = got
    same_items(I, G, want)
    assert lists(R, fm.ROWS) == want[2]
    if not witnesses:
        assert B == {} and T == {} and W == {} and counts == (len(want[2]["item"]), 0, 0)
        return
    assert lists(B, wm.BLOCKS) == want[3]
    assert lists(T, wm.TXS) == want[4]
    assert lists(W, wm.WITS) == want[5]
    assert counts == (len(want[2]["item"]), len(want[4]["block"]), len(want[5]["tx"]))


def golden_layout():
    items = [raw for _, _, raw in golden_items()]
    off = np.cumsum([0] + [len(x) for x in items[:-1]]).tolist()
    arena = b"".join(items)
    ln = [len(x) for x in items]
    heads = [fm.header_of(arena, *fm.unwrap(arena, o, n)[1:], EPOCH_SLOTS) for o, n in zip(off, ln)]
    return arena, off, ln, [0, 8], [0, 8], [h["slot"] for h in heads], [h["header_hash"] for h in heads]


def test_golden_wire_blocks(ctx):
    L = golden_layout()
    got = call(ctx, L, byron_epoch_slots=EPOCH_SLOTS)
    same(got, fm.verify(*L, byron_epoch_slots=EPOCH_SLOTS))
    I, G, R, B, T, W, _ = got
    assert I["verdict"].tolist() == [0] * 8 and I["tag"].tolist() == list(range(8)) and G["status"].tolist() == [0]
    assert R["bits"].tolist() == [0] * 8 and B["n_wit"].tolist() == [0, 0, 2, 2, 2, 1, 1, 1] and W["ok"].tolist() == [1] * 9


def test_whole_corpus(ctx, corp):
    L, want = corp
    same(call(ctx, L), want)
    assert set(want[0]["verdict"]) == {0, 1, 2, 3, 4, 5, 6, 255} and set(want[1]["status"]) == {0, 1, 2}
    assert len(want[5]["tx"]) > 1000 and 0 in want[5]["ok"] and len(want[2]["item"]) < sum(q != fm.NO_ROW for q in want[0]["row"])


def test_ranges_reversed(ctx):
    L = fc.layout(fc.corpus(), reverse=True)
    same(call(ctx, L), fm.verify(*L[:7], byron_epoch_slots=ES))


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 257))
def test_item_counts_at_the_wave_and_workgroup_edges(ctx, n):
    L = fc.layout(fc.corpus(), first=n)
    assert len(L[1]) == n
    same(call(ctx, L), fm.verify(*L[:7], byron_epoch_slots=ES))


@pytest.mark.parametrize("lanes", (64, 100))
def test_slices_do_not_change_the_outputs(ctx, corp, lanes):
    L, want = corp
    same(call(ctx, L, max_lanes=lanes), want)


def test_dedup_off(ctx, corp):
    L, _ = corp
    got = call(ctx, L, dedup=False)
    same(got, fm.verify(*L[:7], byron_epoch_slots=ES, dedup=False))
    assert got[6][0] == sum(q != abi.BF_NO_ROW for q in got[0]["row"].tolist())


def test_dedup_on_is_dedup_off_mapped_through_row(ctx, corp):
    L, _ = corp
    I, G, R, B, *_ = call(ctx, L)
    I0, G0, R0, B0, *_ = call(ctx, L, dedup=False)
    assert I["verdict"].tolist() == I0["verdict"].tolist() and lists(G, fm.RANGES) == lists(G0, fm.RANGES)
    for i, (q, q0) in enumerate(zip(I["row"].tolist(), I0["row"].tolist())):
        assert (q == abi.BF_NO_ROW) == (q0 == abi.BF_NO_ROW)
        if q != abi.BF_NO_ROW:
            for k in ("tag", "slot", "block_no", "header_hash", "body_hash", "bits", "which", "blk_len"):
                assert np.array_equal(R[k][q], R0[k][q0]), (i, k)
            for k in ("n_tx", "n_wit", "n_bad", "n_shape"):
                assert B[k][q] == B0[k][q0], (i, k)


def test_without_witnesses(ctx, corp):
    L, want = corp
    same(call(ctx, L, witnesses=False), want, witnesses=False)


def test_byron_off(ctx, corp):
    L, _ = corp
    got = call(ctx, L, byron_epoch_slots=0)
    same(got, fm.verify(*L[:7], byron_epoch_slots=0))
    items = L[7]
    assert got[0]["verdict"].tolist() == [it.verdict_off for it in items] and abi.BF_UNSUPPORTED in got[0]["verdict"]


def test_caps_one_short(ctx, corp):
    L, want = corp
    nr, nt, nw = len(want[2]["item"]), len(want[4]["block"]), len(want[5]["tx"])
    for cap in ((nr - 1, nt, nw), (nr, nt - 1, nw), (nr, nt, nw - 1)):
        with pytest.raises(abi.PraosError) as e:
            call(ctx, L, cap=cap)
        assert "rc=-2" in str(e.value) and e.value.needed == (nr, nt, nw)
        same_items(e.value.items, e.value.ranges, want)
    same(call(ctx, L, cap=(nr, nt, nw)), want)
    # the per-row witness counts have no cap of their own: they hold rows->cap entries, and a call
    # whose rows do not fit leaves them alone -- guard elements behind them stay as they were
    buf = ctx.fetched_block_buffers(len(L[1]), len(L[3]) - 1, nr - 1, nt, nw)
    big = {k: np.full(len(a) + 64, 0xA5, a.dtype) for k, a in buf[3].items()}
    for k in big:
        buf[3][k] = big[k][:len(buf[3][k])]
    with pytest.raises(abi.PraosError) as e:
        call(ctx, L, out=buf)
    assert e.value.needed == (nr, nt, nw)
    for k, a in big.items():
        assert (a == 0xA5).all(), k
    # with room for the rows they are written, and nothing behind rows->cap (+ 1 for tx_first) is
    buf = ctx.fetched_block_buffers(len(L[1]), len(L[3]) - 1, nr, nt, nw)
    big = {k: np.full(len(a) + 64, 0xA5, a.dtype) for k, a in buf[3].items()}
    for k in big:
        buf[3][k] = big[k][:len(buf[3][k])]
    same(call(ctx, L, out=buf), want)
    for k, a in big.items():
        assert (a[nr + (k == "tx_first"):] == a[-1]).all() and a[-1] != 0, k


def test_no_row_arrays_still_fills_the_items(ctx, corp):
    L, want = corp
    I, G, R, B, T, W, counts = call(ctx, L, rows=False)
    assert R == {} and T == {} and W == {} and counts == (len(want[2]["item"]), len(want[4]["block"]), len(want[5]["tx"]))
    same_items(I, G, want)


def test_the_callers_buffers_are_written_again_in_place(ctx, corp):
    L, want = corp
    nr, nt, nw = len(want[2]["item"]), len(want[4]["block"]), len(want[5]["tx"])
    Lr = fc.layout(fc.corpus(), reverse=True)
    assert len(Lr[1]) == len(L[1]) and len(Lr[3]) == len(L[3])
    rr, rt, rw = call(ctx, Lr, rows=False)[6]                # (the deviants' rows depend on who comes first)
    buf = ctx.fetched_block_buffers(len(L[1]), len(L[3]) - 1, max(nr, rr) + 3, max(nt, rt) + 4, max(nw, rw) + 5)
    call(ctx, Lr, out=buf)                                   # what a call before left behind
    got = call(ctx, L, out=buf)
    same(got, want)
    assert got[2]["header_hash"].base is buf[2]["header_hash"] and got[0]["row"] is buf[0]["row"]


def test_the_empty_call(ctx):
    z = np.zeros((0, 32), np.uint8)
    I, G, R, B, T, W, counts = ctx.verify_fetched_blocks(np.zeros(16, np.uint8), [], [], [0], [0], [], z)
    assert counts == (0, 0, 0) and len(I["verdict"]) == 0 and len(G["status"]) == 0 and len(R["item"]) == 0
    assert T["wit_first"].tolist() == [0] and B["tx_first"].tolist() == [0]
    # ranges that expect points and hold nothing
    I, G, *_ = ctx.verify_fetched_blocks(np.zeros(16, np.uint8), [], [], [0, 0, 0], [0, 0, 2], [5, 6],
                                         np.zeros((2, 32), np.uint8))
    assert G["status"].tolist() == [abi.BF_RANGE_COMPLETE, abi.BF_RANGE_TOO_FEW] and G["stop"].tolist() == [0, 0]
    # items none of which has a row
    g = [x for x in fc.corpus() if x.name.startswith("fault_") and x.name != "fault_range"]
    L = fc.layout(g)
    got = call(ctx, L)
    same(got, fm.verify(*L[:7], byron_epoch_slots=ES))
    assert got[6] == (0, 0, 0) and set(got[0]["verdict"].tolist()) == {abi.BF_WIRE}


def is_deviant(it):
    """an item under another item's header and length with other bytes: the planted deviants and the
    blocks with a byte of one segment changed"""
    return any(t == "deviant" or t.startswith("flip_s") for t in it.tags)


def three_copies(L, want):
    """K copies of a layout, each copy one range that asks every item for its own point"""
    arena, off, ln = L[:3]
    heads = list(zip(want[2]["slot"], want[2]["header_hash"]))
    pts = [heads[q] if q != fm.NO_ROW else fc.NOWHERE for q in want[0]["row"]]
    n, K = len(off), 3
    return (arena, off * K, ln * K, [k * n for k in range(K + 1)], [k * n for k in range(K + 1)],
            [s for s, _ in pts] * K, [h for _, h in pts] * K), K


def test_three_copies_in_three_ranges_have_the_rows_of_one(ctx, corp):
    # without the deviants: exactly the rows of one copy
    L = fc.layout([g for g in fc.corpus() if not any(is_deviant(it) for it in g.items)])
    want = fm.verify(*L[:7], byron_epoch_slots=ES)
    L3, K = three_copies(L, want)
    got = call(ctx, L3)
    I, G, R, B, T, W, _ = got
    assert lists(R, fm.ROWS) == want[2] and lists(B, wm.BLOCKS) == want[3]
    assert lists(T, wm.TXS) == want[4] and lists(W, wm.WITS) == want[5]
    assert I["row"].tolist() == want[0]["row"] * K and I["status"].tolist() == want[0]["status"] * K
    same(got, fm.verify(*L3, byron_epoch_slots=ES))
    # the whole corpus: the rows of one copy, then one more for every deviant of the later copies
    # (a deviant has a row of its own every time it comes: deviants are not classed among themselves)
    L, want = corp
    L3, K = three_copies(L, want)
    got = call(ctx, L3)
    same(got, fm.verify(*L3, byron_epoch_slots=ES))
    R, n, nr = got[2], len(L[1]), len(want[2]["item"])
    assert {k: v[:nr] for k, v in lists(R, fm.ROWS).items()} == want[2]
    extra = R["item"][nr:].tolist()
    assert len(extra) == (K - 1) * 7 and all(is_deviant(L[7][i % n]) and i >= n for i in extra)


def test_the_rows_agree_with_the_stored_block_calls(ctx, corp):
    L, want = corp
    arena = np.frombuffer(L[0], np.uint8)
    I, G, R, B, T, W, (nr, nt, nw) = call(ctx, L)
    off, ln = R["blk_off"], R["blk_len"]
    sh = R["tag"] >= 2
    res, bh = ctx.verify_block_integrity(arena, off[sh], ln[sh], 129600)
    assert ((res & abi.BLK_BODY_HASH) == R["bits"][sh]).all() and not (res & abi.BLK_DECODE).any()
    assert bh.tobytes() == R["body_hash"][sh].tobytes()
    res, which = ctx.verify_byron_integrity(arena, off[~sh], ln[~sh], ES, 764824073)
    assert ((res & abi.BLK_BODY_HASH) == R["bits"][~sh]).all() and which.tolist() == R["which"][~sh].tolist()
    bB, bT, bW, counts = ctx.verify_tx_witnesses(arena, off, ln, byron=True)
    assert counts == (nt, nw)
    for k in wm.BLOCKS:
        assert B[k].tolist() == bB[k].tolist(), k
    for k in wm.TXS:
        assert T[k].tobytes() == bT[k].tobytes(), k
    for k in wm.WITS:
        assert W[k].tobytes() == bW[k].tobytes(), k
