"""GPU: praos_hip.blockfetch.verify_fetched -- three peers answer overlapping requests for the
same chain of blocks; one sends a block whose body was changed, one a block that was not asked
for, one stops early, and two blocks carry a planted bad witness.  Every distinct block is checked
once and every request gets its own blocks' results."""
import random

import pytest

import block_corpus as bc
import blockfetch_corpus as fc
import tx_corpus as tc
import txwit_corpus as wc
from praos_hip import abi, blockfetch as bf


def test_wrap_block_is_the_wire_form():
    for n in (3, 23, 24, 255, 256, 70000):
        blk = b"\x82\x06" + bytes(n - 2)
        w = bf.wrap_block(blk)
        assert w == fc.wrap(blk) and bf.unwrap_block(w) == (bf.WIRE_OK, 6, len(w) - n, n)
    assert bf.unwrap_block(b"\xd8\x18\x43\x82\x08\x80")[:2] == (bf.WIRE_ERA, 8)
    assert bf.unwrap_block(b"\xd8\x17\x43\x82\x06\x80")[0] == bf.WIRE_SYNTAX
    assert bf.unwrap_block(b"\xd8\x18\x43\x82\x06\x80\x00")[0] == bf.WIRE_TRAILING


@pytest.mark.gpu
def test_three_peers_with_overlapping_requests(ctx):
    r = random.Random(20251021)
    g = wc.Gen(20251021)
    chain = []
    for k in range(10):
        dmg = {1: "S"} if k == 3 else ({0: "other_tx"} if k == 7 else {})
        era = 2 + k % 6
        txs = [g.tx(2, k % 2, four=era >= 5, damage=dmg if j == 0 else {}) for j in range(1 + k % 3)]
        stored = tc.block(r, era, [t[0] for t in txs], [t[1] for t in txs])
        b = fc.reheader(r, wc.Case(f"b{k}", stored, (), None))
        n_wit = sum(len(t[2]) for t in txs)
        chain.append((b, len(txs), n_wit, sum(1 for t in txs for ok in t[2] if not ok)))
    pts = [b.point for b, *_ in chain]
    wire = [bf.wrap_block(b.bytes) for b, *_ in chain]
    changed = bf.wrap_block(fc.flip_in_segment(chain[5][0].bytes, 2))
    stranger = bf.wrap_block(bc.make_block(r, fc.SPKP)[0])
    peers = [
        [(pts[0:6], wire[0:6]), (pts[6:10], wire[6:10])],                      # everything, as asked
        [(pts[2:8], wire[2:5] + [changed] + wire[6:8])],                       # block 5 with another body
        [(pts[0:4], wire[0:2] + [stranger, wire[3]]), (pts[4:10], wire[4:7])],  # a block nobody asked for; then too few
    ]
    res, distinct = bf.verify_fetched(ctx, peers)
    assert distinct == 12                                   # the ten, the changed body, the stranger
    (a0, a1), (b0,), (c0, c1) = res
    assert a0.verdicts == [0] * 6 and a0.accepted == 6 and a0.status == abi.BF_RANGE_COMPLETE
    assert a1.verdicts == [0] * 4 and a1.accepted == 4 and a1.status == abi.BF_RANGE_COMPLETE
    assert b0.verdicts == [0, 0, 0, abi.BF_INVALID_BODY, abi.BF_NOT_REACHED, abi.BF_NOT_REACHED]
    assert b0.accepted == 3 and b0.status == abi.BF_RANGE_FAILED
    assert c0.verdicts == [0, 0, abi.BF_WRONG_BLOCK, abi.BF_NOT_REACHED] and c0.accepted == 2
    assert c0.status == abi.BF_RANGE_FAILED
    assert c1.verdicts == [0, 0, 0] and c1.accepted == 3 and c1.status == abi.BF_RANGE_TOO_FEW
    # the accepted blocks: the chain's, the same answer for every peer, the planted witnesses found
    got = {}
    for first, rq in ((0, a0), (6, a1), (2, b0), (0, c0), (4, c1)):
        assert len(rq.blocks) == rq.accepted
        for j, blk in enumerate(rq.blocks):
            k = first + j
            b, n_tx, n_wit, n_bad = chain[k]
            assert (blk.slot, blk.hash) == b.point and (blk.n_tx, blk.n_wit, blk.n_bad, blk.n_shape) == (n_tx, n_wit, n_bad, 0)
            assert got.setdefault(k, blk) == blk
    assert sorted(got) == list(range(10)) and sorted(k for k, b in got.items() if b.n_bad) == [3, 7]
    # without the witness pass the blocks carry their points only
    res, distinct = bf.verify_fetched(ctx, peers, witnesses=False)
    first = res[0][0].blocks[0]
    assert distinct == 12 and (first.slot, first.hash) == pts[0] and first.n_tx is None and first.n_bad is None
