"""GPU: praos_hip.txsubmission.verify_inbound -- three peers offer overlapping lists of wire
transactions, two of them with a planted bad witness; every distinct transaction is verified
once and every peer gets its own items' results."""
import pytest

import gentx_corpus as gc
import txwit_corpus as wc
from praos_hip import abi, txsubmission as ts, wire


def test_wrap_gen_tx_is_the_wire_form():
    g = wc.Gen(7)
    body, wits, _ = g.tx(1, 0, four=True)
    for era in (1, 5, 24):
        inner = gc.tx_bytes(era, body, wits)
        assert ts.wrap_gen_tx(era, inner) == gc.wrap(era, inner)
    assert ts.wrap_gen_tx(0, b"\x82\x00\x41\x00") == b"\x82\x00\x82\x00\x41\x00"


@pytest.mark.gpu
def test_three_peers_with_overlapping_lists(ctx):
    g = wc.Gen(20251018)
    txs = []
    for k in range(12):
        dmg = {1: "S"} if k == 4 else ({0: "other_tx"} if k == 9 else {})
        era = 1 + k % 6
        body, wits, want = g.tx(2, k % 2, four=era >= 4, damage=dmg)
        txs.append((ts.wrap_gen_tx(era, gc.tx_bytes(era, body, wits)), all(want)))
    junk = b"\x82\x05\xd7\x41\x00"
    byron = ts.wrap_gen_tx(0, b"\x82\x01\x43abc")
    pick = [[0, 1, 2, 3, 4, 5, 6, 7], [4, 5, 6, 7, 8, 9, 10, 11, 0], [11, 9, 4, 2]]
    peers = [[txs[k][0] for k in p] for p in pick]
    peers[0].append(junk)
    peers[2].insert(1, byron)
    res, distinct = ts.verify_inbound(ctx, peers)
    assert distinct == 12 and [len(r) for r in res] == [len(p) for p in peers]
    assert res[0][-1].status == wire.WIRE_SYNTAX
    assert res[0][-1].tx_id is None and res[0][-1].witnesses_ok is None
    assert res[2][1].status == abi.GTX_BYRON and res[2][1].tx_id is None
    del res[0][-1], res[2][1]
    seen = {}
    for p, r in zip(pick, res):
        for k, t in zip(p, r):
            assert t.status == 0 and t.witnesses_ok == txs[k][1], k
            assert seen.setdefault(k, t) == t           # the same transaction, the same answer for every peer
            assert t.ex_mem == 0 and t.ex_steps == 0 and t.in_block_size > 4
    assert sorted(k for k, t in seen.items() if not t.witnesses_ok) == [4, 9]
    assert len({t.tx_id for t in seen.values()}) == 12
