"""CPU: the transaction-index model (tx_index_model.py) pinned to the reference's golden blocks
and transactions (tests/golden/tx_golden.json, written by tests/golden/make_tx_golden.py).

Each Shelley-based golden block holds the one transaction of its era's GenTx file: the model
gives one row with one output, tx_id = the hash in GenTxId_<era> (txId = Blake2b-256 of the
stored body bytes), and size = the length of GenTx_<era>'s payload for Shelley, Allegra and Mary,
that length - 1 for Alonzo, Babbage and Conway, whose payload carries the isValid byte that the
ledger's sizeTxF leaves out.  The Byron main block has one transaction of size 236 (the length
of the [tx, witnesses] item of GenTx_Byron) with one output; the EBB has none."""
import json
import os

import pytest

import tx_index_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))
ERAS = ("Shelley", "Allegra", "Mary", "Alonzo", "Babbage", "Conway")
PAYLOAD = {"Shelley": 680, "Allegra": 792, "Mary": 887, "Alonzo": 865, "Babbage": 968, "Conway": 890}


def golden():
    with open(os.path.join(HERE, "golden", "tx_golden.json")) as f:
        return json.load(f)


def unwrap24(b):
    """the content of a tag-24 byte string"""
    assert b[:2] == b"\xd8\x18"
    mt, _, n, p = tm.head(b, 2, len(b))
    assert mt == 2 and p + n == len(b)
    return b[p:]


def stored_block(hexed):
    return unwrap24(bytes.fromhex(hexed))


@pytest.mark.parametrize("era", ERAS)
def test_golden_block_of_each_era(era):
    g = golden()["eras"][era]
    blk = stored_block(g["block"])
    gen_tx = bytes.fromhex(g["gen_tx"])
    assert gen_tx[0] == 0x82 and gen_tx[1] == ERAS.index(era) + 1
    payload = unwrap24(gen_tx[2:])
    assert len(payload) == PAYLOAD[era]
    gen_id = bytes.fromhex(g["gen_tx_id"])
    assert gen_id[:4] == bytes([0x82, ERAS.index(era) + 1, 0x58, 0x20]) and len(gen_id) == 36
    st, rw = tm.index_blocks(blk, [0], [len(blk)])
    assert st["status"] == [tm.OK] and st["n_tx"] == [1] and st["tx_first"] == [0, 1]
    assert rw["n_out"] == [1] and st["n_out"] == [1]
    assert rw["tx_id"] == [gen_id[4:]]
    want = len(payload) - (1 if era in ("Alonzo", "Babbage", "Conway") else 0)
    assert rw["size"] == [want] and st["txs_size"] == [want]
    assert rw["is_valid"] == [1] and rw["block"] == [0]
    # the stored body is the first item of the GenTx payload
    body = blk[rw["body_off"][0]:rw["body_off"][0] + rw["body_len"][0]]
    assert payload[1:1 + len(body)] == body
    if era in ("Shelley", "Allegra", "Mary"):
        assert rw["ex_steps"] == [0]


def test_golden_byron_blocks():
    g = golden()["byron"]
    main, ebb = stored_block(g["main"]), stored_block(g["ebb"])
    gen_tx = bytes.fromhex(g["gen_tx"])
    assert gen_tx[:4] == b"\x82\x00\x82\x00" and len(gen_tx) - 4 == 236
    arena = main + ebb
    st, rw = tm.index_blocks(arena, [0, len(main)], [len(main), len(ebb)], byron=True)
    assert st["status"] == [tm.OK, tm.OK] and st["n_tx"] == [1, 0] and st["tx_first"] == [0, 1, 1]
    assert rw["size"] == [236] and rw["n_out"] == [1] and rw["ex_steps"] == [0] and rw["is_valid"] == [1]
    assert rw["aux_len"] == [0]
    # the block's [tx, witnesses] item is GenTx_Byron's
    s = rw["body_off"][0] - 1
    assert arena[s:s + 236] == gen_tx[4:]
    assert rw["tx_id"] == [tm._tx_id(arena, rw["body_off"][0], rw["body_off"][0] + rw["body_len"][0])]
    # Byron off: both are DECODE, with no rows
    st, rw = tm.index_blocks(arena, [0, len(main)], [len(main), len(ebb)])
    assert st["status"] == [tm.DECODE, tm.DECODE] and st["n_tx"] == [0, 0] and rw["block"] == []
