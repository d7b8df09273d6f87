"""CPU: the key-witness model (tx_witness_model.py) pinned to the reference's golden blocks
(tests/golden/tx_golden.json).

The six Shelley-based golden blocks hold 9 VKey witnesses together: 2 each in Shelley, Allegra
and Mary, 1 each in Alonzo, Babbage and Conway.  Each is a signature by the reference's own
signer over the hash in GenTxId_<era>: the model finds them, marks every one ok over that hash,
and marks every one not ok once a byte of the body is changed.  The Byron main block's row is
SKIPPED."""
import hashlib
import json
import os

import pytest

import tx_witness_model as wm
from test_tx_index_model import ERAS, stored_block

HERE = os.path.dirname(os.path.abspath(__file__))
N_VKEY = {"Shelley": 2, "Allegra": 2, "Mary": 2, "Alonzo": 1, "Babbage": 1, "Conway": 1}


def golden():
    with open(os.path.join(HERE, "golden", "tx_golden.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("era", ERAS)
def test_golden_witnesses_of_each_era(era):
    g = golden()["eras"][era]
    blk = stored_block(g["block"])
    gen_id = bytes.fromhex(g["gen_tx_id"])[4:]
    B, T, W = wm.verify_blocks(blk, [0], [len(blk)])
    k = N_VKEY[era]
    assert B["status"] == [0] and B["n_tx"] == [1] and B["n_wit"] == [k] and B["n_bad"] == [0] and B["n_shape"] == [0]
    assert T["status"] == [wm.OK] and T["n_vkey"] == [k] and T["n_boot"] == [0] and T["n_bad"] == [0]
    assert T["tx_id"] == [gen_id] and T["wit_first"] == [0, k] and T["block"] == [0]
    assert W["tx"] == [0] * k and W["kind"] == [0] * k and W["ok"] == [1] * k
    for ko, so, kh in zip(W["key_off"], W["sig_off"], W["key_hash"]):
        assert so == ko + 34 and blk[ko - 2:ko] == b"\x58\x20" and blk[so - 2:so] == b"\x58\x40"
        assert kh == hashlib.blake2b(blk[ko:ko + 32], digest_size=28).digest()
    # one byte of the body changed: another txId, and none of the signatures is over it
    st, rw = wm.tm.index_blocks(blk, [0], [len(blk)])
    at = rw["body_off"][0] + rw["body_len"][0] - 1
    bad = bytearray(blk)
    bad[at] ^= 1
    B2, T2, W2 = wm.verify_blocks(bytes(bad), [0], [len(bad)])
    assert T2["tx_id"] != [gen_id] and W2["ok"] == [0] * k and B2["n_bad"] == [k] and T2["n_bad"] == [k]
    assert W2["key_off"] == W["key_off"] and W2["key_hash"] == W["key_hash"]


def test_nine_golden_witnesses_in_one_call():
    g = golden()
    blobs = [stored_block(g["eras"][e]["block"]) for e in ERAS]
    off, pos = [], 0
    for b in blobs:
        off.append(pos)
        pos += len(b)
    B, T, W = wm.verify_blocks(b"".join(blobs), off, [len(b) for b in blobs])
    assert B["n_wit"] == [2, 2, 2, 1, 1, 1] and sum(B["n_bad"]) == 0
    assert len(W["ok"]) == 9 and all(W["ok"]) and W["tx"] == [0, 0, 1, 1, 2, 2, 3, 4, 5]
    assert T["wit_first"] == [0, 2, 4, 6, 7, 8, 9]


def test_byron_rows_are_skipped():
    g = golden()["byron"]
    main, ebb = stored_block(g["main"]), stored_block(g["ebb"])
    arena = main + ebb
    B, T, W = wm.verify_blocks(arena, [0, len(main)], [len(main), len(ebb)], byron=True)
    assert B["status"] == [0, 0] and B["n_tx"] == [1, 0] and B["n_wit"] == [0, 0] and B["n_shape"] == [0, 0]
    assert T["status"] == [wm.SKIPPED] and T["n_vkey"] == [0] and T["n_boot"] == [0] and T["wit_first"] == [0, 0]
    assert W["tx"] == []
    # Byron off: no rows at all
    B, T, W = wm.verify_blocks(arena, [0, len(main)], [len(main), len(ebb)])
    assert B["status"] == [1, 1] and T["block"] == [] and T["wit_first"] == [0]
