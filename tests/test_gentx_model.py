"""CPU: the wire-transaction model (gentx_model.py) pinned to the reference's golden GenTx files
(tests/golden/tx_golden.json: GenTx_<era>, GenTxId_<era>, GenTx_Byron).

Each Shelley-based GenTx is [era index, #6.24(bytes)]: the model finds it OK, its tx_id the hash
in GenTxId_<era>, its size the ledger's sizeTxF (the payload's length for the three-item eras,
one less for the four-item eras, whose isValid byte sizeTxF leaves out), in_block_size four more
(perTxOverhead), the one golden redeemer's 5000 / 5000 units for the eras that have redeemers,
and the 9 golden witnesses verifying.  GenTx_Byron is unwrapped only."""
import pytest

import gentx_model as gm
from test_tx_index_model import ERAS, golden

SIZE = {"Shelley": 680, "Allegra": 792, "Mary": 887, "Alonzo": 864, "Babbage": 967, "Conway": 889}
N_WIT = {"Shelley": 2, "Allegra": 2, "Mary": 2, "Alonzo": 1, "Babbage": 1, "Conway": 1}


def golden_items():
    g = golden()
    return [bytes.fromhex(g["eras"][e]["gen_tx"]) for e in ERAS], g


def layout(items):
    off, p = [], 0
    for t in items:
        off.append(p)
        p += len(t)
    return b"".join(items), off, [len(t) for t in items]


@pytest.mark.parametrize("era", ERAS)
def test_golden_gen_tx_of_each_era(era):
    g = golden()["eras"][era]
    k = ERAS.index(era) + 1
    arena, off, ln = layout([bytes.fromhex(g["gen_tx"])])
    I, T, W = gm.verify(arena, off, ln)
    assert I["status"] == [gm.OK] and I["era"] == [k] and I["row"] == [0] and I["byron_kind"] == [0xFF]
    assert I["payload_off"] == [0] and I["payload_len"] == [0]
    assert T["item"] == [0] and T["era"] == [k]
    assert T["tx_id"] == [bytes.fromhex(g["gen_tx_id"])[4:]]
    assert T["size"] == [SIZE[era]] and T["in_block_size"] == [SIZE[era] + 4]
    assert T["is_valid"] == [1]
    want = 5000 if k >= 4 else 0
    assert T["ex_mem"] == [want] and T["ex_steps"] == [want]
    assert T["wstatus"] == [0] and T["n_vkey"][0] + T["n_boot"][0] == N_WIT[era] and T["n_bad"] == [0]
    assert W["ok"] == [1] * N_WIT[era] and T["wit_first"] == [0, N_WIT[era]]
    # the spans tile the inner array: head, body, wits, (isValid,) aux
    assert T["wit_off"][0] == T["body_off"][0] + T["body_len"][0]
    inner = len(arena) - (T["body_off"][0] - 1)
    assert 1 + T["body_len"][0] + T["wit_len"][0] + (T["aux_len"][0] or 1) == inner - (1 if k >= 4 else 0)
    assert T["size"][0] == 1 + T["body_len"][0] + T["wit_len"][0] + (T["aux_len"][0] or 1)


def test_the_six_in_one_call_and_the_nine_witnesses():
    items, _ = golden_items()
    arena, off, ln = layout(items)
    I, T, W = gm.verify(arena, off, ln)
    assert I["status"] == [gm.OK] * 6 and I["row"] == list(range(6)) and T["item"] == list(range(6))
    assert [T["size"][k] for k in range(6)] == [SIZE[e] for e in ERAS]
    assert len(W["ok"]) == 9 and W["ok"] == [1] * 9
    # offered twice: the same six rows
    I2, T2, W2 = gm.verify(arena, off + off, ln + ln)
    assert I2["row"] == list(range(6)) * 2 and T2 == T and W2 == W
    I3, T3, _ = gm.verify(arena, off + off, ln + ln, dedup=False)
    assert I3["row"] == list(range(12)) and T3["tx_id"] == T["tx_id"] * 2


def test_golden_byron_gen_tx_is_unwrapped_only():
    g = golden()["byron"]
    tx = bytes.fromhex(g["gen_tx"])
    I, T, W = gm.verify(tx, [0], [len(tx)])
    assert I["status"] == [gm.BYRON] and I["era"] == [0] and I["byron_kind"] == [0] and I["row"] == [gm.NO_ROW]
    assert I["payload_off"] == [4] and I["payload_len"] == [236]
    assert T["item"] == [] and T["wit_first"] == [0] and W["tx"] == []
