"""CPU: the wire-block model (blockfetch_model.py) pinned to the reference's golden wire blocks
(tests/golden/wire_blocks.json: the distinct Block_* files of CardanoNodeToNodeVersion5-7).

All 8 are OK with the disk tag of their era; blockMatchesHeader holds for each; the header hash is
what wire.unwrap plus the header-hash rule gives for the same era's golden wire *header*
(wire_headers.json: the same header in its other encoding); the 9 golden witnesses verify; and
asked for its own point every block is accepted."""
import hashlib
import json
import os

import pytest

import blockfetch_model as fm
from praos_hip import blockfetch as bf, wire

HERE = os.path.dirname(os.path.abspath(__file__))
EPOCH_SLOTS = 21600
N_WIT = {"Shelley": 2, "Allegra": 2, "Mary": 2, "Alonzo": 1, "Babbage": 1, "Conway": 1}


def golden():
    with open(os.path.join(HERE, "golden", "wire_blocks.json")) as f:
        return json.load(f)


def golden_items():
    return [(b["name"], b["disk_tag"], bytes.fromhex(b["wire"])) for b in golden()["blocks"]]


def wire_header_hash(name):
    """the header hash by the wire-header route: unwrap the golden wire header, hash by its era's rule"""
    with open(os.path.join(HERE, "golden", "wire_headers.json")) as f:
        h = next(x for x in json.load(f)["headers"] if x["name"] == name)
    raw = bytes.fromhex(h["wire"])
    status, era, kind, _, off, ln = wire.unwrap(raw)
    assert status == wire.WIRE_OK
    pre = bytes([0x82, kind]) if era == 0 else b""
    return hashlib.blake2b(pre + raw[off:off + ln], digest_size=32).digest()


def one(raw, **kw):
    hd = fm.header_of(raw, *fm.unwrap(raw, 0, len(raw))[1:], EPOCH_SLOTS)
    return fm.verify(raw, [0], [len(raw)], [0, 1], [0, 1], [hd["slot"]], [hd["header_hash"]],
                     byron_epoch_slots=EPOCH_SLOTS, **kw)


def test_the_fixture_holds_the_eight_blocks():
    g = golden()
    assert g["n_eras"] == 7 and len(g["blocks"]) == 8
    assert [b["disk_tag"] for b in g["blocks"]] == list(range(8))
    assert all(b["versions"] == [5, 6, 7] for b in g["blocks"])


@pytest.mark.parametrize("k", range(8))
def test_golden_wire_block(k):
    name, tag, raw = golden_items()[k]
    assert fm.unwrap(raw, 0, len(raw))[:2] == (fm.OK, tag) == bf.unwrap_block(raw)[:2]
    assert fm.unwrap(raw, 0, len(raw)) == bf.unwrap_block(raw)
    assert bf.wrap_block(raw[bf.unwrap_block(raw)[2]:]) == raw
    I, G, R, B, T, W = one(raw)
    assert I["status"] == [fm.OK] and I["tag"] == [tag] and I["row"] == [0] and I["verdict"] == [fm.BF_OK]
    assert G["stop"] == [1] and G["accepted"] == [1] and G["status"] == [fm.COMPLETE]
    assert R["bits"] == [0] and R["which"] == [0] and R["is_ebb"] == [int(tag == 0)] and R["item"] == [0]
    assert R["header_hash"] == [wire_header_hash(name)]
    assert raw[R["blk_off"][0]:] == raw[-R["blk_len"][0]:] and R["blk_off"][0] + R["blk_len"][0] == len(raw)
    if tag >= 2:
        assert R["body_hash"][0] != bytes(32) and B["n_tx"] == [1] and B["n_wit"] == [N_WIT[name]] and B["n_bad"] == [0]
        assert W["ok"] == [1] * N_WIT[name]
    else:
        assert R["body_hash"] == [bytes(32)] and B["n_wit"] == [0]
        assert T["status"] == ([] if tag == 0 else [fm.wm.SKIPPED])
    # one byte of the last segment changed: the same header, another body
    bad = bytearray(raw)
    bad[-2] ^= 1
    I2, _, R2, *_ = fm.verify(bytes(bad), [0], [len(bad)], [0, 1], [0, 1], R["slot"], R["header_hash"],
                              byron_epoch_slots=EPOCH_SLOTS, witnesses=False)
    if tag:          # (an EBB's body is not compared)
        assert I2["verdict"] in ([fm.BF_INVALID_BODY], [fm.BF_DECODE]) and (I2["row"] == [fm.NO_ROW] or R2["bits"] == [4])


def test_the_eight_in_one_call_and_the_nine_witnesses():
    items = golden_items()
    off, pos = [], 0
    for _, _, raw in items:
        off.append(pos)
        pos += len(raw)
    arena = b"".join(raw for _, _, raw in items)
    ln = [len(raw) for _, _, raw in items]
    heads = [fm.header_of(arena, t, *fm.unwrap(arena, o, n)[2:], EPOCH_SLOTS) for (_, t, _), o, n in zip(items, off, ln)]
    pts = ([h["slot"] for h in heads], [h["header_hash"] for h in heads])
    I, G, R, B, T, W = fm.verify(arena, off, ln, [0, 8], [0, 8], *pts, byron_epoch_slots=EPOCH_SLOTS)
    assert I["verdict"] == [fm.BF_OK] * 8 and I["row"] == list(range(8)) and G["status"] == [fm.COMPLETE]
    assert len(W["ok"]) == 9 and all(W["ok"]) and B["n_wit"] == [0, 0, 2, 2, 2, 1, 1, 1]
    # Byron off: the EBB stops the range, unsupported
    I, G, R, *_ = fm.verify(arena, off, ln, [0, 8], [0, 8], *pts, witnesses=False)
    assert I["verdict"] == [fm.BF_UNSUPPORTED] + [fm.BF_NOT_REACHED] * 7 and G["status"] == [fm.FAILED] and G["stop"] == [0]
    assert I["row"] == [fm.NO_ROW] * 2 + list(range(6))
    # the same eight from a second peer: no new row
    I, G, R, *_ = fm.verify(arena, off * 2, ln * 2, [0, 8, 16], [0, 8, 16], pts[0] * 2, pts[1] * 2,
                            byron_epoch_slots=EPOCH_SLOTS, witnesses=False)
    assert I["row"] == list(range(8)) * 2 and len(R["item"]) == 8 and G["accepted"] == [8, 8]
