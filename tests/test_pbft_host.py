"""CPU: the host half of Byron header validation on a host-only context -- hashVerKey, the
PBftState codec and the sequential fold (praos_pbft_update_chain_dep_state) against
tests/pbft_model.py and the reference's fixtures (tests/golden/pbft_golden.json)."""
import json
import os

import numpy as np
import pytest

import pbft_corpus as pc
import pbft_model as pm
from helpers import rbytes, rng
from praos_hip import abi

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pbft_golden.json")))
K, THR, ES = 10, 4, 40
R = rng(0x9bf7)
GKS = [rbytes(R, 28) for _ in range(3)]
DELEGS = [(g, rbytes(R, 28)) for g in GKS]


@pytest.fixture(scope="module")
def host():
    c = abi.Context(abi.HOST_ONLY)
    yield c
    c.close()


def test_key_hash_of_the_reference_genesis_key(host):
    key = bytes.fromhex(GOLD["issuer_pk"])
    want = bytes.fromhex(GOLD["genesis_key_hash"])
    assert pm.key_hash(key) == want
    assert bytes(host.byron_key_hash(key)[0]) == want
    keys = [rbytes(R, 64) for _ in range(9)]
    got = host.byron_key_hash(b"".join(keys))
    assert [bytes(g) for g in got] == [pm.key_hash(k) for k in keys]


def test_state_codec_golden_bytes_round_trip():
    raw = bytes.fromhex(GOLD["chain_dep_state"])
    st = abi.Context.pbft_state_decode(raw)
    assert [s for s, _ in st] == [1, 2, 3, 4] and len({g for _, g in st}) == 1
    assert st == pm.state_decode(raw)
    assert abi.Context.pbft_state_encode(st) == raw == pm.state_encode(st)


@pytest.mark.parametrize("state", [
    [],
    [(5, GKS[0]), (9, GKS[0]), (300, GKS[0])],
    [(1, GKS[2]), (2, GKS[0]), (3, GKS[1]), (7, GKS[0]), (8, GKS[2]), (1 << 40, GKS[1]), (1 << 40, GKS[0])],
], ids=["empty", "one-key", "three-keys-interleaved"])
def test_state_codec_round_trips(state):
    enc = abi.Context.pbft_state_encode(state)
    assert enc == pm.state_encode(state)
    if not state:
        assert enc == bytes.fromhex("8201a0")
    dec = abi.Context.pbft_state_decode(enc)
    assert dec == pm.state_decode(enc)
    # equal slots come back in key order (sortOn is stable over Map.toList's order)
    assert sorted(dec, key=lambda x: x[0]) == dec and sorted(dec) == sorted(state)
    assert abi.Context.pbft_state_encode(dec) == enc


def test_state_decode_refuses_other_bytes():
    raw = bytes.fromhex(GOLD["chain_dep_state"])
    for bad in (raw[:-1], raw + b"\x00", b"\x82\x00" + raw[2:], b"\x83" + raw[1:], raw.replace(b"\x58\x1c", b"\x58\x1b", 1)):
        with pytest.raises(abi.PraosError):
            abi.Context.pbft_state_decode(bad)
    # definite slot lists decode too (the decoder of [a] takes both forms)
    st = abi.Context.pbft_state_decode(raw.replace(b"\x9f\x04\x03\x02\x01\xff", b"\x84\x04\x03\x02\x01"))
    assert [s for s, _ in st] == [1, 2, 3, 4]


# ---- the fold over synthetic rows: (kind, gk index or -1, options)
def chain_rows(plan, tip=None, epoch0=0):
    """plan: list of dicts {ebb, gk, slot (default: next), bits, bno (offset), prev (override)} ->
    model rows that link up from tip, and the is_ebb bytes."""
    rows, ebbs = [], []
    slot = -1 if tip is None else tip[0]
    bno = -1 if tip is None else tip[1]
    prev = None if tip is None else tip[2]
    last_ebb = False if tip is None else bool(tip[3])
    for p in plan:
        ebb = bool(p.get("ebb"))
        if "slot" in p:
            s = p["slot"]
        elif ebb:
            s = ((slot // ES) + 1) * ES if slot >= 0 else 0
        else:
            s = slot if last_ebb else slot + 1
        b = (bno if (ebb and not last_ebb and prev is not None) else bno + 1) + p.get("bno", 0)
        row = {"bits": p.get("bits", 0), "gk_idx": -1 if ebb else p.get("gk", 0), "slot": s, "block_no": b,
               "prev_hash": bytes(32) if prev is None else prev, "prev_is_genesis": int(prev is None),
               "header_hash": rbytes(R, 32), "delegate_hash": bytes(28)}
        if "prev" in p:
            row["prev_hash"], row["prev_is_genesis"] = p["prev"]
        rows.append(row)
        ebbs.append(int(ebb))
        if not p.get("invalid"):
            slot, bno, prev, last_ebb = s, b, row["header_hash"], ebb
    return rows, ebbs


def run_both(host, rows, ebbs, tip=None, state=(), k=K, thr=THR):
    want = pm.fold(rows, ebbs, k, thr, ES, DELEGS, tip, state)
    params = abi.Context.pbft_params(k, thr, ES, 1)
    v, aux, stop, t, st = host.pbft_update_chain_dep_state(pc.rows_to_columns(rows), ebbs, params, DELEGS, tip, state)
    assert (list(v), [int(a) for a in aux], stop, t, st) == (want[0], want[1], want[2], want[3], want[4])
    return want


def test_fold_round_robin_chain_is_valid(host):
    plan = [{"ebb": 1}] + [{"gk": i % 3} for i in range(25)] + [{"ebb": 1}] + [{"gk": i % 3} for i in range(7)]
    rows, ebbs = chain_rows(plan)
    v, _, stop, tip, st = run_both(host, rows, ebbs)
    assert set(v) == {pm.V_OK} and stop == len(rows) and len(st) == K
    assert tip == (rows[-1]["slot"], rows[-1]["block_no"], rows[-1]["header_hash"], 0)
    assert [s for s, _ in st] == [r["slot"] for r, e in zip(rows, ebbs) if not e][-K:]


def test_fold_threshold_and_trim(host):
    # key 0 signs five times in a row: the fifth exceeds threshold 4 with n = 5
    plan = [{"ebb": 1}] + [{"gk": 0}] * 4 + [{"gk": 0, "invalid": 1}] + [{"gk": 1}] * 3
    rows, ebbs = chain_rows(plan)
    v, aux, stop, _, st = run_both(host, rows, ebbs)
    assert v[5] == pm.V_EXCEEDED and aux[5] == THR + 1 and stop == 5 and len(st) == 4
    assert v[:5] == [0] * 5 and v[6:] == [0] * 3
    # after its old signatures have left the window the same key signs again
    plan = [{"ebb": 1}] + [{"gk": 0}] * 4 + [{"gk": 1}] * 3 + [{"gk": 2}] * 3 + [{"gk": 1}] + [{"gk": 0}] * 4
    rows, ebbs = chain_rows(plan)
    v, _, stop, _, st = run_both(host, rows, ebbs)
    assert set(v) == {0} and stop == len(rows)
    # the trim decrements the very key being appended: a full window whose oldest signer is key 0
    # holds four of key 0; key 0 signs again and stays at four
    state = [(s, GKS[0 if s in (1, 5, 6, 7) else 1 + s % 2]) for s in range(1, K + 1)]
    assert sum(g == GKS[0] for _, g in state) == THR
    tip = (K, K, rbytes(R, 32), 0)
    rows, ebbs = chain_rows([{"gk": 0}], tip)
    v, _, _, _, st = run_both(host, rows, ebbs, tip, state)
    assert v == [0] and len(st) == K and st[0][0] == 2 and sum(g == GKS[0] for _, g in st) == THR
    # the same window with another key oldest: the append makes five
    state2 = [(s, GKS[1] if s == 1 else GKS[0] if s in (2, 5, 6, 7) else GKS[2]) for s in range(1, K + 1)]
    v, aux, _, _, st = run_both(host, rows, ebbs, tip, state2)
    assert v == [pm.V_EXCEEDED] and aux == [THR + 1] and st == state2


def test_fold_pbft_failures_in_the_reference_order(host):
    tip = (9, 4, rbytes(R, 32), 0)
    state = [(3, GKS[0]), (9, GKS[1])]
    for plan, want in (
            ([{"gk": -1}], pm.V_NOT_DELEGATE),
            ([{"gk": 1, "bits": pm.BIT_SIG}], pm.V_INVALID_SIG),
            ([{"gk": -1, "bits": pm.BIT_SIG | pm.BIT_NOT_DELEGATE}], pm.V_INVALID_SIG),     # signature first
            ([{"gk": 1, "bits": pm.BIT_DECODE}], pm.V_INPUT),
            ([{"gk": 1, "bits": pm.BIT_SIG, "bno": 3}], pm.V_ENV_BLOCK_NO),                   # envelope first
            ([{"gk": 1, "bits": pm.BIT_SIG, "slot": 2, "bno": 1}], pm.V_ENV_BLOCK_NO),       # block number before slot
            ([{"gk": 1, "bits": pm.BIT_SIG, "slot": 2}], pm.V_ENV_SLOT_NO),
            ([{"gk": 1, "slot": 9}], pm.V_ENV_SLOT_NO),
            ([{"gk": 1, "prev": (rbytes(R, 32), 0)}], pm.V_ENV_PREV_HASH),
            ([{"gk": 1, "prev": (bytes(32), 1)}], pm.V_ENV_PREV_HASH)):
        rows, ebbs = chain_rows(plan, tip)
        v, _, stop, t, st = run_both(host, rows, ebbs, tip, state)
        assert v == [want] and stop == 0 and t == tip and st == state
    # PBftInvalidSlot needs a window whose last signed slot is ahead of the tip's: through the
    # fold entry directly (an EBB tip at slot 40 after a state that signed slot 45)
    tip = (40, 7, rbytes(R, 32), 1)
    rows, ebbs = chain_rows([{"gk": 2, "slot": 41}], tip)
    v, _, _, _, _ = run_both(host, rows, ebbs, tip, [(45, GKS[0])])
    assert v == [pm.V_INVALID_SLOT]
    rows, ebbs = chain_rows([{"gk": 2, "slot": 45}], tip)                 # equal is allowed (PBFT.hs:338-342)
    assert run_both(host, rows, ebbs, tip, [(45, GKS[0])])[0] == [0]


def test_fold_envelope_cases(host):
    h32 = rbytes(R, 32)
    # the first block at Origin: block number 0, any slot, GenesisHash
    for plan, want in (([{"ebb": 1}], 0), ([{"gk": 0, "slot": 0}], 0), ([{"gk": 0, "slot": 17}], 0),
                       ([{"ebb": 1, "bno": 1}], pm.V_ENV_BLOCK_NO), ([{"ebb": 1, "prev": (h32, 0)}], pm.V_ENV_PREV_HASH)):
        rows, ebbs = chain_rows(plan)
        assert run_both(host, rows, ebbs)[0] == [want]
    main_tip, ebb_tip = (79, 30, h32, 0), (80, 30, h32, 1)
    cases = (
        (main_tip, {"ebb": 1}, 0),                                  # EBB after main: same block number, slot 80
        (main_tip, {"ebb": 1, "bno": 1}, pm.V_ENV_BLOCK_NO),
        (main_tip, {"ebb": 1, "slot": 79}, pm.V_ENV_SLOT_NO),       # an EBB needs tip + 1 (then off the boundary)
        (main_tip, {"ebb": 1, "slot": 81}, pm.V_EBB_IN_SLOT),       # UnexpectedEBBInSlot
        (ebb_tip, {"gk": 0}, 0),                                    # main after EBB: the same slot, number + 1
        (ebb_tip, {"gk": 0, "slot": 79}, pm.V_ENV_SLOT_NO),
        (ebb_tip, {"gk": 0, "bno": -1}, pm.V_ENV_BLOCK_NO),
        (ebb_tip, {"ebb": 1, "slot": 120}, 0),                      # EBB after EBB: number + 1, slot + 1 at least
        (ebb_tip, {"ebb": 1, "slot": 120, "bno": -1}, pm.V_ENV_BLOCK_NO),
        (ebb_tip, {"ebb": 1, "slot": 80}, pm.V_ENV_SLOT_NO),
        (main_tip, {"gk": 0, "slot": 79}, pm.V_ENV_SLOT_NO),        # main after main
    )
    for tip, p, want in cases:
        rows, ebbs = chain_rows([p], tip)
        assert run_both(host, rows, ebbs, tip)[0] == [want], (tip[3], p)


def test_fold_batch_semantics_and_carried_state(host):
    # an invalid header in the middle: chain_stop there, later headers judged against the
    # working copy that skips it, state and tip returned as they were before it
    plan = ([{"ebb": 1}] + [{"gk": i % 3} for i in range(6)] + [{"gk": 0, "bits": pm.BIT_SIG, "invalid": 1}] +
            [{"gk": (i + 1) % 3} for i in range(9)])
    rows, ebbs = chain_rows(plan)
    v, _, stop, tip, st = run_both(host, rows, ebbs)
    assert stop == 7 and v[7] == pm.V_INVALID_SIG and v[:7] == [0] * 7 and v[8:] == [0] * 9
    assert tip[2] == rows[6]["header_hash"] and len(st) == 6
    # two calls carrying state equal one call
    plan = [{"ebb": 1}] + [{"gk": i % 3} for i in range(30)] + [{"ebb": 1}] + [{"gk": i % 3} for i in range(11)]
    rows, ebbs = chain_rows(plan)
    one = run_both(host, rows, ebbs)
    for cut in (1, 12, 32, 33):
        a = run_both(host, rows[:cut], ebbs[:cut])
        b = run_both(host, rows[cut:], ebbs[cut:], a[3], a[4])
        assert a[0] + b[0] == one[0] and (b[3], b[4]) == (one[3], one[4])
