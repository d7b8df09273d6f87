"""GPU: praos_validate_candidates_pbft -- K candidate fragments of Byron wire headers in one call --
against tests/candidates_eras_model.py (rows from tests/pbft_model.py, the client's fold on top)
and against the existing path (praos_verify_pbft_headers + the fold over the inner spans)."""
import copy
import os

import numpy as np
import pytest

import byron_corpus as bc
import candidates_eras_model as cem
import pbft_corpus as pc
import pbft_model as pm
import wire_corpus
from helpers import rng
from praos_hip import abi, wire

pytestmark = pytest.mark.gpu
ES, PMAG = pc.EPOCH_SLOTS, pc.PM
W, T = 14, 2                                   # 7 delegates in turn: two of each in any 14 signers
COLS = [name for name, _, _ in abi.PBFT_OUT_FIELDS]


def params(pmagic=PMAG):
    return abi.Context.pbft_params(W, T, ES, pmagic)


@pytest.fixture(scope="module")
def base(oracle):
    """3 epochs of one EBB and 40 main headers, 7 delegates in turn, and an eighth key outside the
    map.  The intact chain never exceeds the threshold (checked on the CPU first)."""
    r = rng(0x0c4d)
    D = [bc.Delegate(r) for _ in range(8)]
    blocks = pc.make_chain(r, 40, lambda k: D[k % 7], epochs=3)
    delegs = pc.delegation(r, D[:7])
    rows = pc.model_rows(blocks, delegs)
    ebb = [int(b.kind == 0) for b in blocks]
    v, _, stop, _, _ = pm.fold(rows, ebb, W, T, ES, delegs)
    assert stop == len(blocks) == 123 and set(v) == {0}
    model = cem.PbftModel(W, T, ES, PMAG, delegs)

    def at(start):
        """(tip, state) after the chain's first `start` headers"""
        _, _, _, tip, st = pm.fold(rows[:start], ebb[:start], W, T, ES, delegs)
        return {"tip": tip, "state": st}
    return {"r": r, "D": D, "blocks": blocks, "delegs": delegs, "rows": rows, "ebb": ebb, "items": cem.wrap_blocks(blocks),
            "model": model, "at": at}


def call(ctx, base, frag_items, frags_in, pmagic=PMAG, delegs=None, **kw):
    """the fragments' items back to back through the call: (items, frag_first, got, frags_out)"""
    items = [it for f in frag_items for it in f]
    ff = np.concatenate([[0], np.cumsum([len(f) for f in frag_items])]).astype(int).tolist()
    arena, off, ln = cem.pack(items)
    out = copy.deepcopy(frags_in)
    got = ctx.validate_candidates_pbft(arena, off, ln, ff, out, params(pmagic), base["delegs"] if delegs is None else delegs,
                                       **kw)
    return items, ff, got, out


def raw(got, frags):
    """every output byte of a call, for run-to-run comparisons"""
    parts = [got[k].tobytes() for k in ("wire_status", "row", "verdict", "aux", "row_is_ebb")]
    parts += [got["rows"][c].tobytes() for c in COLS if c in got["rows"]]
    return b"".join(parts) + repr([(f["tip"], f["state"], f["chain_stop"], f["processed"]) for f in frags]).encode()


def test_one_fragment_equals_the_existing_path(ctx, base):
    items = base["items"]
    its, ff, got, out = call(ctx, base, [items], [base["at"](0)], delegate_hash=True)
    arena, off, ln = cem.pack(items)
    inner = [wire.unwrap(it) for it in items]
    ioff = np.array([int(o) + u[4] for o, u in zip(off, inner)], np.uint64)
    ilen = np.array([u[5] for u in inner], np.uint32)
    H, v, aux, stop, tip, state = ctx.validate_pbft_headers(arena, ioff, ilen, base["ebb"], params(), base["delegs"])
    assert (got["verdict"] == v).all() and (got["aux"] == aux).all() and set(v) == {0}
    assert (out[0]["chain_stop"], out[0]["processed"], out[0]["tip"], out[0]["state"]) == (stop, len(items), tip, state)
    assert got["n_rows"] == len(items) and list(got["row"]) == list(range(len(items)))
    Hd = ctx.verify_pbft_headers(arena, ioff, ilen, base["ebb"], params(), base["delegs"], delegate_hash=True)
    for c in COLS:
        assert (got["rows"][c] == Hd[c]).all(), c
    assert list(got["row_is_ebb"]) == base["ebb"]
    U = ctx.unwrap_wire_headers(arena, off, ln)
    assert (U["header_hash"] == got["rows"]["header_hash"]).all()
    assert got["stats"] == {"items": 123, "unwrapped": 123, "distinct_headers": 123, "sig_verifies": 120}
    base["model"].check(its, ff, [base["at"](0)], got, out)


STARTS = (0, 1, 2, 41, 42, 60, 100, 122)      # 1 and 42: right after an EBB


def _eight(base):
    items = base["items"]
    return [items[s:s + 45] for s in STARTS], [base["at"](s) for s in STARTS]


def test_eight_fragments_from_their_own_tips(ctx, base):
    frag_items, frags_in = _eight(base)
    its, ff, got, out = call(ctx, base, frag_items, frags_in)
    distinct = base["model"].check(its, ff, frags_in, got, out)
    assert got["n_rows"] == got["stats"]["distinct_headers"] == len(distinct) == 123 < len(its)
    assert all(f["chain_stop"] == f["processed"] == len(fi) for f, fi in zip(out, frag_items))
    assert set(got["verdict"]) == {0}
    # each fragment ends where the single fragment over the same range ends
    for s, f, fi in zip(STARTS, out, frag_items):
        end = base["at"](s + len(fi))
        assert (f["tip"], f["state"]) == (end["tip"], end["state"]), s
    its2, _, got2, out2 = call(ctx, base, frag_items, frags_in)
    assert raw(got, out) == raw(got2, out2)


def test_size_hint_is_no_part_of_the_key_and_the_kind_is(ctx, base):
    blocks = base["blocks"]
    a = cem.wrap_blocks(blocks[:6], hint=lambda i, b: 100 + i)
    b = cem.wrap_blocks(blocks[:6], hint=lambda i, b: 70000 + i)
    assert a[1] != b[1]
    # the EBB's bytes once more as a main header: the same bytes, another hash (82 01 ||), a row of its own
    c = [wire.wrap(0, blocks[0].header, 1, 5)]
    frags_in = [base["at"](0), base["at"](0), base["at"](0)]
    its, ff, got, out = call(ctx, base, [a, b, c], frags_in)
    base["model"].check(its, ff, frags_in, got, out)
    assert got["n_rows"] == 7 and list(got["row"]) == list(range(6)) * 2 + [6]
    assert list(got["row_is_ebb"]) == [1, 0, 0, 0, 0, 0, 0]
    assert bytes(got["rows"]["header_hash"][0]) != bytes(got["rows"]["header_hash"][6]) or got["rows"]["bits"][6] & 1
    assert got["verdict"][12] == pm.V_INPUT and got["rows"]["bits"][6] == pm.BIT_DECODE


EBB_WRAP_EPOCH = ((1 << 64) + 24) // ES         # epoch * 40 wraps to slot 24: an EBB off the boundary


def _failures(base):
    """(name, items, start state, index of the stop, verdict) in the order the fold applies its checks"""
    r, D, blocks, items, at = base["r"], base["D"], base["blocks"], base["items"], base["at"]
    b10 = blocks[10]
    assert b10.kind == 1 and blocks[9].kind == 1 and ES == 40

    def main(dlg, sie=b10.sie, diff=b10.difficulty):
        return bc.Main(r, dlg, blocks[9].header_hash, 0, sie, diff)

    def frag(mid):
        return items[5:10] + [wire.wrap(0, mid.header, mid.kind, 9)] + items[11:14]
    bad_sig = copy.copy(b10).sign(sig=b10.sig[:5] + bytes([b10.sig[5] ^ 1]) + b10.sig[6:])
    late = at(5)
    late["state"] = late["state"][:-1] + [(late["state"][-1][0] + 1000, late["state"][-1][1])]
    off_boundary = bc.EBB(r, blocks[9].header_hash, EBB_WRAP_EPOCH, blocks[9].difficulty)
    return [
        ("signature", frag(bad_sig), at(5), 5, pm.V_INVALID_SIG),
        ("delegate", frag(main(D[7])), at(5), 5, pm.V_NOT_DELEGATE),
        ("threshold", frag(main(blocks[9].dlg)), at(5), 5, pm.V_EXCEEDED),
        ("signed-slot", items[5:9], late, 0, pm.V_INVALID_SLOT),
        ("ebb-slot", frag(off_boundary), at(5), 5, pm.V_EBB_IN_SLOT),
        ("doesnt-fit", items[5:8] + items[9:12], at(5), 3, cem.V_DOESNT_FIT),
        ("undecodable", items[5:7] + [wire.wrap(0, blocks[7].header[:-1], 1, 3)] + items[8:10], at(5), 2, pm.V_INPUT),
        ("era", items[5:7] + [wire.wrap(2, blocks[7].header)] + items[8:10], at(5), 2, pm.V_INPUT),
        ("truncated-item", items[5:7] + [items[7][:-1]] + items[8:10], at(5), 2, pm.V_INPUT),
    ]


def test_each_failure_stops_its_fragment(ctx, base):
    cases = _failures(base)
    frags_in = [c[2] for c in cases]
    its, ff, got, out = call(ctx, base, [c[1] for c in cases], frags_in)
    base["model"].check(its, ff, frags_in, got, out)
    for j, (name, fi, start, stop, verdict) in enumerate(cases):
        v = list(got["verdict"][ff[j]:ff[j + 1]])
        assert v == [0] * stop + [verdict] + [cem.V_NOT_REACHED] * (len(fi) - stop - 1), (name, v)
        assert (out[j]["chain_stop"], out[j]["processed"]) == (stop, stop + 1), name
        assert pm.V_ENV_PREV_HASH not in v
    aux = {c[0]: int(got["aux"][ff[j] + c[3]]) for j, c in enumerate(cases)}
    assert aux["threshold"] == 3 and aux["ebb-slot"] == 24 and aux["signature"] == 0
    # state and tip at the stop: those after the valid items before it
    assert (out[0]["tip"], out[0]["state"]) == (base["at"](10)["tip"], base["at"](10)["state"])
    assert (out[3]["tip"], out[3]["state"]) == (cases[3][2]["tip"], cases[3][2]["state"])
    assert got["row"][ff[7] + 2] == wire.NO_ROW and got["row"][ff[8] + 2] == wire.NO_ROW
    assert got["wire_status"][ff[8] + 2] == wire.WIRE_SYNTAX


def test_forecast_horizon_in_mid_fragment(ctx, base):
    items, rows = base["items"], base["rows"]
    frags_in = [base["at"](0), base["at"](42), base["at"](100)]
    horizon = rows[50]["slot"]
    its, ff, got, out = call(ctx, base, [items[:60], items[42:70], items[100:110]], frags_in, view_end_slot=horizon)
    base["model"].check(its, ff, frags_in, got, out, view_end_slot=horizon)
    assert [(f["chain_stop"], f["processed"]) for f in out] == [(50, 50), (8, 8), (0, 0)]
    assert (out[0]["tip"], out[0]["state"]) == (base["at"](50)["tip"], base["at"](50)["state"])
    assert list(got["verdict"][50:60]) == [cem.V_NOT_REACHED] * 10 and not got["verdict"][:50].any()
    assert out[2]["tip"] == frags_in[2]["tip"] and out[2]["state"] == frags_in[2]["state"]


FORCED = {   # name: (PRAOS_PBFT_CK_MIN, key cache option), as tests/test_gpu_pbft.py forces them
    "cached": ("1", None),
    "uncached": (str(1 << 40), None),
    "off": ("1", 0),
}


@pytest.fixture(scope="module")
def forced():
    made = {}
    old = os.environ.get("PRAOS_PBFT_CK_MIN")
    try:
        for name, (ck, opt) in FORCED.items():
            os.environ["PRAOS_PBFT_CK_MIN"] = ck
            made[name] = abi.Context(0)
            if opt is not None:
                made[name].set_option(abi.OPT_KEYCACHE, opt)
    finally:
        if old is None:
            os.environ.pop("PRAOS_PBFT_CK_MIN", None)
        else:
            os.environ["PRAOS_PBFT_CK_MIN"] = old
    yield made
    for c in made.values():
        c.close()


def test_cached_and_uncached_verify_give_the_same_bytes(forced, base):
    cases = _failures(base)
    frag_items, frags_in = _eight(base)
    frag_items, frags_in = frag_items + [c[1] for c in cases], frags_in + [c[2] for c in cases]
    outs = {}
    for name, c in forced.items():
        its, ff, got, out = call(c, base, frag_items, frags_in, delegate_hash=True)
        base["model"].check(its, ff, frags_in, got, out)
        st = c.pbft_stats()
        assert st["cache"] == (name == "cached"), (name, st)
        # the verifies are counted over the rows, whichever kernel ran them
        assert st["cached_verifies"] + st["uncached_verifies"] == got["stats"]["sig_verifies"], (name, st)
        if name == "cached":
            assert st["keys_cached"] == 7 and st["cached_verifies"] >= 120, st    # D[7] is used once: a miss
        else:
            assert (st["keys_cached"], st["cached_verifies"]) == (0, 0), (name, st)
        outs[name] = raw(got, out)
    assert outs["cached"] == outs["uncached"] == outs["off"]


def test_rows_cap_and_empty_calls(ctx, base):
    frag_items, frags_in = _eight(base)
    with pytest.raises(abi.PraosError) as e:
        call(ctx, base, frag_items, frags_in, rows_cap=122)
    assert e.value.rc == abi.E_ARG and e.value.n_rows == 123
    _, _, got, out = call(ctx, base, frag_items, frags_in, rows_cap=123)
    assert got["n_rows"] == 123
    _, _, got, out = call(ctx, base, [[], []], [base["at"](0), base["at"](7)])           # N = 0
    assert got["n_rows"] == 0 and [(f["chain_stop"], f["processed"]) for f in out] == [(0, 0)] * 2
    assert out[1]["tip"] == base["at"](7)["tip"] and out[1]["state"] == base["at"](7)["state"]
    _, _, got, out = call(ctx, base, [], [])                                             # K = 0
    assert got["n_rows"] == 0 and got["stats"]["items"] == 0
    # an empty fragment between two others
    frags_in = [base["at"](0), base["at"](3), base["at"](3)]
    its, ff, got, out = call(ctx, base, [base["items"][:3], [], base["items"][3:6]], frags_in)
    base["model"].check(its, ff, frags_in, got, out)


def test_golden_byron_wire_headers(ctx, oracle):
    """Header_Byron_regular and Header_Byron_EBB of the reference's golden wire headers, each a
    one-item fragment from the tip its prev hash names: the rows equal verify_pbft_headers on the
    inner span, the verdicts the model's"""
    gold = [h for h in wire_corpus.golden()["headers"] if h["era"] == 0]
    assert sorted(h["name"] for h in gold) == ["Byron_EBB", "Byron_regular"]
    items = [bytes.fromhex(h["wire"]) for h in gold]
    kinds = [h["byron_kind"] for h in gold]
    inner = [wire.unwrap(it) for it in items]
    hdrs = [it[u[4]:u[4] + u[5]] for it, u in zip(items, inner)]
    main = hdrs[kinds.index(1)]
    d = pm.decode_header(main, 0, ES)
    magic = int.from_bytes(main[2:6], "big")
    assert main[1] == 0x1A and d is not None
    delegs = [(pm.key_hash(d["blk"][d["issuer"]:d["issuer"] + 64]), pm.key_hash(d["blk"][d["delegate"]:d["delegate"] + 64]))]
    model = cem.PbftModel(W, T, ES, magic, delegs)
    frags_in = []
    for it in items:
        h = model.row(model.key(it))
        assert not h["bits"] & pm.BIT_DECODE
        ebb = model.key(it)[0] == 0
        if h["prev_is_genesis"]:
            frags_in.append({"tip": None, "state": []})
        else:
            frags_in.append({"tip": (h["slot"] - 1, h["block_no"] - (0 if ebb else 1), bytes(h["prev_hash"]), 0), "state": []})
    base = {"delegs": delegs}
    its, ff, got, out = call(ctx, base, [[it] for it in items], frags_in, pmagic=magic, delegate_hash=True)
    model.check(its, ff, frags_in, got, out)
    arena, off, ln = cem.pack(items)
    ioff = np.array([int(o) + u[4] for o, u in zip(off, inner)], np.uint64)
    H = ctx.verify_pbft_headers(arena, ioff, np.array([u[5] for u in inner], np.uint32), [int(k == 0) for k in kinds],
                                params(magic), delegs, delegate_hash=True)
    for c in COLS:
        assert (got["rows"][c] == H[c]).all(), c
    assert list(got["verdict"]) == [0, 0] and not got["rows"]["bits"].any()
