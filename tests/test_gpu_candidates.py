"""ChainSync candidates on the GPU (praos_unwrap_wire_headers, praos_validate_candidates).

A linked four-epoch chain (the replay tests' shape: 20 pools, f = 1/2, 600-slot epochs, window 200)
is wrapped in the node-to-node encoding (wire era 5, era 6 for one epoch) and handed to the
candidates call as K fragments, each from its own HeaderState.  The checker is
tests/candidates_model.py: unwrap and dedup in Python, each fragment folded as the ChainSync client
does, over crypto bits from praos_verify_header_bytes under every nonce the fold ticks to."""
import copy
from fractions import Fraction

import numpy as np
import pytest

import candidates_model as cm
import wire_corpus as wc
from helpers import b2b
from praos_hip import abi, wire

pytestmark = pytest.mark.gpu

EPOCHS, EPOCH_LEN, WINDOW = 4, 600, 200
LIMITS = (9, 8, 1100, 90_112)


def _genesis_state(eta0):
    return {"last_slot": None, "counters": {}, "evolving": eta0, "candidate": eta0, "epoch_nonce": eta0,
            "lab": None, "leb": None}


def _headers(data):
    return [bytes(data["arena"][int(o):int(o) + int(n)]) for o, n in zip(data["off"], data["len"])]


@pytest.fixture(scope="module")
def world(ctx):
    from praos_hip import immutable
    cfg = dict(npools=20, stake_offset=1, f=Fraction(1, 2), slots_per_kes_period=129600, max_kes_evo=62,
               eta0=b2b(b"replay-genesis"), seed=b"\x2a" * 32)
    data = immutable.make_multi_epoch_chain(ctx, cfg, EPOCHS, EPOCH_LEN, WINDOW)
    hdrs = _headers(data)
    slots = [int(s) for s in data["slots"]]
    items = [wire.wrap(6 if 2 * EPOCH_LEN <= s < 3 * EPOCH_LEN else 5, h) for s, h in zip(slots, hdrs)]
    M = cm.Model(ctx, data["pools"], data["params"], data["epoch_info"], LIMITS)
    W = dict(data=data, cfg=cfg, hdrs=hdrs, items=items, slots=slots, M=M, at={})

    def at(m):
        """(state, tip) after the first m headers (the model's fold from genesis)."""
        if m not in W["at"]:
            r = M.fold(items[:m], _genesis_state(cfg["eta0"]), None)
            assert r["chain_stop"] == m
            W["at"][m] = (r["state"], r["tip"])
        st, tip = W["at"][m]
        return cm.copy_state(st), tip
    W["state_at"] = at
    return W


def run(ctx, W, frags, M=None, check=True, **kw):
    """frags: [(items, state, tip)].  Returns (result, fragments after the call, items, frag_first)."""
    M = M or W["M"]
    items = [it for f in frags for it in f[0]]
    first = np.cumsum([0] + [len(f[0]) for f in frags]).tolist()
    arena = np.frombuffer(b"".join(items) + b"\0", np.uint8)
    ln = np.array([len(it) for it in items], np.uint32)
    off = (np.cumsum(ln, dtype=np.uint64) - ln).astype(np.uint64)
    fin = [{"state": cm.copy_state(f[1]), "tip": f[2]} for f in frags]
    fout = copy.deepcopy(fin)
    ctx.set_epoch(W["data"]["nonces"][0], W["data"]["pools"], W["data"]["params"])
    got = ctx.validate_candidates(arena, off, ln, first, fout, W["data"]["epoch_info"], LIMITS, **kw)
    if check:
        M.check(items, first, fin, got, fout, kw.get("view_end_slot", 1 << 64))
    return got, fout, items, first


def test_golden_and_corpus_unwrap_on_the_gpu(ctx):
    """Every golden header and the whole mutation corpus in one call: status, era, kind, hint, span
    and hash are the host parser's; the Shelley-based hashes are praos_decode_headers' header_hash
    of the inner span, the Byron ones Blake2b-256(82 0k || header)."""
    G = wc.golden()
    cases = [(bytes.fromhex(h["wire"]), G["n_eras"]) for h in G["headers"]] + wc.corpus()
    for ne in sorted({ne for _, ne in cases}):
        sel = [raw for raw, n in cases if n == ne]
        arena = np.frombuffer(b"\xaa" + b"".join(sel) + b"\xbb", np.uint8)
        ln = np.array([len(r) for r in sel], np.uint32)
        off = (1 + np.cumsum(ln, dtype=np.uint64) - ln).astype(np.uint64)
        O = ctx.unwrap_wire_headers(arena, off, ln, n_eras=ne)
        ok_off, ok_len = [], []
        for i, raw in enumerate(sel):
            st, era, kind, hint, o, n = wire.unwrap(raw, n_eras=ne)
            assert (O["status"][i], O["era"][i], O["byron_kind"][i], O["size_hint"][i]) == (st, era, kind, hint), raw.hex()
            if st != wire.WIRE_OK:
                assert O["off"][i] == 0 and O["len"][i] == 0 and not O["header_hash"][i].any()
                continue
            assert (O["off"][i], O["len"][i]) == (int(off[i]) + o, n)
            inner = raw[o:o + n]
            want = b2b(bytes([0x82, kind]) + inner) if era == 0 else b2b(inner)
            assert bytes(O["header_hash"][i]) == want, raw.hex()
            if era != 0:
                ok_off.append(O["off"][i])
                ok_len.append(O["len"][i])
        if ok_off:
            D = ctx.decode_headers(arena, np.array(ok_off, np.uint64), np.array(ok_len, np.uint32))
            sh = [bytes(O["header_hash"][i]) for i in range(len(sel)) if O["status"][i] == 0 and O["era"][i] != 0]
            assert [bytes(h) for h in D["header_hash"]] == sh
    # spans outside the arena, no hash wanted, no items
    O = ctx.unwrap_wire_headers(np.zeros(10, np.uint8), [5, 11, 0], [6, 0, 11], header_hash=False)
    assert list(O["status"]) == [wire.WIRE_RANGE, wire.WIRE_RANGE, wire.WIRE_RANGE] and "header_hash" not in O
    assert len(ctx.unwrap_wire_headers(np.zeros(1, np.uint8), [], [])["status"]) == 0


def test_one_fragment_from_genesis(ctx, world):
    """K = 1: verdicts, final state and tip equal praos_validate_headers_nonces over the inner spans
    (and the model); no duplicates, so rows == items."""
    W, data = world, world["data"]
    n = len(W["items"])
    got, fout, _, _ = run(ctx, W, [(W["items"], _genesis_state(W["cfg"]["eta0"]), None)])
    assert int((got["verdict"] != 0).sum()) == 0 and (fout[0]["chain_stop"], fout[0]["processed"]) == (n, n)
    assert got["stats"] == {"items": n, "unwrapped": n, "distinct_headers": n, "rows": n, "extra_rows": 0}
    assert list(got["row"]) == list(range(n)) and got["etas"] == data["nonces"]
    assert fout[0]["state"] == data["state"]
    assert fout[0]["tip"] == (W["slots"][-1], n - 1, bytes(data["header_hash"][-1]))
    # the existing path: batch verify under per-header nonces, then praos_validate_headers_nonces
    epoch = (data["slots"] // EPOCH_LEN).astype(np.uint8)
    b = ctx.upload_bytes(data["arena"], data["off"], data["len"])
    try:
        ctx.batch_decode(b)
        D = ctx.download_decoded(b, n)
        ctx.set_nonces(b, data["nonces"], epoch)
        ctx.run(b)
        o = ctx.download(b, n)
    finally:
        ctx.free(b)
    z = lambda shape, dt: np.zeros(shape, dt)  # noqa: E731
    H = {k: D[k] for k in ("slot", "cold_vk", "vrf_vk", "vrf_out", "vrf_proof", "hot_vk", "ocert_n", "ocert_c0",
                           "ocert_sig", "kes_sig")}
    H.update(body_off=z(n, np.uint64), body_len=z(n, np.uint32), body_bytes=z(8, np.uint8))
    st = _genesis_state(W["cfg"]["eta0"])
    env = dict(zip(("max_major_pv", "lv_prot_major", "max_header_size", "max_body_size"), LIMITS), tip=None,
               block_no=D["block_no"], header_hash=D["header_hash"], header_size=data["len"], body_size=D["body_size"])
    v, stop, done = ctx.update_chain_dep_state(H, o, D["prev_hash"], st, data["epoch_info"],
                                               prev_is_genesis=D["prev_is_genesis"], envelope=env, etas=data["nonces"],
                                               eta_idx=epoch)
    assert (stop, done) == (n, n) and np.array_equal(v, got["verdict"])
    assert st == fout[0]["state"] and env["tip"] == fout[0]["tip"]
    for k in ("bits", "pool_idx", "beta", "leader", "nonce"):
        assert np.array_equal(got["rows"][k], o[k]), k
    for k in ("status", "slot", "block_no", "prev_hash", "header_hash", "kes_sig", "signed_body"):
        assert np.array_equal(got["dec"][k], D[k]), k


def test_eight_peers_on_the_same_chain(ctx, world):
    """K = 8 fragments over the same headers, two from mid-chain states, one from mid-epoch after the
    candidate freeze: each equals the K = 1 result on its range, the crypto runs once per header of
    the union, rows are in first-appearance order, and two runs give the same bytes."""
    W = world
    n = len(W["items"])
    s = W["slots"]
    mid1 = next(i for i in range(n) if s[i] >= EPOCH_LEN + 100)           # mid-epoch 1, before the freeze
    frozen = next(i for i in range(n) if s[i] >= 2 * EPOCH_LEN + 450)     # epoch 2, after the freeze (slot 1600)
    mid3 = next(i for i in range(n) if s[i] >= 3 * EPOCH_LEN + 7)
    starts = [300, 0, mid1, 0, frozen, 0, mid3, 0]
    ends = [n, n, n, 700, n, n, n - 5, n]
    frags = [(W["items"][a:b], *W["state_at"](a)) for a, b in zip(starts, ends)]
    got, fout, items, first = run(ctx, W, frags)
    assert int((got["verdict"] != 0).sum()) == 0
    for j, (a, b) in enumerate(zip(starts, ends)):
        assert (fout[j]["chain_stop"], fout[j]["processed"]) == (b - a, b - a)
        st, tip = W["state_at"](b)
        assert fout[j]["state"] == st and fout[j]["tip"] == tip
    st = got["stats"]
    assert (st["distinct_headers"], st["rows"], st["extra_rows"]) == (n, n, 0) and st["items"] == sum(ends) - sum(starts)
    # first appearance: fragment 0 brings headers 300.., fragment 1 the first 300
    want_row = {h: r for r, h in enumerate(list(range(300, n)) + list(range(300)))}
    for j, (a, b) in enumerate(zip(starts, ends)):
        assert list(got["row"][first[j]:first[j + 1]]) == [want_row[h] for h in range(a, b)]
    again, fout2, _, _ = run(ctx, W, frags, check=False)
    for k in ("wire_status", "row", "verdict", "eta_idx"):
        assert got[k].tobytes() == again[k].tobytes(), k
    for part in ("rows", "dec"):
        for k in got[part]:
            assert got[part][k].tobytes() == again[part][k].tobytes(), (part, k)
    assert again["etas"] == got["etas"] and again["stats"] == got["stats"] and fout2 == fout


def _forge_fork(ctx, W):
    """Fragment B: the chain without one block of epoch 2 before the freeze point, the rest of
    epoch 2 forged anew on top (same slots and forgers, new links) and epoch 3 forged under B's
    own nonce, the way make_multi_epoch_chain searches each epoch.  Returns (drop, B's items)."""
    from praos_hip import chains
    from praos_hip.chunk import pack_chunk
    data, cfg, s = W["data"], W["cfg"], W["slots"]
    n = len(s)
    drop = next(i for i in range(n) if s[i] >= 2 * EPOCH_LEN + 100)
    p = chains.params(cfg)
    sig = chains.stake(cfg["npools"], cfg["stake_offset"])
    st, tip = W["state_at"](drop)
    items = list(W["items"][:drop])
    sl2, pl2 = data["schedules"][2]
    keep = sl2 > s[drop]
    prev, block_no = tip[2], drop
    ei = data["epoch_info"]
    sl, pl = sl2[keep], pl2[keep]
    for e in (2, 3):
        eta = data["nonces"][2] if e == 2 else cm.cs.combine(st["candidate"], st["leb"])
        if e == 3:
            assert eta != data["nonces"][3]
            lead = ctx.leader_schedule(cfg["seed"], sig, p, eta, e * EPOCH_LEN, EPOCH_LEN)
            idx = np.nonzero(lead >= 0)[0]
            sl, pl = (e * EPOCH_LEN + idx).astype(np.uint64), lead[idx].astype(np.uint32)
        m = len(sl)
        H, _, _ = ctx.synthesize(m, cfg["npools"], p, eta, cfg["seed"], body_len=0, schedule=(sl, pl),
                                 block_no0=block_no, link=True, prev0=prev)
        ctx.set_epoch(eta, data["pools"], p)
        o = ctx.verify_headers(H)
        ph = np.zeros((m, 32), np.uint8)
        ph[0] = np.frombuffer(prev, np.uint8)
        ph[1:] = H["header_hash"][:-1]
        _, stop, _ = ctx.update_chain_dep_state(H, o, ph, st, ei)
        assert stop == m
        a, off, ln = pack_chunk(H)
        items += [wire.wrap(5 + (e == 2), bytes(a[int(x):int(x) + int(y)])) for x, y in zip(off, ln)]
        prev, block_no = bytes(H["header_hash"][-1]), block_no + m
    return drop, items


def test_a_fork_with_its_own_epoch_nonce(ctx, world):
    """A and B share a prefix; B drops a block before an epoch's freeze point, so its next epoch
    runs under another nonce.  Both are fully valid; rows = the shared prefix plus both suffixes."""
    W = world
    n = len(W["items"])
    drop, b_items = _forge_fork(ctx, W)
    g = _genesis_state(W["cfg"]["eta0"])
    got, fout, _, first = run(ctx, W, [(W["items"], g, None), (b_items, g, None)])
    assert int((got["verdict"] != 0).sum()) == 0
    assert [f["chain_stop"] for f in fout] == [n, len(b_items)]
    st = got["stats"]
    assert st["distinct_headers"] == st["rows"] == drop + (n - drop) + (len(b_items) - drop) and st["extra_rows"] == 0
    assert len(got["etas"]) == 5 and got["etas"][:4] == W["data"]["nonces"]
    assert fout[0]["state"] == W["data"]["state"] and fout[1]["state"] != fout[0]["state"]
    assert list(got["row"][first[1]:first[1] + drop]) == list(range(drop))


def test_same_bytes_under_two_nonces(ctx, world):
    """One fragment twice, the second time from a state whose candidate nonce differs: the first
    copy is all valid, the second stops at the first header of the next epoch with VRF_BAD_PROOF,
    and the headers it shares get extra rows."""
    W = world
    n, s = len(W["items"]), W["slots"]
    a = next(i for i in range(n) if s[i] >= EPOCH_LEN + 450)      # epoch 1, after the freeze (slot 1000)
    st, tip = W["state_at"](a)
    st2 = cm.copy_state(st)
    st2["candidate"] = b2b(b"another candidate")
    frag = W["items"][a:]
    got, fout, _, first = run(ctx, W, [(frag, st, tip), (frag, st2, tip)])
    e2 = next(i for i in range(n) if s[i] >= 2 * EPOCH_LEN) - a
    assert fout[0]["chain_stop"] == len(frag) and int((got["verdict"][:len(frag)] != 0).sum()) == 0
    assert (fout[1]["chain_stop"], fout[1]["processed"]) == (e2, e2 + 1)
    assert got["verdict"][first[1] + e2] == abi.V_VRF_BAD_PROOF
    assert set(got["verdict"][first[1] + e2 + 1:]) == {wire.V_NOT_REACHED}
    assert got["stats"]["extra_rows"] > 0 and got["stats"]["distinct_headers"] == len(frag)
    assert got["stats"]["rows"] == len(frag) + got["stats"]["extra_rows"]
    # The second copy's nonce chain runs on as if every header were valid: epoch 2 ticks to its own
    # nonce (extra rows, holding the same decoded headers as their base rows); its candidate nonce is
    # set again inside epoch 2, so epoch 3 ticks to the first copy's nonce and shares its rows.
    e3 = next(i for i in range(n) if s[i] >= 3 * EPOCH_LEN) - a
    assert got["stats"]["extra_rows"] == e3 - e2 and len(got["etas"]) == 4
    for i in range(len(frag)):
        r0, r1 = int(got["row"][i]), int(got["row"][first[1] + i])
        if e2 <= i < e3:
            assert r1 == len(frag) + i - e2 and got["eta_idx"][r0] != got["eta_idx"][r1]
            assert np.array_equal(got["dec"]["kes_sig"][r0], got["dec"]["kes_sig"][r1])
            assert np.array_equal(got["dec"]["signed_body"][r0], got["dec"]["signed_body"][r1])
            assert got["rows"]["bits"][r0] == 0 and got["rows"]["bits"][r1] & abi.BIT_VRF_PROOF
        else:
            assert r1 == r0 == i


def test_a_failure_stops_its_own_fragment_only(ctx, world):
    """A clean fragment beside: a corrupted KES signature in one peer's copy (its own row), a broken
    link (DOESNT_FIT, not ENV_PREV_HASH, even when the block number is wrong too), a wrong block
    number alone (ENV_BLOCK_NO), an era-4 item and a truncated wrapper (INPUT), and empty fragments."""
    W = world
    n, items = len(W["items"]), W["items"]
    g = _genesis_state(W["cfg"]["eta0"])
    lo, hi = 40, 160
    st, tip = W["state_at"](lo)
    base = items[lo:hi]

    def edit(k, f):
        out = list(base)
        out[k] = f(out[k])
        return out

    def flip(at_from_end):
        def f(it):
            b = bytearray(it)
            b[len(b) - at_from_end] ^= 0x40
            return bytes(b)
        return f
    kes = edit(30, flip(100))
    skip = base[:50] + base[51:]                                  # header 51 onto header 49: link and block number
    st5, tip5 = W["state_at"](lo + 5)
    blockno = (base[5:], st5, (tip5[0], tip5[1] - 1, tip5[2]))     # the head's block number off by one
    era4 = edit(20, lambda it: wire.wrap(4, it[wire.unwrap(it)[4]:]))
    trunc = edit(70, lambda it: it[:len(it) - 1])
    frags = [(base, st, tip), (kes, st, tip), ([], g, None), (skip, st, tip), blockno, (era4, st, tip),
             (trunc, st, tip), ([], st, tip), (base, st, tip)]
    got, fout, _, first = run(ctx, W, frags)
    want = {1: (30, abi.V_KES_SIG), 3: (50, wire.V_DOESNT_FIT), 4: (0, abi.V_ENV_BLOCK_NO), 5: (20, abi.V_INPUT),
            6: (70, abi.V_INPUT)}
    for j, f in enumerate(frags):
        v = got["verdict"][first[j]:first[j + 1]]
        if j in want:
            k, code = want[j]
            assert (fout[j]["chain_stop"], fout[j]["processed"]) == (k, k + 1), j
            assert v[k] == code and not v[:k].any() and set(v[k + 1:]) == {wire.V_NOT_REACHED}, j
            st_k, tip_k = W["state_at"](lo + (5 if j == 4 else 0) + k)
            assert fout[j]["state"] == st_k, j
            assert fout[j]["tip"] == (tip_k if j != 4 else f[2]), j
        else:
            assert fout[j]["chain_stop"] == fout[j]["processed"] == len(f[0]) and not v.any(), j
    assert fout[2]["state"] == g and fout[2]["tip"] is None
    # the damaged copies are headers of their own; the era-4 and the truncated item have no row
    assert got["stats"]["distinct_headers"] == len(base) + 1 and got["stats"]["unwrapped"] == got["stats"]["items"] - 2
    assert got["row"][first[5] + 20] == wire.NO_ROW and got["wire_status"][first[6] + 70] == wire.WIRE_SYNTAX
    assert got["row"][first[1] + 30] == len(base)


def test_forecast_horizon_and_no_fragments(ctx, world):
    """view_end_slot in the middle: the items from the first header at or past it are NOT_REACHED,
    nothing failed (chain_stop == processed) and the state is the one before it.  K = 0 is a call."""
    W = world
    n, s = len(W["items"]), W["slots"]
    g = _genesis_state(W["cfg"]["eta0"])
    cut = next(i for i in range(n) if s[i] >= 777)
    got, fout, _, _ = run(ctx, W, [(W["items"][:400], g, None), (W["items"][:cut - 3], g, None)], view_end_slot=777)
    assert (fout[0]["chain_stop"], fout[0]["processed"]) == (cut, cut) and fout[1]["processed"] == cut - 3
    assert not got["verdict"][:cut].any() and set(got["verdict"][cut:400]) == {wire.V_NOT_REACHED}
    st, tip = W["state_at"](cut)
    assert fout[0]["state"] == st and fout[0]["tip"] == tip
    got, fout, _, _ = run(ctx, W, [], check=False)
    assert got["n_rows"] == 0 and got["stats"]["items"] == 0 and len(got["verdict"]) == 0


def test_no_item_unwraps(ctx, world):
    """N > 0 with no row at all: every item fails to unwrap or is of another era.  Each fragment stops
    at its first item with INPUT, nothing is decoded or verified, states and tips stay as they were."""
    W = world
    g = _genesis_state(W["cfg"]["eta0"])
    st, tip = W["state_at"](10)
    era4 = wire.wrap(4, W["hdrs"][10])
    text = bytes.fromhex(wc.golden()["disabled"][0]["wire"])
    frags = [([b"\x00", era4], g, None), ([text, W["items"][10][:-1], era4], st, tip), ([wire.wrap(7, b"x")], st, tip)]
    got, fout, _, first = run(ctx, W, frags)
    assert got["n_rows"] == 0 and got["etas"] == [g["epoch_nonce"], st["epoch_nonce"]][:len(got["etas"])]
    assert got["stats"] == {"items": 6, "unwrapped": 0, "distinct_headers": 0, "rows": 0, "extra_rows": 0}
    assert list(got["row"]) == [wire.NO_ROW] * 6
    assert list(got["wire_status"]) == [wire.WIRE_SYNTAX, wire.WIRE_OK, wire.WIRE_SYNTAX, wire.WIRE_SYNTAX, wire.WIRE_OK,
                                        wire.WIRE_ERA]
    for j, f in enumerate(frags):
        v = list(got["verdict"][first[j]:first[j + 1]])
        assert v == [abi.V_INPUT] + [wire.V_NOT_REACHED] * (len(f[0]) - 1), j
        assert (fout[j]["chain_stop"], fout[j]["processed"]) == (0, 1) and fout[j]["state"] == f[1] and fout[j]["tip"] == f[2]


def test_argument_errors(ctx, world):
    """rows_cap one short: PRAOS_E_ARG and the count needed; the same call with the cap raised
    succeeds.  256 start states that tick to 256 nonces make 256 rows of one header; 257 are refused."""
    W = world
    g = _genesis_state(W["cfg"]["eta0"])
    frags = [(W["items"][:90], g, None), (W["items"][30:120], *W["state_at"](30))]
    with pytest.raises(abi.PraosError) as e:
        run(ctx, W, frags, check=False, rows_cap=119)
    assert (e.value.rc, e.value.n_rows) == (abi.E_ARG, 120)
    got, _, _, _ = run(ctx, W, frags, rows_cap=120)
    assert got["n_rows"] == 120
    n, s = len(W["items"]), W["slots"]
    k = next(i for i in range(n) if s[i] >= EPOCH_LEN)
    st, tip = W["state_at"](k)

    def peers(m):
        out = []
        for j in range(m):
            sj = cm.copy_state(st)
            if j:
                sj["candidate"] = b2b(b"candidate %d" % j)
            out.append((W["items"][k:k + 1], sj, tip))
        return out
    with pytest.raises(abi.PraosError) as e:
        run(ctx, W, peers(257), check=False)
    assert (e.value.rc, e.value.n_etas) == (abi.E_ARG, 257)
    got, fout, _, _ = run(ctx, W, peers(256), check=False)
    assert got["stats"]["distinct_headers"] == 1 and got["n_rows"] == 256 and got["stats"]["extra_rows"] == 255
    assert got["verdict"][0] == 0 and set(got["verdict"][1:]) == {abi.V_VRF_BAD_PROOF}
    with pytest.raises(abi.PraosError):
        ctx.validate_candidates(np.zeros(4, np.uint8), [0], [4], [0, 2], [{"state": g, "tip": None}],
                                W["data"]["epoch_info"], LIMITS)


def test_schedule_independence(world):
    """PRAOS_OPT_CONCURRENT, _KEYCACHE and _DEDUP, each off and on, give identical outputs."""
    import praos_hip
    W = world
    n = len(W["items"])
    frags = [(W["items"][:500], _genesis_state(W["cfg"]["eta0"]), None), (W["items"][200:n], *W["state_at"](200))]
    base = None
    c = praos_hip.Context(0)
    try:
        for opt, off, on in ((abi.OPT_CONCURRENT, 0, 1), (abi.OPT_KEYCACHE, 0, 2), (abi.OPT_DEDUP, 0, 1)):
            for val in (off, on):
                c.set_option(opt, val)
                got, fout, _, _ = run(c, W, frags, check=False)
                flat = ([got[k].tobytes() for k in ("wire_status", "row", "verdict", "eta_idx")] +
                        [got[p][k].tobytes() for p in ("rows", "dec") for k in sorted(got[p])] + [got["etas"], fout])
                if base is None:
                    base = flat
                    assert not got["verdict"].any()
                assert flat == base, (opt, val)
    finally:
        c.close()
