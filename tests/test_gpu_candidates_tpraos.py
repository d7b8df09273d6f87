"""GPU: praos_validate_candidates_tpraos -- K candidate fragments of TPraos wire headers (Shelley ..
Alonzo, wire indices 1 to 4) in one call.

The chain is the replay tests' shape (20 pools, f = 1/2, four 600-slot epochs, window 200) forged
with the TPraos rules and TICKN's extra entropy, wrapped at one wire index per epoch.  The checker
is candidates_eras_model.TPraosModel: unwrap and dedup in Python, each fragment folded as the
ChainSync client does with the rules of oracle/tpraos.py, over bits that
praos_verify_tpraos_header_bytes gives under every nonce the fold ticks to."""
import copy
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import candidates_eras_model as cem
import candidates_model as cm
import wire_corpus as wc
from helpers import b2b, corrupt
from praos_hip import abi, wire

pytestmark = pytest.mark.gpu

EPOCHS, EPOCH_LEN, WINDOW = 4, 600, 200
LIMITS = (9, 8, 1400, 90_112)
EXTRA = b2b(b"x")


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
    data = immutable.make_multi_epoch_chain(ctx, cfg, EPOCHS, EPOCH_LEN, WINDOW, tpraos=True, extra_entropy=EXTRA)
    hdrs = _headers(data)
    slots = [int(s) for s in data["slots"]]
    items = [wire.wrap(1 + s // EPOCH_LEN, h) for s, h in zip(slots, hdrs)]      # one wire index per epoch
    M = cem.TPraosModel(ctx, data["pools"], data["params"], data["epoch_info"], LIMITS, extra_entropy=EXTRA)
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


def run(ctx, W, frags, M=None, check=True, extra=EXTRA, **kw):
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
    got = ctx.validate_candidates_tpraos(arena, off, ln, first, fout, W["data"]["epoch_info"], LIMITS,
                                         extra_entropy=extra, **kw)
    if check:
        M.check(items, first, fin, got, fout, kw.get("view_end_slot", 1 << 64))
    return got, fout, items, first


def raw(got, fout):
    parts = [got[k].tobytes() for k in ("wire_status", "row", "verdict", "failures", "eta_idx")]
    parts += [got[p][k].tobytes() for p in ("rows", "dec") for k in sorted(got[p])]
    return b"".join(parts) + repr((got["etas"], got["stats"], fout)).encode()


def _existing_path(ctx, W, n):
    """upload, decode, set_nonces, run, praos_tpraos_validate_headers_nonces over the stored spans"""
    data = W["data"]
    epoch = (data["slots"] // EPOCH_LEN).astype(np.uint8)
    ctx.set_epoch(data["nonces"][0], data["pools"], data["params"])
    b = ctx.upload_tpraos_bytes(data["arena"], data["off"], data["len"])
    try:
        ctx.batch_decode(b)
        D, d = ctx.alloc_decoded(n, abi.TP_SIGNED_STRIDE)
        ctx.check(ctx.L.praos_batch_download_decoded(ctx.h, b, ctypes.byref(d)))
        ctx.set_nonces(b, data["nonces"], epoch)
        ctx.run(b)
        o = ctx.download_tpraos(b, n)
    finally:
        ctx.free(b)
    z = lambda shape, dt: np.zeros(shape, dt)  # noqa: E731
    H = {k: D[k] for k in ("slot", "cold_vk", "vrf_vk", "vrf_out", "vrf_proof", "hot_vk", "ocert_n", "ocert_c0",
                           "ocert_sig", "kes_sig")}
    H.update(body_off=z(n, np.uint64), body_len=z(n, np.uint32), body_bytes=z(8, np.uint8))
    th = abi.TPHeaders()
    th.h = ctx.headers_struct(H)
    lo, lp = z((n, 64), np.uint8), z((n, 80), np.uint8)
    th.leader_out, th.leader_proof = abi.ptr(lo), abi.ptr(lp)           # (the fold does not read them)
    to = abi.TPOut()
    to.bits, to.pool_idx, to.nonce = abi.ptr(o["bits"], abi.u16p), abi.ptr(o["pool_idx"], abi.i32p), abi.ptr(o["nonce"])
    state = _genesis_state(W["cfg"]["eta0"])
    st, hk, cv = abi._state_struct(state, n + 32)
    E = abi.Envelope()
    hs = np.ascontiguousarray(data["len"], dtype=np.uint32)
    E.block_no, E.header_hash = abi.ptr(D["block_no"], abi.u64p), abi.ptr(D["header_hash"])
    E.header_size, E.body_size = abi.ptr(hs, abi.u32p), abi.ptr(D["body_size"], abi.u32p)
    E.tip_is_origin = 1
    E.max_major_pv, E.lv_prot_major, E.max_header_size, E.max_body_size = LIMITS
    ei = abi.EpochInfo(*data["epoch_info"])
    xe = ctx.nonce_array([EXTRA])
    v, fl = z(n, np.uint8), z(n, np.uint16)
    stop, done = ctypes.c_size_t(0), ctypes.c_size_t(0)
    ctx.check(ctx.L.praos_tpraos_validate_headers_nonces(
        ctx.h, ctypes.byref(th), abi.ptr(D["prev_hash"]), abi.ptr(D["prev_is_genesis"]), ctypes.byref(to), ctypes.byref(E),
        ctypes.byref(ei), xe, ctypes.byref(st), ctx.nonce_array(data["nonces"]), len(data["nonces"]), abi.ptr(epoch),
        abi.ptr(v), abi.ptr(fl, abi.u16p), ctypes.byref(stop), ctypes.byref(done)))
    tip = None if E.tip_is_origin else (int(E.tip_slot), int(E.tip_block_no), bytes(E.tip_hash))
    return dict(D=D, o=o, verdict=v, failures=fl, stop=stop.value, done=done.value, tip=tip,
                state=abi._state_from_struct(st, hk, cv))


def test_one_fragment_from_genesis_equals_the_existing_path(ctx, world):
    W, data = world, world["data"]
    n = len(W["items"])
    got, fout, _, _ = run(ctx, W, [(W["items"], _genesis_state(W["cfg"]["eta0"]), None)])
    assert not got["verdict"].any() and not got["failures"].any()
    assert (fout[0]["chain_stop"], fout[0]["processed"]) == (n, n)
    assert got["stats"] == {"items": n, "unwrapped": n, "distinct_headers": n, "rows": n, "extra_rows": 0}
    assert list(got["row"]) == list(range(n)) and got["etas"] == data["nonces"]
    assert fout[0]["state"] == data["state"]
    assert fout[0]["tip"] == (W["slots"][-1], n - 1, bytes(data["header_hash"][-1]))
    x = _existing_path(ctx, W, n)
    assert (x["stop"], x["done"]) == (n, n) and np.array_equal(x["verdict"], got["verdict"])
    assert np.array_equal(x["failures"], got["failures"])
    assert x["state"] == fout[0]["state"] and x["tip"] == fout[0]["tip"]
    for k in ("bits", "pool_idx", "beta_eta", "beta_leader", "nonce"):
        assert np.array_equal(got["rows"][k], x["o"][k]), k
    for k, v in x["D"].items():
        assert np.array_equal(got["dec"][k], v), k


def test_eight_peers_on_the_same_chain(ctx, world):
    W = world
    n, s = len(W["items"]), W["slots"]
    mid1 = next(i for i in range(n) if s[i] >= EPOCH_LEN + 100)           # mid-epoch 1, before the freeze
    frozen = next(i for i in range(n) if s[i] >= 2 * EPOCH_LEN + 450)     # epoch 2, after the freeze (slot 1600)
    mid3 = next(i for i in range(n) if s[i] >= 3 * EPOCH_LEN + 7)
    starts = [300, 0, mid1, 0, frozen, 0, mid3, 0]
    ends = [n, n, n, 700, n, n, n - 5, n]
    frags = [(W["items"][a:b], *W["state_at"](a)) for a, b in zip(starts, ends)]
    got, fout, items, first = run(ctx, W, frags)
    assert not got["verdict"].any()
    for j, (a, b) in enumerate(zip(starts, ends)):
        assert (fout[j]["chain_stop"], fout[j]["processed"]) == (b - a, b - a)
        st, tip = W["state_at"](b)
        assert fout[j]["state"] == st and fout[j]["tip"] == tip
    st = got["stats"]
    assert (st["distinct_headers"], st["rows"], st["extra_rows"]) == (n, n, 0) and st["items"] == sum(ends) - sum(starts)
    want_row = {h: r for r, h in enumerate(list(range(300, n)) + list(range(300)))}
    for j, (a, b) in enumerate(zip(starts, ends)):
        assert list(got["row"][first[j]:first[j + 1]]) == [want_row[h] for h in range(a, b)]
    again, fout2, _, _ = run(ctx, W, frags, check=False)
    assert raw(got, fout) == raw(again, fout2)


@pytest.mark.parametrize("span", ["last-epoch", "past-the-headroom"])
def test_a_second_nonce_for_the_same_bytes_takes_extra_rows(ctx, world, span):
    """two fragments with identical bytes, one from the true state, one from a state whose candidate
    differs: the epochs they tick into run under two nonces, so those headers take extra rows.
    past-the-headroom: more extra rows than the batch's one-eighth headroom (the re-decode path)."""
    W = world
    n, s = len(W["items"]), W["slots"]
    e = 3 if span == "last-epoch" else 1
    a = next(i for i in range(n) if s[i] >= e * EPOCH_LEN - 100)          # after the freeze of epoch e - 1
    first_e = next(i for i in range(n) if s[i] >= e * EPOCH_LEN)
    st, tip = W["state_at"](a)
    other = cm.copy_state(st)
    other["candidate"] = b2b(b"another candidate")
    items = W["items"][a:]
    got, fout, _, first = run(ctx, W, [(items, st, tip), (items, other, tip)])
    # the second fragment ticks into epoch e under another nonce; in epoch e its candidate follows the
    # evolving nonce again, which is the same in both, so the later epochs' nonces agree
    differ = [i for i in range(first_e, n) if s[i] < (e + 1) * EPOCH_LEN]
    assert got["stats"]["extra_rows"] == len(differ) > 0
    assert got["stats"]["distinct_headers"] == n - a and got["n_rows"] == n - a + len(differ)
    if span == "past-the-headroom":
        assert len(differ) > (n - a) // 8 + 64
    for i in differ:
        r0, r1 = got["row"][i - a], got["row"][first[1] + i - a]
        assert r1 >= n - a > r0 and got["eta_idx"][r0] != got["eta_idx"][r1]
    # the true fragment is valid to its end; the other one's first header of epoch e was forged under
    # another nonce (the model agrees on both: run() checks every fragment against it)
    assert not got["verdict"][:first[1]].any() and fout[0]["chain_stop"] == n - a
    assert fout[1]["chain_stop"] == first_e - a and got["verdict"][first[1] + first_e - a] == cem.V_TPRAOS
    assert got["failures"][first[1] + first_e - a] & abi.TPF_BAD_NONCE


def test_extra_entropy_changes_the_nonces(ctx, world):
    W = world
    k = next(i for i in range(len(W["items"])) if W["slots"][i] >= EPOCH_LEN) + 3
    frag = [(W["items"][:k], _genesis_state(W["cfg"]["eta0"]), None)]
    with_x, fx, _, _ = run(ctx, W, frag)
    M0 = cem.TPraosModel(ctx, W["data"]["pools"], W["data"]["params"], W["data"]["epoch_info"], LIMITS, extra_entropy=None)
    without, f0, _, _ = run(ctx, W, frag, M=M0, extra=None)
    assert with_x["etas"][0] == without["etas"][0] == W["cfg"]["eta0"]
    assert with_x["etas"][1] == W["data"]["nonces"][1] != without["etas"][1]
    assert not with_x["verdict"].any()
    # forged under the other nonce: the first header after the tick fails its VRF checks
    assert without["verdict"][k - 3] == cem.V_TPRAOS and without["failures"][k - 3] & abi.TPF_BAD_NONCE
    assert f0[0]["chain_stop"] == k - 3 and fx[0]["chain_stop"] == k


def _mutate(W, i, field, delta=1):
    """header i with one byte of `field` incremented (the reference's Corruption.hs model), wrapped"""
    h = W["hdrs"][i]
    D = W["M"].cols[h]
    needle = bytes(D[field])
    at = h.index(needle)
    assert h.count(needle) == 1
    return wire.wrap(1 + W["slots"][i] // EPOCH_LEN, corrupt(h, at + delta))


def _counter_jump(W, i, by):
    """header i with its certificate's counter raised by `by`, wrapped.  The counter is the CBOR
    uint right after hot_vk's 32 bytes; below 24 it is one byte before and after, so the header
    keeps its length and still decodes."""
    h = W["hdrs"][i]
    D = W["M"].cols[h]
    needle = bytes(D["hot_vk"])
    assert h.count(needle) == 1
    at = h.index(needle) + 32
    n = int(D["ocert_n"])
    assert h[at] == n and n + by < 24
    return wire.wrap(1 + W["slots"][i] // EPOCH_LEN, h[:at] + bytes([n + by]) + h[at + 1:])


def test_each_failure_stops_its_fragment(ctx, world):
    W = world
    W["state_at"](40)                                         # (fills the model's decoded columns)
    base = 20
    st, tip = W["state_at"](base)
    items = W["items"]

    def frag(mid, at=25):
        return (items[base:at] + [mid] + items[at + 1:at + 4], cm.copy_state(st), tip)
    # a counter two above the state's (currentIssueNo: the issuer's last counter, 0 if it has not
    # issued yet; every certificate of the chain carries 0): CounterOverIncrementedOCERT.  The
    # counter is under the cold key's signature and in the KES-signed body, so both signatures fail
    # with it, and ValidateAll collects the three.
    jump = abi.TPF_COUNTER_OVER_INC | abi.TPF_OCERT_SIG | abi.TPF_KES_SIG
    cases = [
        ("eta-proof", frag(_mutate(W, 25, "vrf_proof", 40)), abi.TPF_BAD_NONCE),
        ("leader-proof", frag(_mutate(W, 25, "leader_proof", 40)), abi.TPF_BAD_LEADER),
        ("ocert-sig", frag(_mutate(W, 25, "ocert_sig", 3)), abi.TPF_OCERT_SIG),
        ("kes-sig", frag(_mutate(W, 25, "kes_sig", 100)), abi.TPF_KES_SIG),
        ("counter-jump", frag(_counter_jump(W, 25, 2)), jump),
    ]
    got, fout, _, first = run(ctx, W, [c[1] for c in cases] + [
        (items[base:24] + items[25:28], cm.copy_state(st), tip),                       # does not fit
        (items[base:23] + [wire.wrap(5, W["hdrs"][23])] + items[24:26], cm.copy_state(st), tip),   # a Praos-era item
        (items[base:23] + [items[23][:-1]] + items[24:26], cm.copy_state(st), tip),    # does not unwrap
    ])
    for j, (name, f, fail) in enumerate(cases):
        v = list(got["verdict"][first[j]:first[j + 1]])
        assert v == [0] * 5 + [cem.V_TPRAOS] + [cem.V_NOT_REACHED] * 3, (name, v)
        fl = [int(x) for x in got["failures"][first[j]:first[j + 1]]]
        assert fl[5] & fail and not any(fl[:5] + fl[6:]), (name, fl)
        assert (fout[j]["chain_stop"], fout[j]["processed"]) == (5, 6) and fout[j]["tip"] == W["state_at"](25)[1]
    assert int(got["failures"][first[4] + 5]) == jump                 # the whole set, other bits with it
    c = len(cases)
    assert list(got["verdict"][first[c]:first[c + 1]]) == [0] * 4 + [cem.V_DOESNT_FIT, 255, 255]
    assert list(got["verdict"][first[c + 1]:first[c + 2]]) == [0] * 3 + [12, 255, 255]
    assert list(got["verdict"][first[c + 2]:first[c + 3]]) == [0] * 3 + [12, 255, 255]
    assert got["row"][first[c + 1] + 3] == wire.NO_ROW and got["wire_status"][first[c + 1] + 3] == wire.WIRE_OK
    assert got["wire_status"][first[c + 2] + 3] == wire.WIRE_SYNTAX and not got["failures"][first[c]:].any()


def test_a_counter_out_of_step_is_a_tpraos_failure(ctx, world):
    """a state whose counter for the next issuer is ahead of its certificate's: CounterTooSmallOCERT
    alone (the crypto of the header holds)"""
    W = world
    W["state_at"](40)
    st, tip = W["state_at"](30)
    d = W["M"].dec[W["hdrs"][30]]
    assert d["ocert_n"] >= 0
    st["counters"][d["hk"]] = d["ocert_n"] + 1                    # the header's counter is now too small
    got, fout, _, first = run(ctx, W, [(W["items"][30:34], st, tip)])
    assert list(got["verdict"]) == [cem.V_TPRAOS, 255, 255, 255] and got["failures"][0] == abi.TPF_COUNTER_TOO_SMALL


def test_forecast_horizon_in_mid_fragment(ctx, world):
    W = world
    st, tip = W["state_at"](10)
    horizon = W["slots"][200]
    got, fout, _, _ = run(ctx, W, [(W["items"][10:260], st, tip), (W["items"][:50], _genesis_state(W["cfg"]["eta0"]), None)],
                          view_end_slot=horizon)
    assert (fout[0]["chain_stop"], fout[0]["processed"]) == (190, 190) and fout[1]["processed"] == 50
    assert (fout[0]["state"], fout[0]["tip"]) == W["state_at"](200)
    assert set(got["verdict"][190:250]) == {cem.V_NOT_REACHED} and not got["verdict"][:190].any()


def test_the_installed_overlay_applies(ctx, world):
    """d = 1/2 with three genesis delegates installed on the context: the d = 0 chain's headers in
    overlay slots now fail OVERLAY (NotActiveSlot / WrongGenesisColdKey ...) exactly as
    praos_verify_tpraos_header_bytes judges them on the same context; the fold stops at the first"""
    W = world
    gen = [(b2b(bytes([k]) + b"g", 28), b2b(bytes([k]) + b"d", 28), b2b(bytes([k]) + b"v")) for k in range(3)]
    frags = [(W["items"][a:a + 12], *W["state_at"](a)) for a in (0, 7, 40)]      # (states under d = 0)
    ctx.set_overlay(Fraction(1, 2), W["cfg"]["f"], 0, EPOCH_LEN, gen)
    try:
        M = cem.TPraosModel(ctx, W["data"]["pools"], W["data"]["params"], W["data"]["epoch_info"], LIMITS,
                            extra_entropy=EXTRA, gen_hashes=[g[1] for g in gen])
        got, fout, _, first = run(ctx, W, frags, M=M)
        stops = [f["chain_stop"] for f in fout]
        assert all(f["processed"] == f["chain_stop"] + 1 for f in fout) and max(stops) < 12
        for j, f in enumerate(fout):
            assert got["verdict"][first[j] + stops[j]] == cem.V_TPRAOS
            assert got["failures"][first[j] + stops[j]] & (abi.TPF_NOT_ACTIVE | abi.TPF_GEN_COLD | abi.TPF_GEN_VRF)
    finally:
        ctx.set_overlay(None, None, 0, 1, [])


def test_an_overlay_chain_as_a_fragment(ctx, oracle):
    """a chain forged under d = 1/2, f = 1: the overlay slots by the scheduled genesis delegates (keys
    outside the pool distribution), the other slots by the pools; valid under the installed overlay
    from genesis and from mid-chain (the model: oracle/tpraos.py's failure sets over the context's
    bits), beside a d = 0 fragment over the same slots by the same pools, which stops at its first
    overlay slot; the overlay chain itself stops there with VRFKeyUnknown once the overlay is cleared"""
    import tpraos as tp
    from praos_hip import chains, fixed
    from praos_hip.chunk import pack_chunk
    d, f, length, n = Fraction(1, 2), Fraction(1), 1000, 48
    p = chains.params(dict(f=f, slots_per_kes_period=129600, max_kes_evo=62))
    eta0 = b2b(b"overlay-candidates")
    genesis = [b2b(b"genesis-key" + bytes([k]), 28) for k in range(3)]
    order = sorted(range(3), key=lambda k: genesis[k])                 # Set.elemAt order
    slots = list(range(3, 3 + n))
    cls = [tp.classify(s, d, f, 0, length, 3) for s in slots]
    assert min(cls) >= -1 and cls.count(-1) > 10 and sum(c >= 0 for c in cls) > 10
    forger = [5 + order[c] if c >= 0 else s % 5 for s, c in zip(slots, cls)]
    H, keys, _ = ctx.synthesize(n, 8, p, eta0, b"\x3a" * 32, body_len=0, tpraos=True, link=True, prev0=None, block_no0=0,
                                schedule=(np.array(slots, np.uint64), np.array(forger, np.uint32)))
    pools = [(h, v, fixed.from_rational(Fraction(1, 5))) for h, v in keys[:5]]
    gen = [(genesis[k], keys[5 + k][0], keys[5 + k][1]) for k in range(3)]
    arena, off, ln = pack_chunk(H, era_tag=5)
    items = [wire.wrap(2, bytes(arena[int(o):int(o) + int(m)])) for o, m in zip(off, ln)]
    # the same slots forged as under d = 0: by the five pools alone
    H0, keys0, _ = ctx.synthesize(n, 8, p, eta0, b"\x3a" * 32, body_len=0, tpraos=True, link=True, prev0=None, block_no0=0,
                                  schedule=(np.array(slots, np.uint64), np.array([s % 5 for s in slots], np.uint32)))
    assert keys0 == keys
    arena0, off0, ln0 = pack_chunk(H0, era_tag=5)
    plain = [wire.wrap(2, bytes(arena0[int(o):int(o) + int(m)])) for o, m in zip(off0, ln0)]
    k = next(i for i in range(n) if cls[i] >= 0)                        # the first overlay slot
    ei = (0, 0, length, 300)
    W = {"data": {"nonces": [eta0], "pools": pools, "params": p, "epoch_info": ei}}
    g = _genesis_state(eta0)
    ctx.set_epoch(eta0, pools, p)
    ctx.set_overlay(d, f, 0, length, gen)
    try:
        assert list(ctx.overlay_classify(np.array(slots, np.uint64))) == cls
        M = cem.TPraosModel(ctx, pools, p, ei, LIMITS, extra_entropy=EXTRA, gen_hashes=[x[1] for x in gen])
        mid = M.fold(items[:20], g, None)
        assert mid["chain_stop"] == 20
        got, fout, _, first = run(ctx, W, [(items, g, None), (items[20:], mid["state"], mid["tip"]), (plain, g, None)], M=M)
        assert not got["verdict"][:first[2]].any() and not got["failures"][:first[2]].any()
        assert [f["chain_stop"] for f in fout[:2]] == [n, n - 20] and fout[0]["state"] == fout[1]["state"]
        # the d = 0 fragment in the same call: its pools' headers hold up to the first overlay slot,
        # where a pool's keys are not the scheduled delegate's (the model agrees: run() checks it)
        assert fout[2]["chain_stop"] == k and got["verdict"][first[2] + k] == cem.V_TPRAOS
        assert got["failures"][first[2] + k] & (abi.TPF_GEN_COLD | abi.TPF_GEN_VRF)
        assert not got["verdict"][first[2]:first[2] + k].any()
        assert got["stats"]["distinct_headers"] == len(set(items + plain))    # (every item is deduplicated)
        # the delegates' counters are in the state: currentIssueNo knew them as genesis delegates
        assert {cm.b2b(bytes(H["cold_vk"][i]), 28) for i in range(n) if cls[i] >= 0} <= set(fout[0]["state"]["counters"])
    finally:
        ctx.set_overlay(None, None, 0, 1, [])
    M0 = cem.TPraosModel(ctx, pools, p, ei, LIMITS, extra_entropy=EXTRA)
    got, fout, _, _ = run(ctx, W, [(items, g, None)], M=M0)
    assert fout[0]["chain_stop"] == k and got["verdict"][k] == cem.V_TPRAOS
    assert got["failures"][k] & abi.TPF_VRF_KEY_UNKNOWN


@pytest.mark.parametrize("opt", ["OPT_CONCURRENT", "OPT_KEYCACHE", "OPT_DEDUP"])
def test_options_do_not_change_the_bytes(ctx, world, opt):
    W = world
    frags = [(W["items"][a:a + 150], *W["state_at"](a)) for a in (0, 100, 100)]
    want, fw, _, _ = run(ctx, W, frags, check=False)
    c = abi.Context(0)
    try:
        c.set_option(getattr(abi, opt), 0)
        got, fg, _, _ = run(c, W, frags, check=False)
    finally:
        c.close()
    assert raw(got, fg) == raw(want, fw)


def test_rows_cap_nonce_limit_and_empty_calls(ctx, world):
    W = world
    n = len(W["items"])
    frag = (W["items"][:64], _genesis_state(W["cfg"]["eta0"]), None)
    with pytest.raises(abi.PraosError) as e:
        run(ctx, W, [frag, frag], check=False, rows_cap=63)
    assert e.value.rc == abi.E_ARG and e.value.n_rows == 64
    got, _, _, _ = run(ctx, W, [frag, frag], check=False, rows_cap=64)
    assert got["n_rows"] == 64
    # 257 one-item fragments, each ticking into epoch 1 from a candidate of its own: 257 nonces
    k = next(i for i in range(n) if W["slots"][i] >= EPOCH_LEN)
    st, tip = W["state_at"](k)
    many = []
    for j in range(257):
        s2 = cm.copy_state(st)
        s2["candidate"] = b2b(b"candidate %d" % j)
        many.append((W["items"][k:k + 1], s2, tip))
    with pytest.raises(abi.PraosError) as e:
        run(ctx, W, many, check=False)
    assert e.value.rc == abi.E_ARG and e.value.n_etas == 257
    got, fout, _, _ = run(ctx, W, many[:256], check=False)
    assert got["n_rows"] == 256 and got["stats"]["extra_rows"] == 255 and len(set(got["eta_idx"])) == 256
    got, fout, _, _ = run(ctx, W, [([], st, tip), ([], st, tip)], check=False)          # N = 0
    assert got["n_rows"] == 0 and fout[0]["state"] == st and fout[0]["tip"] == tip
    got, fout, _, _ = run(ctx, W, [], check=False)                                       # K = 0
    assert got["n_rows"] == 0 and got["stats"]["items"] == 0


def test_golden_tpraos_wire_headers(ctx, world):
    """Header_{Shelley,Allegra,Mary,Alonzo} of the reference's golden wire headers, each a one-item
    fragment: the row's decoded columns equal verify_tpraos_header_bytes(decoded=True) on the inner
    span"""
    W = world
    gold = [h for h in wc.golden()["headers"] if 1 <= h["era"] <= 4]
    assert sorted(h["name"] for h in gold) == ["Allegra", "Alonzo", "Mary", "Shelley"]
    items = [bytes.fromhex(h["wire"]) for h in gold]
    frags = [([it], _genesis_state(W["cfg"]["eta0"]), None) for it in items]
    got, fout, _, _ = run(ctx, W, frags, check=False)
    inner = [it[u[4]:u[4] + u[5]] for it, u in ((it, wire.unwrap(it)) for it in items)]
    distinct = list(dict.fromkeys((h["era"], x) for h, x in zip(gold, inner)))
    assert got["n_rows"] == len(distinct)
    ctx.set_epoch(W["data"]["nonces"][0], W["data"]["pools"], W["data"]["params"])
    arena = np.frombuffer(b"".join(x for _, x in distinct), np.uint8)
    ln = np.array([len(x) for _, x in distinct], np.uint32)
    off = (np.cumsum(ln, dtype=np.uint64) - ln).astype(np.uint64)
    o, D = ctx.verify_tpraos_header_bytes(arena, off, ln, decoded=True)
    for k, v in D.items():
        assert np.array_equal(got["dec"][k], v), k
    assert np.array_equal(got["rows"]["nonce"], o["nonce"])       # (of the eta output: no epoch nonce in it)
    assert [int(got["row"][i]) for i in range(4)] == [distinct.index((h["era"], x)) for h, x in zip(gold, inner)]
