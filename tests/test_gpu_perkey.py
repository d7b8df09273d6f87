"""Per-key work done once per key in the cached VRF and KES kernels.

  - VRF: each VRF key-cache entry carries a pool record (k_vrf_keyrec: its representative's cold key,
    pool index and key bits); a wave of the cached stage F (k_vrf_fin / k_vrf_fin_w) or of the join's
    pool part (k_vrf_pool / k_vrf_join) whose cold keys all equal their records' skips the two
    Blake2b hashes and the pool search.  PRAOS_VRF_PERKEY=0 turns the records off.
  - KES: each leaf-key entry's representative walks the Merkle path once (k_kes_merkle_reps); a wave
    of k_kes_ck / k_kes_ck2 whose paths all equal their representatives' skips the walk.
    PRAOS_KES_DEDUP=0 turns it off.

Both fast paths are taken by whole waves only, so the cases are headers that deviate from their
key's other headers: every result is compared bit for bit with oracle.praos_header and with the
same batch run with the cut off.  Each deviant is placed once at the lowest and once at the highest
index of its key, so that it is the entry's representative in one of the two runs whichever end the
cache picks.  512 headers of 4 pools: about 128 hits per key, so every key has at least one wave
on the fast path alone.  The chain starts in KES period 3 (t = 3), so that ocert_c0 can move
without leaving the certificate's range.
"""
import collections
import os
from fractions import Fraction

import numpy as np
import pytest

from helpers import b2b, rbytes, rng

pytestmark = pytest.mark.gpu
FIELDS = ("bits", "pool_idx", "beta", "leader", "nonce")
BITS_FROM_ORACLE = 0x0001 | 0x0002 | 0x0004 | 0x0008 | 0x0010 | 0x0100 | 0x0200 | 0x0400 | 0x0800 | 0x1000
N, NPOOLS = 512, 4
SLOTS_PER_KES_PERIOD = 129600
KES_T = 3                                    # every header's KES period offset in the base chain
BIT_OCERT_SIG, BIT_KES_MERKLE, BIT_KES_LEAF, BIT_KEY_UNKNOWN, BIT_KEY_WRONG = 0x0004, 0x0008, 0x0010, 0x0100, 0x0200


def _hdr(H, i):
    off, ln = int(H["body_off"][i]), int(H["body_len"][i])
    return {"slot": int(H["slot"][i]), "cold_vk": bytes(H["cold_vk"][i]), "vrf_vk": bytes(H["vrf_vk"][i]),
            "vrf_out": bytes(H["vrf_out"][i]), "vrf_proof": bytes(H["vrf_proof"][i]),
            "hot_vk": bytes(H["hot_vk"][i]), "n": int(H["ocert_n"][i]), "c0": int(H["ocert_c0"][i]),
            "ocert_sig": bytes(H["ocert_sig"][i]), "kes_sig": bytes(H["kes_sig"][i]),
            "body": bytes(H["body_bytes"][off:off + ln])}


@pytest.fixture(scope="module")
def base(ctx, oracle):
    """The base chain (as test_gpu_vrf_wide.batch512: 512 headers of 4 pools, 1 % corrupted) and the
    oracle's result for each header, computed once; variants recompute only the headers they edit."""
    from praos_hip import abi, fixed
    c_raw = fixed.active_slot_log(Fraction(1, 20))
    p = abi.params(slots_per_kes_period=SLOTS_PER_KES_PERIOD, max_kes_evo=62, c_raw=c_raw)
    eta0 = b2b(b"per-key")
    H, pools, corrupted = ctx.synthesize(N, NPOOLS, p, eta0, b"\x71" * 32, first_slot=KES_T * SLOTS_PER_KES_PERIOD + 1000,
                                         slot_stride=20, body_len=397, corrupt_per_10000=100)
    sig = [fixed.from_rational(Fraction(1, NPOOLS))] * NPOOLS
    pool_list = [(h, v, s) for (h, v), s in zip(pools, sig)]
    ep = oracle.make_epoch(eta0, SLOTS_PER_KES_PERIOD, 62, c_raw, pool_list)
    ref = [oracle.praos_header(ep, _hdr(H, i)) for i in range(N)]
    return {"H": H, "pool_list": pool_list, "p": p, "eta0": eta0, "ep": ep, "ref": ref, "corrupted": corrupted}


@pytest.fixture(scope="module")
def make_ctx(base):
    """Contexts opened under the given PRAOS_* settings (read when a context is opened), kept for
    the module."""
    import praos_hip
    cache = {}

    def get(**env):
        key = tuple(sorted(env.items()))
        if key not in cache:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update({k: str(v) for k, v in env.items()})
            try:
                c = praos_hip.Context(0)
            finally:
                for k, v in old.items():
                    if v is None:
                        del os.environ[k]
                    else:
                        os.environ[k] = v
            c.set_epoch(base["eta0"], base["pool_list"], base["p"])
            cache[key] = c
        return cache[key]

    yield get
    for c in cache.values():
        c.close()


def _variant(base, oracle, edit):
    """A copy of the base chain with edit(H) applied -> (H, ref, edited indices)."""
    H = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base["H"].items()}
    edited = sorted(edit(H))
    ref = list(base["ref"])
    for i in edited:
        ref[i] = oracle.praos_header(base["ep"], _hdr(H, i))
    return H, ref, edited


def _run(c, H, wide=0):
    c.set_vrf_wide(wide, 0)
    try:
        b = c.upload(H)
        try:
            c.run(b)
            c.sync()
            out = c.download(b, len(H["slot"]))
            st = c.batch_stats(b)
        finally:
            c.free(b)
    finally:
        c.set_vrf_wide()
    return out, st


def _check_oracle(out, ref, pool_list):
    hash_of = {h: i for i, (h, _, _) in enumerate(pool_list)}
    for i, r in enumerate(ref):
        assert int(out["bits"][i]) & BITS_FROM_ORACLE == r["bits"], (i, hex(out["bits"][i]), hex(r["bits"]))
        assert bytes(out["beta"][i]) == r["beta"], i
        assert bytes(out["leader"][i]) == r["leader"], i
        assert bytes(out["nonce"][i]) == r["nonce"], i
        assert int(out["pool_idx"][i]) == hash_of.get(r["issuer_hash"], -1), i
    return len(ref)


def _same(on, off, idx=None):
    for f in FIELDS:
        a, b = (on[f], off[f]) if idx is None else (on[f][idx], off[f][idx])
        np.testing.assert_array_equal(a, b, err_msg=f)
        assert a.tobytes() == b.tobytes(), f
    return len(on["bits"]) if idx is None else len(idx)


# ---------------------------------------------------------------- VRF
def _vrf_groups(base):
    """The registered pools' VRF keys by use: [(vrf_vk, the pool's cold key, sorted header indices)]."""
    H = base["H"]
    registered = {v for _, v, _ in base["pool_list"]}
    by_key = collections.defaultdict(list)
    for i in range(N):
        by_key[bytes(H["vrf_vk"][i])].append(i)
    groups = []
    for vk, idxs in by_key.items():
        if b2b(vk) in registered:
            cold = collections.Counter(bytes(H["cold_vk"][i]) for i in idxs).most_common(1)[0][0]
            groups.append((vk, cold, idxs))
    groups.sort(key=lambda g: -len(g[2]))
    assert len(groups) == NPOOLS and all(len(g[2]) >= 100 for g in groups)
    return groups


def _unregistered_vrf_key(base, oracle):
    """A VRF key that decodes and that no pool registered."""
    r = rng(24)
    registered = {v for _, v, _ in base["pool_list"]}
    while True:
        k = rbytes(r, 32)
        if oracle.decode_ok(k) and b2b(k) not in registered:
            return k


def _vrf_edit(base, oracle, case, place):
    (vk_a, cold_a, idx_a), (_, cold_b, _) = _vrf_groups(base)[:2]
    pick = (lambda k: idx_a[:k]) if place == "lowest" else (lambda k: idx_a[-k:])
    if case == "other_pool_cold":
        return lambda H: [_set(H, "cold_vk", i, cold_b) for i in pick(1)]
    if case == "unknown_cold":
        stray = rbytes(rng(25), 32)
        assert b2b(stray, 28) not in {h for h, _, _ in base["pool_list"]}
        return lambda H: [_set(H, "cold_vk", i, stray) for i in pick(1)]
    assert case == "unregistered_vrf"
    key = _unregistered_vrf_key(base, oracle)
    return lambda H: [_set(H, "vrf_vk", i, key) for i in pick(3)]


def _set(H, field, i, value):
    H[field][i] = np.frombuffer(value, np.uint8)
    return i


def _assert_vrf_deviants(base, H, ref, edited, case):
    """The constructor made what it was asked for: the oracle reports the case's bit on the edited
    headers, and each still shares its VRF key with the headers the case says it does."""
    hash_of = {h: i for i, (h, _, _) in enumerate(base["pool_list"])}
    uses = collections.Counter(bytes(H["vrf_vk"][i]) for i in range(N))
    want = {"other_pool_cold": (1, BIT_KEY_WRONG), "unknown_cold": (1, BIT_KEY_UNKNOWN),
            "unregistered_vrf": (3, BIT_KEY_WRONG)}[case]
    assert len(edited) == want[0]
    for i in edited:
        assert ref[i]["bits"] & (BIT_KEY_WRONG | BIT_KEY_UNKNOWN) == want[1], (case, i, hex(ref[i]["bits"]))
        assert base["ref"][i]["bits"] & (BIT_KEY_WRONG | BIT_KEY_UNKNOWN) == 0, (case, i)
        pool = hash_of.get(ref[i]["issuer_hash"], -1)
        if case == "unregistered_vrf":
            assert uses[bytes(H["vrf_vk"][i])] == 3                      # a cached key of its own
            assert pool == hash_of[base["ref"][i]["issuer_hash"]]
        else:
            assert uses[bytes(H["vrf_vk"][i])] >= 100                    # one header of a cached key
            others = {bytes(H["cold_vk"][j]) for j in range(N)
                      if j != i and bytes(H["vrf_vk"][j]) == bytes(H["vrf_vk"][i]) and not base["corrupted"][j]}
            assert others and bytes(H["cold_vk"][i]) not in others       # ... whose cold key is another
            assert (pool == -1) == (case == "unknown_cold")
            assert pool != hash_of[base["ref"][i]["issuer_hash"]]
    return len(edited)


@pytest.mark.parametrize("place", ["lowest", "highest"])
@pytest.mark.parametrize("case", ["other_pool_cold", "unknown_cold", "unregistered_vrf"])
def test_vrf_deviant_cold_key(case, place, base, make_ctx, oracle):
    H, ref, edited = _variant(base, oracle, _vrf_edit(base, oracle, case, place))
    deviants = _assert_vrf_deviants(base, H, ref, edited, case)
    compared = runs = 0
    for vrf3 in (1, 0):                       # three-kernel form (k_vrf_pool / k_vrf_join) | fused (k_vrf_fin*)
        on_ctx = make_ctx(PRAOS_VRF3=vrf3, PRAOS_VRF_PERKEY=1)
        off_ctx = make_ctx(PRAOS_VRF3=vrf3, PRAOS_VRF_PERKEY=0)
        for wide in (2, 0):
            on, st = _run(on_ctx, H, wide)
            off, _ = _run(off_ctx, H, wide)
            assert st["vrf_hits"] >= N - 32 and (st["vrf_wide_hits"] >= N - 32) == (wide == 2), st
            compared += _same(on, off)
            compared += _check_oracle(on, ref, base["pool_list"])
            _check_oracle(off, ref, base["pool_list"])
            runs += 1
    assert runs == 4 and compared == 2 * N * runs and deviants == (3 if case == "unregistered_vrf" else 1)


# ---------------------------------------------------------------- KES
def _kes_group(base):
    """The headers of the most used KES path (one pool, one KES period: one leaf key), sorted."""
    H = base["H"]
    by_path = collections.defaultdict(list)
    for i in range(N):
        by_path[bytes(H["hot_vk"][i]) + bytes(H["kes_sig"][i][64:])].append(i)
    idxs = max(by_path.values(), key=len)
    assert len(idxs) >= 100
    for i in idxs:
        assert int(H["slot"][i]) // SLOTS_PER_KES_PERIOD - int(H["ocert_c0"][i]) == KES_T
    return idxs


def _unselected_sibling(t, depth):
    """Offset in the KES signature of the vk the walk does not select at `depth` (6 = the root's pair)."""
    for d in range(6, depth, -1):
        T = 1 << (d - 1)
        t = t - T if t >= T else t
    right = t >= (1 << (depth - 1))
    return 64 + 64 * (depth - 1) + (0 if right else 32)


def _kes_edit(base, case, place):
    idxs = _kes_group(base)
    pick = (lambda k: idxs[:k]) if place == "lowest" else (lambda k: idxs[-k:])
    if case == "sibling_flips":               # one header per depth
        def edit(H):
            for depth, i in zip(range(1, 7), pick(6)):
                H["kes_sig"][i][_unselected_sibling(KES_T, depth) + 5] ^= 0x40
            return pick(6)
        return edit
    if case == "hot_vk":
        def edit(H):
            H["hot_vk"][pick(1)[0]][0] ^= 1
            return pick(1)
        return edit
    step = {"c0_plus_1": 1, "c0_plus_2": 2}[case]

    def edit(H):
        H["ocert_c0"][pick(1)[0]] += step
        return pick(1)
    return edit


def _kes_bit(case):
    """The bit the oracle must report on the case's headers.  t = 2 walks to the other leaf of the
    same depth-1 pair (the path holds, the signature is not that leaf's); every other case breaks a
    hash of the walk."""
    return BIT_KES_LEAF if case == "c0_plus_1" else BIT_KES_MERKLE


def _assert_kes_deviants(base, H, ref, edited, case):
    idxs = _kes_group(base)
    bit = _kes_bit(case)
    rest = [i for i in idxs if i not in edited]
    path = lambda i: bytes(H["kes_sig"][i][64:])
    t_of = lambda i: int(H["slot"][i]) // SLOTS_PER_KES_PERIOD - int(H["ocert_c0"][i])
    assert len(edited) == (6 if case == "sibling_flips" else 1) and len(rest) >= 90
    for i in edited:
        assert base["ref"][i]["bits"] & (BIT_KES_MERKLE | BIT_KES_LEAF) == 0, (case, i)
        assert ref[i]["bits"] & (BIT_KES_MERKLE | BIT_KES_LEAF) == bit, (case, i, hex(ref[i]["bits"]))
        if case == "sibling_flips":           # the same hot key and period, another path
            assert path(i) != path(rest[0]) and bytes(H["hot_vk"][i]) == bytes(H["hot_vk"][rest[0]])
            assert sum(a != b for a, b in zip(path(i), path(rest[0]))) == 1
        elif case == "hot_vk":                # the same path and period under another hot key
            assert path(i) == path(rest[0]) and bytes(H["hot_vk"][i]) != bytes(H["hot_vk"][rest[0]])
            assert ref[i]["bits"] & BIT_OCERT_SIG
        else:                                  # the same bytes, another period offset
            assert path(i) == path(rest[0]) and bytes(H["hot_vk"][i]) == bytes(H["hot_vk"][rest[0]])
            assert 0 <= t_of(i) != t_of(rest[0]) == KES_T
            assert ref[i]["bits"] & BIT_OCERT_SIG
    for i in rest:                             # nobody else changed
        assert ref[i]["bits"] == base["ref"][i]["bits"]
    return len(edited)


# c0_plus_1 is the case as stated (t = 2 selects the other leaf of the depth-1 pair, so the header
# leaves its key's entry); c0_plus_2 (t = 1) keeps the leaf key: same entry, same bytes, another t
@pytest.mark.parametrize("place", ["lowest", "highest"])
@pytest.mark.parametrize("case", ["sibling_flips", "hot_vk", "c0_plus_1", "c0_plus_2"])
def test_kes_deviant_path(case, place, base, make_ctx, oracle):
    from praos_hip import abi
    H, ref, edited = _variant(base, oracle, _kes_edit(base, case, place))
    deviants = _assert_kes_deviants(base, H, ref, edited, case)
    on_ctx = make_ctx(PRAOS_KES_NOCACHE=0, PRAOS_KES_DEDUP=1)
    off_ctx = make_ctx(PRAOS_KES_NOCACHE=0, PRAOS_KES_DEDUP=0)
    compared = runs = 0
    try:
        for pair in (2, 0):                   # k_kes_ck2 (two headers per lane from 2 hits on) | k_kes_ck
            for c in (on_ctx, off_ctx):
                c.set_option(abi.OPT_KES_PAIR, pair)
            on, st = _run(on_ctx, H)
            off, _ = _run(off_ctx, H)
            assert st["kes_hits"] >= N - 32, st
            compared += _same(on, off)
            compared += _check_oracle(on, ref, base["pool_list"])
            _check_oracle(off, ref, base["pool_list"])
            for i in edited:
                assert int(on["bits"][i]) & (BIT_KES_MERKLE | BIT_KES_LEAF) == _kes_bit(case)
            runs += 1
    finally:
        for c in (on_ctx, off_ctx):
            c.set_option(abi.OPT_KES_PAIR, -1)
    assert runs == 2 and compared == 2 * N * runs and deviants == len(edited)


# ---------------------------------------------------------------- one deviant lane in a uniform wave
def test_mixed_wave_neighbours(base, make_ctx, oracle):
    """One VRF deviant and one KES deviant, each in the middle of its key's headers (the hit lists are
    grouped by key, so its wave's other lanes are uniform): the whole wave leaves the fast path, and
    the other headers of the key come out byte for byte as with the cut off."""
    from praos_hip import abi
    (vk_a, cold_a, idx_a), (_, cold_b, _) = _vrf_groups(base)[:2]
    kes_idx = _kes_group(base)
    v_dev, k_dev = idx_a[len(idx_a) // 2], kes_idx[len(kes_idx) // 2]

    def edit(H):
        _set(H, "cold_vk", v_dev, cold_b)
        H["kes_sig"][k_dev][_unselected_sibling(KES_T, 3) + 9] ^= 0x02
        return {v_dev, k_dev}
    H, ref, edited = _variant(base, oracle, edit)
    assert ref[v_dev]["bits"] & BIT_KEY_WRONG and not base["ref"][v_dev]["bits"] & BIT_KEY_WRONG
    assert ref[k_dev]["bits"] & BIT_KES_MERKLE and not base["ref"][k_dev]["bits"] & BIT_KES_MERKLE
    v_nb = np.array([i for i in idx_a if i != v_dev])
    k_nb = np.array([i for i in kes_idx if i != k_dev])
    assert len(v_nb) >= 100 and len(k_nb) >= 100
    neighbours = 0
    for vrf3 in (0, 1):
        on, st = _run(make_ctx(PRAOS_VRF3=vrf3, PRAOS_VRF_PERKEY=1), H)
        off, _ = _run(make_ctx(PRAOS_VRF3=vrf3, PRAOS_VRF_PERKEY=0), H)
        assert st["vrf_hits"] >= N - 32
        neighbours += _same(on, off, v_nb)
        _same(on, off)
        _check_oracle(on, ref, base["pool_list"])
        assert int(on["bits"][v_dev]) & BIT_KEY_WRONG and not np.any(on["bits"][v_nb] & BIT_KEY_WRONG)
    on_ctx = make_ctx(PRAOS_KES_NOCACHE=0, PRAOS_KES_DEDUP=1)
    off_ctx = make_ctx(PRAOS_KES_NOCACHE=0, PRAOS_KES_DEDUP=0)
    try:
        for pair in (0, 2):
            for c in (on_ctx, off_ctx):
                c.set_option(abi.OPT_KES_PAIR, pair)
            on, st = _run(on_ctx, H)
            off, _ = _run(off_ctx, H)
            assert st["kes_hits"] >= N - 32
            neighbours += _same(on, off, k_nb)
            _same(on, off)
            _check_oracle(on, ref, base["pool_list"])
            assert int(on["bits"][k_dev]) & BIT_KES_MERKLE and not np.any(on["bits"][k_nb] & BIT_KES_MERKLE)
    finally:
        for c in (on_ctx, off_ctx):
            c.set_option(abi.OPT_KES_PAIR, -1)
    assert neighbours == 2 * len(v_nb) + 2 * len(k_nb)
