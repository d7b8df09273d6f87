"""Every kernel a schedule knob selects through the crypto launchers (csrc/launch.hpp: the launchers
compute their grid from the item count and take the key-cache lists as KeyItems / KeyHits) gives the
reference's outputs at the sizes where a grid or a list taken in the wrong place goes wrong: one
lane, one short of / exactly / one over a 256-thread block, and two blocks and a lane; with 6 pools
(every key recurs: the hit lists are full) and with n pools (nearly every key is new: the miss lists
are full).  The reference is the CPU twin; in addition every variant equals the default context on
every output array.  PRAOS_CK4 (k_ocert_ck4, k_kes_ck4) and PRAOS_V_EXCL (k_vrf_v4x) are selected by
no other GPU test.

Caches a variant is asserted to have run both lists of (a hit and a miss counter above 0 in some
case): the VRF key cache in every variant with the key cache on; the KES leaf-key cache where
PRAOS_KES_NOCACHE=0 (below that batch size the plan caches no leaf key: every item a miss); the
cold-key cache in every variant with the key cache on.  Under the OCert dedup that cache sees one
representative per distinct certificate, so a pool's cold key recurs, and is a hit, only where a
corrupted certificate made a second tuple (the chains are seeded: the 6-pool cases have such keys);
with OPT_DEDUP 0 every header is an item and the 6-pool cases' hit list is full, which the PRAOS_CK4
variant runs as well, for k_ocert_ck4."""
from fractions import Fraction

import numpy as np
import pytest

from helpers import _context_under, b2b

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 513)
OUT_KEYS = ("bits", "pool_idx", "beta", "leader", "nonce")
KES_CACHE = {"PRAOS_KES_NOCACHE": "0"}
# (name, environment the context opens under, options set after)
VARIANTS = [
    ("kes_cache", KES_CACHE, {}),
    ("kes_cache_ck4", dict(KES_CACHE, PRAOS_CK4="1"), {}),
    ("kes_cache_ck4_no_dedup", dict(KES_CACHE, PRAOS_CK4="1"), {"OPT_DEDUP": 0}),   # k_ocert_ck4's hit list full
    ("kes_cache_pair2", dict(KES_CACHE, PRAOS_KES_PAIR="2"), {}),
    ("kes_cache_dedup", dict(KES_CACHE, PRAOS_KES_DEDUP="1"), {}),
    ("no_ilp4", {"PRAOS_VRF_ILP4": "0", "PRAOS_MISS4": "0", "PRAOS_KEY4": "0", "PRAOS_U4": "0"}, {}),
    ("v_excl", {"PRAOS_VRF_ILP4": "1", "PRAOS_V_EXCL": "1"}, {}),
    ("two_stage", {"PRAOS_VRF3": "0"}, {}),
    ("two_stage_wide", {"PRAOS_VRF3": "0", "PRAOS_VRF_WIDE": "2"}, {}),
    ("three_kernel_wide", {"PRAOS_VRF3": "1", "PRAOS_VRF_WIDE": "2"}, {}),
    ("no_perkey", {"PRAOS_VRF_PERKEY": "0"}, {}),
    ("no_keycache", {}, {"OPT_KEYCACHE": 0}),
    ("no_dedup", {}, {"OPT_DEDUP": 0}),
    ("serial", {}, {"OPT_CONCURRENT": 0}),
]


def _params():
    from praos_hip import abi, fixed
    return abi.params(c_raw=fixed.active_slot_log(Fraction(1, 2)))


def _pool_list(pools):
    from praos_hip import fixed
    sig = fixed.from_rational(Fraction(1, len(pools)))
    return [(h, v, sig) for h, v in pools]


def _run_resident(c, case):
    """(outputs, key-cache statistics) of one resident run of the case on context c"""
    c.set_epoch(case["eta0"], case["pool_list"], case["p"])
    b = c.upload(case["H"])
    try:
        c.run(b)
        return c.download(b, case["n"]), c.batch_stats(b)
    finally:
        c.free(b)


@pytest.fixture(scope="module")
def praos_cases():
    """The synthesized chains, the CPU twin's outputs and the default context's, computed once."""
    from praos_hip import cpu as C
    p, eta0 = _params(), b2b(b"launch-variants")
    cases = []
    c = _context_under({})
    twin = C.CpuContext(threads=16)
    try:
        for n in SIZES:
            for npools in sorted({6, n}):
                H, pools, corrupted = c.synthesize(n, npools, p, eta0, bytes([n & 0xFF, npools & 0xFF]) * 16,
                                                   first_slot=5000, slot_stride=3, corrupt_per_10000=1500)
                case = {"n": n, "npools": npools, "H": H, "pool_list": _pool_list(pools), "p": p, "eta0": eta0,
                        "corrupted": corrupted}
                twin.set_epoch(eta0, case["pool_list"], p)
                case["twin"] = twin.verify_headers(H)
                case["default"], case["default_stats"] = _run_resident(c, case)
                cases.append(case)
    finally:
        twin.close()
        c.close()
    return cases


def _check_stats(name, env, opts, stats):
    """both lists of every cache the variant uses ran in some case"""
    top = {k: max(s[k] for s in stats) for k in stats[0]}
    print(name, top)
    if opts.get("OPT_KEYCACHE", 1) == 0:
        assert all(v == 0 for v in top.values()), top
        return
    assert top["vrf_hits"] > 0 and top["vrf_misses"] > 0, top
    assert top["cold_hits"] > 0 and top["cold_misses"] > 0, top
    if env.get("PRAOS_KES_NOCACHE") == "0":
        assert top["kes_hits"] > 0 and top["kes_misses"] > 0, top
    if "PRAOS_VRF_WIDE" in env:
        assert top["vrf_wide_keys"] > 0 and top["vrf_wide_hits"] > 0, top


def test_default_equals_cpu_twin(praos_cases):
    for case in praos_cases:
        n, o, t = case["n"], case["default"], case["twin"]
        for k in OUT_KEYS:
            assert np.array_equal(o[k], t[k]), (n, case["npools"], k)
        if n >= 255:
            # (a case without a corrupted header would pass whatever the kernels did)
            assert np.count_nonzero(case["corrupted"]) > 0 and np.count_nonzero(o["bits"]) > 0, (n, case["npools"])
    _check_stats("default", {}, {}, [case["default_stats"] for case in praos_cases])


@pytest.mark.parametrize("name,env,opts", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_variant_equals_reference(praos_cases, name, env, opts):
    from praos_hip import abi
    c = _context_under(env)
    stats = []
    try:
        for opt, value in opts.items():
            c.set_option(getattr(abi, opt), value)
        for case in praos_cases:
            o, st = _run_resident(c, case)
            stats.append(st)
            assert set(o) == set(case["default"])
            for k in o:
                assert np.array_equal(o[k], case["default"][k]), (name, case["n"], case["npools"], k)
            for k in OUT_KEYS:
                assert np.array_equal(o[k], case["twin"][k]), (name, case["n"], case["npools"], k)
    finally:
        c.close()
    _check_stats(name, env, opts, stats)


@pytest.fixture(scope="module")
def tpraos_cases():
    from praos_hip import cpu as C
    p, eta0 = _params(), b2b(b"launch-variants-tpraos")
    cases = []
    c = _context_under({})
    twin = C.CpuContext(threads=16)
    try:
        for n in (256, 257):
            H, pools, corrupted = c.synthesize(n, 6, p, eta0, bytes([n & 0xFF]) * 32, first_slot=5000, slot_stride=3,
                                               corrupt_per_10000=1500, tpraos=True)
            pool_list = _pool_list(pools)
            twin.set_epoch(eta0, pool_list, p)
            c.set_epoch(eta0, pool_list, p)
            cases.append({"n": n, "H": H, "pool_list": pool_list, "p": p, "eta0": eta0, "corrupted": corrupted,
                          "twin": twin.verify_tpraos_headers(H), "default": c.verify_tpraos_headers(H)})
    finally:
        twin.close()
        c.close()
    return cases


@pytest.mark.parametrize("staged", ["1", "0"])
def test_tpraos_variant_equals_reference(tpraos_cases, staged):
    c = _context_under({"PRAOS_TP_STAGED": staged})
    try:
        for case in tpraos_cases:
            c.set_epoch(case["eta0"], case["pool_list"], case["p"])
            o = c.verify_tpraos_headers(case["H"])
            assert set(o) == set(case["default"]) == set(case["twin"])
            for k in o:
                assert np.array_equal(np.asarray(o[k]), np.asarray(case["default"][k])), (staged, case["n"], k)
                assert np.array_equal(np.asarray(o[k]), np.asarray(case["twin"][k])), (staged, case["n"], k)
            assert np.count_nonzero(case["corrupted"]) > 0 and np.count_nonzero(o["bits"]) > 0, case["n"]
    finally:
        c.close()
