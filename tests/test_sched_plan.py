"""Host check of the run schedule as a value (csrc/sched.hpp): knobs, their environment, the plan.

The header is plain C++17, so the text the host modules include is compiled here with g++ alone and
driven through a small shim.  The plan is compared field by field with a Python restatement of the
rules, written from the scheduler as it stood before the plan existed (the inline conditions of
batch_run_impl / kc_lists / kc_precompute and the predicate methods of the context), not from
sched.hpp: a rule that drifts in the header fails here without a GPU.  The GPU side -- the plan a
432,000-header batch gets, forced onto a small batch -- is tests/test_gpu_group.py::
test_large_batch_plan_equals_default.
"""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

HDR = os.path.join(os.path.dirname(__file__), "..", "ouroboros-consensus_amd", "csrc")

# SchedKnobs, in the shim's order (kc_min as three entries)
KNOBS = ["vrf3", "vrf_prio", "vrf_ilp4", "v_excl", "miss4", "miss_prio", "key4", "u4", "ck4", "kes_dedup",
         "kes_pair", "kes_nocache", "kc_min[0]", "kc_min[1]", "kc_min[2]", "vrf_perkey", "vrf_keys_first",
         "vrf_wide", "vrf_wide_cap", "wide_prio", "pre_join", "v_main", "tp_staged", "key_wave_prio",
         "stream_chunk_v", "pipe_head", "pipe_tail", "pbft_ck_min"]
SHAPE = ["n", "concurrent", "kernels", "keycache", "dedup", "tp_only", "v_done", "pool_keys", "replaying"]
PLAN = ["kc", "dedup", "pk_on", "do_ocert", "do_kes", "do_vrf", "tp_staged", "vrf3", "vm_mode", "v_main", "v_first",
        "wprio_v", "pre_join", "vrf_keys_first", "v_ilp4", "ck4", "miss4", "u4", "key4", "miss_prio", "kes_dd",
        "kes_pair_min", "kes_ck4", "min_uses[0]", "min_uses[1]", "min_uses[2]", "min_uses_store[0]",
        "min_uses_store[1]", "min_uses_store[2]", "wide_min", "vrf_wide_cap", "key_prio", "key_prio_wide",
        "vrf_perkey"]

# the documented defaults (DESIGN, "The schedule as a value")
DEFAULTS = {"vrf3": -1, "vrf_prio": 0, "vrf_ilp4": 120000, "v_excl": 0, "miss4": -1, "miss_prio": -1, "key4": -1,
            "u4": -1, "ck4": 0, "kes_dedup": -1, "kes_pair": -1, "kes_nocache": 58000, "kc_min[0]": 0,
            "kc_min[1]": 0, "kc_min[2]": 0, "vrf_perkey": 1, "vrf_keys_first": 0, "vrf_wide": -1,
            "vrf_wide_cap": 4096, "wide_prio": 1, "pre_join": -1, "v_main": -1, "tp_staged": 1, "key_wave_prio": -1,
            "stream_chunk_v": 1, "pipe_head": 25, "pipe_tail": 100, "pbft_ck_min": 163840}

# environment name -> (knob, kind)
ENV = {"PRAOS_VRF3": ("vrf3", "bool"), "PRAOS_VRF_PRIO": ("vrf_prio", "int"), "PRAOS_VRF_ILP4": ("vrf_ilp4", "int"),
       "PRAOS_V_EXCL": ("v_excl", "int"), "PRAOS_MISS4": ("miss4", "int"), "PRAOS_MISS_PRIO": ("miss_prio", "int"),
       "PRAOS_KEY4": ("key4", "int"), "PRAOS_U4": ("u4", "int"), "PRAOS_CK4": ("ck4", "int"),
       "PRAOS_KES_DEDUP": ("kes_dedup", "int"), "PRAOS_KES_PAIR": ("kes_pair", "int"),
       "PRAOS_KES_NOCACHE": ("kes_nocache", "size"), "PRAOS_KC_MIN": ("kc_min", "int3"),
       "PRAOS_VRF_PERKEY": ("vrf_perkey", "int"), "PRAOS_VRF_KEYS_FIRST": ("vrf_keys_first", "int"),
       "PRAOS_VRF_WIDE": ("vrf_wide", "wide"), "PRAOS_VRF_WIDE_CAP": ("vrf_wide_cap", "wide_cap"),
       "PRAOS_WIDE_PRIO": ("wide_prio", "int"), "PRAOS_PRE_JOIN": ("pre_join", "int"),
       "PRAOS_V_MAIN": ("v_main", "int"), "PRAOS_TP_STAGED": ("tp_staged", "bool"),
       "PRAOS_KEY_PRIO": ("key_wave_prio", "int"), "PRAOS_STREAM_CHUNK_V": ("stream_chunk_v", "int"),
       "PRAOS_PIPE_HEAD": ("pipe_head", "percent"), "PRAOS_PIPE_TAIL": ("pipe_tail", "percent"),
       "PRAOS_PBFT_CK_MIN": ("pbft_ck_min", "size")}


def _shim():
    rd = "\n".join(f"  k.{f} = (std::decay_t<decltype(k.{f})>)v[{i}];" for i, f in enumerate(KNOBS))
    wr = "\n".join(f"  v[{i}] = (long long)k.{f};" for i, f in enumerate(KNOBS))
    sh = "\n".join(f"  s.{f} = (std::decay_t<decltype(s.{f})>)v[{i}];" for i, f in enumerate(SHAPE))
    pl = "\n".join(f"  out[{i}] = (long long)p.{f};" for i, f in enumerate(PLAN))
    return f"""
#include <type_traits>
#include "sched.hpp"
static void knobs_in(SchedKnobs& k, const long long* v) {{
{rd}
}}
static void knobs_out(const SchedKnobs& k, long long* v) {{
{wr}
}}
extern "C" void sp_defaults(long long* v) {{ SchedKnobs k; knobs_out(k, v); }}
extern "C" void sp_from_env(long long* v) {{ SchedKnobs k; sched_knobs_from_env(k); knobs_out(k, v); }}
extern "C" void sp_plan(long m, const long long* knobs, const long long* shapes, long long* outs) {{
  for (long j = 0; j < m; j++) {{
    SchedKnobs k;
    knobs_in(k, knobs + {len(KNOBS)} * j);
    RunShape s;
    const long long* v = shapes + {len(SHAPE)} * j;
{sh}
    const RunPlan p = plan_run(k, s);
    long long* out = outs + {len(PLAN)} * j;
{pl}
  }}
}}
extern "C" int sp_v_ilp4(const long long* knobs, long long n) {{
  SchedKnobs k;
  knobs_in(k, knobs);
  return sched_v_ilp4(k, (size_t)n);
}}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("sched")
    src = d / "shim.cpp"
    src.write_text(_shim())
    so = d / "libsched.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I",
                    os.path.abspath(HDR), str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


# ---- the rules, restated ----------------------------------------------------------------------

def expected_plan(k, s):
    n = s["n"]
    kc_min = [k["kc_min[0]"], k["kc_min[1]"], k["kc_min[2]"]]

    def auto_below(v, cut):
        return v > 0 or (v < 0 and n < cut)

    p = {}
    p["kc"] = s["keycache"] > 0 and n >= 2
    p["dedup"] = bool(s["dedup"]) and n >= 2
    p["pk_on"] = s["keycache"] > 0 and (s["pool_keys"] > 0 or (s["pool_keys"] < 0 and bool(s["replaying"])))
    p["do_ocert"] = bool(s["kernels"] & 1)
    p["do_kes"] = bool(s["kernels"] & 2)
    p["do_vrf"] = bool(s["kernels"] & 4)
    p["tp_staged"] = p["do_vrf"] and bool(s["tp_only"]) and bool(k["tp_staged"])
    p["vrf3"] = p["do_vrf"] and not s["tp_only"] and auto_below(k["vrf3"], 300000)
    p["vm_mode"] = k["v_main"] if k["v_main"] >= 0 else (2 if n < 120000 else 3)
    p["v_main"] = (p["vm_mode"] > 0 and bool(s["concurrent"]) and p["do_vrf"] and not s["tp_only"]
                   and not s["v_done"] and p["vrf3"])
    p["v_first"] = bool(s["concurrent"]) and p["do_vrf"] and (p["tp_staged"] or (not s["tp_only"] and not s["v_done"]))
    p["wprio_v"] = auto_below(k["vrf_prio"], 80000)
    p["pre_join"] = p["vrf3"] and p["kc"] and auto_below(k["pre_join"], 80000)
    p["vrf_keys_first"] = p["vrf3"] and p["kc"] and bool(s["concurrent"]) and bool(k["vrf_keys_first"])
    v_on = k["vrf_ilp4"] == 1 or (k["vrf_ilp4"] > 1 and n < k["vrf_ilp4"])
    p["v_ilp4"] = (2 if k["v_excl"] else 1) if v_on else 0
    for f in ("ck4", "miss4", "u4", "key4"):
        p[f] = auto_below(k[f], 120000)
    p["miss_prio"] = k["miss_prio"] if k["miss_prio"] >= 0 else (0 if n < 60000 else 1)
    p["kes_dd"] = k["kes_dedup"] > 0 or (k["kes_dedup"] < 0 and n >= 400000)
    p["kes_pair_min"] = (k["kes_pair"] & 0xFFFFFFFF) if k["kes_pair"] >= 0 else (0 if s["kernels"] & 5 else 196608)
    p["kes_ck4"] = p["ck4"] and not p["kes_pair_min"] and not p["kes_dd"]
    for t in range(3):
        m = kc_min[t] if kc_min[t] > 0 else s["keycache"]
        if t == 2 and kc_min[2] <= 0 and n < k["kes_nocache"]:
            m = 2**31 - 1
        p[f"min_uses[{t}]"] = m
        p[f"min_uses_store[{t}]"] = 1 if t < 2 else m
    p["wide_min"] = k["vrf_wide"] if k["vrf_wide"] > 0 else (43 if k["vrf_wide"] < 0 and n >= 300000 else 0)
    p["vrf_wide_cap"] = k["vrf_wide_cap"]
    kp = k["key_wave_prio"]
    p["key_prio"] = kp > 0 or (kp < 0 and n < 400000)
    p["key_prio_wide"] = kp > 0 or (kp < 0 and (n < 400000 or bool(k["wide_prio"])))
    p["vrf_perkey"] = k["vrf_perkey"]
    return [int(p[f]) for f in PLAN]


def _plans(lib, cases):
    m = len(cases)
    kn = np.array([[k[f] for f in KNOBS] for k, _ in cases], dtype=np.int64)
    sh = np.array([[int(s[f]) for f in SHAPE] for _, s in cases], dtype=np.int64)
    out = np.zeros((m, len(PLAN)), dtype=np.int64)
    lib.sp_plan(ctypes.c_long(m), kn.ctypes.data_as(ctypes.c_void_p), sh.ctypes.data_as(ctypes.c_void_p),
                out.ctypes.data_as(ctypes.c_void_p))
    return out


def _check(lib, cases):
    got = _plans(lib, cases)
    for (k, s), g in zip(cases, got):
        want = expected_plan(k, s)
        if list(g) != want:
            bad = {f: (int(a), b) for f, a, b in zip(PLAN, g, want) if int(a) != b}
            changed = {f: k[f] for f in KNOBS if k[f] != DEFAULTS[f]}
            raise AssertionError(f"plan (got, want) {bad} for shape {s}, knobs {changed}")


# 1, 2 and both sides of every cut-off, and the headline batch
N_VALUES = [1, 2, 57999, 58000, 59999, 60000, 79999, 80000, 119999, 120000, 196607, 196608, 299999, 300000,
            399999, 400000, 432000]


def _shape(n, concurrent=1, kernels=7, tp_only=0, v_done=0, keycache=2, replaying=0, dedup=1, pool_keys=-1):
    return {"n": n, "concurrent": concurrent, "kernels": kernels, "keycache": keycache, "dedup": dedup,
            "tp_only": tp_only, "v_done": v_done, "pool_keys": pool_keys, "replaying": replaying}


def test_plan_default_knobs_every_shape(lib):
    cases = [(DEFAULTS, _shape(n, cc, kern, tp, vd, kcache, rep))
             for n, cc, kern, tp, vd, kcache, rep in itertools.product(N_VALUES, (0, 1), (7, 2, 5), (0, 1), (0, 1),
                                                                       (0, 2), (0, 1))]
    assert len(cases) == len(N_VALUES) * 96
    _check(lib, cases)
    # the options the cross leaves at their defaults
    _check(lib, [(DEFAULTS, _shape(n, dedup=dd, pool_keys=pk, replaying=rep, keycache=kcache))
                 for n in (1, 2, 54000) for dd in (0, 1) for pk in (-1, 0, 1) for rep in (0, 1) for kcache in (0, 3)])


# every value a knob accepts, -1 (auto, where there is one) and values outside the documented range
TRI = [-1, 0, 1, 2, -7, 100]
KNOB_VALUES = {
    "vrf3": TRI, "vrf_prio": TRI, "v_excl": TRI, "miss4": TRI, "miss_prio": [-1, 0, 1, 3, -7], "key4": TRI, "u4": TRI,
    "ck4": TRI, "kes_dedup": TRI, "vrf_perkey": [0, 1, -1, 2], "vrf_keys_first": [0, 1, -1, 2],
    "wide_prio": [0, 1, -1, 2], "pre_join": TRI, "v_main": [-1, 0, 1, 2, 3, 4, -7], "tp_staged": [0, 1, 2, -1],
    "key_wave_prio": TRI, "vrf_ilp4": [0, 1, 2, -1, 58000, 120000, 300000, 10**9],
    "kes_pair": [-1, 0, 1, 196608, 2**31, -7], "kes_nocache": [0, 1, 2, 58000, 60000, 10**7],
    "kc_min[0]": [0, 1, 3, -1], "kc_min[1]": [0, 1, 3, -1], "kc_min[2]": [0, 1, 3, -1],
    "vrf_wide": [-1, 0, 1, 2, 43, 1000, -7], "vrf_wide_cap": [1, 4096, 65536, 0, -1],
    # not inputs of the plan: it must not move with them
    "stream_chunk_v": [0, 1], "pipe_head": [5, 100], "pipe_tail": [5, 100], "pbft_ck_min": [0, 10**6],
}


@pytest.mark.parametrize("knob", KNOBS)
def test_plan_each_knob(lib, knob):
    shapes = [_shape(n, **kw) for n in N_VALUES
              for kw in ({}, {"concurrent": 0}, {"tp_only": 1}, {"v_done": 1}, {"keycache": 0}, {"kernels": 2},
                         {"kernels": 5}, {"replaying": 1})]
    _check(lib, [(dict(DEFAULTS, **{knob: v}), s) for v in KNOB_VALUES[knob] for s in shapes])


def test_v_ilp4_of_the_pipeline(lib):
    """sched_v_ilp4, which the stored-bytes pipeline calls for its per-chunk stage V, is the plan's v_ilp4"""
    for ilp, excl, n in itertools.product(KNOB_VALUES["vrf_ilp4"], (0, 1), N_VALUES):
        k = dict(DEFAULTS, vrf_ilp4=ilp, v_excl=excl)
        kn = np.array([k[f] for f in KNOBS], dtype=np.int64)
        want = expected_plan(k, _shape(n))[PLAN.index("v_ilp4")]
        assert lib.sp_v_ilp4(kn.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(n)) == want, (ilp, excl, n)


# ---- the environment --------------------------------------------------------------------------

def _atoi(text):
    m = re.match(r"\s*([+-]?\d+)", text)
    return int(m.group(1)) if m else 0


def expected_env(env):
    k = dict(DEFAULTS)
    for name, text in env.items():
        knob, kind = ENV[name]
        v = _atoi(text)
        if kind == "int":
            k[knob] = v
        elif kind == "bool":
            k[knob] = int(v != 0)
        elif kind == "size":
            k[knob] = v
        elif kind == "percent":
            k[knob] = max(5, min(100, v))
        elif kind == "wide":
            k[knob] = -1 if v < 0 else v
        elif kind == "wide_cap":
            k[knob] = 4096 if v < 1 else min(v, 1 << 16)
        elif kind == "int3":                       # "%d,%d,%d": the fields the text leaves out keep their values
            parts = text.split(",")
            for t in range(3):
                if t >= len(parts) or not re.fullmatch(r"\s*[+-]?\d+", parts[t]):
                    break
                k[f"kc_min[{t}]"] = int(parts[t])
    return k


def _from_env(lib, monkeypatch, env):
    for name in list(os.environ):
        if name.startswith("PRAOS_"):
            monkeypatch.delenv(name)
    for name, text in env.items():
        monkeypatch.setenv(name, text)
    v = np.zeros(len(KNOBS), dtype=np.int64)
    lib.sp_from_env(v.ctypes.data_as(ctypes.c_void_p))
    return {f: int(x) for f, x in zip(KNOBS, v)}


ENV_CASES = [{"PRAOS_VRF3": "2"}, {"PRAOS_VRF3": "0"}, {"PRAOS_VRF3": "-1"}, {"PRAOS_TP_STAGED": "0"},
             {"PRAOS_TP_STAGED": "5"}, {"PRAOS_PIPE_HEAD": "1"}, {"PRAOS_PIPE_HEAD": "500"}, {"PRAOS_PIPE_HEAD": "12"},
             {"PRAOS_PIPE_TAIL": "0"}, {"PRAOS_PIPE_TAIL": "101"}, {"PRAOS_PIPE_TAIL": "50"},
             {"PRAOS_KC_MIN": "3,0,5"}, {"PRAOS_KC_MIN": "7"}, {"PRAOS_KC_MIN": "4,9"}, {"PRAOS_KC_MIN": "x"},
             {"PRAOS_VRF_WIDE_CAP": "0"}, {"PRAOS_VRF_WIDE_CAP": "-3"}, {"PRAOS_VRF_WIDE_CAP": "100000"},
             {"PRAOS_VRF_WIDE_CAP": "17"}, {"PRAOS_VRF_WIDE": "-7"}, {"PRAOS_VRF_WIDE": "0"}, {"PRAOS_VRF_WIDE": "2"},
             {"PRAOS_VRF_WIDE": "2", "PRAOS_VRF_WIDE_CAP": "8"}, {"PRAOS_KES_NOCACHE": "0"},
             {"PRAOS_KES_NOCACHE": "5000000000"}, {"PRAOS_PBFT_CK_MIN": "0"}, {"PRAOS_PBFT_CK_MIN": "1000000"},
             {"PRAOS_KES_PAIR": "0"}, {"PRAOS_KES_PAIR": "196608"}, {"PRAOS_KES_PAIR": "-4"},
             {"PRAOS_VRF_ILP4": "300000"}, {"PRAOS_MISS4": "abc"}, {"PRAOS_V_MAIN": " 3"}]
# every plain knob at 0, 1, -1 and a value outside its range
ENV_CASES += [{name: text} for name, (_, kind) in ENV.items() if kind == "int" for text in ("0", "1", "-1", "9")]
# the large-batch plan's environment (tests/test_gpu_group.py), all at once
ENV_CASES += [{"PRAOS_VRF3": "0", "PRAOS_VRF_ILP4": "0", "PRAOS_MISS4": "0", "PRAOS_KEY4": "0", "PRAOS_U4": "0",
               "PRAOS_KES_DEDUP": "1", "PRAOS_KES_NOCACHE": "0", "PRAOS_PRE_JOIN": "0", "PRAOS_KEY_PRIO": "0",
               "PRAOS_MISS_PRIO": "1", "PRAOS_VRF_WIDE": "2"}]


def test_knobs_from_environment(lib, monkeypatch):
    seen = set()
    for env in ENV_CASES:
        got = _from_env(lib, monkeypatch, env)
        assert got == expected_env(env), env
        seen.update(env)
    assert seen == set(ENV)                        # every variable of the table was set at least once
    # the values the issue names, spelled out
    assert _from_env(lib, monkeypatch, {"PRAOS_VRF3": "2"})["vrf3"] == 1
    assert _from_env(lib, monkeypatch, {"PRAOS_PIPE_HEAD": "1"})["pipe_head"] == 5
    assert _from_env(lib, monkeypatch, {"PRAOS_PIPE_HEAD": "500"})["pipe_head"] == 100
    g = _from_env(lib, monkeypatch, {"PRAOS_KC_MIN": "3,0,5"})
    assert [g[f"kc_min[{t}]"] for t in range(3)] == [3, 0, 5]
    assert _from_env(lib, monkeypatch, {"PRAOS_VRF_WIDE_CAP": "0"})["vrf_wide_cap"] == 4096


def test_default_knobs(lib, monkeypatch):
    v = np.zeros(len(KNOBS), dtype=np.int64)
    lib.sp_defaults(v.ctypes.data_as(ctypes.c_void_p))
    assert {f: int(x) for f, x in zip(KNOBS, v)} == DEFAULTS
    assert _from_env(lib, monkeypatch, {}) == DEFAULTS   # nothing set: the environment changes nothing
    # variables that are not the schedule's leave it alone
    assert _from_env(lib, monkeypatch, {}) == _from_env(lib, monkeypatch, {})
    monkeypatch.setenv("PRAOS_POOL_KEYS", "1")
    monkeypatch.setenv("PRAOS_SIDE_PRIO", "111")
    v[:] = 0
    lib.sp_from_env(v.ctypes.data_as(ctypes.c_void_p))
    assert {f: int(x) for f, x in zip(KNOBS, v)} == DEFAULTS
