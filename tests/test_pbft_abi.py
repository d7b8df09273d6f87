"""CPU: the PBFT surface of the ABI.  The four structs have the C compiler's layout in the ctypes
binding, the bits and verdict values agree with the header and with tests/pbft_model.py, the
build reaches the new module, and bad arguments and a host-only context are refused before
anything touches a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pbft_model as pm
from praos_hip import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_STATE = -4
STRUCTS = {"praos_pbft_params": abi.PbftParams, "praos_pbft_out": abi.PbftOut, "praos_pbft_tip": abi.PbftTip,
           "praos_pbft_state": abi.PbftStateC}
CONSTS = ("PRAOS_PBFT_BIT_DECODE", "PRAOS_PBFT_BIT_SIG", "PRAOS_PBFT_BIT_NOT_DELEGATE", "PRAOS_V_INPUT",
          "PRAOS_V_ENV_BLOCK_NO", "PRAOS_V_ENV_SLOT_NO", "PRAOS_V_ENV_PREV_HASH", "PRAOS_V_TPRAOS",
          "PRAOS_V_PBFT_INVALID_SIG", "PRAOS_V_PBFT_INVALID_SLOT", "PRAOS_V_PBFT_NOT_DELEGATE", "PRAOS_V_PBFT_EXCEEDED",
          "PRAOS_V_ENV_EBB_IN_SLOT", "PRAOS_ABI_VERSION")


def test_struct_layouts_and_constants(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "praos_hip.h"', "int main(void) {"]
    for cname, st in STRUCTS.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for name, _ in st._fields_:
            lines.append(f'  printf(" {name}@%zu", offsetof({cname}, {name}));')
        lines.append('  printf("\\n");')
    lines.append('  printf("consts' + " %d" * len(CONSTS) + '\\n", ' + ", ".join(f"(int){c}" for c in CONSTS) + ");")
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(abi.HEADER_PATH), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    for line, (cname, st) in zip(out, STRUCTS.items()):
        parts = line.split()
        assert parts[0] == cname and int(parts[1]) == ctypes.sizeof(st), cname
        assert {k: int(v) for k, v in (p.split("@") for p in parts[2:])} == \
            {n: getattr(st, n).offset for n, _ in st._fields_}, cname
    assert ctypes.sizeof(abi.PbftParams) == 32 and ctypes.sizeof(abi.PbftTip) == 56
    # the Haskell binding's offsets: its "layout-pbft" lines are the C compiler's, and
    # validatePBftHeaderBatch allocates and pokes by them
    hs = open(os.path.join(ROOT, "integration", "haskell", "Ouroboros", "Consensus", "Protocol", "Praos", "Batch.hs")).read()
    seen = {}
    for m in re.finditer(r"^-- layout-pbft (\w+) \((\d+) bytes\): (.*)$", hs, flags=re.M):
        seen[m.group(1)] = (int(m.group(2)), {f.split("@")[0]: int(f.split("@")[1]) for f in m.group(3).split()})
    assert set(seen) == set(STRUCTS)
    for cname, st in STRUCTS.items():
        assert seen[cname] == (ctypes.sizeof(st), {n: getattr(st, n).offset for n, _ in st._fields_}), cname
    body = hs[hs.index("validatePBftHeaderBatch ctx@(PraosBatchCtx p)"):hs.index("-- ---------------------------------------------------------------- errors")]
    for var, cname in (("prm", "praos_pbft_params"), ("out", "praos_pbft_out"), ("tp", "praos_pbft_tip"),
                       ("stp", "praos_pbft_state")):
        size, offs = seen[cname]
        assert f"allocaBytes {size} $ \\{var} ->" in body, cname
        for name, off in offs.items():
            if not name.startswith("pad_") or cname == "praos_pbft_params":
                assert re.search(rf"(poke|peek)ByteOff {var} {off}\b", body) or \
                    re.search(rf"castPtr {var} `plusPtr` {off}\b", body), (cname, name)
    vals = [int(x) for x in out[len(STRUCTS)].split()[1:]]
    assert vals == [abi.PBFT_BIT_DECODE, abi.PBFT_BIT_SIG, abi.PBFT_BIT_NOT_DELEGATE, abi.V_INPUT, abi.V_ENV_BLOCK_NO,
                    abi.V_ENV_SLOT_NO, abi.V_ENV_PREV_HASH, 19, abi.V_PBFT_INVALID_SIG, abi.V_PBFT_INVALID_SLOT,
                    abi.V_PBFT_NOT_DELEGATE, abi.V_PBFT_EXCEEDED, abi.V_ENV_EBB_IN_SLOT, 15]
    assert vals[8:13] == [20, 21, 22, 23, 24]                       # after the ones in use, nothing renumbered
    assert (pm.BIT_DECODE, pm.BIT_SIG, pm.BIT_NOT_DELEGATE) == tuple(vals[:3])
    assert (pm.V_INPUT, pm.V_ENV_BLOCK_NO, pm.V_ENV_SLOT_NO, pm.V_ENV_PREV_HASH) == tuple(vals[3:7])
    assert (pm.V_INVALID_SIG, pm.V_INVALID_SLOT, pm.V_NOT_DELEGATE, pm.V_EXCEEDED, pm.V_EBB_IN_SLOT) == tuple(vals[8:13])


def test_the_build_reaches_the_new_module():
    lib = abi.load()
    for f in ("praos_byron_key_hash", "praos_verify_pbft_headers", "praos_pbft_update_chain_dep_state",
              "praos_pbft_state_encode", "praos_pbft_state_decode", "praos_pbft_stats"):
        assert hasattr(lib, f) and f in abi.SIGNATURES, f
    mk = open(os.path.join(ROOT, "ouroboros-consensus_amd", "csrc", "Makefile")).read()
    assert re.search(r"^MODS := .*\bk_pbft\b.*\bpraos_pbft\b", mk, flags=re.M) and re.search(r"for m in .*\bk_pbft\b", mk)
    assert re.search(r"^HDRS := .*\bsha3\.hpp\b", mk, flags=re.M) and re.search(r"^HDRS := .*\bbyron_dev\.hpp\b", mk, flags=re.M)
    hdr = open(abi.HEADER_PATH).read()
    for pin in ("Protocol/PBFT.hs:320-353", "Protocol/PBFT/State.hs:206-228", "Protocol/PBFT/State.hs:277-305",
                "Byron/Ledger/PBFT.hs:43-69", "Byron/Ledger/HeaderValidation.hs:39-75", "HeaderValidation.hs:297-344"):
        assert pin in hdr, pin


def _args(n=1):
    arena = np.zeros(100, np.uint8)
    hb = abi.Context.header_bytes_struct(arena, np.zeros(n, np.uint64), np.full(n, 10, np.uint32))
    H = {name: np.zeros((n,) + shp, dt) for name, dt, shp in abi.PBFT_OUT_FIELDS}
    return arena, hb, H, abi.Context._pbft_out(H), np.zeros(n, np.uint8), abi.Context.pbft_params(10, 4, 40, 1)


def test_argument_checks_need_no_device():
    c = abi.Context(abi.HOST_ONLY)
    try:
        L = c.L
        arena, hb, H, o, ebb, p = _args()
        R = np.random.default_rng(5)
        d = R.integers(0, 256, (3, 56), dtype=np.uint8)
        ok = (ctypes.byref(hb), abi.ptr(ebb), ctypes.byref(p), abi.ptr(d), 3, ctypes.byref(o))
        assert L.praos_verify_pbft_headers(None, *ok) == abi.E_ARG
        assert L.praos_verify_pbft_headers(c.h, *ok) == E_STATE           # the per-header half needs a device
        assert L.praos_verify_pbft_headers(c.h, None, *ok[1:]) == abi.E_ARG
        assert L.praos_verify_pbft_headers(c.h, ok[0], None, *ok[2:]) == abi.E_ARG
        p0 = abi.Context.pbft_params(10, 4, 0, 1)                           # epoch_slots 0
        assert L.praos_verify_pbft_headers(c.h, ok[0], ok[1], ctypes.byref(p0), *ok[3:]) == abi.E_ARG
        # a span outside the arena
        hb2 = abi.Context.header_bytes_struct(arena, np.array([95], np.uint64), np.array([10], np.uint32))
        assert L.praos_verify_pbft_headers(c.h, ctypes.byref(hb2), *ok[1:]) == abi.E_ARG
        # a duplicate in either column of the Bimap
        for col in (0, 28):
            dd = d.copy()
            dd[2, col:col + 28] = dd[0, col:col + 28]
            args = (ctypes.byref(hb), abi.ptr(ebb), ctypes.byref(p), abi.ptr(dd), 3, ctypes.byref(o))
            assert L.praos_verify_pbft_headers(c.h, *args) == abi.E_ARG
            tip, st = abi.PbftTip(), abi.PbftStateC(10, 0, abi.ptr(np.zeros(10, np.uint64), abi.u64p),
                                                     abi.ptr(np.zeros((10, 28), np.uint8)))
            tip.origin = 1
            v, stop = np.zeros(1, np.uint8), ctypes.c_size_t(0)
            assert L.praos_pbft_update_chain_dep_state(c.h, 1, ctypes.byref(o), abi.ptr(ebb), ctypes.byref(p),
                                                       abi.ptr(dd), 3, ctypes.byref(tip), ctypes.byref(st), abi.ptr(v),
                                                       None, ctypes.byref(stop)) == abi.E_ARG
        # the fold: a state larger than the window, a window larger than the state's capacity, a
        # gk_idx outside the map
        ss, sh = np.zeros(12, np.uint64), np.zeros((12, 28), np.uint8)
        tip = abi.PbftTip()
        tip.origin = 1
        v, stop = np.zeros(1, np.uint8), ctypes.c_size_t(0)

        def fold(st, Hx=H):
            ox = abi.Context._pbft_out(Hx)
            return L.praos_pbft_update_chain_dep_state(c.h, 1, ctypes.byref(ox), abi.ptr(ebb), ctypes.byref(p), abi.ptr(d),
                                                       3, ctypes.byref(tip), ctypes.byref(st), abi.ptr(v), None,
                                                       ctypes.byref(stop))
        assert fold(abi.PbftStateC(12, 11, abi.ptr(ss, abi.u64p), abi.ptr(sh))) == abi.E_ARG
        assert fold(abi.PbftStateC(9, 0, abi.ptr(ss, abi.u64p), abi.ptr(sh))) == abi.E_ARG
        # window_size 0: no window the reference's append could keep a signer in
        p10, p = p, abi.Context.pbft_params(0, 4, 40, 1)
        assert fold(abi.PbftStateC(12, 0, abi.ptr(ss, abi.u64p), abi.ptr(sh))) == abi.E_ARG
        p = p10
        assert L.praos_pbft_stats(c.h, None) == abi.E_ARG
        assert L.praos_pbft_stats(None, abi.ptr(np.zeros(4, np.uint32), abi.u32p)) == abi.E_ARG
        assert c.pbft_stats() == {"cache": False, "keys_cached": 0, "cached_verifies": 0, "uncached_verifies": 0}
        H2 = {k: a.copy() for k, a in H.items()}
        H2["gk_idx"][0] = 3
        assert fold(abi.PbftStateC(12, 0, abi.ptr(ss, abi.u64p), abi.ptr(sh)), H2) == abi.E_ARG
        H2["gk_idx"][0] = 2
        H2["prev_is_genesis"][0] = 1
        assert fold(abi.PbftStateC(12, 0, abi.ptr(ss, abi.u64p), abi.ptr(sh)), H2) == 0 and v[0] == 0
        # the key hash and the codec refuse null pointers
        assert L.praos_byron_key_hash(c.h, None, 1, abi.ptr(np.zeros(28, np.uint8))) == abi.E_ARG
        assert L.praos_byron_key_hash(None, abi.ptr(np.zeros(64, np.uint8)), 1, abi.ptr(np.zeros(28, np.uint8))) == abi.E_ARG
        assert L.praos_pbft_state_decode(None, 0, ctypes.byref(abi.PbftStateC())) == abi.E_ARG
        assert L.praos_pbft_state_encode(None, None, 0, None) == abi.E_ARG
        # a decode into too small a state reports the count
        small = abi.PbftStateC(2, 0, abi.ptr(ss, abi.u64p), abi.ptr(sh))
        raw = np.frombuffer(bytes.fromhex("8201a1581c" + "ab" * 28 + "9f04030201ff"), np.uint8).copy()
        assert L.praos_pbft_state_decode(abi.ptr(raw), len(raw), ctypes.byref(small)) == abi.E_ARG and small.n == 4
        with pytest.raises(abi.PraosError):
            c.verify_pbft_headers(arena, [0], [10], [0], p, [])
    finally:
        c.close()
