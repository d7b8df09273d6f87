"""CPU: libpraos_hip.so loads without a GPU and exports every entry point that
include/praos_hip.h declares; the Python binding covers all of them; context
creation fails loudly (no silent CPU fallback) when no device is present."""
import ctypes
import os
import re

import pytest


def _declared():
    from praos_hip import abi
    src = open(abi.HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(praos_[a-z0-9_]+)\s*\(", src))
    return names


def test_header_declares_expected_surface():
    names = _declared()
    for n in ("praos_open", "praos_set_epoch", "praos_verify_headers", "praos_verify_ocert", "praos_verify_kes",
              "praos_verify_vrf", "praos_check_leader", "praos_apply_batch", "praos_synthesize",
              "praos_batch_upload", "praos_batch_run"):
        assert n in names


def test_library_exports_every_declared_symbol():
    from praos_hip import abi
    lib = ctypes.CDLL(abi.LIB_PATH)
    missing = [n for n in _declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_binding_covers_header():
    from praos_hip import abi
    assert _declared() == set(abi.SIGNATURES)


def test_struct_sizes_match_c_layout():
    from praos_hip import abi
    assert ctypes.sizeof(abi.Params) == 40
    assert ctypes.sizeof(abi.Pool) == 76
    assert ctypes.sizeof(abi.Headers) == 15 * 8
    assert ctypes.sizeof(abi.HeaderBytes) == 5 * 8
    assert ctypes.sizeof(abi.Decoded) == 21 * 8


def test_abi_version():
    from praos_hip import abi
    assert abi.load().praos_abi_version() == 15


def test_no_silent_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from praos_hip import abi
    with pytest.raises(abi.PraosError):
        abi.Context(0)


# C struct -> (ctypes class name in praos_hip.abi)
_STRUCTS = {"praos_params": "Params", "praos_pool": "Pool", "praos_headers": "Headers",
            "praos_header_bytes": "HeaderBytes", "praos_out": "Out", "praos_nonce": "Nonce",
            "praos_chain_state": "ChainState", "praos_epoch_info": "EpochInfo", "praos_envelope": "Envelope",
            "praos_replay_stats": "ReplayStats", "praos_decoded": "Decoded", "praos_counters": "Counters",
            "praos_synth_params": "SynthParams", "praos_tpraos_headers": "TPHeaders",
            "praos_tpraos_out": "TPOut", "praos_gen_deleg": "GenDeleg", "praos_overlay": "Overlay",
            "praos_ledger_view": "LedgerView"}
HASKELL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "integration", "haskell",
                       "Ouroboros", "Consensus", "Protocol", "Praos", "Batch.hs")


def _c_layout(tmp_path):
    """sizeof / offsetof of every field, from the C compiler over include/praos_hip.h."""
    import subprocess
    from praos_hip import abi
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "praos_hip.h"', "int main(void) {"]
    for cs, py in _STRUCTS.items():
        S = getattr(abi, py)
        lines.append(f'  printf("{cs} %zu", sizeof({cs}));')
        for name, _ in S._fields_:
            lines.append(f'  printf(" {name}@%zu", offsetof({cs}, {name}));')
        lines.append('  printf("\\n");')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(abi.HEADER_PATH), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {}
    for ln in out.splitlines():
        parts = ln.split()
        lay[parts[0]] = (int(parts[1]), {k: int(v) for k, v in (p.split("@") for p in parts[2:])})
    return lay


def test_ctypes_and_haskell_layouts_match_c(tmp_path):
    """Every ctypes struct of the Python binding and every '-- struct' layout line of the
    Haskell binding (the offsets its pokeByteOff calls use) equal the C compiler's."""
    from praos_hip import abi
    lay = _c_layout(tmp_path)
    for cs, py in _STRUCTS.items():
        S = getattr(abi, py)
        size, offs = lay[cs]
        assert ctypes.sizeof(S) == size, cs
        assert {n: getattr(S, n).offset for n, _ in S._fields_} == offs, cs
    hs = open(HASKELL).read()
    seen = 0
    for m in re.finditer(r"^-- struct (\w+) \((\d+) bytes\): (.*)$", hs, flags=re.M):
        cs, size, fields = m.group(1), int(m.group(2)), m.group(3).split()
        assert lay[cs][0] == size, cs
        for f in fields:
            name, off = f.split("@")
            assert lay[cs][1][name] == int(off), (cs, name)
        seen += 1
    assert seen >= 10


def test_haskell_imports_declared_symbols():
    hs = open(HASKELL).read()
    imported = set(re.findall(r'foreign import ccall safe "(praos_[a-z0-9_]+)"', hs))
    assert imported and imported <= _declared()


def test_option_ids_match_header():
    """praos_set_option ids: the Python constants and the Haskell binding's literal (pool-key
    store, 7) are the header's PRAOS_OPT_* values."""
    from praos_hip import abi
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "praos_hip.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define PRAOS_OPT_([A-Z_]+) (\d+)", hdr)}
    assert ids == {"CONCURRENT": 1, "KERNELS": 2, "KEYCACHE": 3, "DEDUP": 4, "PIPELINE": 5, "KES_PAIR": 6,
                   "POOL_KEYS": 7, "KES_NOCACHE": 8}
    for name, v in ids.items():
        assert getattr(abi, "OPT_" + name) == v, name
    assert "c_set_option p 7" in open(HASKELL).read()


def test_haskell_abi_version_matches_header():
    """Batch.hs checks praos_abi_version against its own constant: it must be the header's."""
    from praos_hip import abi
    hdr = open(abi.HEADER_PATH).read()
    v = int(re.search(r"#define PRAOS_ABI_VERSION (\d+)", hdr).group(1))
    assert re.search(r"^abiVersion = (\d+)$", open(HASKELL).read(), flags=re.M).group(1) == str(v)


def test_haskell_binds_group_entry_points():
    """The Haskell binding reaches several GPUs: the group entry points validateEpochHeaders[TPraos]
    and the replay use (withPraosBatchDevices) are imported."""
    hs = open(HASKELL).read()
    imported = set(re.findall(r'foreign import ccall safe "(praos_[a-z0-9_]+)"', hs))
    for name in ("praos_group_open", "praos_group_close", "praos_group_set_epoch", "praos_group_set_overlay",
                 "praos_group_verify_header_bytes", "praos_group_verify_tpraos_header_bytes",
                 "praos_group_host_register", "praos_group_host_unregister", "praos_group_replay_immutable",
                 "praos_group_replay_immutable_tpraos"):
        assert name in imported, name


def test_tpraos_error_table_matches_haskell():
    """The PRAOS_TPF_* -> ChainTransitionError table of Batch/Errors.hs (tpraosFailureTable, the
    order ValidateAll collects the failures in) and the one ffi_harness.c prints the stopping
    header's errors with are the same list, over the header's PRAOS_TPF_* values, and cover
    every bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "praos_hip.h")).read()
    tpf = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define PRAOS_TPF_([A-Z_]+)\s+0x([0-9a-f]+)u", hdr)}
    errs = open(os.path.join(os.path.dirname(HASKELL), "Batch", "Errors.hs")).read()
    block = errs[errs.index("tpraosFailureTable =") :]
    block = block[: block.index("]")]
    hs = [(int(a, 16), b) for a, b in re.findall(r"\(0x([0-9A-Fa-f]{4}), TP(\w+)\)", block)]
    harness = open(os.path.join(root, "integration", "c", "ffi_harness.c")).read()
    cblock = harness[harness.index("TPF_NAMES[] = {") :]
    cblock = cblock[: cblock.index("};")]
    c = [(tpf[a], b.split()[-1]) for a, b in re.findall(r'\{PRAOS_TPF_([A-Z_]+), "([^"]+)"\}', cblock)]
    assert hs == c
    assert sorted(b for b, _ in hs) == sorted(tpf.values()) and len(hs) == 15
    # the Haskell names carry the ledger constructors' names (TP prefix dropped)
    assert {n for _, n in hs} >= {"KESBeforeStartOCERT", "VRFKeyBadNonce", "WrongGenesisVRFKeyOVERLAY"}


def test_fe_cols_header_is_generated():
    """csrc/fe_cols.hpp (the software-pipelined field products) is exactly what
    tools/gen_fe_cols.py prints: the header is generated, never hand-edited."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "gen_fe_cols.py")], check=True,
                         capture_output=True, text=True).stdout
    with open(os.path.join(root, "ouroboros-consensus_amd", "csrc", "fe_cols.hpp")) as f:
        assert f.read() == out


def test_haskell_binds_abi14_entry_points():
    """ABI 14 reaches the reference side: the per-epoch ledger views of the replay and the
    block-integrity batch (single context and group) are imported by Batch.hs."""
    hs = open(HASKELL).read()
    imported = set(re.findall(r'foreign import ccall safe "(praos_[a-z0-9_]+)"', hs))
    for name in ("praos_replay_immutable_views", "praos_group_replay_immutable_views",
                 "praos_verify_block_integrity", "praos_group_verify_block_integrity"):
        assert name in imported, name
    for fn in ("praosReplayImmutableViews", "verifyChunkIntegrity", "praosHostRegister"):
        assert re.search(rf"^{fn} ::", hs, flags=re.M), fn


def test_db_analyser_patch_wires_the_analysis():
    """integration/haskell/db-analyser.patch adds the AnalysisName constructor, its runAnalysis
    equation, the --benchmark-header-batch flag and the cabal modules; the analysis module exists."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    patch = open(os.path.join(root, "integration", "haskell", "db-analyser.patch")).read()
    added = "\n".join(ln[1:] for ln in patch.splitlines() if ln.startswith("+") and not ln.startswith("+++"))
    assert "| BenchmarkHeaderBatch HeaderBatchArgs" in added
    assert "go (BenchmarkHeaderBatch args)" in added
    assert 'long "benchmark-header-batch"' in added
    assert "Cardano.Tools.DBAnalyser.Analysis.BenchmarkHeaderBatch" in added
    assert "processAll db registry ((,) <$> GetBlock <*> GetRawHeader)" in added
    mod = open(os.path.join(root, "integration", "haskell", "Cardano", "Tools", "DBAnalyser", "Analysis",
                            "BenchmarkHeaderBatch.hs")).read()
    for needle in ("ledgerViewForecastAt", "forecastFor", "tickThenReapply", "validateEpochHeaders",
                   "validateEpochHeadersTPraos", "instance CardanoHardForkConstraints c => HasHeaderBatch (CardanoBlock c)",
                   "praosHostRegister"):
        assert needle in mod, needle


def test_selftest_entry_points_declared_and_bound():
    """The self tests of the field products, group formulas and scalar-multiplication schedules are
    declared next to the other praos_debug_* functions, bound, and reachable from Context; the
    ABI version did not move for them."""
    from praos_hip import abi
    names = _declared()
    for n, method in (("praos_debug_fe_multi", "debug_fe_multi"), ("praos_debug_ge", "debug_ge"),
                      ("praos_debug_msm", "debug_msm")):
        assert n in names and n in abi.SIGNATURES and callable(getattr(abi.Context, method)), n
    assert len(abi.SIGNATURES["praos_debug_ge"][1]) == 7 and len(abi.SIGNATURES["praos_debug_msm"][1]) == 10
    hdr = open(abi.HEADER_PATH).read()
    assert hdr.index("praos_debug_hash_to_curve(") < hdr.index("praos_debug_fe_multi(") < hdr.index("praos_debug_msm(")
    assert int(re.search(r"#define PRAOS_ABI_VERSION (\d+)", hdr).group(1)) == 15


def test_hash_bytes_entry_point_and_argument_checks():
    """praos_debug_hash_bytes is declared after the other self tests, bound with its 11 arguments and
    reachable from Context; the ABI version did not move; its argument checks need no device and
    come before anything is uploaded or launched; its kernels are a module of their own."""
    import numpy as np
    from praos_hip import abi
    assert "praos_debug_hash_bytes" in _declared() and callable(abi.Context.debug_hash_bytes)
    assert len(abi.SIGNATURES["praos_debug_hash_bytes"][1]) == 11
    hdr = open(abi.HEADER_PATH).read()
    assert hdr.index("praos_debug_msm(") < hdr.index("praos_debug_hash_bytes(")
    assert int(re.search(r"#define PRAOS_ABI_VERSION (\d+)", hdr).group(1)) == 15
    mk = open(os.path.join(os.path.dirname(abi.LIB_PATH), "csrc", "Makefile")).read()
    assert re.search(r"^MODS := .*\bk_selftest_hash\b", mk, flags=re.M)
    E_STATE = -4
    LIT = 1 << 63
    c = abi.Context(abi.HOST_ONLY)
    try:
        arena = np.arange(1, 65, dtype=np.uint8)
        u64 = lambda *v: np.array(v, np.uint64)
        u32 = lambda *v: np.array(v, np.uint32)
        u8 = lambda *v: np.array(v, np.uint8)
        out = np.zeros(4 * 64, np.uint8)

        def call(kind, n, off, ln, aux=None, parts=None, h=c.h, a=arena, alen=64):
            return c.L.praos_debug_hash_bytes(h, kind, n, abi.ptr(a), alen, abi.ptr(off, abi.u64p), abi.ptr(ln, abi.u32p),
                                              abi.ptr(aux), abi.ptr(parts, abi.u64p),
                                              len(parts) // 2 if parts is not None else 0, abi.ptr(out))

        assert call(0, 1, u64(0), u32(64), h=None) == abi.E_ARG
        for kind in (-1, 5):
            assert call(kind, 1, u64(0), u32(64)) == abi.E_ARG
        assert call(0, 1, u64(0), u32(64), a=None) == abi.E_ARG               # no arena, but a length
        # well-formed calls get as far as the device check
        assert call(0, 1, u64(0), u32(64)) == E_STATE
        assert call(0, 1, u64(64), u32(0)) == E_STATE
        assert call(1, 1, u64(2), u32(62), aux=u8(2, 9, 9, 0)) == E_STATE
        assert call(2, 1, u64(0, 8, 16, 63), u32(8, 8, 8, 1), aux=u8(4)) == E_STATE
        assert call(3, 1, u64(0), u32(2), parts=u64(0, 64, 0x11, LIT | 8)) == E_STATE
        assert call(4, 1, u64(2), u32(0), parts=u64(0, 64, 0x11, LIT | 1)) == E_STATE   # the empty message
        # off + len > arena_len
        assert call(0, 2, u64(0, 60), u32(64, 5)) == abi.E_ARG
        assert call(0, 1, u64(65), u32(0)) == abi.E_ARG
        assert call(0, 1, u64(2 ** 64 - 1), u32(2)) == abi.E_ARG              # no wrap-around
        assert call(1, 1, u64(60), u32(5), aux=u8(0, 0, 0, 0)) == abi.E_ARG
        assert call(2, 1, u64(0, 8, 16, 63), u32(8, 8, 8, 2), aux=u8(4)) == abi.E_ARG
        # kind 1: off < npre, npre > 2, no aux
        assert call(1, 1, u64(1), u32(5), aux=u8(2, 9, 9, 0)) == abi.E_ARG
        assert call(1, 1, u64(0), u32(5), aux=u8(1, 9, 0, 0)) == abi.E_ARG
        assert call(1, 1, u64(8), u32(5), aux=u8(3, 9, 9, 9)) == abi.E_ARG
        assert call(1, 1, u64(8), u32(5)) == abi.E_ARG
        # kind 2: more than 4 segments
        assert call(2, 1, u64(0, 8, 16, 24), u32(8, 8, 8, 8), aux=u8(5)) == abi.E_ARG
        # kinds 3, 4: a part longer than the arena or outside it, a literal of 0 or 9 bytes, a part
        # list outside the table
        for kind in (3, 4):
            assert call(kind, 1, u64(0), u32(1), parts=u64(0, 65)) == abi.E_ARG
            assert call(kind, 1, u64(0), u32(1), parts=u64(1, 64)) == abi.E_ARG
            assert call(kind, 1, u64(0), u32(1), parts=u64(7, LIT)) == abi.E_ARG
            assert call(kind, 1, u64(0), u32(1), parts=u64(7, LIT | 9)) == abi.E_ARG
            assert call(kind, 1, u64(1), u32(1), parts=u64(0, 8)) == abi.E_ARG
            assert call(kind, 1, u64(0), u32(2), parts=u64(0, 8)) == abi.E_ARG
        assert b"praos_debug_hash_bytes" in c.L.praos_last_error(c.h)
    finally:
        c.close()


def test_debug_int_entry_point_and_argument_checks():
    """praos_debug_int is declared after praos_debug_hash_bytes, bound with its 7 arguments and
    reachable from Context; the ABI version did not move; its argument checks need no device and
    come before anything is uploaded or launched; the kernel sits beside the other self tests."""
    import numpy as np
    from praos_hip import abi
    assert "praos_debug_int" in _declared() and callable(abi.Context.debug_int)
    assert len(abi.SIGNATURES["praos_debug_int"][1]) == 7
    hdr = open(abi.HEADER_PATH).read()
    assert hdr.index("praos_debug_hash_bytes(") < hdr.index("praos_debug_int(")
    assert int(re.search(r"#define PRAOS_ABI_VERSION (\d+)", hdr).group(1)) == 15
    csrc = os.path.join(os.path.dirname(abi.LIB_PATH), "csrc")
    assert "k_selftest_int" in open(os.path.join(csrc, "k_selftest.hpp")).read()
    E_STATE = -4
    c = abi.Context(abi.HOST_ONLY)
    try:
        val = lambda *v: np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in v), np.uint8).copy()
        out = np.zeros(2 * 32, np.uint8)

        def call(op, n, a=None, b=None, cc=None, h=c.h, o=out):
            return c.L.praos_debug_int(h, op, n, abi.ptr(a), abi.ptr(b), abi.ptr(cc), abi.ptr(o))

        one = val(1)
        assert call(0, 1, one, h=None) == abi.E_ARG
        for op in (-1, 9):
            assert call(op, 1, one, one, one) == abi.E_ARG
            assert call(op, 0) == abi.E_ARG
        assert b"praos_debug_int" in c.L.praos_last_error(c.h)
        for op in range(9):                                                   # n = 0 needs no array
            assert call(op, 0) == 0
        # well-formed calls get as far as the device check
        for op in (0, 2, 3, 4, 5, 6, 7):
            assert call(op, 1, one) == E_STATE
        assert call(1, 1, one, one, one) == E_STATE
        assert call(8, 2, val(7, 2 ** 256 - 1), val(2, 65535)) == E_STATE
        assert call(3, 1, val(2 ** 253 - 1)) == E_STATE and call(6, 1, val(2 ** 128 - 1)) == E_STATE
        # null arrays the op reads
        assert call(0, 1) == abi.E_ARG and call(0, 1, one, o=None) == abi.E_ARG
        assert call(1, 1, one, one) == abi.E_ARG and call(1, 1, one, None, one) == abi.E_ARG
        assert call(8, 1, one) == abi.E_ARG
        # preconditions: the recoders' ranges, the divisor's
        for op in (3, 4, 5):
            assert call(op, 2, val(1, 2 ** 253)) == abi.E_ARG
            assert call(op, 1, val(2 ** 255)) == abi.E_ARG
        assert call(6, 2, val(1, 2 ** 128)) == abi.E_ARG and call(6, 1, val(2 ** 255)) == abi.E_ARG
        for k in (0, 1, 65536, 2 ** 32 - 1):
            assert call(8, 2, val(9, 9), val(2, k)) == abi.E_ARG
        assert b"praos_debug_int" in c.L.praos_last_error(c.h)
    finally:
        c.close()
