"""CPU: the TPraos and Byron candidates surface of the ABI (praos_validate_candidates_tpraos,
praos_validate_candidates_pbft).  The new structs have the C compiler's layout in the ctypes binding (praos_hip.wire) and in the Haskell binding's
"layout-eras" lines, a host-only context and bad arguments are refused before anything touches a
device, and the checker of the GPU tests (tests/candidates_eras_model.py) agrees with
pbft_model.fold on an intact chain."""
import ctypes
import os
import re
import subprocess

import numpy as np

import byron_corpus as bc
import candidates_eras_model as cem
import pbft_corpus as pc
import pbft_model as pm
from helpers import rng
from praos_hip import abi, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_STATE = -4
STRUCTS = {"praos_tpraos_candidates_in": wire.TPraosCandidatesIn, "praos_tpraos_candidates_out": wire.TPraosCandidatesOut,
           "praos_pbft_candidates_in": wire.PbftCandidatesIn, "praos_pbft_fragment": wire.PbftFragment,
           "praos_pbft_fragments": wire.PbftFragments, "praos_pbft_candidates_out": wire.PbftCandidatesOut}
HS = os.path.join(ROOT, "integration", "haskell", "Ouroboros", "Consensus", "Protocol", "Praos")


def test_struct_layouts(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "praos_hip.h"', "int main(void) {"]
    for cname, st in STRUCTS.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for name, _ in st._fields_:
            lines.append(f'  printf(" {name}@%zu", offsetof({cname}, {name}));')
        lines.append('  printf("\\n");')
    lines.append('  printf("abi %d\\n", (int)PRAOS_ABI_VERSION);')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(abi.HEADER_PATH), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    lay = {}
    for line, (cname, st) in zip(out, STRUCTS.items()):
        parts = line.split()
        assert parts[0] == cname and int(parts[1]) == ctypes.sizeof(st), cname
        offs = {k: int(v) for k, v in (p.split("@") for p in parts[2:])}
        assert offs == {n: getattr(st, n).offset for n, _ in st._fields_}, cname
        lay[cname] = (int(parts[1]), offs)
    assert out[len(STRUCTS)] == "abi 15"                          # additive: the version stays
    hs = open(os.path.join(HS, "Batch.hs")).read()
    seen = {}
    for m in re.finditer(r"^-- layout-eras (\w+) \((\d+) bytes\): (.*)$", hs, flags=re.M):
        seen[m.group(1)] = (int(m.group(2)), {f.split("@")[0]: int(f.split("@")[1]) for f in m.group(3).split()})
    assert seen == lay
    assert re.search(r'foreign import ccall safe "praos_validate_candidates_pbft"', hs)
    assert re.search(r'foreign import ccall safe "praos_validate_candidates_tpraos"', hs)
    assert "validateCandidateFragmentsPBft" in hs and "validateCandidateFragmentsTPraos" in hs


def test_the_build_reaches_the_new_call():
    lib = abi.load()
    for f in ("praos_validate_candidates_pbft", "praos_validate_candidates_tpraos"):
        assert hasattr(lib, f) and f in abi.SIGNATURES, f
        assert f in open(abi.HEADER_PATH).read()
    assert callable(abi.Context.validate_candidates_pbft) and callable(abi.Context.validate_candidates_tpraos)


def _args(window=4):
    arena = np.zeros(100, np.uint8)
    cin, fs, out = wire.PbftCandidatesIn(), wire.PbftFragments(), wire.PbftCandidatesOut()
    keep = [arena, np.zeros(1, np.uint64), np.full(1, 10, np.uint32)]
    cin.items = abi.Context.header_bytes_struct(*keep)
    cin.n_eras, cin.view_end_slot = 7, (1 << 64) - 1
    cin.params = abi.Context.pbft_params(window, 1, 40, 7)
    dl = np.arange(2 * 56, dtype=np.uint8).reshape(2, 56).copy()
    cin.delegs, cin.n_delegs = abi.ptr(dl), 2
    ff = (ctypes.c_size_t * 2)(0, 1)
    fr = (wire.PbftFragment * 1)()
    fr[0].tip.origin = 1
    ss, sh = np.zeros(window, np.uint64), np.zeros((window, 28), np.uint8)
    fr[0].state = abi.PbftStateC(window, 0, abi.ptr(ss, abi.u64p), abi.ptr(sh))
    fs.k, fs.frag_first, fs.frag = 1, ff, fr
    v, row, ws = np.zeros(1, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint8)
    out.wire_status, out.row, out.verdict = abi.ptr(ws), abi.ptr(row, abi.u32p), abi.ptr(v)
    out.rows_cap = 1
    keep += [dl, ff, fr, ss, sh, v, row, ws]
    return cin, fs, out, ff, fr, dl, keep


def test_argument_checks_need_no_device():
    c = abi.Context(abi.HOST_ONLY)
    try:
        L = c.L
        cin, fs, out, ff, fr, dl, keep = _args()
        call = lambda a=cin, b=fs, d=out: L.praos_validate_candidates_pbft(  # noqa: E731
            c.h, a and ctypes.byref(a), b and ctypes.byref(b), d and ctypes.byref(d))
        assert L.praos_validate_candidates_pbft(None, ctypes.byref(cin), ctypes.byref(fs), ctypes.byref(out)) == abi.E_ARG
        assert call(a=None) == abi.E_ARG and call(b=None) == abi.E_ARG and call(d=None) == abi.E_ARG
        assert call() == E_STATE                                    # everything in order: needs a device
        ff[1] = 2                                                   # the fragments do not cover the items
        assert call() == abi.E_ARG
        ff[1] = 1
        assert call() == E_STATE
        fr[0].state.cap = 3                                         # a state with cap < window_size
        assert call() == abi.E_ARG
        fr[0].state.cap = 4
        fr[0].state.n = 5                                           # more signers than the window holds
        assert call() == abi.E_ARG
        fr[0].state.n = 0
        dl[1, :28] = dl[0, :28]                                     # a duplicate genesis key hash
        assert call() == abi.E_ARG
        dl[1, :28] = 99
        dl[1, 28:] = dl[0, 28:]                                     # a duplicate delegate key hash
        assert call() == abi.E_ARG
        dl[1, 28:] = 98
        assert call() == E_STATE
        cin.params.epoch_slots = 0
        assert call() == abi.E_ARG
        cin.params.epoch_slots = 40
        cin.params.window_size = 0
        assert call() == abi.E_ARG
        cin.params.window_size = 4
        out.verdict = None
        assert call() == abi.E_ARG
    finally:
        c.close()


def test_tpraos_argument_checks_need_no_device():
    c = abi.Context(abi.HOST_ONLY)
    try:
        L = c.L
        arena = np.zeros(100, np.uint8)
        hb = abi.Context.header_bytes_struct(arena, np.zeros(1, np.uint64), np.full(1, 10, np.uint32))
        cin, fs, out = wire.TPraosCandidatesIn(), wire.Fragments(), wire.TPraosCandidatesOut()
        cin.items = hb
        cin.ei = abi.EpochInfo(0, 0, 100, 10)
        ff = (ctypes.c_size_t * 2)(0, 1)
        fr = (wire.Fragment * 1)()
        fs.k, fs.frag_first, fs.frag = 1, ff, fr
        v, row, ws = np.zeros(1, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint8)
        out.wire_status, out.row, out.verdict = abi.ptr(ws), abi.ptr(row, abi.u32p), abi.ptr(v)
        call = lambda a=cin, b=fs, d=out: L.praos_validate_candidates_tpraos(  # noqa: E731
            c.h, a and ctypes.byref(a), b and ctypes.byref(b), d and ctypes.byref(d))
        assert L.praos_validate_candidates_tpraos(None, ctypes.byref(cin), ctypes.byref(fs), ctypes.byref(out)) == abi.E_ARG
        assert call(a=None) == abi.E_ARG and call(b=None) == abi.E_ARG and call(d=None) == abi.E_ARG
        assert call() == E_STATE                                    # everything in order: needs a device
        ff[1] = 2                                                   # the fragments do not cover the items
        assert call() == abi.E_ARG
        ff[1] = 1
        cin.ei = abi.EpochInfo(0, 0, 0, 10)                         # epoch_length == 0
        assert call() == abi.E_ARG
        cin.ei = abi.EpochInfo(0, 0, 100, 10)
        fr[0].state.m, fr[0].state.cap = 2, 1                       # a counter map without room
        assert call() == abi.E_ARG
        fr[0].state.m = 0
        out.verdict = None
        assert call() == abi.E_ARG
    finally:
        c.close()


def _chain():
    r = rng(0x0c4d)
    D = [bc.Delegate(r) for _ in range(7)]
    blocks = pc.make_chain(r, 40, lambda k: D[k % 7], epochs=3)
    return blocks, pc.delegation(r, D)


def test_model_equals_the_fold_on_an_intact_chain(oracle):
    """the checker's client fold over a pbft_corpus chain, from several of the chain's own tips,
    against pbft_model.fold over the same headers: on an intact chain the two agree"""
    blocks, delegs = _chain()
    W, T = 14, 2
    rows = pc.model_rows(blocks, delegs)
    ebb = [int(b.kind == 0) for b in blocks]
    whole = pm.fold(rows, ebb, W, T, pc.EPOCH_SLOTS, delegs)
    assert whole[2] == len(blocks) and set(whole[0]) == {0}
    items = cem.wrap_blocks(blocks)
    m = cem.PbftModel(W, T, pc.EPOCH_SLOTS, pc.PM, delegs)
    for start in (0, 1, 41, 42, 77):
        _, _, _, tip, st = pm.fold(rows[:start], ebb[:start], W, T, pc.EPOCH_SLOTS, delegs)
        want = pm.fold(rows[start:], ebb[start:], W, T, pc.EPOCH_SLOTS, delegs, tip, st)
        got = m.fold(items[start:], tip, st)
        assert (got["verdict"], got["aux"], got["chain_stop"], got["tip"], got["state"]) == tuple(want), start
        assert got["processed"] == len(blocks) - start
    # the client's own rules: a header that does not fit is DoesntFit, not UnexpectedPrevHash, and
    # the forecast horizon ends the fold without a verdict
    _, _, _, tip, st = pm.fold(rows[:5], ebb[:5], W, T, pc.EPOCH_SLOTS, delegs)
    got = m.fold(items[6:], tip, st)
    assert got["verdict"][0] == cem.V_DOESNT_FIT and got["chain_stop"] == 0 and got["processed"] == 1
    assert set(got["verdict"][1:]) == {cem.V_NOT_REACHED} and got["tip"] == tip and got["state"] == st
    assert pm.fold(rows[6:], ebb[6:], W, T, pc.EPOCH_SLOTS, delegs, tip, st)[0][0] == pm.V_ENV_BLOCK_NO
    got = m.fold(items[5:], tip, st, view_end_slot=rows[9]["slot"])
    assert got["processed"] == got["chain_stop"] == 4 and got["verdict"][:5] == [0, 0, 0, 0, cem.V_NOT_REACHED]
    assert got["tip"][0] == rows[8]["slot"]
