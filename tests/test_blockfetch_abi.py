"""CPU: the wire-block surface of the ABI (praos_verify_fetched_blocks, praos_debug_span_equal).

The ctypes structs of the Python binding and the '-- layout-bf' lines of the Haskell binding (the
offsets praosVerifyFetchedBlocks pokes) equal the C compiler's layout of include/praos_hip.h; the
constants agree; every layer reaches the entry point; bad arguments are refused before anything
touches a device."""
import ctypes
import os
import re
import subprocess

import numpy as np

from praos_hip import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_HS = os.path.join(ROOT, "integration", "haskell", "Ouroboros", "Consensus", "Protocol", "Praos", "Batch.hs")
STRUCTS = {"praos_bf_ranges": "BfRanges", "praos_bf_cfg": "BfCfg", "praos_bf_items": "BfItems",
           "praos_bf_range_out": "BfRangeOut", "praos_bf_rows": "BfRows"}
CODES = ("PRAOS_BF_OK", "PRAOS_BF_WIRE", "PRAOS_BF_DECODE", "PRAOS_BF_WRONG_BLOCK", "PRAOS_BF_INVALID_BODY",
         "PRAOS_BF_TOO_MANY", "PRAOS_BF_UNSUPPORTED", "PRAOS_BF_NOT_REACHED", "PRAOS_BF_RANGE_COMPLETE",
         "PRAOS_BF_RANGE_FAILED", "PRAOS_BF_RANGE_TOO_FEW")


def _layout(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "praos_hip.h"', "int main(void) {"]
    for cs, py in STRUCTS.items():
        lines.append(f'  printf("{cs} %zu", sizeof({cs}));')
        for name, _ in getattr(abi, py)._fields_:
            lines.append(f'  printf(" {name}@%zu", offsetof({cs}, {name}));')
        lines.append('  printf("\\n");')
    lines.append('  printf("codes' + " %d" * len(CODES) + ' norow %u eq %u %u %u abi %d\\n", ' + ", ".join(CODES) +
                 ", PRAOS_BF_NO_ROW, PRAOS_SPAN_EQ_VEC, PRAOS_SPAN_EQ_WAVE, PRAOS_SPAN_EQ_TILE, PRAOS_ABI_VERSION);")
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(abi.HEADER_PATH), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    lay = {}
    for ln in out[:-1]:
        parts = ln.split()
        lay[parts[0]] = (int(parts[1]), {k: int(v) for k, v in (p.split("@") for p in parts[2:])})
    return lay, out[-1]


def test_struct_layouts_and_constants(tmp_path):
    lay, consts = _layout(tmp_path)
    for cs, py in STRUCTS.items():
        S = getattr(abi, py)
        assert ctypes.sizeof(S) == lay[cs][0], cs
        assert {n: getattr(S, n).offset for n, _ in S._fields_} == lay[cs][1], cs
    py_codes = (abi.BF_OK, abi.BF_WIRE, abi.BF_DECODE, abi.BF_WRONG_BLOCK, abi.BF_INVALID_BODY, abi.BF_TOO_MANY,
                abi.BF_UNSUPPORTED, abi.BF_NOT_REACHED, abi.BF_RANGE_COMPLETE, abi.BF_RANGE_FAILED, abi.BF_RANGE_TOO_FEW)
    assert py_codes == (0, 1, 2, 3, 4, 5, 6, 255, 0, 1, 2)
    assert consts == ("codes " + " ".join(str(c) for c in py_codes) + f" norow {abi.BF_NO_ROW} eq {abi.SPAN_EQ_VEC} "
                      f"{abi.SPAN_EQ_WAVE} {abi.SPAN_EQ_TILE} abi 15")
    assert (abi.SPAN_EQ_VEC, abi.SPAN_EQ_WAVE, abi.SPAN_EQ_TILE, abi.BF_NO_ROW) == (16, 1024, 4096, 0xFFFFFFFF)
    # every field of the C structs is bound: the header's members in order
    hdr = open(abi.HEADER_PATH).read()
    for cs, py in STRUCTS.items():
        body = re.search(r"typedef struct \{([^}]*)\} " + cs + ";", hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+);", body)
        assert names == [n for n, _ in getattr(abi, py)._fields_], cs
    shapes = dict((n, s) for n, _, s in abi.BF_ROW_FIELDS)
    assert shapes["header_hash"] == shapes["prev_hash"] == shapes["body_hash"] == (32,)
    # the Haskell binding's offsets
    hs = open(BATCH_HS).read()
    seen = set()
    for m in re.finditer(r"^-- layout-bf (\w+) \((\d+) bytes\): (.*)$", hs, flags=re.M):
        cs, size, fields = m.group(1), int(m.group(2)), m.group(3).split()
        assert lay[cs][0] == size, cs
        assert [f.split("@")[0] for f in fields] == list(lay[cs][1]), cs
        for f in fields:
            name, off = f.split("@")
            assert lay[cs][1][name] == int(off), (cs, name)
        assert f"allocaBytes {size}" in hs
        seen.add(cs)
    assert seen == set(STRUCTS)
    # the pokes of praosVerifyFetchedBlocks land on the members they mean
    fn = hs[hs.index("praosVerifyFetchedBlocks ctx nEras"):hs.index("-- | What the TxSubmission inbound side learns")]
    L = {cs: lay[cs][1] for cs in STRUCTS}
    assert [int(x) for x in re.findall(r"pokeByteOff rgs (\d+)", fn)] == list(L["praos_bf_ranges"].values())
    assert [int(x) for x in re.findall(r"pokeByteOff bcfg (\d+)", fn)] == list(L["praos_bf_cfg"].values())
    assert [int(x) for x in re.findall(r"pokeByteOff its (\d+)", fn)] == [L["praos_bf_items"][k] for k in ("verdict", "row")]
    assert [int(x) for x in re.findall(r"pokeByteOff rout (\d+)", fn)] == [L["praos_bf_range_out"][k]
                                                                          for k in ("accepted", "status")]
    want = ["cap", "slot", "block_no", "header_hash"]
    assert [int(x) for x in re.findall(r"pokeByteOff rws (\d+)", fn)] == [L["praos_bf_rows"][k] for k in want]
    assert f"peekByteOff rws {L['praos_bf_rows']['n_rows']}" in fn
    tb = {n: getattr(abi.TxwBlocks, n).offset for n, _ in abi.TxwBlocks._fields_}
    assert [int(x) for x in re.findall(r"pokeByteOff blks (\d+)", fn)] == [tb[k] for k in ("n_tx", "n_wit", "n_bad", "n_shape")]
    for name, size in (("its", 32), ("rout", 24), ("rws", 128), ("blks", ctypes.sizeof(abi.TxwBlocks)),
                       ("txs", ctypes.sizeof(abi.TxwTxs)), ("wits", ctypes.sizeof(abi.TxwWits))):
        assert f"fillBytes {name} 0 {size}" in fn, name


def test_every_layer_reaches_the_entry_point():
    hs = open(BATCH_HS).read()
    assert 'foreign import ccall safe "praos_verify_fetched_blocks"' in hs
    assert re.search(r"^praosVerifyFetchedBlocks ::", hs, flags=re.M) and "  , praosVerifyFetchedBlocks" in hs
    hdr = open(abi.HEADER_PATH).read()
    assert "#define PRAOS_ABI_VERSION 15" in hdr
    assert re.search(r"^int praos_verify_fetched_blocks\(", hdr, flags=re.M)
    assert re.search(r"^int praos_debug_span_equal\(", hdr, flags=re.M)
    L = abi.load()
    for sym in ("praos_verify_fetched_blocks", "praos_debug_span_equal"):
        assert hasattr(L, sym) and sym in abi.SIGNATURES
    for cite in ("MiniProtocol/BlockFetch/ClientInterface.hs:157-176", "ClientInterface.hs:208-221",
                 "Shelley/Ledger/Block.hs:150-158", "Byron/Ledger/Block.hs:161-162",
                 "HardFork/Combinator/Serialisation/SerialiseNodeToNode.hs:113"):
        assert cite in hdr, cite
    mk = open(os.path.join(ROOT, "ouroboros-consensus_amd", "csrc", "Makefile")).read()
    assert re.search(r"^MODS := .*\bk_blockfetch\b.*\bpraos_blockfetch\b", mk, flags=re.M)
    assert re.search(r"for m in .*\bk_blockfetch\b", mk)
    from praos_hip import blockfetch
    assert callable(blockfetch.verify_fetched) and callable(abi.Context.verify_fetched_blocks)
    assert blockfetch.wrap_block(b"\x82\x06\x80") == b"\xd8\x18\x43\x82\x06\x80"
    assert blockfetch.unwrap_block(b"\xd8\x18\x43\x82\x06\x80") == (0, 6, 3, 3)


def test_argument_checks_need_no_device():
    lib = abi.load()
    arena = np.zeros(64, np.uint8)
    off, ln = np.array([0], np.uint64), np.array([10], np.uint32)
    hb = abi.Context.header_bytes_struct(arena, off, ln)
    first = np.array([0, 1], np.uint64)
    rg = abi.BfRanges(1, abi.ptr(first, abi.u64p), abi.ptr(first, abi.u64p), None, None)
    cfg = abi.BfCfg(7, 1, 1, 0, 0)
    args = [ctypes.byref(x) for x in (abi.BfItems(), abi.BfRangeOut(), abi.BfRows(), abi.TxwBlocks(), abi.TxwTxs(),
                                      abi.TxwWits())]
    assert lib.praos_verify_fetched_blocks(None, ctypes.byref(hb), ctypes.byref(rg), ctypes.byref(cfg), *args) == abi.E_ARG
    assert lib.praos_debug_span_equal(None, 1, None, 0, None, None, None, None) == abi.E_ARG
