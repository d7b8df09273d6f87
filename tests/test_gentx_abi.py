"""CPU: the wire-transaction surface of the ABI (praos_verify_gen_txs).

The ctypes structs of the Python binding and the '-- layout-gtx' lines of the Haskell binding (the
offsets praosVerifyGenTxs pokes) equal the C compiler's layout of include/praos_hip.h; the
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
STRUCTS = {"praos_gtx_cfg": "GtxCfg", "praos_gtx_items": "GtxItems", "praos_gtx_txs": "GtxTxs"}


def _layout(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "praos_hip.h"', "int main(void) {"]
    for cs, py in STRUCTS.items():
        lines.append(f'  printf("{cs} %zu", sizeof({cs}));')
        for name, _ in getattr(abi, py)._fields_:
            lines.append(f'  printf(" {name}@%zu", offsetof({cs}, {name}));')
        lines.append('  printf("\\n");')
    lines.append('  printf("codes %d %d %d %d %d %d %d overhead %u abi %d\\n", PRAOS_WIRE_OK, PRAOS_WIRE_RANGE, '
                 "PRAOS_WIRE_SYNTAX, PRAOS_WIRE_ERA, PRAOS_WIRE_TRAILING, PRAOS_GTX_SHAPE, PRAOS_GTX_BYRON, "
                 "PRAOS_GTX_PER_TX_OVERHEAD, PRAOS_ABI_VERSION);")
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
    assert consts == f"codes 0 1 2 3 4 {abi.GTX_SHAPE} {abi.GTX_BYRON} overhead {abi.GTX_PER_TX_OVERHEAD} abi 15"
    assert (abi.GTX_SHAPE, abi.GTX_BYRON, abi.GTX_PER_TX_OVERHEAD, abi.GTX_NO_ROW) == (5, 6, 4, 0xFFFFFFFF)
    # every field of the C structs is bound: the header's members in order
    hdr = open(abi.HEADER_PATH).read()
    for cs, py in STRUCTS.items():
        body = re.search(r"typedef struct \{([^}]*)\} " + cs + ";", hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+);", body)
        assert names == [n for n, _ in getattr(abi, py)._fields_], cs
    assert dict((n, s) for n, _, s in abi.GTX_TX_FIELDS)["tx_id"] == (32,)
    # the Haskell binding's offsets
    hs = open(BATCH_HS).read()
    seen = set()
    for m in re.finditer(r"^-- layout-gtx (\w+) \((\d+) bytes\): (.*)$", hs, flags=re.M):
        cs, size, fields = m.group(1), int(m.group(2)), m.group(3).split()
        assert lay[cs][0] == size, cs
        assert [f.split("@")[0] for f in fields] == list(lay[cs][1]), cs
        for f in fields:
            name, off = f.split("@")
            assert lay[cs][1][name] == int(off), (cs, name)
        assert f"allocaBytes {size}" in hs
        seen.add(cs)
    assert seen == set(STRUCTS)
    # the pokes of praosVerifyGenTxs land on the members they mean
    fn = hs[hs.index("praosVerifyGenTxs ctx nEras"):hs.index("-- | Per stored block what db-analyser's")]
    L = {cs: lay[cs][1] for cs in STRUCTS}
    assert [int(x) for x in re.findall(r"pokeByteOff gcfg (\d+)", fn)] == list(L["praos_gtx_cfg"].values())
    assert [int(x) for x in re.findall(r"pokeByteOff its (\d+)", fn)] == [L["praos_gtx_items"][k] for k in ("status", "row")]
    want = ["cap", "in_block_size", "ex_mem", "ex_steps", "tx_id", "wstatus", "n_bad"]
    assert [int(x) for x in re.findall(r"pokeByteOff txs (\d+)", fn)] == [L["praos_gtx_txs"][k] for k in want]
    assert f"peekByteOff txs {L['praos_gtx_txs']['n_rows']}" in fn
    assert "fillBytes its 0 48" in fn and "fillBytes txs 0 168" in fn and "fillBytes wits 0 64" in fn


def test_every_layer_reaches_the_entry_point():
    hs = open(BATCH_HS).read()
    assert 'foreign import ccall safe "praos_verify_gen_txs"' in hs
    assert re.search(r"^praosVerifyGenTxs ::", hs, flags=re.M) and "  , praosVerifyGenTxs" in hs
    hdr = open(abi.HEADER_PATH).read()
    assert "#define PRAOS_ABI_VERSION 15" in hdr
    assert re.search(r"^int praos_verify_gen_txs\(", hdr, flags=re.M)
    assert hasattr(abi.load(), "praos_verify_gen_txs") and "praos_verify_gen_txs" in abi.SIGNATURES
    assert "Shelley/Ledger/Mempool.hs:186-193" in hdr and "Shelley/Ledger/Mempool.hs:125-143" in hdr
    mk = open(os.path.join(ROOT, "ouroboros-consensus_amd", "csrc", "Makefile")).read()
    assert re.search(r"^MODS := .*\bk_gentx\b.*\bpraos_gentx\b", mk, flags=re.M)
    assert re.search(r"for m in .*\bk_gentx\b", mk)
    from praos_hip import txsubmission
    assert callable(txsubmission.verify_inbound) and callable(abi.Context.verify_gen_txs)
    assert txsubmission.wrap_gen_tx(3, b"\x83\xa0\xa0\xf6") == b"\x82\x03\xd8\x18\x44\x83\xa0\xa0\xf6"


def test_argument_checks_need_no_device():
    lib = abi.load()
    arena = np.zeros(64, np.uint8)
    off, ln = np.array([0], np.uint64), np.array([10], np.uint32)
    hb = abi.Context.header_bytes_struct(arena, off, ln)
    cfg, it, ts, ws = abi.GtxCfg(7, 1, 0, 0), abi.GtxItems(), abi.GtxTxs(), abi.TxwWits()
    assert lib.praos_verify_gen_txs(None, ctypes.byref(hb), ctypes.byref(cfg), ctypes.byref(it), ctypes.byref(ts),
                                    ctypes.byref(ws)) == abi.E_ARG
