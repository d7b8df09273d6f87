"""CPU: the key-witness surface of the ABI (praos_verify_tx_witnesses,
praos_block_batch_tx_witnesses).

The ctypes structs of the Python binding and the '-- layout-txw' lines of the Haskell binding
(the offsets praosVerifyTxWitnesses pokes) equal the C compiler's layout of include/praos_hip.h;
the constants agree; every layer reaches the entry points; bad arguments are refused before
anything touches a device."""
import ctypes
import os
import re
import subprocess

import numpy as np

from praos_hip import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_HS = os.path.join(ROOT, "integration", "haskell", "Ouroboros", "Consensus", "Protocol", "Praos", "Batch.hs")
STRUCTS = {"praos_txw_cfg": "TxwCfg", "praos_txw_blocks": "TxwBlocks", "praos_txw_txs": "TxwTxs",
           "praos_txw_wits": "TxwWits"}


def _layout(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "praos_hip.h"', "int main(void) {"]
    for cs, py in STRUCTS.items():
        lines.append(f'  printf("{cs} %zu", sizeof({cs}));')
        for name, _ in getattr(abi, py)._fields_:
            lines.append(f'  printf(" {name}@%zu", offsetof({cs}, {name}));')
        lines.append('  printf("\\n");')
    lines.append('  printf("codes %u %u %u abi %d\\n", PRAOS_TXW_OK, PRAOS_TXW_SHAPE, PRAOS_TXW_SKIPPED, '
                 "PRAOS_ABI_VERSION);")
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
    assert consts == f"codes {abi.TXW_OK} {abi.TXW_SHAPE} {abi.TXW_SKIPPED} abi 15"
    assert (abi.TXW_OK, abi.TXW_SHAPE, abi.TXW_SKIPPED) == (0, 1, 2)
    # every field of the C structs is bound: the header's members in order
    hdr = open(abi.HEADER_PATH).read()
    for cs, py in STRUCTS.items():
        body = re.search(r"typedef struct \{([^}]*)\} " + cs + ";", hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+);", body)
        assert names == [n for n, _ in getattr(abi, py)._fields_], cs
    # the record shapes of the binding's arrays: tx_id 32 bytes, key_hash 28
    assert dict((n, s) for n, _, s in abi.TXW_TX_FIELDS)["tx_id"] == (32,)
    assert dict((n, s) for n, _, s in abi.TXW_WIT_FIELDS)["key_hash"] == (28,)
    # the Haskell binding's offsets
    hs = open(BATCH_HS).read()
    seen = set()
    for m in re.finditer(r"^-- layout-txw (\w+) \((\d+) bytes\): (.*)$", hs, flags=re.M):
        cs, size, fields = m.group(1), int(m.group(2)), m.group(3).split()
        assert lay[cs][0] == size, cs
        assert [f.split("@")[0] for f in fields] == list(lay[cs][1]), cs
        for f in fields:
            name, off = f.split("@")
            assert lay[cs][1][name] == int(off), (cs, name)
        assert f"allocaBytes {size}" in hs
        seen.add(cs)
    assert seen == set(STRUCTS)
    # the pokes of praosVerifyTxWitnesses land on members of the structs they fill
    fn = hs[hs.index("praosVerifyTxWitnesses ctx byron"):hs.index("-- | Per stored block what db-analyser's")]
    for var, cs in (("wcfg", "praos_txw_cfg"), ("blks", "praos_txw_blocks")):
        offs = [int(x) for x in re.findall(rf"pokeByteOff {var} (\d+)", fn)]
        assert offs and set(offs) <= set(lay[cs][1].values()), var
    assert "fillBytes blks 0 48" in fn and "fillBytes txs 0 72" in fn and "fillBytes wits 0 64" in fn


def test_every_layer_reaches_the_entry_points():
    hs = open(BATCH_HS).read()
    assert 'foreign import ccall safe "praos_verify_tx_witnesses"' in hs
    assert re.search(r"^praosVerifyTxWitnesses ::", hs, flags=re.M) and "  , praosVerifyTxWitnesses" in hs
    hdr = open(abi.HEADER_PATH).read()
    assert "#define PRAOS_ABI_VERSION 15" in hdr
    for fn in ("praos_verify_tx_witnesses", "praos_block_batch_tx_witnesses"):
        assert re.search(rf"^int {fn}\(", hdr, flags=re.M), fn
        assert hasattr(abi.load(), fn) and fn in abi.SIGNATURES
    # the entry cites the reference code it replaces
    assert "Shelley/Ledger/Ledger.hs:335-352" in hdr and "Shelley/Ledger/Mempool.hs:215-239" in hdr
    mk = open(os.path.join(ROOT, "ouroboros-consensus_amd", "csrc", "Makefile")).read()
    assert re.search(r"^MODS := .*\bk_txwit\b.*\bpraos_txwit\b", mk, flags=re.M)
    assert re.search(r"for m in .*\bk_txwit\b", mk)
    from praos_hip import analysis, witnesses
    assert len(analysis.ANALYSES) == 6 and callable(witnesses.verify_immutable_witnesses)


def test_argument_checks_need_no_device():
    lib = abi.load()
    arena = np.zeros(64, np.uint8)
    off, ln = np.array([0], np.uint64), np.array([10], np.uint32)
    hb = abi.Context.header_bytes_struct(arena, off, ln)
    cfg, bs, ts, ws = abi.TxwCfg(0, 0), abi.TxwBlocks(), abi.TxwTxs(), abi.TxwWits()
    assert lib.praos_verify_tx_witnesses(None, ctypes.byref(hb), ctypes.byref(cfg), ctypes.byref(bs), ctypes.byref(ts),
                                         ctypes.byref(ws)) == abi.E_ARG
    assert lib.praos_block_batch_tx_witnesses(None, None, ctypes.byref(cfg), ctypes.byref(bs), ctypes.byref(ts),
                                              ctypes.byref(ws)) == abi.E_ARG
