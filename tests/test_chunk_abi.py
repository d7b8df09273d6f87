"""CPU: the chunk-validation surface of the ABI (praos_crc32, praos_validate_chunk).

The ctypes structs of the Python binding and the '-- layout' lines of the Haskell binding (the
offsets validateChunkBatch pokes and peeks) equal the C compiler's layout of include/praos_hip.h;
the constants agree; the C harness, the Haskell module and the validation patch reach the entry
point; a host-only context refuses both calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from praos_hip import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASKELL = os.path.join(ROOT, "integration", "haskell")
STRUCTS = {"praos_chunk": "Chunk", "praos_chunk_result": "ChunkResult", "praos_chunk_out": "ChunkOut"}


def _layout(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "praos_hip.h"', "int main(void) {"]
    for cs, py in STRUCTS.items():
        lines.append(f'  printf("{cs} %zu", sizeof({cs}));')
        for name, _ in getattr(abi, py)._fields_:
            lines.append(f'  printf(" {name}@%zu", offsetof({cs}, {name}));')
        lines.append('  printf("\\n");')
    lines.append('  printf("tile %d entry %d codes %d %d %d %d %d\\n", PRAOS_CRC_TILE, PRAOS_CHUNK_ENTRY_SIZE, '
                 "PRAOS_CHUNK_OK, PRAOS_CHUNK_ERR_READ, PRAOS_CHUNK_ERR_CORRUPT, PRAOS_CHUNK_ERR_HASH_MISMATCH, "
                 "PRAOS_CHUNK_UNSUPPORTED);")
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
    assert consts == (f"tile {abi.CRC_TILE[0]} entry {abi.CHUNK_ENTRY_SIZE} codes {abi.CHUNK_OK} {abi.CHUNK_ERR_READ} "
                      f"{abi.CHUNK_ERR_CORRUPT} {abi.CHUNK_ERR_HASH_MISMATCH} {abi.CHUNK_UNSUPPORTED}")
    assert len(abi.CRC_TILE) == 1 and len(abi.CHUNK_OUTCOMES) == 5
    from praos_hip import immutable
    assert immutable.ENTRY == abi.CHUNK_ENTRY_SIZE
    # the Haskell binding's offsets
    hs = open(os.path.join(HASKELL, "Ouroboros", "Consensus", "Protocol", "Praos", "Batch.hs")).read()
    seen = set()
    for m in re.finditer(r"^-- layout (\w+) \((\d+) bytes\): (.*)$", hs, flags=re.M):
        cs, size, fields = m.group(1), int(m.group(2)), m.group(3).split()
        assert lay[cs][0] == size, cs
        for f in fields:
            name, off = f.split("@")
            assert lay[cs][1][name] == int(off), (cs, name)
        assert f"allocaBytes {size}" in hs
        seen.add(cs)
    assert seen == set(STRUCTS)


def test_every_layer_reaches_the_entry_points():
    hs = open(os.path.join(HASKELL, "Ouroboros", "Consensus", "Protocol", "Praos", "Batch.hs")).read()
    assert 'foreign import ccall safe "praos_validate_chunk"' in hs
    assert re.search(r"^validateChunkBatch ::", hs, flags=re.M) and "  , validateChunkBatch" in hs
    patch = open(os.path.join(HASKELL, "immutabledb-validation.patch")).read()
    body = [ln for ln in patch.splitlines() if ln[:1] in ("+", "-") and ln[:3] not in ("+++", "---")]
    assert body and all(ln.startswith("+") for ln in body)       # additions only
    for needle in ("ChunkUnsupported -> Parser.parseChunkFile", "chunkBatch", "ChunkErrHashMismatch",
                   "let parseChunkFile = batchedParseChunkFile entriesFromSecondaryIndex"):
        assert needle in patch, needle
    harness = open(os.path.join(ROOT, "integration", "c", "ffi_harness.c")).read()
    assert '"--validate-chunk"' in harness and "praos_validate_chunk(ctx, &ch, spkp, &res, &out)" in harness
    hdr = open(abi.HEADER_PATH).read()
    assert "#define PRAOS_ABI_VERSION 15" in hdr and "added without a version bump; purely additive" in hdr
    lib = abi.load()
    assert hasattr(lib, "praos_crc32") and hasattr(lib, "praos_validate_chunk")
    mk = open(os.path.join(ROOT, "ouroboros-consensus_amd", "csrc", "Makefile")).read()
    assert re.search(r"^MODS := .*\bk_crc32\b", mk, flags=re.M) and re.search(r"for m in .*\bk_crc32\b", mk)


def test_argument_checks_need_no_device():
    """Bad arguments are refused before anything touches a device (NULL context included)."""
    lib = abi.load()
    arena = np.zeros(100, np.uint8)
    off, ln = np.array([0, 95], np.uint64), np.array([10, 6], np.uint32)
    hb = abi.Context.header_bytes_struct(arena, off, ln)
    crc = np.zeros(2, np.uint32)
    assert lib.praos_crc32(None, ctypes.byref(hb), abi.ptr(crc, abi.u32p)) == abi.E_ARG
    ch, res, out = abi.Chunk(), abi.ChunkResult(), abi.ChunkOut()
    assert lib.praos_validate_chunk(None, ctypes.byref(ch), 129600, ctypes.byref(res), ctypes.byref(out)) == abi.E_ARG
