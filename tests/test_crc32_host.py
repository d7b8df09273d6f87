"""Host checks of the chunk-validation headers (csrc/crc32_gf2.hpp, csrc/chunk_scan.hpp).

Both are plain C++, so the exact text the library includes is compiled here with g++: the
bytewise CRC-32 restatement and the GF(2) combine against zlib, and the host item walk
against the oracle's cbor_skip (accept / reject and end offset) over the block mutation
corpus, alone and concatenated with random bytes in between."""
import ctypes
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

import block_corpus as bc
import block_integrity as bi
from helpers import rbytes

HDR = os.path.join(os.path.dirname(__file__), "..", "ouroboros-consensus_amd", "csrc")
INC = os.path.join(os.path.dirname(__file__), "..", "include")
SPKP = 129600

SHIM = r"""
#include "crc32_gf2.hpp"
#include "chunk_scan.hpp"
extern "C" uint32_t t_crc(const uint8_t* p, size_t n) { return crc32_bytes(p, n); }
extern "C" uint32_t t_combine(uint32_t a, uint32_t b, uint64_t lb) { return crc_combine(a, b, lb); }
extern "C" uint32_t t_finish(const uint8_t* p, size_t n) { return crc_finish(crc_raw_bytes(0, p, n), n); }
extern "C" uint32_t t_words(const uint8_t* p, size_t nwords) {   // raw(0, .) word by word, as the kernel runs it
  uint32_t s = 0;
  for (size_t i = 0; i < nwords; i++)
    s = crc_word(s, (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 |
                        (uint32_t)p[4 * i + 3] << 24);
  return crc_finish(s, 4 * nwords);
}
extern "C" long long t_item_end(const uint8_t* a, uint64_t pos, uint64_t end) {
  return chunk_scan::chunk_item_end(a, pos, end);
}
extern "C" int t_byron(const uint8_t* a, uint64_t pos, uint64_t end) { return chunk_scan::is_byron_item(a, pos, end); }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("crc")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "libcrc.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.abspath(HDR), str(src), "-o",
                    str(so)], check=True)
    L = ctypes.CDLL(str(so))
    L.t_crc.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.t_crc.restype = ctypes.c_uint32
    L.t_finish.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.t_finish.restype = ctypes.c_uint32
    L.t_words.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.t_words.restype = ctypes.c_uint32
    L.t_combine.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    L.t_combine.restype = ctypes.c_uint32
    L.t_item_end.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64]
    L.t_item_end.restype = ctypes.c_longlong
    L.t_byron.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64]
    return L


def _tile():
    from praos_hip import abi
    return abi.CRC_TILE


def test_bytewise_equals_zlib(lib):
    r = random.Random(1)
    for n in range(301):
        d = rbytes(r, n)
        assert lib.t_crc(d, n) == zlib.crc32(d), n
        assert lib.t_finish(d, n) == zlib.crc32(d), n      # raw(0, D) + F x^(8n) + F
    for n in (4096, 65537, 1 << 20):
        d = rbytes(r, n)
        assert lib.t_crc(d, n) == zlib.crc32(d)
    for n in (0, 4, 16, 64, 4096):
        d = rbytes(r, n)
        assert lib.t_words(d, n // 4) == zlib.crc32(d), n
    assert lib.t_crc(bytes(70001), 70001) == zlib.crc32(bytes(70001))
    assert lib.t_crc(b"\xff" * 70001, 70001) == zlib.crc32(b"\xff" * 70001)


def test_combine_equals_zlib(lib):
    r = random.Random(2)
    for _ in range(2000):
        a, b = rbytes(r, r.randrange(0, 3000)), rbytes(r, r.randrange(0, 3000))
        assert lib.t_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b)
    big = rbytes(r, (1 << 20) + 100)
    lens = {0, 1} | {1 << k for k in range(21)}
    for t in _tile():
        lens |= {t - 1, t, t + 1}
    for lb in sorted(lens):
        a, b = big[:100], big[100:100 + lb]
        assert lib.t_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), lb


def _oracle_end(buf, p):
    try:
        return bi.cbor_skip(buf, p, len(buf))
    except bi._Bad:
        return -1


def test_item_walk_equals_oracle(lib):
    r = random.Random(3)
    variants = []
    for era in (5, 6, 7):
        blk, f, _ = bc.make_block(r, SPKP, era=era)
        variants += [bc.mutate(blk, f, r, kind) for kind in bc.MUTATIONS]
    for v in variants:
        assert lib.t_item_end(v, 0, len(v)) == _oracle_end(v, 0)
    # concatenated, random bytes in between: walk item by item until the first reject
    for trial in range(20):
        r.shuffle(variants)
        buf = b"".join(v + rbytes(r, r.randrange(0, 6)) for v in variants)
        p = 0
        while p < len(buf):
            want = _oracle_end(buf, p)
            assert lib.t_item_end(buf, p, len(buf)) == want, (trial, p)
            p = want if want >= 0 else p + 1 + r.randrange(50)
    for _ in range(300):                                  # random items, every prefix length
        it = bc.rand_item(r)
        for n in range(len(it) + 1) if len(it) < 64 else (0, 1, len(it) - 1, len(it)):
            assert lib.t_item_end(it[:n], 0, n) == _oracle_end(it[:n], 0)


def test_byron_shape(lib):
    H = bc.H
    for item, want in ((H(4, 2) + H(0, 0) + H(2, 3) + b"abc", 1), (H(4, 2) + H(0, 1) + H(4, 0), 1),
                       (H(4, 2) + H(0, 2) + H(4, 0), 0), (H(4, 2) + H(0, 6) + H(4, 0), 0), (H(0, 0), 0),
                       (H(4, 0), 0), (b"\x9f\x00\xff", 0), (H(4, 1) + b"\x18\x01", 1), (H(4, 1) + H(1, 0), 0)):
        assert lib.t_byron(item, 0, len(item)) == want, item.hex()
