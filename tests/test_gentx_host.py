"""Host checks of the wire-transaction wrapper parser (csrc/wire_scan.hpp gen_tx_unwrap).

The header is plain C++, so the exact text k_gentx.hip includes is compiled here with g++ and held
to the model's wrapper walk (gentx_model.unwrap): on the golden GenTx files, on every wrapper of
the corpus (gentx_corpus.py), on every truncation of a few of them and on single-byte mutations of
their first bytes, inside a larger arena and with spans that leave it.  The same items run through
a stand-alone program built with -fsanitize=address,undefined, each in a heap buffer of exactly its
size."""
import ctypes
import os
import random
import subprocess

import pytest

import gentx_corpus as gc
import gentx_model as gm
from test_gentx_model import golden_items

HDR = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "ouroboros-consensus_amd", "csrc"))

SHIM = r"""
#include "wire_scan.hpp"
extern "C" void t_gen_tx(const uint8_t* a, uint64_t arena_len, uint64_t pos, uint64_t len, uint32_t n_eras,
                         uint64_t out[5]) {
  const wire_scan::Item r = wire_scan::gen_tx_unwrap(a, arena_len, pos, len, n_eras);
  const bool span = r.status == wire_scan::OK || r.status == wire_scan::TRAILING || r.status == wire_scan::GTX_BYRON;
  out[0] = r.status; out[1] = r.era; out[2] = r.byron_kind; out[3] = span ? r.off : 0; out[4] = span ? r.len : 0;
}
"""

# reads "n_eras hex\n" lines, prints the five fields of each item parsed from an exact-size heap copy
MAIN = r"""
#include "wire_scan.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<char> line(1 << 20);
  while (std::fgets(line.data(), (int)line.size(), f)) {
    char* sp = std::strchr(line.data(), ' ');
    if (!sp) return 3;
    const unsigned n_eras = (unsigned)std::strtoul(line.data(), nullptr, 10);
    const char* hex = sp + 1;
    size_t nh = std::strlen(hex);
    while (nh && (hex[nh - 1] == '\n' || hex[nh - 1] == '\r')) nh--;
    const size_t n = nh / 2;
    uint8_t* buf = (uint8_t*)std::malloc(n ? n : 1);          // exactly the item: a read past it is caught
    for (size_t k = 0; k < n; k++) {
      unsigned v;
      std::sscanf(hex + 2 * k, "%2x", &v);
      buf[k] = (uint8_t)v;
    }
    const wire_scan::Item r = wire_scan::gen_tx_unwrap(buf, n, 0, n, n_eras);
    const bool span = r.status == wire_scan::OK || r.status == wire_scan::TRAILING || r.status == wire_scan::GTX_BYRON;
    std::printf("%u %u %u %llu %u\n", (unsigned)r.status, (unsigned)r.era, (unsigned)r.byron_kind,
                (unsigned long long)(span ? r.off : 0), (unsigned)(span ? r.len : 0));
    if (wire_scan::gen_tx_unwrap(buf, n, n / 2, n - n / 2 + 1, n_eras).status != wire_scan::RANGE) return 4;
    std::free(buf);
  }
  std::fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("gentx")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "libgentx.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", HDR, str(src), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    L.t_gen_tx.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                           ctypes.POINTER(ctypes.c_uint64)]
    L.t_gen_tx.restype = None
    return L


def c_unwrap(L, buf, pos=0, length=None, n_eras=7):
    out = (ctypes.c_uint64 * 5)()
    L.t_gen_tx(bytes(buf), len(buf), pos, len(buf) - pos if length is None else length, n_eras, out)
    return tuple(int(x) for x in out)


def py_unwrap(buf, pos=0, length=None, n_eras=7):
    st, era, kind, off, ln = gm.unwrap(bytes(buf), pos, len(buf) - pos if length is None else length, n_eras)
    span = st in (gm.OK, gm.TRAILING, gm.BYRON)
    return (st, era, kind, off if span else 0, ln if span else 0)


def wrappers():
    """(item bytes, n_eras): the corpus's items, every truncation of five of them to the wrapper's
    end and a little further, and seeded single-byte mutations of the first 12 bytes"""
    items, g = golden_items()
    items.append(bytes.fromhex(g["byron"]["gen_tx"]))
    items += [it.bytes for it in gc.corpus()]
    out = [(b, 7) for b in items]
    picks = [it.bytes for it in gc.corpus() if it.name in ("wide_wrapper", "byron_2", "two_eras_4", "aux_null", "era_7")]
    assert len(picks) == 5
    for b in picks:
        out += [(b[:k], 7) for k in range(min(len(b), 16))]
    r = random.Random(20251019)
    for b in picks + items[:7]:
        for _ in range(60):
            v = bytearray(b[:64])
            v[r.randrange(min(12, len(v)))] = r.randrange(256)
            out.append((bytes(v), r.choice((7, 7, 1, 6, 32))))
    return out


def test_golden_gen_txs_unwrap(lib):
    items, g = golden_items()
    for k, raw in enumerate(items):
        st, era, kind, off, ln = c_unwrap(lib, raw)
        assert (st, era, kind, off + ln) == (gm.OK, k + 1, 0xFF, len(raw))
    raw = bytes.fromhex(g["byron"]["gen_tx"])
    assert c_unwrap(lib, raw) == (gm.BYRON, 0, 0, 4, 236)


def test_host_parser_equals_the_model_over_the_wrappers(lib):
    C = wrappers()
    hist = {}
    for raw, ne in C:
        got = c_unwrap(lib, raw, n_eras=ne)
        assert got == py_unwrap(raw, n_eras=ne), (raw.hex(), ne)
        hist[got[0]] = hist.get(got[0], 0) + 1
    assert all(hist.get(s, 0) > 0 for s in (gm.OK, gm.SYNTAX, gm.ERA, gm.TRAILING, gm.BYRON)), hist
    # the corpus's own expectations of the wrapper: every status but SHAPE is the wrapper's
    for it in gc.corpus():
        if "range" in it.tags:
            continue
        want = gm.OK if it.status == gm.SHAPE else it.status
        assert c_unwrap(lib, it.bytes)[0] == want, it.name
    # spans inside a larger arena, and spans that leave it
    raw = golden_items()[0][-1]
    arena = b"\x01\x02\x03" + raw + b"\x04"
    got = c_unwrap(lib, arena, 3, len(raw))
    assert (got[0], got[3] + got[4]) == (gm.OK, 3 + len(raw)) and got == py_unwrap(arena, 3, len(raw))
    assert c_unwrap(lib, arena, 3, len(raw) + 1)[0] == gm.TRAILING
    for pos, ln_ in ((len(arena) + 1, 0), (3, len(arena)), (0, len(arena) + 1), (1 << 63, 1 << 63)):
        assert c_unwrap(lib, arena, pos, ln_)[0] == gm.RANGE == py_unwrap(arena, pos, ln_)[0]
    assert c_unwrap(lib, arena, len(arena), 0)[0] == gm.SYNTAX


def test_wrappers_under_address_and_ub_sanitizers(tmp_path):
    """The parser over the same items in a stand-alone program built with ASan + UBSan: no read
    outside an item's own bytes, no undefined shift or overflow; its answers are the model's."""
    src = tmp_path / "gentx_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "gentx_main"
    # the sanitizer runtimes are linked into the program itself: it needs nothing from its environment
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", HDR, str(src), "-o", str(exe)], check=True)
    C = [(raw, ne) for raw, ne in wrappers() if len(raw) < 400000]
    inp = tmp_path / "items.txt"
    inp.write_text("".join(f"{ne} {raw.hex()}\n" for raw, ne in C))
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(C)
    for ln, (raw, ne) in zip(lines, C):
        assert tuple(int(x) for x in ln.split()) == py_unwrap(raw, n_eras=ne), raw.hex()
