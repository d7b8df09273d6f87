"""Host checks of the wire-header parser (csrc/wire_scan.hpp).

The header is plain C++, so the exact text k_wire.hip includes is compiled here with g++: every
golden node-to-node header of the reference unwraps to the header item of the matching disk block,
the three disabled-era texts do not decode, and the C++ parser and praos_hip.wire agree on a
mutation corpus (wire_corpus.corpus).  The same corpus runs through a stand-alone program built with
-fsanitize=address,undefined, every item in a heap buffer of exactly its size."""
import ctypes
import os
import subprocess

import pytest

import wire_corpus as wc
from praos_hip import wire

HDR = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "ouroboros-consensus_amd", "csrc"))

SHIM = r"""
#include "wire_scan.hpp"
extern "C" void t_unwrap(const uint8_t* a, uint64_t arena_len, uint64_t pos, uint64_t len, uint32_t n_eras,
                         uint64_t out[6]) {
  const wire_scan::Item r = wire_scan::wire_unwrap(a, arena_len, pos, len, n_eras);
  const bool span = r.status == wire_scan::OK || r.status == wire_scan::TRAILING;
  out[0] = r.status; out[1] = r.era; out[2] = r.byron_kind; out[3] = r.size_hint;
  out[4] = span ? r.off : 0; out[5] = span ? r.len : 0;
}
"""

# reads "n_eras hex\n" lines, prints the six fields of each item parsed from an exact-size heap copy
MAIN = r"""
#include "wire_scan.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<char> line(1 << 16);
  unsigned long cases = 0;
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
    const wire_scan::Item r = wire_scan::wire_unwrap(buf, n, 0, n, n_eras);
    const bool span = r.status == wire_scan::OK || r.status == wire_scan::TRAILING;
    std::printf("%u %u %u %u %llu %u\n", (unsigned)r.status, (unsigned)r.era, (unsigned)r.byron_kind, (unsigned)r.size_hint,
                (unsigned long long)(span ? r.off : 0), (unsigned)(span ? r.len : 0));
    // the same item inside a larger arena, at an offset, and a span that leaves the arena
    const wire_scan::Item q = wire_scan::wire_unwrap(buf, n, n / 2, n - n / 2 + 1, n_eras);
    if (q.status != wire_scan::RANGE) return 4;
    std::free(buf);
    cases++;
  }
  std::fclose(f);
  std::fprintf(stderr, "%lu cases\n", cases);
  return 0;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("wire")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "libwire.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", HDR, str(src), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    L.t_unwrap.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                           ctypes.POINTER(ctypes.c_uint64)]
    L.t_unwrap.restype = None
    return L


def c_unwrap(L, buf, pos=0, length=None, n_eras=wire.N_ERAS):
    out = (ctypes.c_uint64 * 6)()
    L.t_unwrap(bytes(buf), len(buf), pos, len(buf) - pos if length is None else length, n_eras, out)
    return tuple(int(x) for x in out)


def py_unwrap(buf, pos=0, length=None, n_eras=wire.N_ERAS):
    st, era, kind, hint, off, ln = wire.unwrap(buf, pos, length, n_eras)
    return (st, era, kind, hint, off, ln)


def test_golden_headers_unwrap_to_the_disk_headers(lib):
    G = wc.golden()
    assert sum(len(h["versions"]) for h in G["headers"]) == 21
    seen = set()
    for h in G["headers"]:
        raw = bytes.fromhex(h["wire"])
        st, era, kind, hint, off, ln = c_unwrap(lib, raw)
        assert st == wire.WIRE_OK, h["name"]
        assert raw[off:off + ln] == bytes.fromhex(G["disk"][h["name"]]["header"]), h["name"]
        assert (era, kind, hint) == (h["era"], h["byron_kind"], h["size_hint"])
        seen.add(h["name"])
        if h["name"] == "Byron_EBB":
            assert (era, kind, hint) == (0, 0, 94)
        elif h["name"] == "Byron_regular":
            assert (era, kind, hint) == (0, 1, 869)
        else:
            assert kind == wire.NOT_BYRON and hint == 0
            # the wire index is not the disk tag: Byron takes two disk tags, one wire index
            assert era == G["disk"][h["name"]]["disk_tag"] - 1
    assert seen == {"Byron_EBB", "Byron_regular", "Shelley", "Allegra", "Mary", "Alonzo", "Babbage", "Conway"}
    babbage = next(h for h in G["headers"] if h["name"] == "Babbage")
    assert babbage["era"] == 5 and G["disk"]["Babbage"]["disk_tag"] == 6 and babbage["versions"] == [6, 7]


def test_disabled_era_texts_do_not_decode(lib):
    G = wc.golden()
    assert sorted((d["name"], d["version"]) for d in G["disabled"]) == [("Babbage", 5), ("Conway", 5), ("Conway", 6)]
    for d in G["disabled"]:
        raw = bytes.fromhex(d["wire"])
        assert raw.startswith(b"HardForkEncoderDisabledEra")
        assert c_unwrap(lib, raw)[0] == wire.WIRE_SYNTAX and py_unwrap(raw)[0] == wire.WIRE_SYNTAX


def test_host_parser_equals_python_over_the_corpus(lib):
    C = wc.corpus()
    assert len(C) >= 2000
    hist = {}
    for raw, ne in C:
        got, want = c_unwrap(lib, raw, n_eras=ne), py_unwrap(raw, n_eras=ne)
        assert got == want, (raw.hex(), ne)
        hist[got[0]] = hist.get(got[0], 0) + 1
    # the corpus reaches every status but RANGE (below), and accepts widened heads
    assert all(hist.get(s, 0) > 0 for s in (wire.WIRE_OK, wire.WIRE_SYNTAX, wire.WIRE_ERA, wire.WIRE_TRAILING)), hist
    assert hist[wire.WIRE_OK] >= 40
    # spans inside a larger arena, and spans that leave it
    raw = bytes.fromhex(wc.golden()["headers"][-1]["wire"])
    arena = b"\x01\x02\x03" + raw + b"\x04"
    st, era, kind, hint, off, ln = c_unwrap(lib, arena, 3, len(raw))
    assert (st, off + ln) == (wire.WIRE_OK, 3 + len(raw)) and py_unwrap(arena, 3, len(raw)) == (st, era, kind, hint, off, ln)
    assert c_unwrap(lib, arena, 3, len(raw) + 1)[0] == wire.WIRE_TRAILING
    for pos, ln_ in ((len(arena) + 1, 0), (3, len(arena)), (0, len(arena) + 1), (1 << 63, 1 << 63)):
        assert c_unwrap(lib, arena, pos, ln_)[0] == wire.WIRE_RANGE == py_unwrap(arena, pos, ln_)[0]
    assert c_unwrap(lib, arena, len(arena), 0)[0] == wire.WIRE_SYNTAX


def test_wrap_round_trips_and_widened_heads_are_accepted(lib):
    for era, kind, hint in ((0, 0, 94), (0, 1, 869), (1, None, 0), (5, None, 0), (6, None, 0)):
        hdr = bytes(range(200)) * 3
        raw = wire.wrap(era, hdr, kind, hint)
        st, e, k, h, off, ln = c_unwrap(lib, raw)
        assert (st, e, h, raw[off:off + ln]) == (wire.WIRE_OK, era, hint, hdr)
        assert k == (wire.NOT_BYRON if kind is None else kind)
        wide = wc.rebuild(era, kind if kind is not None else 0, hint, hdr, {j: 9 for j in range(8)})
        assert len(wide) > len(raw) and c_unwrap(lib, wide)[:4] == (st, e, k, h)


def test_corpus_under_address_and_ub_sanitizers(tmp_path):
    """The parser over the whole corpus in a stand-alone program built with ASan + UBSan: no read
    outside an item's own bytes, no undefined shift or overflow; its answers are the Python ones."""
    src = tmp_path / "wire_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "wire_main"
    # the sanitizer runtimes are linked into the program itself: it needs nothing from its environment
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", HDR, str(src), "-o", str(exe)], check=True)
    C = wc.corpus()
    inp = tmp_path / "corpus.txt"
    inp.write_text("".join(f"{ne} {raw.hex()}\n" for raw, ne in C))
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(C)
    for ln, (raw, ne) in zip(lines, C):
        assert tuple(int(x) for x in ln.split()) == py_unwrap(raw, n_eras=ne), raw.hex()
