// chunk_scan.hpp -- host-only item walk over a chunk file: the block boundaries
// parseChunkFile gets from decoding (Util/CBOR.hs:217-290), for the part of a
// chunk whose index offsets the device could not confirm.  chunk_item_end is
// k_block.hip's cbor_skip restated for the host (same rules as the oracle's
// block_integrity.cbor_skip); plain C++, compiled by g++ in tests/test_crc32_host.py.
#pragma once
#include <cstddef>
#include <cstdint>

namespace chunk_scan {

constexpr uint32_t MAX_INDEF = 16;
constexpr uint64_t BIG = 1ull << 62;

struct Cur {
  const uint8_t* a;
  uint64_t p, end;
};

inline bool head(Cur& c, uint32_t& mt, uint32_t& ai, uint64_t& arg, bool& indef) {
  if (c.p >= c.end) return false;
  const uint32_t ib = c.a[c.p++];
  mt = ib >> 5;
  ai = ib & 31u;
  indef = false;
  if (ai < 24) { arg = ai; return true; }
  if (ai <= 27) {
    const uint32_t nb = 1u << (ai - 24);
    if (nb > c.end - c.p) return false;
    uint64_t v = 0;
    for (uint32_t k = 0; k < nb; k++) v = (v << 8) | c.a[c.p + k];
    c.p += nb;
    arg = v;
    return true;
  }
  if (ai == 31 && (mt == 2 || mt == 3 || mt == 4 || mt == 5 || mt == 7)) { indef = true; arg = 0; return true; }
  return false;
}

// end offset of the ONE well-formed item at a[pos, end), or -1
inline int64_t chunk_item_end(const uint8_t* a, uint64_t pos, uint64_t end) {
  Cur c{a, pos, end};
  uint64_t need = 1;
  uint64_t st_need[MAX_INDEF];
  uint8_t st_kind[MAX_INDEF];
  uint32_t sp = 0;
  while (need || sp) {
    if (c.p >= c.end) return -1;
    if (c.a[c.p] == 0xFF) {
      if (!sp || need != BIG) return -1;
      need = st_need[--sp];
      c.p++;
      continue;
    }
    uint32_t mt, ai;
    uint64_t arg;
    bool indef;
    if (!head(c, mt, ai, arg, indef)) return -1;
    if (sp && need == BIG && st_kind[sp - 1] != 0 && (mt != st_kind[sp - 1] || indef)) return -1;
    if (need != BIG) need -= 1;
    if (mt == 2 || mt == 3) {
      if (indef) {
        if (sp == MAX_INDEF) return -1;
        st_need[sp] = need; st_kind[sp] = (uint8_t)mt; sp++;
        need = BIG;
      } else {
        if (arg > c.end - c.p) return -1;
        c.p += arg;
      }
    } else if (mt == 4 || mt == 5) {
      if (indef) {
        if (sp == MAX_INDEF) return -1;
        st_need[sp] = need; st_kind[sp] = 0; sp++;
        need = BIG;
      } else {
        const uint64_t k = mt == 5 ? 2 * arg : arg;
        if (arg > c.end - c.p || k > c.end - c.p) return -1;
        need += k;
      }
    } else if (mt == 6) {
      need += 1;
    } else if (mt == 7) {
      if (ai == 24 && arg < 32) return -1;
    }
  }
  return (int64_t)c.p;
}

// a Byron block or EBB of the HardForkBlock encoding: [0, ...] / [1, ...]
// (a definite-length array whose first element is the unsigned integer 0 or 1).  Names the
// verdict of an item that ended the parse: UNSUPPORTED while Byron is off, ERR_READ once
// praos_validate_chunk_cfg decodes Byron items itself (k_byron.hip).
inline bool is_byron_item(const uint8_t* a, uint64_t pos, uint64_t end) {
  Cur c{a, pos, end};
  uint32_t mt, ai;
  uint64_t arg;
  bool indef;
  if (!head(c, mt, ai, arg, indef) || mt != 4 || indef || arg < 1) return false;
  return head(c, mt, ai, arg, indef) && mt == 0 && arg <= 1;
}

}  // namespace chunk_scan
