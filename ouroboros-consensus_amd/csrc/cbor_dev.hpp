// cbor_dev.hpp -- the device-side CBOR item walk shared by the stored-bytes kernels
// (k_block.hip, k_byron.hip, k_pbft.hip, k_wire.hip, k_txindex.hip, k_txwit.hip, k_gentx.hip):
// item heads and the skip over one well-formed item, the rules of the oracle's
// block_integrity.cbor_skip; the strict readers of one item of a given form; and the walk of
// one level of an array or a map, definite or indefinite (Lvl: open*, more, shut).  Include
// inside the module's namespace-free scope; everything here has internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t MAX_INDEF = 16;          // nested indefinite items (oracle MAX_INDEF)
constexpr uint64_t BIG = 1ull << 62;        // "at an indefinite level" marker for `need`

struct Cur {
  const uint8_t* __restrict__ a;
  uint64_t p, end;
  bool ok;
};

// item head: major type, additional info, argument (indef = true for ai 31)
__device__ __forceinline__ bool head(Cur& c, uint32_t& mt, uint32_t& ai, uint64_t& arg, bool& indef) {
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
  return false;   // 28..30 reserved; indefinite uint / nint / tag
}

// advance c.p past ONE well-formed CBOR item (oracle block_integrity.cbor_skip)
__device__ bool cbor_skip(Cur& c) {
  uint64_t need = 1;
  uint64_t st_need[MAX_INDEF];
  uint8_t st_kind[MAX_INDEF];
  uint32_t sp = 0;
  while (need || sp) {
    if (c.p >= c.end) return false;
    if (c.a[c.p] == 0xFF) {
      if (!sp || need != BIG) return false;
      need = st_need[--sp];
      c.p++;
      continue;
    }
    uint32_t mt, ai;
    uint64_t arg;
    bool indef;
    if (!head(c, mt, ai, arg, indef)) return false;
    if (sp && need == BIG && st_kind[sp - 1] != 0 && (mt != st_kind[sp - 1] || indef)) return false;
    if (need != BIG) need -= 1;
    if (mt == 2 || mt == 3) {
      if (indef) {
        if (sp == MAX_INDEF) return false;
        st_need[sp] = need; st_kind[sp] = (uint8_t)mt; sp++;
        need = BIG;
      } else {
        if (arg > c.end - c.p) return false;
        c.p += arg;
      }
    } else if (mt == 4 || mt == 5) {
      if (indef) {
        if (sp == MAX_INDEF) return false;
        st_need[sp] = need; st_kind[sp] = 0; sp++;
        need = BIG;
      } else {
        const uint64_t k = mt == 5 ? 2 * arg : arg;
        if (arg > c.end - c.p || k > c.end - c.p) return false;   // each item takes >= 1 byte
        need += k;
      }
    } else if (mt == 6) {
      need += 1;
    } else if (mt == 7) {
      if (ai == 24 && arg < 32) return false;
    }
  }
  return true;
}

// cbor_skip with the indefinite-level stack held in registers (the saved counts selected by
// compares, the kinds packed two bits each): same rules, no scratch memory, for kernels that
// walk many items per lane
__device__ bool cbor_skip_regs(Cur& c) {
  uint64_t need = 1;
  uint64_t st_need[MAX_INDEF];
  uint32_t kinds = 0;   // 2 bits per level: 0 container, 2 / 3 string of that major type
  uint32_t sp = 0;
#pragma unroll
  for (uint32_t j = 0; j < MAX_INDEF; j++) st_need[j] = 0;
  while (need || sp) {
    if (c.p >= c.end) return false;
    if (c.a[c.p] == 0xFF) {
      if (!sp || need != BIG) return false;
      sp--;
#pragma unroll
      for (uint32_t j = 0; j < MAX_INDEF; j++) need = j == sp ? st_need[j] : need;
      c.p++;
      continue;
    }
    uint32_t mt, ai;
    uint64_t arg;
    bool indef;
    if (!head(c, mt, ai, arg, indef)) return false;
    const uint32_t top = sp ? (kinds >> (2 * (sp - 1))) & 3u : 0u;
    if (sp && need == BIG && top != 0 && (mt != top || indef)) return false;
    if (need != BIG) need -= 1;
    if (mt == 2 || mt == 3 || mt == 4 || mt == 5) {
      if (indef) {
        if (sp == MAX_INDEF) return false;
#pragma unroll
        for (uint32_t j = 0; j < MAX_INDEF; j++) st_need[j] = j == sp ? need : st_need[j];
        kinds = (kinds & ~(3u << (2 * sp))) | ((mt <= 3 ? mt : 0u) << (2 * sp));
        sp++;
        need = BIG;
      } else if (mt <= 3) {
        if (arg > c.end - c.p) return false;
        c.p += arg;
      } else {
        const uint64_t k = mt == 5 ? 2 * arg : arg;
        if (arg > c.end - c.p || k > c.end - c.p) return false;   // each item takes >= 1 byte
        need += k;
      }
    } else if (mt == 6) {
      need += 1;
    } else if (mt == 7) {
      if (ai == 24 && arg < 32) return false;
    }
  }
  return true;
}

// ---- strict readers: one item of exactly the given form
__device__ __forceinline__ bool rd_uint(Cur& c, uint64_t limit, uint64_t& v) {
  uint32_t mt, ai;
  bool indef;
  return head(c, mt, ai, v, indef) && mt == 0 && v <= limit;
}
__device__ __forceinline__ bool rd_list(Cur& c, uint64_t n) {
  uint32_t mt, ai;
  uint64_t arg;
  bool indef;
  return head(c, mt, ai, arg, indef) && mt == 4 && !indef && arg == n;
}
// a definite byte string of exactly n bytes; at = offset of the raw bytes
__device__ __forceinline__ bool rd_bytes(Cur& c, uint64_t n, uint64_t& at) {
  uint32_t mt, ai;
  uint64_t arg;
  bool indef;
  if (!(head(c, mt, ai, arg, indef) && mt == 2 && !indef && arg == n && n <= c.end - c.p)) return false;
  at = c.p;
  c.p += n;
  return true;
}

// ---- the level walker: an array or a map, definite or indefinite, item by item
// one level of an array or a map: items (pairs) left, or indefinite
struct Lvl {
  uint64_t left;
  bool indef;
};

__device__ __forceinline__ bool open_any(Cur& c, uint32_t& mt, Lvl& l) {
  uint32_t ai;
  uint64_t arg;
  bool indef;
  if (!head(c, mt, ai, arg, indef)) return false;
  l.left = arg;
  l.indef = indef;
  return true;
}
__device__ __forceinline__ bool open(Cur& c, uint32_t want, Lvl& l) {
  uint32_t mt;
  return open_any(c, mt, l) && mt == want;
}
// an array of exactly k items (a definite head says so; an indefinite one is checked by shut)
__device__ __forceinline__ bool open_k(Cur& c, uint64_t k, Lvl& l) {
  return open(c, 4, l) && (l.indef || l.left == k);
}
__device__ __forceinline__ bool shut(Cur& c, const Lvl& l) {
  if (!l.indef) return true;
  if (c.p >= c.end || c.a[c.p] != 0xFF) return false;
  c.p++;
  return true;
}
// another item (pair) at this level?  Consumes the break of an indefinite level.
__device__ __forceinline__ bool more(Cur& c, Lvl& l, bool& ok) {
  if (l.indef) {
    if (c.p >= c.end) { ok = false; return false; }
    if (c.a[c.p] == 0xFF) { c.p++; return false; }
    return true;
  }
  if (l.left == 0) return false;
  l.left--;
  return true;
}

// items of the array at c (count only; c is left inside a definite array)
__device__ bool count_array(Cur& c, uint64_t& cnt) {
  Lvl l;
  if (!open(c, 4, l)) return false;
  if (!l.indef) { cnt = l.left; return true; }
  bool ok = true;
  uint64_t k = 0;
  while (more(c, l, ok)) {
    if (!cbor_skip_regs(c)) return false;
    k++;
  }
  cnt = k;
  return ok;
}

}  // namespace
