// tx_dev.hpp -- the transaction-level walks shared by k_txindex.hip (stored blocks), k_txwit.hip
// (their key witnesses) and k_gentx.hip (wire GenTxs): the block kinds of the index, a map's
// walk to its first unsigned key, and the redeemers' ExUnits under key 5 of a witness set.
// Everything here has internal linkage, as in cbor_dev.hpp.
#pragma once
#include "cbor_dev.hpp"

namespace {

// what k_txi_count found a block to be
enum : uint8_t { TXK_NONE = 0, TXK_SHELLEY3 = 1, TXK_SHELLEY4 = 2, TXK_BYRON = 3, TXK_EBB = 4 };

// [mem, steps], both unsigned: the ExUnits of a redeemer
__device__ __forceinline__ bool rd_exunits(Cur& c, uint64_t& mem, uint64_t& steps) {
  Lvl x;
  return open_k(c, 2, x) && rd_uint(c, ~0ull, mem) && rd_uint(c, ~0ull, steps) && shut(c, x);
}

// the value under key 5 of a witness set: [[tag, index, data, [mem, steps]], ...] or Conway's
// {[tag, index]: [data, [mem, steps]], ...}; the sums mod 2^64, which mean something only when
// the walk succeeds (a caller drops them otherwise)
__device__ bool redeemer_units(Cur& c, uint64_t& mem_sum, uint64_t& steps_sum) {
  uint32_t mt;
  Lvl l;
  if (!open_any(c, mt, l) || (mt != 4 && mt != 5)) return false;
  bool ok = true;
  uint64_t sm = 0, ss = 0;
  while (ok && more(c, l, ok)) {
    Lvl e;
    uint64_t mem = 0, steps = 0;
    if (mt == 4) {
      ok = open_k(c, 4, e) && cbor_skip_regs(c) && cbor_skip_regs(c) && cbor_skip_regs(c) &&
           rd_exunits(c, mem, steps) && shut(c, e);
    } else {
      ok = cbor_skip_regs(c) && open_k(c, 2, e) && cbor_skip_regs(c) && rd_exunits(c, mem, steps) && shut(c, e);
    }
    sm += mem;
    ss += steps;
  }
  mem_sum = sm;
  steps_sum = ss;
  return ok;
}

// past a map's key, whose head (major type kmt) was read from ks, and its value; ok as in more()
__device__ __forceinline__ void skip_pair(Cur& c, uint64_t ks, uint32_t kmt, bool& ok) {
  if (kmt > 1) {   // not an integer: the head alone is not the whole key
    c.p = ks;
    ok = cbor_skip_regs(c);
  }
  ok = ok && cbor_skip_regs(c);
}

// the value under the first unsigned key `want` of the map at c: found = false when there is
// none (or c is no map and need_map is off); c is left at the value
__device__ bool find_key(Cur& c, uint64_t want, bool need_map, bool& found) {
  found = false;
  uint32_t mt;
  Lvl m;
  if (!open_any(c, mt, m)) return false;
  if (mt != 5) return !need_map;
  bool ok = true;
  while (ok && more(c, m, ok)) {
    const uint64_t ks = c.p;
    uint32_t kmt, ai;
    uint64_t arg;
    bool indef;
    if (!head(c, kmt, ai, arg, indef)) return false;
    if (kmt == 0 && arg == want) { found = true; return true; }
    skip_pair(c, ks, kmt, ok);
  }
  return ok;
}

}  // namespace
