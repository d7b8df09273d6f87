// k_gentx.hip -- transactions as the TxSubmission server receives them: wire
// GenTxs of several peers, each distinct one indexed and hashed once; its key witnesses go through
// k_txwit.hip's passes unchanged (praos_gentx.hip).
//   k_gtx_split   one lane per item: wire_scan.hpp's gen_tx_unwrap, then the top-level walk of the
//                 inner bytes -- one array [body, wits, (isValid,) aux / null], definite or
//                 indefinite, nothing after it -- with cbor_skip_regs (spans, is_valid, size), and
//                 Blake2b-256 of the inner bytes (b2b256_range), the key of the dedup.
//   k_gtx_ident   the hash set's arrays for a numbering without a hash set: every flagged index
//                 its own class (dedup off; the second numbering that drops the rows k_gtx_rows
//                 refused).  k_wire.hip's count / scan / rows / map kernels number both.
//   k_gtx_rep     row_item[row] = the representative item of each provisional row.
//   k_gtx_rows    one lane per provisional row: the body is a map; for eras >= 4 the witness set's
//                 first key 5 (ex_mem, ex_steps, both redeemer forms); tx_id = Blake2b-256 of the
//                 body with the message blocks staged through LDS as k_txi_final stages them.
//   k_gtx_final   one lane per index, in two roles: as a provisional row that stayed, its fields
//                 gathered to its final row; as an item, its final row -- or PRAOS_GTX_SHAPE and no
//                 row when k_gtx_rows refused its transaction.
// The walks read item heads with byte loads, one lane per transaction, as k_txi_rows does: they
// are latency-bound and short beside the verifies.
// CPU restatement: tests/gentx_model.py.
#include "byron_dev.hpp"
#include "wire_scan.hpp"

namespace {

constexpr uint32_t NONE = 0xffffffffu;

// one level of an array or a map, as k_txindex.hip walks them (its helpers are local to it)
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
__device__ __forceinline__ bool open_k(Cur& c, uint64_t k, Lvl& l) {
  uint32_t mt;
  return open_any(c, mt, l) && mt == 4 && (l.indef || l.left == k);
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
__device__ __forceinline__ bool rd_u(Cur& c, uint64_t& v) {
  uint32_t mt, ai;
  bool indef;
  return head(c, mt, ai, v, indef) && mt == 0;
}

__global__ void __launch_bounds__(NT) k_gtx_split(size_t n, const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                  const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                  uint32_t n_eras, praos_gtx_dev_items d) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const wire_scan::Item r = wire_scan::gen_tx_unwrap(arena, arena_len, off[i], len[i], n_eras);
  uint8_t st = r.status, valid = 1;
  uint64_t b0 = 0, w0 = 0, x0 = 0;
  uint32_t bl = 0, wl = 0, xl = 0, sz = 0;
  if (st == wire_scan::OK) {
    Cur c{arena, r.off, r.off + r.len, true};
    const uint64_t want = r.era <= 3 ? 3 : 4;
    Lvl l;
    bool ok = open_k(c, want, l);
    b0 = c.p;
    ok = ok && cbor_skip_regs(c);
    w0 = c.p;
    ok = ok && cbor_skip_regs(c);
    const uint64_t w1 = c.p;
    if (ok && want == 4) {
      ok = c.p < c.end && (c.a[c.p] == 0xF4 || c.a[c.p] == 0xF5);
      if (ok) valid = c.a[c.p++] == 0xF5 ? 1 : 0;
    }
    x0 = c.p;
    ok = ok && cbor_skip_regs(c);
    const uint64_t x1 = c.p;
    ok = ok && shut(c, l) && c.p == c.end;
    if (ok) {
      bl = (uint32_t)(w0 - b0);
      wl = (uint32_t)(w1 - w0);
      xl = (uint32_t)(x1 - x0);
      sz = 1u + bl + wl + xl;                     // sizeTxF: the last item as stored (null: one byte)
      if (xl == 1 && arena[x0] == 0xF6) { x0 = 0; xl = 0; }
    } else {
      st = PRAOS_GTX_SHAPE;
    }
  }
  const bool ok = st == wire_scan::OK, byr = st == wire_scan::GTX_BYRON;
  d.status[i] = st;
  d.era[i] = r.era;
  d.kind[i] = r.byron_kind;
  d.ioff[i] = byr ? r.off : 0ull;               // a Byron item's payload span (the numbering copies it,
  d.ilen[i] = byr ? r.len : 0u;                 // unread: Byron items have no row)
  d.body_off[i] = ok ? b0 : 0ull;
  d.body_len[i] = bl;
  d.wit_off[i] = ok ? w0 : 0ull;
  d.wit_len[i] = wl;
  d.aux_off[i] = ok ? x0 : 0ull;
  d.aux_len[i] = xl;
  d.size[i] = sz;
  d.is_valid[i] = valid;
  if (d.hash) {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) b2b256_range(w, arena, r.off, r.len);
    store_words(d.hash + 32 * i, w, 8);
  }
}

// item_slot[i] = i and slot_min[i] = i for a flagged index below *limit (limit NULL: n), NONE
// otherwise: k_hdr_count then finds every flagged index to be its own representative.  flag_ok:
// the value of flag[i] that counts.
__global__ void __launch_bounds__(NT) k_gtx_ident(size_t n, const uint32_t* __restrict__ limit,
                                                  const uint8_t* __restrict__ flag, uint8_t flag_ok,
                                                  uint32_t* __restrict__ item_slot, uint32_t* __restrict__ slot_min) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool in = (!limit || i < *limit) && flag[i] == flag_ok;
  item_slot[i] = in ? (uint32_t)i : NONE;
  slot_min[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(NT) k_gtx_rep(size_t n, const uint32_t* __restrict__ item_slot,
                                                const uint32_t* __restrict__ item_rep,
                                                const uint32_t* __restrict__ rep_row, uint32_t* __restrict__ row_item) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || item_slot[i] == NONE || item_rep[i] != (uint32_t)i) return;
  const uint32_t row = rep_row[i];
  if (row < n) row_item[row] = (uint32_t)i;
}

// [mem, steps], both unsigned: the ExUnits of a redeemer
__device__ __forceinline__ bool rd_exunits(Cur& c, uint64_t& mem, uint64_t& steps) {
  Lvl x;
  return open_k(c, 2, x) && rd_u(c, mem) && rd_u(c, steps) && shut(c, x);
}

// the value under key 5 of a witness set: [[tag, index, data, [mem, steps]], ...] or Conway's
// {[tag, index]: [data, [mem, steps]], ...}; the sums mod 2^64 (k_txindex.hip's redeemer_steps
// with the memory units kept)
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
    if (ok) { sm += mem; ss += steps; }
  }
  mem_sum = sm;
  steps_sum = ss;
  return ok;
}

// the value under the first unsigned key `want` of the map at c: found = false when there is
// none or c is no map; c is left at the value
__device__ bool find_key(Cur& c, uint64_t want, bool& found) {
  found = false;
  uint32_t mt;
  Lvl m;
  if (!open_any(c, mt, m)) return false;
  if (mt != 5) return true;
  bool ok = true;
  while (ok && more(c, m, ok)) {
    const uint64_t ks = c.p;
    uint32_t kmt, ai;
    uint64_t arg;
    bool indef;
    if (!head(c, kmt, ai, arg, indef)) return false;
    if (kmt == 0 && arg == want) { found = true; return true; }
    if (kmt > 1) {   // not an integer: the head alone is not the whole key
      c.p = ks;
      ok = cbor_skip_regs(c);
    }
    ok = ok && cbor_skip_regs(c);
  }
  return ok;
}

constexpr uint32_t GTX_STRIDE = 17;   // u64 words per staged message block (16 + 1 pad), as k_txi_final

// Provisional rows [0, *total).  tx_id: the workgroup loads the next 128-byte block of its 256
// bodies cooperatively (8 lanes x 16 bytes per body) into LDS and each lane compresses its own;
// the loop runs to the workgroup's longest body.
__global__ void __launch_bounds__(NT) k_gtx_rows(size_t n, const uint32_t* __restrict__ total,
                                                 const uint8_t* __restrict__ arena,
                                                 const uint32_t* __restrict__ row_item, praos_gtx_dev_items d,
                                                 uint8_t* __restrict__ row_ok, uint64_t* __restrict__ ex_mem,
                                                 uint64_t* __restrict__ ex_steps, uint8_t* __restrict__ tx_id) {
  __shared__ uint64_t sm[NT * GTX_STRIDE];
  __shared__ uint64_t s_pos[NT];
  __shared__ uint32_t s_len[NT];
  __shared__ uint32_t s_max;
  const uint32_t t = threadIdx.x;
  const size_t p = (size_t)blockIdx.x * NT + t;
  const size_t P = min((size_t)*total, n);
  bool act = false;
  uint64_t pos = 0;
  uint32_t len = 0;
  if (p < P) {
    const uint32_t i = row_item[p];
    if (i < n) {
      act = true;
      pos = d.body_off[i];
      len = d.body_len[i];
      bool ok = len != 0 && (arena[pos] >> 5) == 5;   // the body is a map
      uint64_t mem = 0, steps = 0;
      if (ok && d.era[i] >= 4) {
        const uint64_t wo = d.wit_off[i];
        Cur w{arena, wo, wo + d.wit_len[i], true};
        bool found;
        ok = find_key(w, 5, found);
        if (ok && found) ok = redeemer_units(w, mem, steps);
      }
      row_ok[p] = ok ? 1 : 0;
      ex_mem[p] = ok ? mem : 0ull;
      ex_steps[p] = ok ? steps : 0ull;
    } else {
      row_ok[p] = 0;   // a row without a representative: the numbering leaves none
      ex_mem[p] = 0;
      ex_steps[p] = 0;
    }
  }
  const uint32_t nblk = act ? (len == 0 ? 1u : (len + 127u) / 128u) : 0u;
  s_pos[t] = pos;
  s_len[t] = act ? len : 0u;
  if (t == 0) s_max = 0;
  __syncthreads();
  if (nblk) atomicMax(&s_max, nblk);
  __syncthreads();
  const uint32_t nb = s_max;
  uint64_t h[8];
#pragma unroll
  for (int w = 0; w < 8; w++) h[w] = B2B_IV[w];
  h[0] ^= 0x01010000ULL ^ 32u;
  for (uint32_t b = 0; b < nb; b++) {
#pragma unroll
    for (uint32_t rr = 0; rr < 8; rr++) {
      const uint32_t c = rr * NT + t, owner = c >> 3, part = c & 7u;
      const uint32_t olen = s_len[owner];
      const uint64_t off = (uint64_t)b * 128 + 16 * part;
      uint64_t w0 = 0, w1 = 0;
      if (off < olen) {
        const uint64_t opos = s_pos[owner];
        w0 = ld64u(arena, opos + off);
        if (off + 8 < olen) w1 = ld64u(arena, opos + off + 8);
      }
      sm[owner * GTX_STRIDE + 2 * part] = w0;
      sm[owner * GTX_STRIDE + 2 * part + 1] = w1;
    }
    __syncthreads();
    if (b < nblk) {
      uint64_t m[16];
      const uint64_t base = (uint64_t)b * 128;
#pragma unroll
      for (int k = 0; k < 16; k++) {
        const uint64_t off = base + 8 * k;
        uint64_t w = off < len ? sm[t * GTX_STRIDE + k] : 0;
        if (off < len && len - off < 8) w &= (1ull << (8 * (len - off))) - 1;
        m[k] = w;
      }
      const bool last = b + 1 == nblk;
      b2b_compress(h, m, last ? (uint64_t)len : base + 128, last);
    }
    __syncthreads();
  }
  if (!act) return;
  uint32_t out[8];
#pragma unroll
  for (int w = 0; w < 4; w++) { out[2 * w] = (uint32_t)h[w]; out[2 * w + 1] = (uint32_t)(h[w] >> 32); }
  store_words(tx_id + 32 * p, out, 8);
}

// index j as a provisional row: kept (row_ok) -> its final row row_final[j], the fields gathered
// there (rows below n always: the arrays hold n).  Index j as an item: item_row[j] is its
// provisional row on entry and its final row on return; an item whose row was refused becomes
// PRAOS_GTX_SHAPE.
__global__ void __launch_bounds__(NT) k_gtx_final(size_t n, const uint32_t* __restrict__ total,
                                                  const uint32_t* __restrict__ row_item,
                                                  const uint8_t* __restrict__ row_ok,
                                                  const uint32_t* __restrict__ row_final,
                                                  const uint64_t* __restrict__ ex_mem,
                                                  const uint64_t* __restrict__ ex_steps,
                                                  const uint8_t* __restrict__ tx_id, praos_gtx_dev_items d,
                                                  uint32_t* __restrict__ item_row, praos_gtx_dev_rows o) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const size_t P = min((size_t)*total, n);
  if (j < P && row_ok[j]) {
    const uint32_t q = row_final[j], i = row_item[j];
    if (q < n && i < n) {
      o.item[q] = i;
      o.era[q] = d.era[i];
      o.body_off[q] = d.body_off[i];
      o.body_len[q] = d.body_len[i];
      o.wit_off[q] = d.wit_off[i];
      o.wit_len[q] = d.wit_len[i];
      o.aux_off[q] = d.aux_off[i];
      o.aux_len[q] = d.aux_len[i];
      o.size[q] = d.size[i];
      o.in_block_size[q] = d.size[i] + PRAOS_GTX_PER_TX_OVERHEAD;
      o.ex_mem[q] = ex_mem[j];
      o.ex_steps[q] = ex_steps[j];
      o.is_valid[q] = d.is_valid[i];
      o.block[q] = 0;
      uint32_t w[8];
      load_words(w, tx_id + 32 * j, 8);
      store_words(o.tx_id + 32 * (size_t)q, w, 8);
    }
  }
  const uint32_t pr = item_row[j];
  if (pr != NONE) {
    const bool kept = pr < P && row_ok[pr];
    item_row[j] = kept ? row_final[pr] : NONE;
    if (!kept) d.status[j] = PRAOS_GTX_SHAPE;
  }
}

}  // namespace

// ---- host launchers (kernels are only launchable from their own module)
void launch_gtx_split(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                      const uint32_t* len, uint32_t n_eras, const praos_gtx_dev_items* items) {
  hipLaunchKernelGGL(k_gtx_split, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, arena, arena_len, off,
                     len, n_eras, *items);
}

void launch_gtx_ident(hipStream_t stream, size_t n, const uint32_t* limit, const uint8_t* flag, uint8_t flag_ok,
                      uint32_t* item_slot, uint32_t* slot_min) {
  hipLaunchKernelGGL(k_gtx_ident, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, limit, flag, flag_ok,
                     item_slot, slot_min);
}

void launch_gtx_rep(hipStream_t stream, size_t n, const uint32_t* item_slot, const uint32_t* item_rep,
                    const uint32_t* rep_row, uint32_t* row_item) {
  hipLaunchKernelGGL(k_gtx_rep, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, item_slot, item_rep,
                     rep_row, row_item);
}

void launch_gtx_rows(hipStream_t stream, size_t n, const uint32_t* total, const uint8_t* arena, const uint32_t* row_item,
                     const praos_gtx_dev_items* items, uint8_t* row_ok, uint64_t* ex_mem, uint64_t* ex_steps,
                     uint8_t* tx_id) {
  hipLaunchKernelGGL(k_gtx_rows, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, total, arena, row_item,
                     *items, row_ok, ex_mem, ex_steps, tx_id);
}

void launch_gtx_final(hipStream_t stream, size_t n, const uint32_t* total, const uint32_t* row_item,
                      const uint8_t* row_ok, const uint32_t* row_final, const uint64_t* ex_mem, const uint64_t* ex_steps,
                      const uint8_t* tx_id, const praos_gtx_dev_items* items, uint32_t* item_row,
                      const praos_gtx_dev_rows* rows) {
  hipLaunchKernelGGL(k_gtx_final, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, total, row_item, row_ok,
                     row_final, ex_mem, ex_steps, tx_id, *items, item_row, *rows);
}
