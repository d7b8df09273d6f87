// k_gentx.hip -- transactions as the TxSubmission server receives them: wire
// GenTxs of several peers, each distinct one indexed and hashed once; its key witnesses go through
// k_txwit.hip's passes unchanged (praos_gentx.hip).
//   k_gtx_split   one lane per item: wire_scan.hpp's gen_tx_unwrap, then the top-level walk of the
//                 inner bytes -- one array [body, wits, (isValid,) aux / null], definite or
//                 indefinite, nothing after it -- with cbor_skip_regs (spans, is_valid, size), and
//                 Blake2b-256 of the inner bytes (b2b256_range), the key of the dedup.
//   (the provisional and the final rows are numbered by k_wire.hip's row set kernels: the hash
//   set or k_hdr_ident, the count / scan / rows / map kernels, k_hdr_rep.)
//   k_gtx_rows    one lane per provisional row: the body is a map; for eras >= 4 the witness set's
//                 first key 5 (ex_mem, ex_steps, both redeemer forms); tx_id = Blake2b-256 of the
//                 body with the message blocks staged through LDS (arena.hpp b2b256_staged, as
//                 k_txi_final).
//   k_gtx_final   one lane per index, in two roles: as a provisional row that stayed, its fields
//                 gathered to its final row; as an item, its final row -- or PRAOS_GTX_SHAPE and no
//                 row when k_gtx_rows refused its transaction.
// The walks read item heads with byte loads, one lane per transaction, as k_txi_rows does: they
// are latency-bound and short beside the verifies.
// CPU restatement: tests/gentx_model.py.
#include "byron_dev.hpp"
#include "tx_dev.hpp"
#include "wire_scan.hpp"

namespace {

constexpr uint32_t NONE = 0xffffffffu;

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

// Provisional rows [0, *total).  tx_id: the workgroup hashes its 256 bodies together
// (b2b256_staged); its loop runs to the workgroup's longest body.
__global__ void __launch_bounds__(NT) k_gtx_rows(size_t n, const uint32_t* __restrict__ total,
                                                 const uint8_t* __restrict__ arena,
                                                 const uint32_t* __restrict__ row_item, praos_gtx_dev_items d,
                                                 uint8_t* __restrict__ row_ok, uint64_t* __restrict__ ex_mem,
                                                 uint64_t* __restrict__ ex_steps, uint8_t* __restrict__ tx_id) {
  const size_t p = (size_t)blockIdx.x * NT + threadIdx.x;
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
        ok = find_key(w, 5, false, found);
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
  uint32_t out[8];
  b2b256_staged(out, arena, act, pos, len);   // every lane: it holds barriers
  if (!act) return;
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
