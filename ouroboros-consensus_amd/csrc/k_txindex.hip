// k_txindex.hip -- the transaction index of stored blocks: one row per
// transaction, built from the spans k_block_split / k_byron_split leave, and the per-block
// statistics db-analyser's ledger-free analyses print (HasAnalysis.countTxOutputs / blockTxSizes /
// blockStats, DBAnalyser/Block/Shelley.hs:61-98, Block/Byron.hs:34-86).
//
// A Shelley-based block is [header, s1 bodies, s2 witness sets, s3 {index: aux}, (s4 [invalid])],
// a Byron main block's txPayload a list of [tx, witnesses]; arrays and maps definite or
// indefinite at every level.
//   k_txi_count   one lane per block: the transaction count and the segment-level shape (s1, s2,
//                 s4 arrays, s3 a map, |s2| = |s1|, s3 keys and s4 entries unsigned < n).  A
//                 definite head gives its count without a walk (the split already found the
//                 segment to be one well-formed item).
//   k_txi_emit    the row spans at first[i] + t: one lane per (segment, block), segment-major as
//                 k_seg_hash is laid out (lane k*n + i walks segment k + 1 of block i: bodies,
//                 witness sets, the aux scatter, the invalid scatter), so the three long walks
//                 of a block run on different lanes (one lane per block walking the four in
//                 turn measured 0.11 ms slower over 4,096 blocks).
//   k_txi_rows    one lane per row: the body map's first key 1 (n_out), the witness set's first
//                 key 5 (ex_steps, both redeemer forms), size; a row that does not fit the shapes
//                 marks its block.
//   k_txi_reduce  one lane per block: the marked blocks become SHAPE with no rows, the others'
//                 row values are summed (u64).
//   k_txi_final   one lane per provisional row: its place among the rows of the blocks that
//                 stayed OK, the row's fields copied there, and tx_id = Blake2b-256 of the stored
//                 body bytes with the message blocks staged through LDS (arena.hpp
//                 b2b256_staged, which k_seg_hash calls too).
// The walks read item heads with byte loads, one lane per item sequence: neighbouring lanes
// are in different blocks (count, emit) or different transactions (rows), so their loads do not
// coalesce and their loops diverge; they are latency-bound and hidden by occupancy, as
// k_block_split's are.  Every byte of a body is read once more, coalesced, by k_txi_final.
// This is as far as the library decodes transactions: the reference's transaction decoders are
// stricter (duplicate keys, field types, canonical forms: a body whose items are well-formed
// CBOR but not a valid TxBody is a ReadFailure there, accepted here).
// CPU restatement: tests/tx_index_model.py.
#include "kcommon.hpp"
#include "arena.hpp"
#include "tx_dev.hpp"

namespace {

__global__ void __launch_bounds__(NT) k_txi_count(size_t n, const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                  const uint64_t* __restrict__ blk_off,
                                                  const uint32_t* __restrict__ blk_len, int byron,
                                                  const uint64_t* __restrict__ seg_off,
                                                  const uint32_t* __restrict__ seg_len, const uint8_t* __restrict__ nseg,
                                                  const uint8_t* __restrict__ split_status,
                                                  const uint8_t* __restrict__ byr_kind,
                                                  const uint32_t* __restrict__ txp_o, const uint32_t* __restrict__ txp_l,
                                                  uint32_t* __restrict__ cnt, uint8_t* __restrict__ status,
                                                  uint8_t* __restrict__ kind) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t off = blk_off[i];
  const uint32_t len = blk_len[i];
  uint8_t st = PRAOS_TXI_DECODE, kd = TXK_NONE;
  uint64_t nt = 0;
  if (off <= arena_len && len <= arena_len - off) {
    // a Byron item is a definite array whose first element is the unsigned integer 0 or 1
    // (chunk_scan.hpp is_byron_item): never read as a bare Shelley-based block
    Cur c{arena, off, off + len, true};
    uint32_t mt, ai;
    uint64_t arg, k01;
    bool indef;
    const bool byr = head(c, mt, ai, arg, indef) && mt == 4 && !indef && arg >= 1 && head(c, mt, ai, k01, indef) &&
                     mt == 0 && k01 <= 1;
    if (byr) {
      const uint32_t kb = byron ? byr_kind[i] : 3u;
      if (kb == 1) {
        st = PRAOS_TXI_OK;
        kd = TXK_EBB;
      } else if (kb == 2) {
        Cur t{arena, off + txp_o[i], off + txp_o[i] + txp_l[i], true};
        kd = TXK_BYRON;
        st = count_array(t, nt) ? PRAOS_TXI_OK : PRAOS_TXI_SHAPE;
      }
    } else if (split_status[i] == 0) {
      const uint32_t ns = nseg[i];
      kd = ns == 4 ? TXK_SHELLEY4 : TXK_SHELLEY3;
      auto seg = [&](uint32_t k) {
        const uint64_t o = seg_off[(size_t)k * n + i];
        return Cur{arena, o, o + seg_len[(size_t)k * n + i], true};
      };
      Cur s1 = seg(0), s2 = seg(1), s3 = seg(2);
      uint64_t n2 = 0;
      bool ok = count_array(s1, nt) && count_array(s2, n2) && n2 == nt;
      Lvl l;
      ok = ok && open(s3, 5, l);
      while (ok && more(s3, l, ok)) {
        uint64_t key;
        ok = rd_uint(s3, ~0ull, key) && key < nt && cbor_skip_regs(s3);
      }
      if (ok && ns == 4) {
        Cur s4 = seg(3);
        ok = open(s4, 4, l);
        while (ok && more(s4, l, ok)) {
          uint64_t idx;
          ok = rd_uint(s4, ~0ull, idx) && idx < nt;
        }
      }
      st = ok ? PRAOS_TXI_OK : PRAOS_TXI_SHAPE;
    }
  }
  if (st != PRAOS_TXI_OK) nt = 0;
  cnt[i] = (uint32_t)nt;   // an item takes a byte at least and a block's length is u32
  status[i] = st;
  kind[i] = kd;
}

// the row arrays (provisional rows, and the caller's selection of the final ones)
typedef praos_txi_dev_rows TxRows;

// part k of block i: 0 bodies (Byron: the [tx, witnesses] pairs), 1 witness sets, 2 aux, 3 invalid.
// The arrays come zeroed (is_valid: ones); t < nt and idx < nt hold by k_txi_count's walk and
// are checked again before every store.
__device__ void emit_part(uint32_t k, size_t i, size_t n, const uint8_t* __restrict__ arena,
                          const uint64_t* __restrict__ blk_off, const uint64_t* __restrict__ seg_off,
                          const uint32_t* __restrict__ seg_len, const uint32_t* __restrict__ txp_o,
                          const uint32_t* __restrict__ txp_l, uint32_t kd, uint32_t base, uint32_t nt,
                          const TxRows& r) {
  bool ok = true;
  Lvl l;
  if (kd == TXK_BYRON) {
    if (k != 0) return;
    const uint64_t o = blk_off[i] + txp_o[i];
    Cur c{arena, o, o + txp_l[i], true};
    ok = open(c, 4, l);
    for (uint32_t t = 0; ok && t < nt && more(c, l, ok); t++) {
      const uint64_t s = c.p;
      Lvl pr;
      ok = open_k(c, 2, pr);
      const uint64_t b0 = c.p;
      ok = ok && cbor_skip_regs(c);
      const uint64_t w0 = c.p;
      ok = ok && cbor_skip_regs(c);
      const uint64_t w1 = c.p;
      ok = ok && shut(c, pr);
      if (!ok) break;
      r.body_off[base + t] = b0;
      r.body_len[base + t] = (uint32_t)(w0 - b0);
      r.wit_off[base + t] = w0;
      r.wit_len[base + t] = (uint32_t)(w1 - w0);
      r.size[base + t] = (uint32_t)(c.p - s);   // the annotation of the whole [tx, witnesses] item
    }
    return;
  }
  if (k == 3 && kd != TXK_SHELLEY4) return;
  const uint64_t o = seg_off[(size_t)k * n + i];
  Cur c{arena, o, o + seg_len[(size_t)k * n + i], true};
  if (k <= 1) {
    ok = open(c, 4, l);
    for (uint32_t t = 0; ok && t < nt && more(c, l, ok); t++) {
      const uint64_t s = c.p;
      if (!cbor_skip_regs(c)) break;
      if (k == 0) {
        r.body_off[base + t] = s;
        r.body_len[base + t] = (uint32_t)(c.p - s);
      } else {
        r.wit_off[base + t] = s;
        r.wit_len[base + t] = (uint32_t)(c.p - s);
      }
    }
  } else if (k == 2) {
    ok = open(c, 5, l);
    while (ok && more(c, l, ok)) {
      uint64_t key;
      if (!rd_uint(c, ~0ull, key)) break;
      const uint64_t s = c.p;
      if (!cbor_skip_regs(c)) break;
      if (key < nt) {   // a repeated key: the later entry stands
        r.aux_off[base + key] = s;
        r.aux_len[base + key] = (uint32_t)(c.p - s);
      }
    }
  } else {
    ok = open(c, 4, l);
    while (ok && more(c, l, ok)) {
      uint64_t idx;
      if (!rd_uint(c, ~0ull, idx)) break;
      if (idx < nt) r.is_valid[base + idx] = 0;
    }
  }
}

__global__ void __launch_bounds__(NT) k_txi_emit(size_t n, const uint8_t* __restrict__ arena,
                                                 const uint64_t* __restrict__ blk_off,
                                                 const uint64_t* __restrict__ seg_off,
                                                 const uint32_t* __restrict__ seg_len,
                                                 const uint32_t* __restrict__ txp_o, const uint32_t* __restrict__ txp_l,
                                                 const uint8_t* __restrict__ kind, const uint8_t* __restrict__ status,
                                                 const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ first,
                                                 TxRows r) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= 4 * n) return;
  const size_t k0 = j / n, i = j - k0 * n;
  if (status[i] != PRAOS_TXI_OK || cnt[i] == 0) return;
  const uint32_t kd = kind[i], base = first[i], nt = cnt[i];
  if (k0 == 0)   // every row knows its block, whatever the walks reach
    for (uint32_t t = 0; t < nt; t++) r.block[base + t] = (uint32_t)i;
  emit_part((uint32_t)k0, i, n, arena, blk_off, seg_off, seg_len, txp_o, txp_l, kd, base, nt, r);
}

__global__ void __launch_bounds__(NT) k_txi_rows(size_t nrows, const uint8_t* __restrict__ arena,
                                                 const uint8_t* __restrict__ kind, TxRows r,
                                                 uint32_t* __restrict__ bad) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nrows) return;
  const uint32_t i = r.block[p], kd = kind[i];
  const uint32_t bl = r.body_len[p], wl = r.wit_len[p], al = r.aux_len[p];
  Cur b{arena, r.body_off[p], r.body_off[p] + bl, true};
  bool ok = bl != 0 && wl != 0;   // a row the emit pass did not reach
  uint64_t nout = 0, mem = 0, steps = 0;   // the index keeps no memory units
  if (ok && kd == TXK_BYRON) {
    // tx = [inputs, outputs, attributes]: the items of tx[1]
    Lvl t;
    ok = open(b, 4, t);
    if (ok && more(b, t, ok)) ok = cbor_skip_regs(b); else ok = false;
    if (ok && more(b, t, ok)) ok = count_array(b, nout); else ok = false;
  } else if (ok) {
    bool found;
    ok = find_key(b, 1, true, found);
    if (ok && found) ok = count_array(b, nout);
    if (ok && kd == TXK_SHELLEY4) {
      Cur w{arena, r.wit_off[p], r.wit_off[p] + wl, true};
      ok = find_key(w, 5, false, found);
      if (ok && found) ok = redeemer_units(w, mem, steps);
    }
    r.size[p] = 1u + bl + wl + (al ? al : 1u);   // sizeTxF: [body, wits, aux or null]
  }
  if (!ok) { atomicOr(&bad[i], 1u); return; }
  r.n_out[p] = (uint32_t)nout;
  r.ex_steps[p] = steps;
}

__global__ void __launch_bounds__(NT) k_txi_reduce(size_t n, const uint32_t* __restrict__ cnt,
                                                   const uint32_t* __restrict__ first, const uint32_t* __restrict__ bad,
                                                   TxRows r, uint8_t* __restrict__ status, uint32_t* __restrict__ n_tx,
                                                   uint64_t* __restrict__ txs_size, uint64_t* __restrict__ n_out,
                                                   uint64_t* __restrict__ ex_steps) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t st = status[i];
  if (st == PRAOS_TXI_OK && bad[i]) st = PRAOS_TXI_SHAPE;
  uint64_t sz = 0, no = 0, ex = 0;
  uint32_t nt = 0;
  if (st == PRAOS_TXI_OK) {
    nt = cnt[i];
    const uint32_t base = first[i];
    for (uint32_t t = 0; t < nt; t++) {
      sz += r.size[base + t];
      no += r.n_out[base + t];
      ex += r.ex_steps[base + t];
    }
  }
  status[i] = st;
  n_tx[i] = nt;
  txs_size[i] = sz;
  n_out[i] = no;
  ex_steps[i] = ex;
}

// Provisional row p of a block that stayed OK lands at tfirst[i] + (p - first[i]).  tx_id: the
// workgroup hashes its 256 bodies together (b2b256_staged); rows neighbouring in a block are of
// similar size, and its loop runs to the workgroup's longest body.
__global__ void __launch_bounds__(NT) k_txi_final(size_t nrows, const uint8_t* __restrict__ arena,
                                                  const uint8_t* __restrict__ status,
                                                  const uint32_t* __restrict__ first,
                                                  const uint32_t* __restrict__ tfirst, TxRows r, TxRows o) {
  const size_t p = (size_t)blockIdx.x * NT + threadIdx.x;
  bool act = false;
  uint64_t pos = 0;
  uint32_t len = 0;
  size_t q = 0;
  if (p < nrows) {
    const uint32_t i = r.block[p];
    if (status[i] == PRAOS_TXI_OK && p - first[i] < tfirst[i + 1] - tfirst[i]) {
      act = true;
      q = (size_t)tfirst[i] + (p - first[i]);
      pos = r.body_off[p];
      len = r.body_len[p];
      if (o.block) o.block[q] = i;
      if (o.body_off) o.body_off[q] = pos;
      if (o.body_len) o.body_len[q] = len;
      if (o.wit_off) o.wit_off[q] = r.wit_off[p];
      if (o.wit_len) o.wit_len[q] = r.wit_len[p];
      if (o.aux_off) o.aux_off[q] = r.aux_off[p];
      if (o.aux_len) o.aux_len[q] = r.aux_len[p];
      if (o.size) o.size[q] = r.size[p];
      if (o.n_out) o.n_out[q] = r.n_out[p];
      if (o.ex_steps) o.ex_steps[q] = r.ex_steps[p];
      if (o.is_valid) o.is_valid[q] = r.is_valid[p];
    }
  }
  if (!o.tx_id) return;   // the same for every lane
  uint32_t out[8];
  b2b256_staged(out, arena, act, pos, len);   // every lane: it holds barriers
  if (!act) return;
  store_words(o.tx_id + 32 * q, out, 8);
}

}  // namespace

// ---- host launchers (kernels are only launchable from their own module)
void launch_txi_count(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* blk_off,
                      const uint32_t* blk_len, int byron, const uint64_t* seg_off, const uint32_t* seg_len,
                      const uint8_t* nseg, const uint8_t* split_status, const uint8_t* byr_kind, const uint32_t* txp_o,
                      const uint32_t* txp_l, uint32_t* cnt, uint8_t* status, uint8_t* kind) {
  hipLaunchKernelGGL(k_txi_count, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, arena, arena_len,
                     blk_off, blk_len, byron, seg_off, seg_len, nseg, split_status, byr_kind, txp_o, txp_l, cnt, status,
                     kind);
}

void launch_txi_emit(hipStream_t stream, size_t n, const uint8_t* arena, const uint64_t* blk_off,
                     const uint64_t* seg_off, const uint32_t* seg_len, const uint32_t* txp_o, const uint32_t* txp_l,
                     const uint8_t* kind, const uint8_t* status, const uint32_t* cnt, const uint32_t* first,
                     const praos_txi_dev_rows* rows) {
  hipLaunchKernelGGL(k_txi_emit, dim3((unsigned)((4 * n + NT - 1) / NT)), dim3(NT), 0, stream, n, arena, blk_off,
                     seg_off, seg_len, txp_o, txp_l, kind, status, cnt, first, *rows);
}

void launch_txi_rows(hipStream_t stream, size_t nrows, const uint8_t* arena, const uint8_t* kind,
                     const praos_txi_dev_rows* rows, uint32_t* bad) {
  hipLaunchKernelGGL(k_txi_rows, dim3((unsigned)((nrows + NT - 1) / NT)), dim3(NT), 0, stream, nrows, arena, kind,
                     *rows, bad);
}

void launch_txi_reduce(hipStream_t stream, size_t n, const uint32_t* cnt, const uint32_t* first, const uint32_t* bad,
                       const praos_txi_dev_rows* rows, uint8_t* status, uint32_t* n_tx, uint64_t* txs_size,
                       uint64_t* n_out, uint64_t* ex_steps) {
  hipLaunchKernelGGL(k_txi_reduce, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, cnt, first, bad,
                     *rows, status, n_tx, txs_size, n_out, ex_steps);
}

void launch_txi_final(hipStream_t stream, size_t nrows, const uint8_t* arena, const uint8_t* status,
                      const uint32_t* first, const uint32_t* tfirst, const praos_txi_dev_rows* rows,
                      const praos_txi_dev_rows* out) {
  hipLaunchKernelGGL(k_txi_final, dim3((unsigned)((nrows + NT - 1) / NT)), dim3(NT), 0, stream, nrows, arena, status,
                     first, tfirst, *rows, *out);
}
