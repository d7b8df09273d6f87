// k_wire.hip -- wire headers (the node-to-node encoding a ChainSync client receives) on the
// device: unwrap + hash, and the row set of every wire call (candidates, GenTxs, BlockFetch blocks;
// api_internal.hpp RowSet): which of n items are the same, and the row of each
// distinct one in order of first appearance.
//   k_wire_split   one lane per item: wire_scan.hpp's unwrap, then the header hash of the inner
//                  bytes -- Blake2b-256 (b2b256_range) for a Shelley-based item, Blake2b-256 of
//                  82 0k || header (b2b256_pre, what k_pbft_decode writes) for a Byron one.
//   k_hdr_dedup    the set: a hash set over (tag, 32-byte key), whole keys compared; every member
//                  of a class lowers the slot's minimum item index (atomicMin), so the class's
//                  representative is its lowest item whatever order the lanes arrive in.
//   k_hdr_ident    the set's arrays without a set: every flagged index below a limit its own class.
//   k_hdr_count / k_hdr_scan / k_hdr_rows / k_hdr_map
//                  the numbering: flag the representatives, scan the flags (block counts, one block
//                  over the counts, block-local offsets) so that rows are numbered in order of
//                  first appearance, write the representatives' spans compacted and each item's row.
//   k_hdr_rep      the representative item of each row.
//   k_hdr_row_kind gathers the Byron kind of each row's representative (the PBFT candidates call).
#include "byron_dev.hpp"
#include "wire_scan.hpp"

namespace {

constexpr uint32_t NONE = 0xffffffffu;

__global__ void __launch_bounds__(NT) k_wire_split(size_t n, const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                   const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                   uint32_t n_eras, uint8_t* __restrict__ status,
                                                   uint8_t* __restrict__ era, uint8_t* __restrict__ kind,
                                                   uint32_t* __restrict__ hint, uint64_t* __restrict__ ioff,
                                                   uint32_t* __restrict__ ilen, uint8_t* __restrict__ hash) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const wire_scan::Item r = wire_scan::wire_unwrap(arena, arena_len, off[i], len[i], n_eras);
  const bool ok = r.status == wire_scan::OK;
  status[i] = r.status;
  era[i] = r.era;
  kind[i] = r.byron_kind;
  hint[i] = r.size_hint;
  ioff[i] = ok ? r.off : 0ull;
  ilen[i] = ok ? r.len : 0u;
  if (hash) {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
      // (a Byron inner span starts at least 8 bytes into its item, so the two prefix bytes
      // b2b256_pre overlays lie inside the arena)
      if (r.era == 0) b2b256_pre(w, arena, r.off, r.len, 2, 0x82u | (r.byron_kind ? 0x100u : 0u));
      else b2b256_range(w, arena, r.off, r.len);
    }
    store_words(hash + 32 * i, w, 8);
  }
}

// slot_item[h] = 1 + some item of the class (0: empty), slot_min[h] = the class's lowest item
// (NONE before the first), item_slot[i] = the item's slot (NONE: not in the set).  Probing is
// bounded by the table size; a table of >= 2n slots always has room.  In the set: flag[i] 0
// (wire_scan::OK where it is an unwrap status) and tag[i] below 32 and in tag_mask.
__global__ void __launch_bounds__(NT) k_hdr_dedup(size_t n, const uint8_t* __restrict__ flag,
                                                  const uint8_t* __restrict__ tag, const uint8_t* __restrict__ key,
                                                  uint32_t tag_mask, uint32_t mask, uint32_t* slot_item,
                                                  uint32_t* slot_min, uint32_t* __restrict__ item_slot) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t mine = NONE;
  const uint32_t e = tag[i];
  if (flag[i] == wire_scan::OK && e < 32 && ((tag_mask >> e) & 1u)) {
    uint32_t t[8];
    load_words(t, key + 32 * i, 8);
    uint32_t h = (t[0] ^ (e * 0x9E3779B1u)) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++) {
      const uint32_t cur = atomicCAS(&slot_item[h], 0u, (uint32_t)i + 1u);
      bool same = cur == 0u;                          // first of its class to arrive
      if (!same) {
        uint32_t o[8];
        load_words(o, key + 32 * (size_t)(cur - 1u), 8);
        same = tag[cur - 1u] == e;
#pragma unroll
        for (int q = 0; q < 8; q++) same &= o[q] == t[q];
      }
      if (same) { mine = h; atomicMin(&slot_min[h], (uint32_t)i); break; }
      h = (h + 1u) & mask;
    }
  }
  item_slot[i] = mine;
}

// item_slot[i] = i and slot_min[i] = i for a flagged index below *limit (limit NULL: n), NONE
// otherwise: k_hdr_count then finds every flagged index to be its own representative.  flag_ok:
// the value of flag[i] that counts.
__global__ void __launch_bounds__(NT) k_hdr_ident(size_t n, const uint32_t* __restrict__ limit,
                                                  const uint8_t* __restrict__ flag, uint8_t flag_ok,
                                                  uint32_t* __restrict__ item_slot, uint32_t* __restrict__ slot_min) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool in = (!limit || i < *limit) && flag[i] == flag_ok;
  item_slot[i] = in ? (uint32_t)i : NONE;
  slot_min[i] = (uint32_t)i;
}

// item_rep[i] = the class's lowest item (i itself for an item outside the set: it gets no row);
// blk_cnt[b] = representatives in block b
__global__ void __launch_bounds__(NT) k_hdr_count(size_t n, const uint32_t* __restrict__ item_slot,
                                                  const uint32_t* __restrict__ slot_min,
                                                  uint32_t* __restrict__ item_rep, uint32_t* __restrict__ blk_cnt) {
  __shared__ uint32_t wcnt[NT / 64];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool flag = false;
  if (i < n) {
    const uint32_t s = item_slot[i];
    const uint32_t rep = s == NONE ? (uint32_t)i : slot_min[s];
    item_rep[i] = rep;
    flag = s != NONE && rep == (uint32_t)i;
  }
  const unsigned long long b = __ballot(flag);
  if ((threadIdx.x & 63u) == 0) wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < NT / 64; w++) s += wcnt[w];
    blk_cnt[blockIdx.x] = s;
  }
}

// exclusive scan of blk_cnt[0, nb) in place by one block; *total = the sum
constexpr int SCAN_NT = 1024;
__global__ void __launch_bounds__(SCAN_NT) k_hdr_scan(uint32_t nb, uint32_t* blk_cnt, uint32_t* total) {
  __shared__ uint32_t part[SCAN_NT];
  const uint32_t per = (nb + SCAN_NT - 1) / SCAN_NT;
  const uint32_t lo = min(nb, threadIdx.x * per), hi = min(nb, lo + per);
  uint32_t s = 0;
  for (uint32_t k = lo; k < hi; k++) s += blk_cnt[k];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < SCAN_NT; d <<= 1) {             // inclusive scan of the partial sums
    const uint32_t v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0u;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t base = threadIdx.x ? part[threadIdx.x - 1] : 0u;
  for (uint32_t k = lo; k < hi; k++) {
    const uint32_t c = blk_cnt[k];
    blk_cnt[k] = base;
    base += c;
  }
  if (threadIdx.x == SCAN_NT - 1) *total = part[SCAN_NT - 1];
}

// row of each representative = representatives before it; its span goes to row_off / row_len
// (rows below rows_cap only: the caller learns the count from *total and asks again)
__global__ void __launch_bounds__(NT) k_hdr_rows(size_t n, const uint32_t* __restrict__ item_slot,
                                                 const uint32_t* __restrict__ item_rep,
                                                 const uint32_t* __restrict__ blk_base,
                                                 const uint64_t* __restrict__ ioff, const uint32_t* __restrict__ ilen,
                                                 uint32_t rows_cap, uint64_t* __restrict__ row_off,
                                                 uint32_t* __restrict__ row_len, uint32_t* __restrict__ rep_row) {
  __shared__ uint32_t wcnt[NT / 64];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool flag = i < n && item_slot[i] != NONE && item_rep[i] == (uint32_t)i;
  const unsigned long long b = __ballot(flag);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  if (!flag) return;
  uint32_t row = blk_base[blockIdx.x] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
  for (uint32_t w = 0; w < wave; w++) row += wcnt[w];
  rep_row[i] = row;
  if (row < rows_cap) {
    row_off[row] = ioff[i];
    row_len[row] = ilen[i];
  }
}

__global__ void __launch_bounds__(NT) k_hdr_map(size_t n, const uint32_t* __restrict__ item_slot,
                                                const uint32_t* __restrict__ item_rep,
                                                const uint32_t* __restrict__ rep_row, uint32_t* __restrict__ item_row) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  item_row[i] = item_slot[i] == NONE ? NONE : rep_row[item_rep[i]];
}

// row_item[row] = the representative of each row below n (row_item set to 0xff by the caller)
__global__ void __launch_bounds__(NT) k_hdr_rep(size_t n, const uint32_t* __restrict__ item_slot,
                                                const uint32_t* __restrict__ item_rep,
                                                const uint32_t* __restrict__ rep_row, uint32_t* __restrict__ row_item) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || item_slot[i] == NONE || item_rep[i] != (uint32_t)i) return;
  const uint32_t row = rep_row[i];
  if (row < n) row_item[row] = (uint32_t)i;
}

// row_is_ebb[row] = 1 when the row's representative is a Byron item of kind 0 (an EBB): a Byron
// row's kind travels with its span (k_pbft_decode reads a header by its kind).  After k_hdr_rows;
// rows below rows_cap only, as there.
__global__ void __launch_bounds__(NT) k_hdr_row_kind(size_t n, const uint32_t* __restrict__ item_slot,
                                                     const uint32_t* __restrict__ item_rep,
                                                     const uint32_t* __restrict__ rep_row,
                                                     const uint8_t* __restrict__ kind, uint32_t rows_cap,
                                                     uint8_t* __restrict__ row_is_ebb) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || item_slot[i] == NONE || item_rep[i] != (uint32_t)i) return;
  const uint32_t row = rep_row[i];
  if (row < rows_cap) row_is_ebb[row] = kind[i] == 0 ? 1 : 0;
}

}  // namespace

// ---- host launchers
void launch_wire_split(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                       const uint32_t* len, uint32_t n_eras, uint8_t* status, uint8_t* era, uint8_t* kind,
                       uint32_t* hint, uint64_t* ioff, uint32_t* ilen, uint8_t* hash) {
  if (!n) return;
  hipLaunchKernelGGL(k_wire_split, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, arena, arena_len, off,
                     len, n_eras, status, era, kind, hint, ioff, ilen, hash);
}

// ---- the row set (launch.hpp has the arrays' sizes)
void launch_hdr_set(hipStream_t stream, size_t n, const uint8_t* flag, const uint8_t* tag, const uint8_t* key,
                    uint32_t tag_mask, uint32_t mask, uint32_t* slot_item, uint32_t* slot_min, uint32_t* item_slot) {
  if (!n) return;
  hipLaunchKernelGGL(k_hdr_dedup, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, flag, tag, key, tag_mask,
                     mask, slot_item, slot_min, item_slot);
}

void launch_hdr_ident(hipStream_t stream, size_t n, const uint32_t* limit, const uint8_t* flag, uint8_t flag_ok,
                      uint32_t* item_slot, uint32_t* slot_min) {
  if (!n) return;
  hipLaunchKernelGGL(k_hdr_ident, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, limit, flag, flag_ok,
                     item_slot, slot_min);
}

void launch_hdr_count(hipStream_t stream, size_t n, const uint32_t* item_slot, const uint32_t* slot_min,
                      uint32_t* item_rep, uint32_t* blk) {
  if (!n) return;
  hipLaunchKernelGGL(k_hdr_count, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, item_slot, slot_min,
                     item_rep, blk);
}

void launch_hdr_number(hipStream_t stream, size_t n, const uint32_t* item_slot, const uint32_t* slot_min,
                       uint32_t* item_rep, uint32_t* blk, uint32_t* total, const uint64_t* ioff, const uint32_t* ilen,
                       uint32_t rows_cap, uint64_t* row_off, uint32_t* row_len, uint32_t* rep_row, uint32_t* item_row) {
  if (!n) return;
  const dim3 g((unsigned)((n + NT - 1) / NT)), b(NT);
  launch_hdr_count(stream, n, item_slot, slot_min, item_rep, blk);
  hipLaunchKernelGGL(k_hdr_scan, dim3(1), dim3(SCAN_NT), 0, stream, g.x, blk, total);
  hipLaunchKernelGGL(k_hdr_rows, g, b, 0, stream, n, item_slot, item_rep, blk, ioff, ilen, rows_cap, row_off, row_len,
                     rep_row);
  hipLaunchKernelGGL(k_hdr_map, g, b, 0, stream, n, item_slot, item_rep, rep_row, item_row);
}

// after launch_hdr_number on the same stream
void launch_hdr_rep(hipStream_t stream, size_t n, const uint32_t* item_slot, const uint32_t* item_rep,
                    const uint32_t* rep_row, uint32_t* row_item) {
  if (!n) return;
  hipLaunchKernelGGL(k_hdr_rep, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, item_slot, item_rep,
                     rep_row, row_item);
}

// after launch_hdr_number on the same stream: row_is_ebb (rows_cap bytes) of the Byron rows
void launch_hdr_row_kind(hipStream_t stream, size_t n, const uint32_t* item_slot, const uint32_t* item_rep,
                         const uint32_t* rep_row, const uint8_t* kind, uint32_t rows_cap, uint8_t* row_is_ebb) {
  if (!n) return;
  hipLaunchKernelGGL(k_hdr_row_kind, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, item_slot, item_rep,
                     rep_row, kind, rows_cap, row_is_ebb);
}
