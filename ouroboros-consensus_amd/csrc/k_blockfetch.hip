// k_blockfetch.hip -- blocks as the BlockFetch client receives them: wire
// blocks of several peers, each distinct one split, hashed and indexed once.  The splits, the
// header decoders, the segment hashes, the Byron body proof, the hash set and the transaction
// passes are the stored-block kernels, launched unchanged by praos_blockfetch.hip; here are
//   k_bf_unwrap    one lane per item: wire_scan.hpp's wire_block_unwrap; status, disk tag and the
//                  inner span, which is the stored block every other kernel reads.
//   k_bf_key       one lane per item: whether it splits and decodes (it takes part in the
//                  numbering), the hash set's key -- the header hash with the inner length
//                  folded into its last word, so that (tag, hash, length) is what is classed --
//                  and a flag when any such item is a Byron one.
//   k_bf_class     one wave per item: a member of a class that is not its representative is
//                  compared with it byte for byte (span_equal_wave); equal, it keeps the
//                  representative; not equal, it becomes a class of its own.  Writes the arrays
//                  k_wire.hip's numbering kernels read (launch_hdr_number).
//   k_span_equal   the compare alone, one wave per pair (praos_debug_span_equal).
//   k_bf_rows      one lane per item: a representative's columns gathered to its row, the segment
//                  spans segment-major over the rows.
//   k_bf_bits      one lane per row: a Byron row takes k_byron_integrity's body half (the PBFT
//                  signature and protocol-magic bits are dropped: ChainSync checked the header).
//   k_bf_verdict   one lane per item: PRAOS_BF_* in the order of praos_hip.h.
//
// span_equal_wave is the one new hot path: a duplicate block costs one read of its bytes and of
// its representative's at memory speed, not a second Blake2b-256.  The two spans start at
// arbitrary, different offsets.  Span a is walked in 16-byte vectors from its first 16-byte
// boundary, lane l of the wave at vector l of each 1 KiB step, so that one load instruction
// covers whole consecutive lines; the same vectors of span b are loaded at whatever alignment
// they have (the unit splits a vector that straddles a line).  Four steps are loaded before the
// wave votes (4 KiB in flight per wave), and a difference ends the walk for every lane at once.
// The bytes before the first boundary and after the last whole vector are one byte per lane.
// Only bytes of the two spans are read.
// CPU restatement: tests/blockfetch_model.py.
#include "byron_dev.hpp"
#include "wire_scan.hpp"

namespace {

constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t EQ_VEC = PRAOS_SPAN_EQ_VEC, EQ_WAVE = PRAOS_SPAN_EQ_WAVE, EQ_TILE = PRAOS_SPAN_EQ_TILE;
constexpr uint32_t EQ_STEPS = EQ_TILE / EQ_WAVE;
static_assert(EQ_VEC == sizeof(uint4) && EQ_WAVE == 64 * EQ_VEC && EQ_TILE == EQ_STEPS * EQ_WAVE, "compare geometry");

__device__ __forceinline__ uint4 ld128a(const uint8_t* __restrict__ p) { return *(const uint4*)p; }
// 16 bytes at any alignment: one global_load_dwordx4 (the target takes unaligned vector loads)
__device__ __forceinline__ uint4 ld128u(const uint8_t* __restrict__ p) {
  uint4 v;
  __builtin_memcpy(&v, p, sizeof v);
  return v;
}
__device__ __forceinline__ uint32_t diff128(uint4 x, uint4 y) {
  return (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
}

// arena[a, a + len) == arena[b, b + len), by the whole wave (lane = 0..63); the result is uniform
__device__ __forceinline__ bool span_equal_wave(const uint8_t* __restrict__ arena, uint64_t a, uint64_t b, uint32_t len,
                                                uint32_t lane) {
  const uint32_t to_edge = (uint32_t)((0 - a) & (EQ_VEC - 1));
  const uint32_t pre = len < to_edge ? len : to_edge;
  bool diff = lane < pre && arena[a + lane] != arena[b + lane];
  const uint8_t* __restrict__ pa = arena + a + pre;        // 16-byte aligned from here on (or len is spent)
  const uint8_t* __restrict__ pb = arena + b + pre;
  const uint32_t rem = len - pre, nvec = rem / EQ_VEC, tail = rem % EQ_VEC;
  // the bytes after the last whole vector
  const uint64_t tb = (uint64_t)nvec * EQ_VEC;
  diff |= lane < tail && pa[tb + lane] != pb[tb + lane];
  if (__ballot(diff) != 0ull) return false;
  uint32_t v = 0;
  for (; v + EQ_STEPS * 64 <= nvec; v += EQ_STEPS * 64) {   // whole tiles
    uint4 x[EQ_STEPS], y[EQ_STEPS];
#pragma unroll
    for (uint32_t k = 0; k < EQ_STEPS; k++) {
      const uint64_t o = (uint64_t)(v + k * 64 + lane) * EQ_VEC;
      x[k] = ld128a(pa + o);
      y[k] = ld128u(pb + o);
    }
    uint32_t d = 0;
#pragma unroll
    for (uint32_t k = 0; k < EQ_STEPS; k++) d |= diff128(x[k], y[k]);
    if (__ballot(d != 0) != 0ull) return false;
  }
  uint32_t d = 0;
  for (; v < nvec; v += 64) {                               // the last, partial tile: wave steps
    const uint32_t idx = v + lane;
    if (idx < nvec) {
      const uint64_t o = (uint64_t)idx * EQ_VEC;
      d |= diff128(ld128a(pa + o), ld128u(pb + o));
    }
  }
  return __ballot(d != 0) == 0ull;
}

__global__ void __launch_bounds__(NT) k_span_equal(size_t n, const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                   const uint64_t* __restrict__ a_off,
                                                   const uint64_t* __restrict__ b_off, const uint32_t* __restrict__ len,
                                                   uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (i >= n) return;                                        // uniform over the wave
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t a = a_off[i], b = b_off[i];
  const uint32_t ln = len[i];
  const bool inside = a <= arena_len && ln <= arena_len - a && b <= arena_len && ln <= arena_len - b;
  const bool eq = inside && span_equal_wave(arena, a, b, ln, lane);
  if (lane == 0) out[i] = eq ? 1 : 0;
}

__global__ void __launch_bounds__(NT) k_bf_unwrap(size_t n, const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                  const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                  uint32_t n_eras, uint8_t* __restrict__ status,
                                                  uint8_t* __restrict__ tag, uint64_t* __restrict__ ioff,
                                                  uint32_t* __restrict__ ilen, uint64_t* __restrict__ hoff,
                                                  uint32_t* __restrict__ hlen) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const wire_scan::Item r = wire_scan::wire_block_unwrap(arena, arena_len, off[i], len[i], n_eras);
  const bool ok = r.status == wire_scan::OK;
  status[i] = r.status;
  tag[i] = r.era;
  ioff[i] = ok ? r.off : 0ull;
  ilen[i] = ok ? r.len : 0u;
  hoff[i] = ok ? r.off : 0ull;       // k_block_split's in / out columns: the block in, the header out
  hlen[i] = ok ? r.len : 0u;
}

// elig[i] = 0 (the hash set's "in" value, wire_scan::OK) for an item with a row, 1 otherwise
__global__ void __launch_bounds__(NT) k_bf_key(size_t n, const uint8_t* __restrict__ status,
                                               const uint8_t* __restrict__ split_status,
                                               const uint16_t* __restrict__ dec_status,
                                               const uint8_t* __restrict__ tag, const uint32_t* __restrict__ ilen,
                                               const uint8_t* __restrict__ header_hash, uint8_t* __restrict__ elig,
                                               uint8_t* __restrict__ key, uint32_t* __restrict__ any_byron) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool in = status[i] == wire_scan::OK && split_status[i] == 0 && !(dec_status[i] & PRAOS_DEC_FAILED);
  elig[i] = in ? 0 : 1;
  if (in && tag[i] <= 1) *any_byron = 1u;                    // (every writer stores the same word)
  if (key) {
    uint32_t w[8];
    load_words(w, header_hash + 32 * i, 8);
    w[7] ^= ilen[i];
    store_words(key + 32 * i, w, 8);
  }
}

__global__ void __launch_bounds__(NT) k_bf_class(size_t n, const uint8_t* __restrict__ arena,
                                                 const uint32_t* __restrict__ item_slot,
                                                 const uint32_t* __restrict__ item_rep,
                                                 const uint64_t* __restrict__ ioff, const uint32_t* __restrict__ ilen,
                                                 uint32_t* __restrict__ slot2, uint32_t* __restrict__ min2) {
  const size_t i = (size_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (i >= n) return;                                        // uniform over the wave
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t mine = NONE;
  if (item_slot[i] != NONE) {
    const uint32_t rep = item_rep[i];
    mine = (uint32_t)i;
    if (rep < i) {
      const uint32_t ln = ilen[i];
      if (ilen[rep] == ln && span_equal_wave(arena, ioff[i], ioff[rep], ln, lane)) mine = rep;
    }
  }
  if (lane == 0) {
    slot2[i] = mine;
    min2[i] = (uint32_t)i;
  }
}

__global__ void __launch_bounds__(NT) k_bf_rows(size_t n, size_t R, const uint32_t* __restrict__ slot2,
                                                const uint32_t* __restrict__ rep_row, praos_bf_dev_items d,
                                                praos_bf_dev_rows o) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || slot2[i] != (uint32_t)i) return;
  const size_t q = rep_row[i];
  if (q >= R) return;
  o.item[q] = (uint32_t)i;
  o.tag[q] = d.tag[i];
  o.is_ebb[q] = d.kind[i] == 1 ? 1 : 0;
  o.slot[q] = d.slot[i];
  o.block_no[q] = d.block_no[i];
  o.hdr_off[q] = d.hoff[i];
  o.hdr_len[q] = d.hlen[i];
  uint32_t w[8];
  load_words(w, d.header_hash + 32 * i, 8);
  store_words(o.header_hash + 32 * q, w, 8);
  load_words(w, d.prev_hash + 32 * i, 8);
  store_words(o.prev_hash + 32 * q, w, 8);
  load_words(w, d.body_hash + 32 * i, 8);
  store_words(o.claimed + 32 * q, w, 8);
  const uint32_t ns = d.kind[i] ? 0u : d.nseg[i];           // a Byron row has no segments
  o.nseg[q] = (uint8_t)ns;
  for (uint32_t k = 0; k < 4; k++) {
    o.seg_off[(size_t)k * R + q] = k < ns ? d.seg_off[(size_t)k * n + i] : 0ull;
    o.seg_len[(size_t)k * R + q] = k < ns ? d.seg_len[(size_t)k * n + i] : 0u;
  }
}

// byr_result / byr_which: k_byron_integrity's over the rows, NULL with Byron off (no Byron rows)
__global__ void __launch_bounds__(NT) k_bf_bits(size_t R, const uint8_t* __restrict__ tag,
                                                const uint8_t* __restrict__ byr_result,
                                                const uint8_t* __restrict__ byr_which, uint8_t* __restrict__ bits,
                                                uint8_t* __restrict__ which, uint8_t* __restrict__ body_hash) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= R) return;
  uint8_t wh = 0;
  if (tag[q] <= 1) {
    bits[q] = byr_result ? (byr_result[q] & (PRAOS_BLK_DECODE | PRAOS_BLK_BODY_HASH)) : PRAOS_BLK_DECODE;
    wh = byr_which ? byr_which[q] : 0;
    const uint4 z = make_uint4(0, 0, 0, 0);
    ((uint4*)(body_hash + 32 * q))[0] = z;
    ((uint4*)(body_hash + 32 * q))[1] = z;
  }
  which[q] = wh;                                             // PRAOS_BYRON_W_ONE_TX still in it: k_bf_verdict reads it
}

__global__ void __launch_bounds__(NT) k_bf_verdict(size_t n, size_t R, int byron_on, const uint8_t* __restrict__ status,
                                                   const uint8_t* __restrict__ tag, const uint32_t* __restrict__ item_row,
                                                   const uint32_t* __restrict__ exp_idx,
                                                   const uint64_t* __restrict__ exp_slot,
                                                   const uint8_t* __restrict__ exp_hash,
                                                   const uint64_t* __restrict__ slot,
                                                   const uint8_t* __restrict__ header_hash,
                                                   const uint8_t* __restrict__ bits, const uint8_t* __restrict__ which,
                                                   uint8_t* __restrict__ verdict) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t row = item_row[i], e = exp_idx[i];
  const bool has_row = row != NONE && row < R;
  uint8_t v = PRAOS_BF_OK;
  if (status[i] != wire_scan::OK) {
    v = PRAOS_BF_WIRE;
  } else if (e == NONE) {
    v = PRAOS_BF_TOO_MANY;
  } else if (tag[i] <= 1 && !byron_on) {
    v = PRAOS_BF_UNSUPPORTED;
  } else if (has_row && tag[i] == 1 && bits[row] == PRAOS_BLK_BODY_HASH && which[row] == PRAOS_BYRON_W_ROOT) {
    v = PRAOS_BF_UNSUPPORTED;                                // the Merkle root of n /= 1 transactions: unpinned
  } else if (!has_row) {
    v = PRAOS_BF_DECODE;
  } else {
    uint32_t h[8], x[8];
    load_words(h, header_hash + 32 * i, 8);
    load_words(x, exp_hash + 32 * (size_t)e, 8);
    bool same = slot[i] == exp_slot[e];
#pragma unroll
    for (int k = 0; k < 8; k++) same &= h[k] == x[k];
    if (!same) v = PRAOS_BF_WRONG_BLOCK;
    else if (bits[row]) v = PRAOS_BF_INVALID_BODY;
  }
  verdict[i] = v;
}

// which[] as the caller sees it: without the host-internal one-transaction flag
__global__ void __launch_bounds__(NT) k_bf_which(size_t R, uint8_t* __restrict__ which) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < R) which[q] &= (uint8_t)~PRAOS_BYRON_W_ONE_TX;
}

}  // namespace

// ---- host launchers (kernels are only launchable from their own module)
void launch_span_equal(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* a_off,
                       const uint64_t* b_off, const uint32_t* len, uint8_t* out) {
  if (!n) return;
  hipLaunchKernelGGL(k_span_equal, dim3((unsigned)((n + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, stream, n, arena,
                     arena_len, a_off, b_off, len, out);
}

void launch_bf_unwrap(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                      const uint32_t* len, uint32_t n_eras, uint8_t* status, uint8_t* tag, uint64_t* ioff,
                      uint32_t* ilen, uint64_t* hoff, uint32_t* hlen) {
  hipLaunchKernelGGL(k_bf_unwrap, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, arena, arena_len, off, len,
                     n_eras, status, tag, ioff, ilen, hoff, hlen);
}

void launch_bf_key(hipStream_t stream, size_t n, const uint8_t* status, const uint8_t* split_status,
                   const uint16_t* dec_status, const uint8_t* tag, const uint32_t* ilen, const uint8_t* header_hash,
                   uint8_t* elig, uint8_t* key, uint32_t* any_byron) {
  hipLaunchKernelGGL(k_bf_key, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, status, split_status,
                     dec_status, tag, ilen, header_hash, elig, key, any_byron);
}

void launch_bf_class(hipStream_t stream, size_t n, const uint8_t* arena, const uint32_t* item_slot,
                     const uint32_t* item_rep, const uint64_t* ioff, const uint32_t* ilen, uint32_t* slot2,
                     uint32_t* min2) {
  hipLaunchKernelGGL(k_bf_class, dim3((unsigned)((n + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, stream, n, arena,
                     item_slot, item_rep, ioff, ilen, slot2, min2);
}

void launch_bf_rows(hipStream_t stream, size_t n, size_t R, const uint32_t* slot2, const uint32_t* rep_row,
                    const praos_bf_dev_items* items, const praos_bf_dev_rows* rows) {
  hipLaunchKernelGGL(k_bf_rows, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, R, slot2, rep_row, *items,
                     *rows);
}

void launch_bf_bits(hipStream_t stream, size_t R, const uint8_t* tag, const uint8_t* byr_result,
                    const uint8_t* byr_which, uint8_t* bits, uint8_t* which, uint8_t* body_hash) {
  hipLaunchKernelGGL(k_bf_bits, dim3((unsigned)((R + NT - 1) / NT)), dim3(NT), 0, stream, R, tag, byr_result, byr_which,
                     bits, which, body_hash);
}

void launch_bf_verdict(hipStream_t stream, size_t n, size_t R, int byron_on, const uint8_t* status, const uint8_t* tag,
                       const uint32_t* item_row, const uint32_t* exp_idx, const uint64_t* exp_slot,
                       const uint8_t* exp_hash, const uint64_t* slot, const uint8_t* header_hash, const uint8_t* bits,
                       uint8_t* which, uint8_t* verdict) {
  hipLaunchKernelGGL(k_bf_verdict, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, R, byron_on, status, tag,
                     item_row, exp_idx, exp_slot, exp_hash, slot, header_hash, bits, which, verdict);
  if (R) hipLaunchKernelGGL(k_bf_which, dim3((unsigned)((R + NT - 1) / NT)), dim3(NT), 0, stream, R, which);
}
