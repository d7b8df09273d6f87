// k_selftest_hash.hip -- self-test kernels of the hashes over stored bytes
// (praos_debug_hash_bytes): one lane per item runs the product routine on a caller's arena.
//   kind 0  b2b256_range (arena.hpp)
//   kind 1  b2b256_pre (byron_dev.hpp)
//   kind 2  is k_block.hip's own k_seg_hash through launch_seg_hash: no kernel here
//   kind 3  Hs<true>: the parts fed by the product's loop, then sha512_finish
//   kind 4  Hs<false>: the same, ended by compress(true)
// The host side has checked every range against the arena, so no lane reads past its 16-byte pad.
#include "byron_dev.hpp"

namespace {

__global__ void __launch_bounds__(NT) k_st_b2b_range(size_t n, const uint8_t* __restrict__ arena,
                                                     const uint64_t* __restrict__ off,
                                                     const uint32_t* __restrict__ len, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  b2b256_range(w, arena, off[i], len[i]);
  store_words(out + 32 * i, w, 8);
}

__global__ void __launch_bounds__(NT) k_st_b2b_pre(size_t n, const uint8_t* __restrict__ arena,
                                                   const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                   const uint8_t* __restrict__ aux, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t npre = aux[4 * i];
  const uint64_t pre = npre == 0 ? 0u : npre == 1 ? aux[4 * i + 1] : aux[4 * i + 1] | ((uint32_t)aux[4 * i + 2] << 8);
  uint32_t w[8];
  b2b256_pre(w, arena, off[i], len[i], npre, pre);
  store_words(out + 32 * i, w, 8);
}

template <bool SHA>
__global__ void __launch_bounds__(NT) k_st_stream(size_t n, const uint8_t* __restrict__ arena,
                                                  const uint64_t* __restrict__ first,
                                                  const uint32_t* __restrict__ count,
                                                  const uint64_t* __restrict__ parts, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Hs<SHA> s;
  s.init();
  const uint64_t p0 = first[i], p1 = p0 + count[i];
#pragma nounroll
  for (uint64_t p = p0; p < p1; p++) {
    const uint64_t a = parts[2 * p], b = parts[2 * p + 1];
    const bool is_lit = (b >> 63) != 0;
    uint64_t pos = is_lit ? 0 : a, len = b & ~(1ull << 63);
    const uint64_t lit = a;
    while (len) {   // the loop of k_pbft_decode and k_byron_integrity
      const uint32_t k = len < 8 ? (uint32_t)len : 8u;
      s.put(is_lit ? lit : ld64u(arena, pos), k);
      pos += k;
      len -= k;
    }
  }
  if (SHA) {
    uint32_t w[16];
    s.sha512_finish(w);
    store_words(out + 64 * i, w, 16);
  } else {
    s.compress(true);
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 4; k++) { w[2 * k] = (uint32_t)s.h[k]; w[2 * k + 1] = (uint32_t)(s.h[k] >> 32); }
    store_words(out + 32 * i, w, 8);
  }
}

}  // namespace

// ---- host launcher
void launch_selftest_hash(hipStream_t stream, int kind, size_t n, const uint8_t* arena, const uint64_t* off,
                          const uint32_t* len, const uint8_t* aux, const uint64_t* parts, uint8_t* out) {
  const dim3 g((unsigned)((n + NT - 1) / NT)), b(NT);
  switch (kind) {
    case 0: hipLaunchKernelGGL(k_st_b2b_range, g, b, 0, stream, n, arena, off, len, out); break;
    case 1: hipLaunchKernelGGL(k_st_b2b_pre, g, b, 0, stream, n, arena, off, len, aux, out); break;
    case 3: hipLaunchKernelGGL(k_st_stream<true>, g, b, 0, stream, n, arena, off, len, parts, out); break;
    case 4: hipLaunchKernelGGL(k_st_stream<false>, g, b, 0, stream, n, arena, off, len, parts, out); break;
    default: break;
  }
}
