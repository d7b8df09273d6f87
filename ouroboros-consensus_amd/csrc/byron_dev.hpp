// byron_dev.hpp -- device helpers shared by the Byron kernels (k_byron.hip blocks, k_pbft.hip
// headers): Blake2b-256 with a literal prefix, and the 128-byte register streaming buffer of the
// SHA-512 / Blake2b-256 streams.  The strict CBOR readers they parse with are cbor_dev.hpp's.
#pragma once
#include "kcommon.hpp"
#include "arena.hpp"
#include "cbor_dev.hpp"

namespace {

// Blake2b-256 of (npre <= 2 literal bytes, the low bytes of pre) || a[pos, pos + len): the range
// a[pos - npre, pos + len) with its first bytes replaced, so pos >= npre must hold (a Byron
// header starts at offset 3 of its block, a transaction after its pair's list head).
__device__ void b2b256_pre(uint32_t out[8], const uint8_t* __restrict__ a, uint64_t pos, uint64_t len, uint32_t npre,
                           uint64_t pre) {
  const uint64_t vp = pos - npre, tot = len + npre;
  uint64_t h[8];
  b2b_init(h);
  const uint64_t nblk = tot == 0 ? 1 : (tot + 127) / 128;
  for (uint64_t b = 0; b < nblk; b++) {
    uint64_t m[16];
    b2b_load_block(m, a, vp, tot, 128 * b);
    if (b == 0) m[0] = (m[0] & ~((1ull << (8 * npre)) - 1)) | pre;
    const bool last = b + 1 == nblk;
    b2b_compress(h, m, last ? tot : 128 * b + 128, last);
  }
  b2b_digest_words(out, h);
}

__device__ __forceinline__ void ld_bytes32(uint32_t w[8], const uint8_t* __restrict__ a, uint64_t pos) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint64_t v = ld64u(a, pos + 8 * k);
    w[2 * k] = (uint32_t)v;
    w[2 * k + 1] = (uint32_t)(v >> 32);
  }
}

// 128-byte streaming buffer in registers: the word a byte lands in is selected by compares, so
// m[] is never indexed by a runtime value
__device__ __forceinline__ void buf_put(uint64_t m[16], uint32_t fill, uint64_t w, uint32_t k) {
  const uint32_t idx = fill >> 3, sh = (fill & 7u) * 8u;
  if (k < 8) w &= (1ull << (8 * k)) - 1;
  const uint64_t lo = w << sh, hi = sh ? w >> (64u - sh) : 0;
#pragma unroll
  for (uint32_t j = 0; j < 16; j++) {
    if (j == idx) m[j] |= lo;
    if (j == idx + 1) m[j] |= hi;
  }
}

// SHA = true: SHA-512 (digest words as sha512_digest_words); false: Blake2b-256
template <bool SHA>
struct Hs {
  uint64_t h[8], m[16];
  uint64_t total;
  uint32_t fill;
  __device__ __forceinline__ void init() {
    if (SHA) sha512_init(h); else b2b_init(h);
#pragma unroll
    for (int j = 0; j < 16; j++) m[j] = 0;
    total = 0;
    fill = 0;
  }
  __device__ __forceinline__ void compress(bool last) {
    if (SHA) {
      uint64_t W[16];
#pragma unroll
      for (int j = 0; j < 16; j++) W[j] = bswap64(m[j]);
      sha512_block(h, W);
    } else {
      b2b_compress(h, m, total, last);
    }
#pragma unroll
    for (int j = 0; j < 16; j++) m[j] = 0;
    fill = 0;
  }
  // the k (1..8) low bytes of w; a full buffer is compressed only when more bytes come, so
  // Blake2b's last block is still here at the end
  __device__ __forceinline__ void put(uint64_t w, uint32_t k) {
    while (k) {
      if (fill == 128) compress(false);
      const uint32_t r = k < 128 - fill ? k : 128 - fill;
      buf_put(m, fill, w, r);
      fill += r;
      total += r;
      k -= r;
      if (k) w >>= 8 * r;
    }
  }
  // SHA-512 only: the padding (80, zeros, the bit length in the block's last word -- a second
  // block when fewer than 16 bytes are left after the 80) and the digest words
  __device__ __forceinline__ void sha512_finish(uint32_t out[16]) {
    put(0x80, 1);
    const uint64_t nbits = (total - 1) * 8;
    for (bool done = false; !done;) {
      if (fill <= 112) { m[15] = bswap64(nbits); done = true; }
      compress(false);
    }
    sha512_digest_words(out, h);
  }
};

// 09 || CBOR(pm) || 85 (the sign tag's magic and the ToSign list head) as the little-endian
// bytes of one word; len = its length
__device__ __forceinline__ uint64_t sign_tag_mid(uint32_t pm, uint32_t& len) {
  uint64_t enc;
  uint32_t el;
  if (pm < 24) { enc = pm; el = 1; }
  else if (pm < 0x100u) { enc = 0x18u | ((uint64_t)pm << 8); el = 2; }
  else if (pm < 0x10000u) { enc = 0x19u | ((uint64_t)(pm >> 8) << 8) | ((uint64_t)(pm & 0xffu) << 16); el = 3; }
  else { enc = 0x1au | ((uint64_t)__builtin_bswap32(pm) << 8); el = 5; }
  len = 2 + el;
  return 0x09u | (enc << 8) | (0x85ull << (8 * (1 + el)));
}

}  // namespace
