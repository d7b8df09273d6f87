// sha3.hpp -- Keccak-f[1600] and SHA3-256 (FIPS 202) of messages of one rate block (<= 135
// bytes), host and device.
//
// Byron's hashVerKey (cardano-crypto-wrapper AddressHash) is Blake2b-224(SHA3-256(CBOR(xpub))),
// CBOR(xpub) = 58 40 || the 64 key bytes: 66 bytes, one block of the 136-byte rate.
// The 25 lanes are named members (s0 .. s24, lane x + 5y), every access is a compile-time
// name: the state lives in 50 VGPRs on the device.  Rho and pi are written out with their
// literal rotation amounts and lane numbers; only the loop over the 24 round constants is
// rolled (a runtime-indexed state array would go to scratch).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHA3_HD __host__ __device__ inline
#else
#define SHA3_HD inline
#endif

struct keccak_state {
  uint64_t s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15, s16, s17, s18, s19, s20, s21, s22,
      s23, s24;
};

#define SHA3_ROTL(x, n) (((x) << (n)) | ((x) >> (64 - (n))))
// one step of the rho-pi chain: lane j takes the carried lane rotated by n
#define SHA3_RP(j, n)               \
  do {                              \
    const uint64_t b_ = k.s##j;     \
    k.s##j = SHA3_ROTL(t, n);       \
    t = b_;                         \
  } while (0)
// chi on the row a, b, c, d, e
#define SHA3_CHI(a, b, c, d, e)                        \
  do {                                                 \
    const uint64_t a_ = k.s##a, b_ = k.s##b;           \
    k.s##a ^= ~b_ & k.s##c;                            \
    k.s##b ^= ~k.s##c & k.s##d;                        \
    k.s##c ^= ~k.s##d & k.s##e;                        \
    k.s##d ^= ~k.s##e & a_;                            \
    k.s##e ^= ~a_ & b_;                                \
  } while (0)

SHA3_HD void keccak_f1600(keccak_state& k) {
  constexpr uint64_t RC[24] = {
      0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
      0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
      0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
      0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
      0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
      0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang loop unroll(disable)
#endif
  for (int r = 0; r < 24; r++) {
    // theta
    const uint64_t c0 = k.s0 ^ k.s5 ^ k.s10 ^ k.s15 ^ k.s20;
    const uint64_t c1 = k.s1 ^ k.s6 ^ k.s11 ^ k.s16 ^ k.s21;
    const uint64_t c2 = k.s2 ^ k.s7 ^ k.s12 ^ k.s17 ^ k.s22;
    const uint64_t c3 = k.s3 ^ k.s8 ^ k.s13 ^ k.s18 ^ k.s23;
    const uint64_t c4 = k.s4 ^ k.s9 ^ k.s14 ^ k.s19 ^ k.s24;
    const uint64_t d0 = c4 ^ SHA3_ROTL(c1, 1), d1 = c0 ^ SHA3_ROTL(c2, 1), d2 = c1 ^ SHA3_ROTL(c3, 1),
                   d3 = c2 ^ SHA3_ROTL(c4, 1), d4 = c3 ^ SHA3_ROTL(c0, 1);
    k.s0 ^= d0; k.s5 ^= d0; k.s10 ^= d0; k.s15 ^= d0; k.s20 ^= d0;
    k.s1 ^= d1; k.s6 ^= d1; k.s11 ^= d1; k.s16 ^= d1; k.s21 ^= d1;
    k.s2 ^= d2; k.s7 ^= d2; k.s12 ^= d2; k.s17 ^= d2; k.s22 ^= d2;
    k.s3 ^= d3; k.s8 ^= d3; k.s13 ^= d3; k.s18 ^= d3; k.s23 ^= d3;
    k.s4 ^= d4; k.s9 ^= d4; k.s14 ^= d4; k.s19 ^= d4; k.s24 ^= d4;
    // rho and pi: one chain through the 24 lanes other than lane 0
    uint64_t t = k.s1;
    SHA3_RP(10, 1);  SHA3_RP(7, 3);   SHA3_RP(11, 6);  SHA3_RP(17, 10); SHA3_RP(18, 15); SHA3_RP(3, 21);
    SHA3_RP(5, 28);  SHA3_RP(16, 36); SHA3_RP(8, 45);  SHA3_RP(21, 55); SHA3_RP(24, 2);  SHA3_RP(4, 14);
    SHA3_RP(15, 27); SHA3_RP(23, 41); SHA3_RP(19, 56); SHA3_RP(13, 8);  SHA3_RP(12, 25); SHA3_RP(2, 43);
    SHA3_RP(20, 62); SHA3_RP(14, 18); SHA3_RP(22, 39); SHA3_RP(9, 61);  SHA3_RP(6, 20);  SHA3_RP(1, 44);
    // chi
    SHA3_CHI(0, 1, 2, 3, 4);
    SHA3_CHI(5, 6, 7, 8, 9);
    SHA3_CHI(10, 11, 12, 13, 14);
    SHA3_CHI(15, 16, 17, 18, 19);
    SHA3_CHI(20, 21, 22, 23, 24);
    // iota
    k.s0 ^= RC[r];
  }
}

// SHA3-256 of one padded rate block: m = the 17 little-endian lanes of msg || 06 || 00.. || 80
// (for a 135-byte message the last byte is 86)
SHA3_HD void sha3_256_block(uint64_t out[4], const uint64_t m[17]) {
  keccak_state k;
  k.s0 = m[0]; k.s1 = m[1]; k.s2 = m[2]; k.s3 = m[3]; k.s4 = m[4]; k.s5 = m[5]; k.s6 = m[6]; k.s7 = m[7];
  k.s8 = m[8]; k.s9 = m[9]; k.s10 = m[10]; k.s11 = m[11]; k.s12 = m[12]; k.s13 = m[13]; k.s14 = m[14];
  k.s15 = m[15]; k.s16 = m[16];
  k.s17 = k.s18 = k.s19 = k.s20 = k.s21 = k.s22 = k.s23 = k.s24 = 0;
  keccak_f1600(k);
  out[0] = k.s0; out[1] = k.s1; out[2] = k.s2; out[3] = k.s3;
}

// SHA3-256(58 40 || key), key = 8 little-endian words of the 64-byte extended public key
SHA3_HD void sha3_256_xpub(uint64_t out[4], const uint64_t key[8]) {
  uint64_t m[17];
  m[0] = 0x4058ULL | (key[0] << 16);
  m[1] = (key[0] >> 48) | (key[1] << 16);
  m[2] = (key[1] >> 48) | (key[2] << 16);
  m[3] = (key[2] >> 48) | (key[3] << 16);
  m[4] = (key[3] >> 48) | (key[4] << 16);
  m[5] = (key[4] >> 48) | (key[5] << 16);
  m[6] = (key[5] >> 48) | (key[6] << 16);
  m[7] = (key[6] >> 48) | (key[7] << 16);
  m[8] = (key[7] >> 48) | (0x06ULL << 16);          // byte 66: the domain bits and the first pad bit
  m[9] = m[10] = m[11] = m[12] = m[13] = m[14] = m[15] = 0;
  m[16] = 0x80ULL << 56;                             // byte 135: the last pad bit
  sha3_256_block(out, m);
}

// SHA3-256 of msg[0, len), len <= 135 (host side: tests and the generic form)
SHA3_HD bool sha3_256_small(uint8_t out[32], const uint8_t* msg, uint32_t len) {
  if (len > 135) return false;
  uint8_t blk[136];
  for (uint32_t i = 0; i < 136; i++) blk[i] = i < len ? msg[i] : 0;
  blk[len] ^= 0x06;
  blk[135] ^= 0x80;
  uint64_t m[17], h[4];
  for (int w = 0; w < 17; w++) {
    uint64_t v = 0;
    for (int b = 7; b >= 0; b--) v = (v << 8) | blk[8 * w + b];
    m[w] = v;
  }
  sha3_256_block(h, m);
  for (int w = 0; w < 4; w++)
    for (int b = 0; b < 8; b++) out[8 * w + b] = (uint8_t)(h[w] >> (8 * b));
  return true;
}
