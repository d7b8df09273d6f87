// crc32_gf2.hpp -- CRC-32 (zlib / System.FS.CRC.computeCRC: reflected polynomial
// 0xEDB88320, initial value and final xor 0xFFFFFFFF) as arithmetic in
// GF(2)[x] / P.  Plain integers only: k_crc32.hip includes it for the device
// and g++ compiles it for the host tests (tests/test_crc32_host.py).
//
// Representation (zlib's): a uint32 holds a polynomial of degree < 32 with the
// coefficient of x^0 in bit 31 and of x^31 in bit 0, so "times x" is a right
// shift.  With raw(s, D) the register after running the bytes D from state s
// without the two xors,
//   raw(s, D)   = s * x^(8|D|) + raw(0, D)                 (linear in s and D)
//   raw(0, A|B) = raw(0, A) * x^(8|B|) + raw(0, B)
//   raw(0, 0..0|B) = raw(0, B)                            (leading zeros vanish)
//   crc(D)      = raw(0, D) + F * x^(8|D|) + F,  F = 0xFFFFFFFF
//   crc(A|B)    = crc(A) * x^(8|B|) + crc(B)              (crc_combine)
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define CRC_HD __host__ __device__ __forceinline__
#else
#define CRC_HD inline
#endif

constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t CRC_ONE = 0x80000000u;   // x^0

// v * x mod P
CRC_HD constexpr uint32_t crc_mulx(uint32_t v) { return (v >> 1) ^ (CRC_POLY & (0u - (v & 1u))); }

// a * b mod P: 32 steps, no table
CRC_HD constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 31; i >= 0; i--) {
    r ^= b & (0u - ((a >> i) & 1u));
    b = crc_mulx(b);
  }
  return r;
}

// x^(8 * 2^k) mod P, k = 0..31, by repeated squaring
struct CrcX2N { uint32_t v[32]; };
constexpr CrcX2N crc_make_x2n() {
  CrcX2N t{};
  uint32_t p = CRC_ONE;
  for (int i = 0; i < 8; i++) p = crc_mulx(p);   // x^8
  for (int k = 0; k < 32; k++) { t.v[k] = p; p = crc_mulmod(p, p); }
  return t;
}

// x^(8 * nbytes) mod P: square-and-multiply over the x^(8 * 2^k) table
CRC_HD constexpr uint32_t crc_xpow8(uint64_t nbytes) {
  constexpr CrcX2N T = crc_make_x2n();
  uint32_t r = CRC_ONE;
  for (int k = 0; k < 32 && (nbytes >> k); k++)
    if ((nbytes >> k) & 1u) r = crc_mulmod(r, T.v[k]);
  return r;
}

// Multiplication by a constant c as 32 xor terms: row i = c * (the polynomial of bit i).
// The terms do not depend on each other, so a lane has 32-way ILP where the
// bit-serial form has a 32-step dependency chain.
struct CrcRows { uint32_t v[32]; };
constexpr CrcRows crc_make_rows(uint32_t c) {
  CrcRows t{};
  for (int i = 0; i < 32; i++) t.v[i] = crc_mulmod(c, 1u << i);
  return t;
}
CRC_HD constexpr uint32_t crc_apply(const CrcRows& t, uint32_t s) {
  uint32_t r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 32; i++) r ^= t.v[i] & (0u - ((s >> i) & 1u));
  return r;
}

// one little-endian 32-bit word into the raw register: (s + w) * x^32
CRC_HD uint32_t crc_word(uint32_t s, uint32_t w) {
  constexpr CrcRows X32 = crc_make_rows(crc_xpow8(4));
  return crc_apply(X32, s ^ w);
}

// bytewise restatement (bit-serial, no table): raw register over p[0, n)
CRC_HD uint32_t crc_raw_bytes(uint32_t s, const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) {
    s ^= p[i];
    for (int k = 0; k < 8; k++) s = crc_mulx(s);
  }
  return s;
}
CRC_HD uint32_t crc32_bytes(const uint8_t* p, size_t n) { return ~crc_raw_bytes(0xFFFFFFFFu, p, n); }

// crc(D) from raw(0, D)
CRC_HD uint32_t crc_finish(uint32_t raw0, uint64_t nbytes) {
  return raw0 ^ crc_mulmod(0xFFFFFFFFu, crc_xpow8(nbytes)) ^ 0xFFFFFFFFu;
}
// crc(A|B) from crc(A), crc(B), |B|
CRC_HD uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return crc_mulmod(crc_a, crc_xpow8(len_b)) ^ crc_b;
}
