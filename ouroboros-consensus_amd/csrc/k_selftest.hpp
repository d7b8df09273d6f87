// k_selftest.hpp -- self-test kernels of the field, group and scalar-multiplication layers
// (praos_debug_fe_multi, praos_debug_fe ops 9.., praos_debug_ge, praos_debug_msm) and of the
// integer routines under them (praos_debug_int, default build only), shared by
// the default build (k_selftest.hip) and the ILP-4 build (k_selftest4.hip, PRAOS_ILP4 = 1).
// They call the routines of fe25519.hpp / ge25519.hpp / scalarmult.hpp with the templates and
// arguments of the product code and return raw limbs or encodings; no product kernel is touched.
#pragma once
#include "kcommon.hpp"

#if PRAOS_ILP4
#define ST_LAUNCH(name) launch_selftest4_##name
#else
#define ST_LAUNCH(name) launch_selftest_##name
#endif

// The kernels are templates on the build so the two modules' host stubs have distinct names.
template <int BUILD>
__global__ void __launch_bounds__(64) k_selftest_fe_multi(int op, size_t n, const uint8_t* __restrict__ in,
                                                          uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe a[4], b[4], r[4];
#pragma unroll
  for (int m = 0; m < 4; m++) {
    load_words(a[m].v, in + 256 * i + 64 * m, 8);
    load_words(b[m].v, in + 256 * i + 64 * m + 32, 8);
    fe_set(r[m], 0);
  }
  // aliased forms (op | 8): output m is the object that product (m + 1) mod M reads as its
  // b (multiplies) or a (squarings); the result is then copied out of that object
  switch (op) {
    case 0: fe_mul2(r[0], a[0], b[0], r[1], a[1], b[1]); break;
    case 1: fe_sq2(r[0], a[0], r[1], a[1]); break;
    case 2: fe_mul3(r[0], a[0], b[0], r[1], a[1], b[1], r[2], a[2], b[2]); break;
    case 3: fe_mul4(r[0], a[0], b[0], r[1], a[1], b[1], r[2], a[2], b[2], r[3], a[3], b[3]); break;
    case 4: fe_sq4(r[0], a[0], r[1], a[1], r[2], a[2], r[3], a[3]); break;
    case 8:
      fe_mul2(b[1], a[0], b[0], b[0], a[1], b[1]);
      r[0] = b[1]; r[1] = b[0];
      break;
    case 9:
      fe_sq2(a[1], a[0], a[0], a[1]);
      r[0] = a[1]; r[1] = a[0];
      break;
    case 10:
      fe_mul3(b[1], a[0], b[0], b[2], a[1], b[1], b[0], a[2], b[2]);
      r[0] = b[1]; r[1] = b[2]; r[2] = b[0];
      break;
    case 11:
      fe_mul4(b[1], a[0], b[0], b[2], a[1], b[1], b[3], a[2], b[2], b[0], a[3], b[3]);
      r[0] = b[1]; r[1] = b[2]; r[2] = b[3]; r[3] = b[0];
      break;
    case 12:
      fe_sq4(a[1], a[0], a[2], a[1], a[3], a[2], a[0], a[3]);
      r[0] = a[1]; r[1] = a[2]; r[2] = a[3]; r[3] = a[0];
      break;
    default: break;
  }
#pragma unroll
  for (int m = 0; m < 4; m++) store_words(out + 128 * i + 32 * m, r[m].v, 8);
}

// praos_debug_fe ops 9 .. 14
template <int BUILD>
__global__ void __launch_bounds__(64) k_selftest_fe(int op, size_t n, const uint8_t* __restrict__ a,
                                                    const uint8_t* __restrict__ b, uint8_t* __restrict__ r) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe x, y, z;
  load_words(x.v, a + 32 * i, 8);
  load_words(y.v, b + 32 * i, 8);
  fe_set(z, 0);
  switch (op) {
    case 9: fe_neg(z, x); break;
    case 10: fe_chi(z, x); break;
    case 11: z.v[0] = (fe_iszero(x) ? 1u : 0u) | (fe_isnegative(x) ? 2u : 0u); break;
    case 12: fe_mul(x, x, y); z = x; break;
    case 13: fe_mul(y, x, y); z = y; break;
    case 14: fe_sq(x, x); z = x; break;
    default: break;
  }
  store_words(r + 32 * i, z.v, 8);
}

FE_INLINE void st_load4(fe& a, fe& b, fe& c, fe& d, const uint8_t* p) {
  load_words(a.v, p, 8);
  load_words(b.v, p + 32, 8);
  load_words(c.v, p + 64, 8);
  load_words(d.v, p + 96, 8);
}
FE_INLINE void st_store4(uint8_t* p, const fe& a, const fe& b, const fe& c, const fe& d) {
  store_words(p, a.v, 8);
  store_words(p + 32, b.v, 8);
  store_words(p + 64, c.v, 8);
  store_words(p + 96, d.v, 8);
}

// praos_debug_ge: one group formula per lane on raw coordinates (layouts in praos_hip.h)
template <int BUILD>
__global__ void __launch_bounds__(64) k_selftest_ge(int op, size_t n, const uint8_t* __restrict__ p,
                                                    const uint8_t* __restrict__ q, uint8_t* __restrict__ out,
                                                    const ge_niels* __restrict__ gbtab) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe p0, p1, p2, p3, q0, q1, q2, q3, zero;
  st_load4(p0, p1, p2, p3, p + 128 * i);
  st_load4(q0, q1, q2, q3, q + 128 * i);
  fe_set(zero, 0);
  uint8_t* o = out + 128 * i;
  switch (op) {
    case 0: {
      ge_p2 P = {p0, p1, p2};
      ge_p1p1 r;
      ge_p2_dbl(r, P);
      st_store4(o, r.X, r.Y, r.Z, r.T);
    } break;
    case 1: {
      ge_p3 P = {p0, p1, p2, p3};
      ge_cached Q = {q0, q1, q2, q3};
      ge_p1p1 r;
      ge_add(r, P, Q);
      st_store4(o, r.X, r.Y, r.Z, r.T);
    } break;
    case 2: {
      ge_p3 P = {p0, p1, p2, p3};
      ge_niels Q = {q0, q1, q2};
      ge_p1p1 r;
      ge_madd(r, P, Q);
      st_store4(o, r.X, r.Y, r.Z, r.T);
    } break;
    case 3: {
      ge_p1p1 P = {p0, p1, p2, p3};
      ge_p2 r;
      ge_p1p1_to_p2(r, P);
      st_store4(o, r.X, r.Y, r.Z, zero);
    } break;
    case 4: {
      ge_p1p1 P = {p0, p1, p2, p3};
      ge_p3 r;
      ge_p1p1_to_p3(r, P);
      st_store4(o, r.X, r.Y, r.Z, r.T);
    } break;
    case 5: {
      ge_p3 P = {p0, p1, p2, p3};
      ge_cached r;
      ge_p3_to_cached(r, P);
      st_store4(o, r.YpX, r.YmX, r.Z, r.T2d);
    } break;
    case 6: {
      ge_p3 P = {p0, p1, p2, p3};
      ge_p3 r;
      ge_p3_dbl_to_p3(r, P);
      st_store4(o, r.X, r.Y, r.Z, r.T);
    } break;
    case 7: {                                          // digit in [-8, 7] (the host checks it)
      ge_p3 P = {p0, p1, p2, p3};
      ge_cached tab[8], r;
      build_cached_table(tab, P);
      select_cached(r, tab, (int)q0.v[0]);
      st_store4(o, r.YpX, r.YmX, r.Z, r.T2d);
    } break;
    case 8: {                                          // digit in [-128, 127], table < BCOMB_T
      ge_niels r;
      select_niels(r, gbtab + (size_t)BTAB_N * q0.v[1], (int)q0.v[0]);
      st_store4(o, r.ypx, r.ymx, r.xy2d, zero);
    } break;
    default: break;
  }
}

// praos_debug_msm, one kernel per variant V (the chains and their arguments are the product's:
// praos_core.hpp ed25519_verify_core / ed25519_cached_point / vrf_u_core / vrf_v_core).
//   V 0: [sb]B - [sp]P   STRAUS<64, 64, 0, 32, false>, P decoded negated, lane table in global memory
//   V 1: [sb]B - [sp]P   STRAUS<33, 33, 0, 16, true>, sp < 2^128
//   V 2: [sp]P - [sq]Q   STRAUS<64, 64, 33, 0, false>, sq < 2^128
//   V 3: [sb]B - [sp]P   straus_comb<16, false> over key tables of kind 0 (ktab) and the comb
//   V 4: [sb]B - [sp]P   straus_comb<8, true> over key tables of kind 1, sp < 2^128
//   V 5: [sp]P           ge_scalarmult_var
//   V 6: [sb]B - [sp]P   straus_pos over the wide tables of kind 1, sp < 2^128
// tabs: 16 cached entries per lane (V 0 .. 2); ktab: KT_STRIDE entries per lane (V 3, 4),
// WT_STRIDE entries per lane (V 6).
template <int BUILD, int V>
__global__ void __launch_bounds__(NT) k_selftest_msm(size_t n, const uint8_t* __restrict__ Penc,
                                                     const uint8_t* __restrict__ Qenc, const uint8_t* __restrict__ sp,
                                                     const uint8_t* __restrict__ sq, const uint8_t* __restrict__ sb,
                                                     const ge_niels* __restrict__ gbtab,
                                                     const ge_niels* __restrict__ comb, ge_cached* __restrict__ tabs,
                                                     const ge_cached* __restrict__ ktab, uint8_t* __restrict__ out) {
  __shared__ ge_niels sbtab[(V == 0 || V == 1) ? 2 * BTAB_N : 1];
  const ge_niels* btab = nullptr;
  if constexpr (V == 0) btab = stage_btab<1>(gbtab, sbtab);
  if constexpr (V == 1) btab = stage_btab<5>(gbtab, sbtab);
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  uint32_t pk[8], s1[8], s2[8], w1[8], w2[8], enc[8];
  ge_p1p1 x;
  ge_p2 R;
  if constexpr (V == 0) {
    load_words(pk, Penc + 32 * i, 8);
    load_words(s1, sp + 32 * i, 8);
    load_words(s2, sb + 32 * i, 8);
    ge_p3 A;
    ge_frombytes(A, pk, /*negate=*/true);
    ge_cached* tab = lane_tab(tabs, i, 16);
    build_cached_table(tab, A);
    sc_recode16(w1, s1);
    sc_recode256(w2, s2);
    STRAUS<64, 64, 0, 32, false>(x, tab, w1, nullptr, nullptr, btab, w2);
    ge_p1p1_to_p2(R, x);
  } else if constexpr (V == 1) {
    load_words(pk, Penc + 32 * i, 8);
    load_words(s1, sp + 32 * i, 8);
    load_words(s2, sb + 32 * i, 8);
    ge_p3 Y;
    ge_frombytes(Y, pk, false);
    fe_neg(Y.X, Y.X);
    fe_neg(Y.T, Y.T);
    ge_cached* vt = lane_tab(tabs, i, 16);
    build_cached_table(vt, Y);
    sc_recode16(w1, s1);
    sc_recode256(w2, s2);
    STRAUS<33, 33, 0, 16, true>(x, vt, w1, nullptr, nullptr, btab, w2);
    ge_p1p1_to_p2(R, x);
  } else if constexpr (V == 2) {
    load_words(pk, Penc + 32 * i, 8);
    load_words(s1, sp + 32 * i, 8);
    load_words(s2, sq + 32 * i, 8);
    ge_p3 H, G;
    ge_frombytes(H, pk, false);
    load_words(pk, Qenc + 32 * i, 8);
    ge_frombytes(G, pk, false);
    fe_neg(G.X, G.X);
    fe_neg(G.T, G.T);
    ge_cached* vt = lane_tab(tabs, i, 16);
    build_cached_table(vt, H);
    build_cached_table(vt + 8, G);
    sc_recode16(w1, s1);
    sc_recode16(w2, s2);
    STRAUS<64, 64, 33, 0, false>(x, vt, w1, vt + 8, w2, nullptr, nullptr);
    ge_p1p1_to_p2(R, x);
  } else if constexpr (V == 3) {
    load_words(s1, sp + 32 * i, 8);
    load_words(s2, sb + 32 * i, 8);
    sc_recode16(w1, s1);
    sc_recode65536(w2, s2);
    straus_comb<16, false>(x, ktab + i * KT_STRIDE, w1, comb, w2);
    ge_p1p1_to_p2(R, x);
  } else if constexpr (V == 4) {
    load_words(s1, sp + 32 * i, 8);
    load_words(s2, sb + 32 * i, 8);
    sc_recode16(w1, s1);
    sc_recode65536(w2, s2);
    straus_comb<8, true>(x, ktab + i * KT_STRIDE, w1, comb, w2);
    ge_p1p1_to_p2(R, x);
  } else if constexpr (V == 6) {
    load_words(s1, sp + 32 * i, 8);
    load_words(s2, sb + 32 * i, 8);
    sc_recode65536(w2, s2);
    straus_pos(x, ktab + i * WT_STRIDE, s1, comb, w2);
    ge_p1p1_to_p2(R, x);
  } else {
    load_words(pk, Penc + 32 * i, 8);
    load_words(s1, sp + 32 * i, 8);
    ge_p3 P, S;
    ge_frombytes(P, pk, false);
    ge_scalarmult_var(S, s1, P);
    ge_p3_to_p2(R, S);
  }
  ge_tobytes(enc, R.X, R.Y, R.Z);
  store_words(out + 32 * i, enc, 8);
}

#if !PRAOS_ILP4
// praos_debug_int: one integer routine per lane (sc25519.hpp, the recoders of scalarmult.hpp, the
// Fixed E34 helpers of leader.hpp), 32 bytes per item and array; the host checks the preconditions
//   op 0 sc_reduce256   1 sc_muladd   2 sc_is_canonical   3, 4, 5 sc_recode16 / 256 / 65536
//   op 6 sc_recode64 (5 words)   7 fx_div_R   8 mp_div_small by word 0 of b
template <int BUILD>
__global__ void __launch_bounds__(64) k_selftest_int(int op, size_t n, const uint8_t* __restrict__ a,
                                                     const uint8_t* __restrict__ b, const uint8_t* __restrict__ c,
                                                     uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t x[8], y[8], z[8], r[8];
  load_words(x, a + 32 * i, 8);
#pragma unroll
  for (int k = 0; k < 8; k++) { y[k] = 0; z[k] = 0; r[k] = 0; }
  if (op == 1) {
    load_words(y, b + 32 * i, 8);
    load_words(z, c + 32 * i, 8);
  }
  if (op == 8) load_words(y, b + 32 * i, 8);
  switch (op) {
    case 0: sc_reduce256(r, x); break;
    case 1: sc_muladd(r, x, y, z); break;
    case 2: r[0] = sc_is_canonical(x) ? 1u : 0u; break;
    case 3: sc_recode16(r, x); break;
    case 4: sc_recode256(r, x); break;
    case 5: sc_recode65536(r, x); break;
    case 6: {
      uint32_t w[5];
      sc_recode64(w, x);
#pragma unroll
      for (int k = 0; k < 5; k++) r[k] = w[k];
    } break;
    case 7: fx_div_R(r, x); break;
    case 8: mp_div_small(r, x, y[0]); break;
    default: break;
  }
  store_words(out + 32 * i, r, 8);
}
#endif

// ---- host launchers
void ST_LAUNCH(ge)(hipStream_t stream, int op, size_t n, const uint8_t* p, const uint8_t* q, uint8_t* out,
                   const ge_niels* gbtab) {
  hipLaunchKernelGGL(k_selftest_ge<PRAOS_ILP4>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, op, n, p, q, out,
                     gbtab);
}
void ST_LAUNCH(msm)(hipStream_t stream, int variant, size_t n, const uint8_t* P, const uint8_t* Q, const uint8_t* sp,
                    const uint8_t* sq, const uint8_t* sb, const ge_niels* gbtab, const ge_niels* comb, ge_cached* tabs,
                    const ge_cached* ktab, uint8_t* out) {
  const dim3 grid((unsigned)((n + NT - 1) / NT)), block(NT);
#define ST_MSM(V)                                                                                                  \
  case V:                                                                                                          \
    hipLaunchKernelGGL((k_selftest_msm<PRAOS_ILP4, V>), grid, block, 0, stream, n, P, Q, sp, sq, sb, gbtab, comb, \
                       tabs, ktab, out);                                                                           \
    break
  switch (variant) {
    ST_MSM(0);
    ST_MSM(1);
    ST_MSM(2);
    ST_MSM(3);
    ST_MSM(4);
    ST_MSM(5);
    ST_MSM(6);
    default: break;
  }
#undef ST_MSM
}
#if !PRAOS_ILP4
void launch_selftest_fe_multi(hipStream_t stream, int op, size_t n, const uint8_t* in, uint8_t* out) {
  hipLaunchKernelGGL(k_selftest_fe_multi<0>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, op, n, in, out);
}
void launch_selftest_fe(hipStream_t stream, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* r) {
  hipLaunchKernelGGL(k_selftest_fe<0>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, op, n, a, b, r);
}
void launch_selftest_int(hipStream_t stream, int op, size_t n, const uint8_t* a, const uint8_t* b, const uint8_t* c,
                         uint8_t* out) {
  hipLaunchKernelGGL(k_selftest_int<0>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, op, n, a, b, c, out);
}
#endif
