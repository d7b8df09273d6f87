// k_vrf_stage.hip -- the header pipeline's VRF verify in stages (praos_core.hpp): V over every
// header, U per key-cache partition, the join (k_vrf_join); the two-stage form (k_vrf_fin*)
// kept for A/B (PRAOS_VRF3=0).
#include "k_vrf.hpp"

// waves per SIMD the launch bounds ask for: stage V (the largest kernel, 168 VGPRs at 3) and
// the U / join kernels (at 3 they spill SHA-512 and point state to scratch)
#ifndef LB_VRF_V
#define LB_VRF_V LB_VRF
#endif
#ifndef LB_VRF_F
#define LB_VRF_F LB_VRF
#endif
// the join / U + join kernels (one batched inversion, the SHA-512 challenge and beta, the
// Blake2b range extensions): at 3 waves per SIMD they spill ~370 bytes per lane
#ifndef LB_VRF_J
#define LB_VRF_J LB_VRF_F
#endif

// ---- two-stage form of the header mode (praos_core.hpp vrf_v_core / vrf_fin_core)
// stage V over every header of the batch: no dependence on the key cache
__global__ void __launch_bounds__(NT, LB_VRF_V) k_vrf_v(size_t n, size_t i0, size_t i1, VrfIn a, uint4* __restrict__ mid) {
  const size_t i = i0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // headers [i0, i1), record stride n
  if (i >= i1) return;
  if (a.wave_prio) __builtin_amdgcn_s_setprio(3);
  vrf_v_item(a, n, i, mid);
}

// stage F: pool lookup and key hash (Praos.hs:533-541), U + challenge + beta, the output
// check and the range extension -- the same results vrf_item writes in header mode
template <int CACHED>
__device__ __forceinline__ void vrf_fin_item(const VrfIn& a, size_t i, size_t stride, const uint4* __restrict__ mid,
                                             const ge_niels* __restrict__ btab, const ge_cached* __restrict__ ktab,
                                             const uint32_t* __restrict__ kinfo,
                                             const uint32_t* __restrict__ rec = nullptr) {
  uint32_t pk[8], pr[20];
  load_words(pk, a.vrf_vk + 32 * i, 8);
  load_words(pr, a.vrf_proof + 80 * i, 20);
  uint16_t b;
  int32_t sidx, pidx;
  {
    uint32_t cv[8];
    load_words(cv, a.cold_vk + 32 * i, 8);
    if (CACHED && a.rec) {                     // (rec: the entry's record; a.rec null: no records this run)
      b = vrf_pool_part_rec(a, rec, true, cv, pk, sidx, pidx);
    } else {
      b = vrf_pool_part(a, cv, pk, sidx);
      pidx = sidx < 0 ? -1 : a.pool_map[sidx];
    }
  }
  uint32_t beta[16];
  bool gamma_ok;
  const bool proof_ok = vrf_fin_core<CACHED>(beta, gamma_ok, mid, stride, i, pk, pr + 8, pr + 12, btab,
                                             lane_tab(a.tabs, i, LT_VRF), ktab, kinfo);
  if (!gamma_ok) {
#pragma unroll
    for (int k = 0; k < 16; k++) beta[k] = 0;
  }
  uint32_t out[16];
  load_words(out, a.vrf_out + 64 * i, 16);
  bool out_eq = true;
#pragma unroll
  for (int k = 0; k < 16; k++) out_eq &= out[k] == beta[k];
  if (!proof_ok) b |= PRAOS_BIT_VRF_PROOF;
  if (!out_eq && a.check_output) b |= PRAOS_BIT_VRF_OUTPUT;
  uint32_t lv[8], nv[8], nn[8];
  blake2b256_tag64(lv, 'L', out);
  blake2b256_tag64(nv, 'N', out);
  blake2b_32(nn, nv, 32);
  store_words(a.leader_out + 32 * i, lv, 8);
  store_words(a.nonce_out + 32 * i, nn, 8);
  store_words(a.beta_out + 64 * i, beta, 16);
  a.pool_idx[i] = pidx;
  a.pool_sorted_idx[i] = sidx;
  a.bits[i] = b;
}

// cached keys (the hit list): U from the key's tables and the radix-2^16 comb
__global__ void __launch_bounds__(NT, LB_VRF_J) k_vrf_fin(size_t stride, const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ count,
                                                        const int32_t* __restrict__ item_entry,
                                                        const ge_cached* __restrict__ ktab,
                                                        const uint32_t* __restrict__ kinfo,
                                                        const ge_niels* __restrict__ comb, VrfIn a,
                                                        const uint4* __restrict__ mid) {
  const size_t items = *count;
  const size_t t = (size_t)blockIdx.x * NT + threadIdx.x;
  if (t >= items) return;
  const size_t i = list[t];
  const size_t e = (size_t)item_entry[i];
  vrf_fin_item<true>(a, i, stride, mid, comb, ktab + e * KT_STRIDE, kinfo + 9 * e,
                     a.rec ? a.rec + VREC_WORDS * e : nullptr);
}

// keys of the wide tier (their own hit list): U from the key's positional tables, no doublings
__global__ void __launch_bounds__(NT, LB_VRF_J) k_vrf_fin_w(size_t stride, const uint32_t* __restrict__ list,
                                                          const uint32_t* __restrict__ count,
                                                          const int32_t* __restrict__ item_entry,
                                                          const int32_t* __restrict__ entry_wide,
                                                          const ge_cached* __restrict__ wtab,
                                                          const uint32_t* __restrict__ kinfo,
                                                          const ge_niels* __restrict__ comb, VrfIn a,
                                                          const uint4* __restrict__ mid) {
  const size_t items = *count;
  const size_t t = (size_t)blockIdx.x * NT + threadIdx.x;
  if (t >= items) return;
  const size_t i = list[t];
  const size_t e = (size_t)item_entry[i];
  vrf_fin_item<2>(a, i, stride, mid, comb, wtab + (size_t)entry_wide[e] * WT_STRIDE, kinfo + 9 * e,
                  a.rec ? a.rec + VREC_WORDS * e : nullptr);
}

// uncached keys (the miss list, or every header): U on a per-lane chain
__global__ void __launch_bounds__(NT, LB_VRF_J) k_vrf_fin_nc(size_t n, const uint32_t* __restrict__ list,
                                                           const uint32_t* __restrict__ count,
                                                           const ge_niels* __restrict__ gbtab, VrfIn a,
                                                           const uint4* __restrict__ mid) {
  const size_t items = list ? (size_t)*count : n;
  if ((size_t)blockIdx.x * NT >= items) return;
  __shared__ ge_niels sbtab[2 * BTAB_N];
  const ge_niels* btab = stage_btab<5>(gbtab, sbtab);
  const size_t t = (size_t)blockIdx.x * NT + threadIdx.x;
  if (t >= items) return;
  vrf_fin_item<false>(a, list ? list[t] : t, n, mid, btab, nullptr, nullptr);
}

// ---- three-kernel form (praos_core.hpp vrf_u_core / vrf_join_core): U apart from V
// U of a cached key (the hit list): the key's tables and the radix-2^16 comb
__global__ void __launch_bounds__(NT, LB_VRF_F) k_vrf_u(size_t stride, const uint32_t* __restrict__ list,
                                                      const uint32_t* __restrict__ count,
                                                      const int32_t* __restrict__ item_entry,
                                                      const ge_cached* __restrict__ ktab,
                                                      const uint32_t* __restrict__ kinfo,
                                                      const ge_niels* __restrict__ comb,
                                                      const uint8_t* __restrict__ vrf_proof, uint4* __restrict__ mid,
                                                      int prio) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)*count) return;
  wave_setprio(prio);
  vrf_u_item(mid, stride, list[t], item_entry, ktab, kinfo, comb, vrf_proof);
}

// U of a key of the wide tier (their own hit list): the key's positional tables
__global__ void __launch_bounds__(NT, LB_VRF_F) k_vrf_u_w(size_t stride, const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ count,
                                                        const int32_t* __restrict__ item_entry,
                                                        const int32_t* __restrict__ entry_wide,
                                                        const ge_cached* __restrict__ wtab,
                                                        const uint32_t* __restrict__ kinfo,
                                                        const ge_niels* __restrict__ comb,
                                                        const uint8_t* __restrict__ vrf_proof, uint4* __restrict__ mid,
                                                        int prio) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)*count) return;
  wave_setprio(prio);
  const size_t i = list[t];
  const size_t e = (size_t)item_entry[i];
  uint32_t pr[20];
  load_words(pr, vrf_proof + 80 * i, 20);
  vrf_u_core<2>(mid, stride, i, nullptr, pr + 8, pr + 12, comb, nullptr, wtab + (size_t)entry_wide[e] * WT_STRIDE,
                kinfo + 9 * e);
}

// U of an uncached key (the miss list, or every header): a per-lane chain; vt = an 8-entry
// lane table region of its own (stage V runs at the same time on the 16-entry one)
__global__ void __launch_bounds__(NT, LB_VRF_F) k_vrf_u_nc(size_t n, const uint32_t* __restrict__ list,
                                                         const uint32_t* __restrict__ count,
                                                         const ge_niels* __restrict__ gbtab,
                                                         const uint8_t* __restrict__ vrf_vk,
                                                         const uint8_t* __restrict__ vrf_proof,
                                                         ge_cached* __restrict__ tabs, uint4* __restrict__ mid) {
  const size_t items = list ? (size_t)*count : n;
  if ((size_t)blockIdx.x * NT >= items) return;
  __shared__ ge_niels sbtab[2 * BTAB_N];
  const ge_niels* btab = stage_btab<5>(gbtab, sbtab);
  const size_t t = (size_t)blockIdx.x * NT + threadIdx.x;
  if (t >= items) return;
  const size_t i = list ? list[t] : t;
  uint32_t pk[8], pr[20];
  load_words(pk, vrf_vk + 32 * i, 8);
  load_words(pr, vrf_proof + 80 * i, 20);
  vrf_u_core<false>(mid, n, i, pk, pr + 8, pr + 12, btab, lane_tab(tabs, i, LT_ED), nullptr, nullptr);
}

// the header-only part of the join: pool lookup and key hash (Praos.hs:533-541), the pool
// indices and the leader / nonce values of the stated output (Praos.hs:468-502); returns the
// key bits
__device__ __forceinline__ uint16_t vrf_pool_item(const VrfIn& a, size_t i) {
  uint16_t b;
  int32_t sidx, pidx;
  {
    uint32_t pk[8], cv[8];
    load_words(cv, a.cold_vk + 32 * i, 8);
    load_words(pk, a.vrf_vk + 32 * i, 8);
    if (a.rec) {                               // cached VRF keys: the pool part from the key's record
      const int32_t e = a.rec_entry[i];
      b = vrf_pool_part_rec(a, a.rec + VREC_WORDS * (size_t)(e < 0 ? 0 : e), e >= 0, cv, pk, sidx, pidx);
    } else {
      b = vrf_pool_part(a, cv, pk, sidx);
      pidx = sidx < 0 ? -1 : a.pool_map[sidx];
    }
  }
  uint32_t out[16], lv[8], nv[8], nn[8];
  load_words(out, a.vrf_out + 64 * i, 16);
  blake2b256_tag64(lv, 'L', out);
  blake2b256_tag64(nv, 'N', out);
  blake2b_32(nn, nv, 32);
  store_words(a.leader_out + 32 * i, lv, 8);
  store_words(a.nonce_out + 32 * i, nn, 8);
  a.pool_idx[i] = pidx;
  a.pool_sorted_idx[i] = sidx;
  return b;
}

// The pool record of each VRF key-cache entry (VREC_WORDS words, k_vrf.hpp): the pool part of
// the entry's representative header, one lane per entry.
__global__ void __launch_bounds__(NT) k_vrf_keyrec(const uint32_t* __restrict__ counters, uint32_t max_entries,
                                                   const uint32_t* __restrict__ entry_rep, VrfIn a,
                                                   uint32_t* __restrict__ rec) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= min(counters[0], max_entries)) return;
  const size_t i = entry_rep[e];
  uint32_t cv[8], pk[8];
  load_words(cv, a.cold_vk + 32 * i, 8);
  load_words(pk, a.vrf_vk + 32 * i, 8);
  int32_t sidx;
  const uint16_t b = vrf_pool_part(a, cv, pk, sidx);
  uint4* o = (uint4*)(rec + VREC_WORDS * (size_t)e);
  o[0] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
  o[1] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
  o[2] = make_uint4((uint32_t)sidx, b, (uint32_t)(sidx < 0 ? -1 : a.pool_map[sidx]), 0u);
}

// ... ahead of the join (small batches, on a stream with slack): the join's lanes then end
// after the inversion and the two SHA-512s (its dependent pool-search loads and five Blake2b
// compressions no longer follow stage V)
__global__ void __launch_bounds__(NT) k_vrf_pool(size_t n, VrfIn a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a.bits[i] = vrf_pool_item(a, i);
}

// join over every header: the pool part (vrf_pool_item, or its bits from k_vrf_pool when
// a.pre), the batched inversion, the challenge, beta and the output check
__global__ void __launch_bounds__(NT, LB_VRF_J) k_vrf_join(size_t n, VrfIn a, const uint4* __restrict__ mid) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (a.wave_prio) __builtin_amdgcn_s_setprio(3);
  uint16_t b = a.pre ? 0 : vrf_pool_item(a, i);
  uint32_t c4[4];
  {
    const uint4 q = *(const uint4*)(a.vrf_proof + 80 * i + 32);
    c4[0] = q.x; c4[1] = q.y; c4[2] = q.z; c4[3] = q.w;
  }
  uint32_t beta[16];
  bool gamma_ok;
  const bool proof_ok = vrf_join_core(beta, gamma_ok, mid, n, i, c4);
  if (!gamma_ok) {
#pragma unroll
    for (int k = 0; k < 16; k++) beta[k] = 0;
  }
  uint32_t out[16];
  load_words(out, a.vrf_out + 64 * i, 16);
  bool out_eq = true;
#pragma unroll
  for (int k = 0; k < 16; k++) out_eq &= out[k] == beta[k];
  if (!proof_ok) b |= PRAOS_BIT_VRF_PROOF;
  if (!out_eq && a.check_output) b |= PRAOS_BIT_VRF_OUTPUT;
  store_words(a.beta_out + 64 * i, beta, 16);
  a.bits[i] = a.pre ? (uint16_t)(a.bits[i] | b) : b;
}

// TPraos join of certificate `cert` (0: eta / nonce cert, 1: leader cert), the staged form of
// k_vrf_tp: cert 0 classifies the slot (overlay classes from praos_set_overlay: -2 not
// active, >= 0 a genesis delegate's slot checked against gen; else the pool lookup and VRF
// key hash, Praos.hs:533-541 as TPraos.hs:304-387 uses them) and writes beta_eta + the nonce
// (mkNonceFromOutputVRF of the stated output); cert 1 adds its bit to bits[i] and writes beta_l.
// Runs after cert 0's join on the same stream (bits read-modify-write).
__global__ void __launch_bounds__(NT, LB_VRF_J) k_vrf_join_tp(size_t n, int cert, VrfIn a,
                                                            const uint4* __restrict__ mid,
                                                            const int32_t* __restrict__ ovl_class,
                                                            const uint32_t* __restrict__ gen) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t cls = ovl_class ? ovl_class[i] : -1;
  uint16_t b = 0;
  if (cert == 0) {
    uint32_t pk[8], cv[8], hk[8];
    load_words(cv, a.cold_vk + 32 * i, 8);
    blake2b_32(hk, cv, 28);
    load_words(pk, a.vrf_vk + 32 * i, 8);
    int32_t sidx = -1;
    if (cls == -2) {
      b |= PRAOS_BIT_TP_NOT_ACTIVE;                  // NotActiveSlotOVERLAY
    } else if (cls >= 0) {                           // pbftVrfChecks vs the genesis delegate
      b |= PRAOS_BIT_TP_OVERLAY;
      const uint32_t* gd = gen + 16 * cls;
      bool cold_ok = true, vrf_ok = true;
#pragma unroll
      for (int k = 0; k < 7; k++) cold_ok &= hk[k] == gd[k];
      uint32_t vh[8];
      blake2b_32(vh, pk, 32);
#pragma unroll
      for (int k = 0; k < 8; k++) vrf_ok &= vh[k] == gd[8 + k];
      if (!cold_ok) b |= PRAOS_BIT_TP_GEN_COLD;
      if (!vrf_ok) b |= PRAOS_BIT_TP_GEN_VRF;
    } else {
      sidx = pool_search(hk, a.pool_hash, a.npools);
      if (sidx < 0) {
        b |= PRAOS_BIT_VRF_KEY_UNKNOWN;
      } else {
        uint32_t vh[8];
        blake2b_32(vh, pk, 32);
        bool same = true;
#pragma unroll
        for (int k = 0; k < 8; k++) same &= vh[k] == a.pool_vrf[8 * sidx + k];
        if (!same) b |= PRAOS_BIT_VRF_KEY_WRONG;
      }
    }
    a.pool_idx[i] = sidx < 0 ? -1 : a.pool_map[sidx];
    a.pool_sorted_idx[i] = sidx;
  } else {
    b = a.bits[i];
  }
  uint32_t c4[4];
  {
    const uint4 q = *(const uint4*)(a.vrf_proof + 80 * i + 32);
    c4[0] = q.x; c4[1] = q.y; c4[2] = q.z; c4[3] = q.w;
  }
  uint32_t beta[16], out[16];
  bool gamma_ok;
  const bool ok = vrf_join_core(beta, gamma_ok, mid, n, i, c4);
  if (!gamma_ok) {
#pragma unroll
    for (int k = 0; k < 16; k++) beta[k] = 0;
  }
  load_words(out, a.vrf_out + 64 * i, 16);
  bool eq = true;
#pragma unroll
  for (int k = 0; k < 16; k++) eq &= beta[k] == out[k];
  if ((!ok || (a.check_output && !eq)) && cls != -2) b |= cert ? PRAOS_BIT_TP_VRF_LEADER : PRAOS_BIT_TP_VRF_NONCE;
  store_words(a.beta_out + 64 * i, beta, 16);
  if (cert == 0) {
    uint32_t nn[8];
    blake2b256_of64(nn, out);                        // mkNonceFromOutputVRF
    store_words(a.nonce_out + 32 * i, nn, 8);
  }
  a.bits[i] = b;
}

// ---- host launchers (kernels are only launchable from their own module; the ILP-4 twins'
// launchers are k_vrf_v4.hip's).
void launch_vrf_v(hipStream_t stream, size_t n, const VrfIn& a, void* mid, size_t i0, size_t i1, int ilp4) {
  i1 = i1 < n ? i1 : n;
  if (i1 <= i0) return;
  if (ilp4) return launch_vrf_v4(stream, n, i0, i1, a, mid, ilp4 > 1);
  hipLaunchKernelGGL(k_vrf_v, launch_grid(i1 - i0), dim3(NT), 0, stream, n, i0, i1, a, (uint4*)mid);
}
void launch_vrf_fin(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const VrfIn& in,
                    const void* mid) {
  VrfIn a = in;
  a.rec = nullptr;                              // (the records are the cached keys')
  hipLaunchKernelGGL(k_vrf_fin_nc, launch_grid(n), dim3(NT), 0, stream, n, items.list, items.count, gbtab, a,
                     (const uint4*)mid);
}
void launch_vrf_fin(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const VrfIn& a,
                    const void* mid, const int32_t* entry_wide) {
  if (entry_wide)
    hipLaunchKernelGGL(k_vrf_fin_w, launch_grid(n), dim3(NT), 0, stream, n, h.list, h.count, h.item_entry, entry_wide,
                       h.ktab, h.kinfo, comb, a, (const uint4*)mid);
  else
    hipLaunchKernelGGL(k_vrf_fin, launch_grid(n), dim3(NT), 0, stream, n, h.list, h.count, h.item_entry, h.ktab,
                       h.kinfo, comb, a, (const uint4*)mid);
}
void launch_vrf_u(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const VrfIn& a,
                  ge_cached* utabs, void* mid) {
  hipLaunchKernelGGL(k_vrf_u_nc, launch_grid(n), dim3(NT), 0, stream, n, items.list, items.count, gbtab, a.vrf_vk,
                     a.vrf_proof, utabs, (uint4*)mid);
}
void launch_vrf_u(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const VrfIn& a, void* mid,
                  int ilp4, const int32_t* entry_wide) {
  if (entry_wide)
    hipLaunchKernelGGL(k_vrf_u_w, launch_grid(n), dim3(NT), 0, stream, n, h.list, h.count, h.item_entry, entry_wide,
                       h.ktab, h.kinfo, comb, a.vrf_proof, (uint4*)mid, a.wave_prio);
  else if (ilp4)
    launch_vrf_u4(stream, n, h, comb, a.vrf_proof, mid, a.wave_prio);
  else
    hipLaunchKernelGGL(k_vrf_u, launch_grid(n), dim3(NT), 0, stream, n, h.list, h.count, h.item_entry, h.ktab, h.kinfo,
                       comb, a.vrf_proof, (uint4*)mid, a.wave_prio);
}
void launch_vrf_join(hipStream_t stream, size_t n, const VrfIn& in, const void* mid) {
  VrfIn a = in;
  a.rec = a.rec_entry ? a.rec : nullptr;
  hipLaunchKernelGGL(k_vrf_join, launch_grid(n), dim3(NT), 0, stream, n, a, (const uint4*)mid);
}
void launch_vrf_pool(hipStream_t stream, size_t n, const VrfIn& in) {
  VrfIn a = in;
  a.rec = a.rec_entry ? a.rec : nullptr;
  hipLaunchKernelGGL(k_vrf_pool, launch_grid(n), dim3(NT), 0, stream, n, a);
}
void launch_vrf_keyrec(hipStream_t stream, const uint32_t* counters, uint32_t max_entries, const uint32_t* entry_rep,
                       const VrfIn& a, uint32_t* rec) {
  hipLaunchKernelGGL(k_vrf_keyrec, launch_grid(max_entries), dim3(NT), 0, stream, counters, max_entries, entry_rep, a,
                     rec);
}
void launch_vrf_join_tp(hipStream_t stream, size_t n, int cert, const VrfIn& a, const void* mid,
                        const int32_t* ovl_class, const uint32_t* gen) {
  hipLaunchKernelGGL(k_vrf_join_tp, launch_grid(n), dim3(NT), 0, stream, n, cert, a, (const uint4*)mid, ovl_class, gen);
}
