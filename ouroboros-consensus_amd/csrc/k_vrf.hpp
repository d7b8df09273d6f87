#pragma once
// k_vrf.hpp -- pieces shared by the VRF kernel modules (k_vrf.hip: the one-kernel verify and
// TPraos; k_vrf_stage.hip: the staged header pipeline)
#include "kcommon.hpp"

// issuer pool: hashKey (Blake2b-224 of the cold vk, Praos.hs:552) -> sorted index or -1
__device__ __forceinline__ int32_t pool_search(const uint32_t hk[8], const uint32_t* __restrict__ pool_hash,
                                               uint32_t npools) {
  int lo = 0, hi = (int)npools - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const uint32_t* ph = pool_hash + 7 * mid;
    int c = 0;
    for (int k = 0; k < 7 && c == 0; k++) {
      const uint32_t x = __builtin_bswap32(ph[k]), q = __builtin_bswap32(hk[k]);   // byte order
      c = x < q ? -1 : (x > q ? 1 : 0);
    }
    if (c == 0) return mid;
    if (c < 0) lo = mid + 1; else hi = mid - 1;
  }
  return -1;
}

// the pool part of a header (Praos.hs:533-541): issuer hash -> pool, the VRF key's hash against
// the pool's registered one; returns the key bits
__device__ __forceinline__ uint16_t vrf_pool_part(const VrfIn& a, const uint32_t cv[8], const uint32_t pk[8],
                                                  int32_t& sidx) {
  uint32_t hk[8];
  blake2b_32(hk, cv, 28);
  sidx = pool_search(hk, a.pool_hash, a.npools);
  if (sidx < 0) return PRAOS_BIT_VRF_KEY_UNKNOWN;
  uint32_t vh[8];
  blake2b_32(vh, pk, 32);
  bool same = true;
#pragma unroll
  for (int k = 0; k < 8; k++) same &= vh[k] == a.pool_vrf[8 * sidx + k];
  return same ? 0 : PRAOS_BIT_VRF_KEY_WRONG;
}

// Per-key pool record of the VRF key cache (k_vrf_keyrec, one per entry): the pool part is a
// function of (cold_vk, vrf_vk), and a cached key's headers nearly always carry one cold key.
// Words 0..7 the representative's cold key, 8 its sorted pool index, 9 its key bits, 10 its
// pool index (pool_map), 11 unused (VREC_WORDS, launch.hpp).

// The pool part through the record: rec = the record of the lane's entry (has: the lane has
// one).  The branch is on the wave: only when every lane's cold key equals its record's are the
// hashes and the search skipped; one deviant lane sends the whole wave through vrf_pool_part.
__device__ __forceinline__ uint16_t vrf_pool_part_rec(const VrfIn& a, const uint32_t* __restrict__ rec, bool has,
                                                      const uint32_t cv[8], const uint32_t pk[8], int32_t& sidx,
                                                      int32_t& pidx) {
  uint32_t r[VREC_WORDS];
#pragma unroll
  for (int k = 0; k < VREC_WORDS / 4; k++) {
    const uint4 q = ((const uint4*)rec)[k];
    r[4 * k] = q.x; r[4 * k + 1] = q.y; r[4 * k + 2] = q.z; r[4 * k + 3] = q.w;
  }
  bool same = has;
#pragma unroll
  for (int k = 0; k < 8; k++) same &= r[k] == cv[k];
  if (__ballot(!same) == 0) {
    sidx = (int32_t)r[8];
    pidx = (int32_t)r[10];
    return (uint16_t)r[9];
  }
  const uint16_t b = vrf_pool_part(a, cv, pk, sidx);
  pidx = sidx < 0 ? -1 : a.pool_map[sidx];
  return b;
}

// alpha = mkInputVRF(slot, eta) of header i (Praos/VRF.hs:55-69), or for a TPraos
// certificate mkSeed(ucNonce, slot, eta) (TPraos.hs:378-387 -> BHeader.mkSeed)
__device__ __forceinline__ void header_alpha(uint32_t alpha[8], const VrfIn& a, size_t i) {
  uint32_t e0[8];
  const uint32_t* ep = a.eta_idx ? a.eta0 + 9 * (uint32_t)a.eta_idx[i] : a.eta0;
#pragma unroll
  for (int k = 0; k < 8; k++) e0[k] = ep[k];
  const bool neutral = a.eta_idx ? ep[8] != 0 : a.eta0_neutral != 0;
  if (a.tp_seed) tpraos_seed(alpha, a.slot[i], e0, neutral, (uint64_t)(a.tp_seed - 1));
  else mk_input_vrf(alpha, a.slot[i], e0, neutral);
}

// Stage V of header i (k_vrf_stage.hip k_vrf_v; k_vrf_v4 / k_vrf_v4x from the ILP-4 build): alpha, H,
// Gamma and V into the stage record (stride n)
__device__ __forceinline__ void vrf_v_item(const VrfIn& a, size_t n, size_t i, uint4* mid) {
  uint32_t pk[8], pr[20], alpha[8];
  load_words(pk, a.vrf_vk + 32 * i, 8);
  load_words(pr, a.vrf_proof + 80 * i, 20);
  header_alpha(alpha, a, i);
  vrf_v_core(mid, n, i, pk, pr, pr + 8, pr + 12, alpha, lane_tab(a.tabs, i, LT_VRF));
}

// Stage U of header i, a hit of the VRF key cache (k_vrf_u; k_vrf_u4): the key's tables and the comb
__device__ __forceinline__ void vrf_u_item(uint4* mid, size_t stride, size_t i,
                                           const int32_t* item_entry,
                                           const ge_cached* ktab, const uint32_t* kinfo,
                                           const ge_niels* comb, const uint8_t* vrf_proof) {
  const size_t e = (size_t)item_entry[i];
  uint32_t pr[20];
  load_words(pr, vrf_proof + 80 * i, 20);
  vrf_u_core<true>(mid, stride, i, nullptr, pr + 8, pr + 12, comb, nullptr, ktab + e * KT_STRIDE, kinfo + 9 * e);
}
