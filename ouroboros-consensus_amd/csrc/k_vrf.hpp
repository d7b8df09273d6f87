#pragma once
// k_vrf.hpp -- pieces shared by the VRF kernel modules (k_vrf.hip: the one-kernel verify and
// TPraos; k_vrf_stage.hip: the staged header pipeline)
#include "kcommon.hpp"

// Header mode: issuer hash -> pool (binary search), VRF key hash, alpha =
// mkInputVRF(slot, eta0), proof verify, beta, output check, leader/nonce values.
// Plain mode (ok_out != null): alpha given per item; ok_out, beta only.
struct VrfIn {
  const uint8_t* __restrict__ cold_vk;
  const uint8_t* __restrict__ vrf_vk;
  const uint8_t* __restrict__ vrf_out;
  const uint8_t* __restrict__ vrf_proof;
  const uint64_t* __restrict__ slot;
  const uint32_t* __restrict__ eta0;     // eta_idx == null: the epoch nonce (8 words)
  int eta0_neutral;
  const uint8_t* __restrict__ eta_idx;   // several epochs per batch: header i uses entry eta_idx[i]
                                         // of eta0 = table of 9-word entries (nonce, neutral flag)
  const uint32_t* __restrict__ pool_hash;
  const uint32_t* __restrict__ pool_vrf;
  const int32_t* __restrict__ pool_map;
  uint32_t npools;
  int check_output;
  const uint8_t* __restrict__ alpha_in;
  uint16_t* __restrict__ bits;
  int32_t* __restrict__ pool_idx;
  int32_t* __restrict__ pool_sorted_idx;
  uint8_t* __restrict__ beta_out;
  uint8_t* __restrict__ leader_out;
  uint8_t* __restrict__ nonce_out;
  uint8_t* __restrict__ ok_out;
  ge_cached* __restrict__ tabs;          // per-lane tables (LT_VRF entries per item)
  int wave_prio;                         // stage V / join waves at s_setprio 3 (small batches)
  int tp_seed;                           // stage V alpha: 0 Praos mkInputVRF; 1 + k TPraos mkSeed
                                         // with ucNonce k (0 seedEta, 1 seedL)
  int pre;                               // join: the pool part ran ahead (k_vrf_pool wrote bits[i])
  const int32_t* __restrict__ rec_entry; // join / k_vrf_pool: header i's VRF key-cache entry or -1 ...
  const uint32_t* __restrict__ rec;      // ... and the per-entry pool records (k_vrf_keyrec), or null
};

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

static inline VrfIn vrf_in(const uint8_t* cold_vk, const uint8_t* vrf_vk, const uint8_t* vrf_out, const uint8_t* vrf_proof,
                    const uint64_t* slot, const uint32_t* eta0, int eta0_neutral, const uint8_t* eta_idx,
                    const uint32_t* pool_hash, const uint32_t* pool_vrf, const int32_t* pool_map, uint32_t npools,
                    int check_output, uint16_t* bits, int32_t* pool_idx, int32_t* pool_sorted_idx, uint8_t* beta_out,
                    uint8_t* leader_out, uint8_t* nonce_out, ge_cached* tabs) {
  return VrfIn{cold_vk, vrf_vk, vrf_out, vrf_proof, slot, eta0, eta0_neutral, eta_idx, pool_hash, pool_vrf, pool_map,
               npools, check_output, nullptr, bits, pool_idx, pool_sorted_idx, beta_out, leader_out, nonce_out, nullptr,
               tabs};
}
