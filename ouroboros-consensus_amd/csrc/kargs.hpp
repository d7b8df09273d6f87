// kargs.hpp -- the argument structs of the OCert, KES and VRF kernels and of the key-cache lists:
// what a host module fills in by field name and hands to a launcher (launch.hpp), and what the
// kernel receives as its kernarg unchanged.  Plain structs, no device code.  Field order and types
// are the kernarg layout.  Each launcher's comment in launch.hpp names the fields its kernel reads;
// the others may hold anything.
#pragma once
#include <cstddef>
#include <cstdint>
struct ge_niels;
struct ge_cached;

// Items of a list-mode launch: list[0 .. *count), or every i in [0, n) when list is null (the
// ILP-4 builds and the cached kernels take a list only).
struct KeyItems {
  const uint32_t *list, *count;
};

// Hits of a key cache (k_keys.hip): item i = list[t], t < *count, has entry e = item_entry[i].  A
// kernel reads the key's flag (and, VRF keys, its encoding) at kinfo + 9 * e and its tables at
// ktab + e * KT_STRIDE (the wide tier: at ktab + entry_wide[e] * WT_STRIDE, ktab = the wide tables).
struct KeyHits {
  const uint32_t *list, *count;
  const int32_t* item_entry;
  const ge_cached* ktab;
  const uint32_t* kinfo;
};

// ------------------------------------------------------------------ OCert + KES period checks
// bits |= KES_BEFORE_START / KES_AFTER_END / OCERT_SIG.  If ok_out != null the
// kernel is the plain praos_verify_ocert batch (ok_out[i] = 1 when valid).
// Items: i in [0, n), or list[0 .. *count) when list != null (key-cache
// partition, k_keys.hip): k_ocert takes the misses, k_ocert_ck the hits.
struct OcertIn {
  const uint8_t* __restrict__ cold_vk;
  const uint8_t* __restrict__ hot_vk;
  const uint64_t* __restrict__ ocert_n;
  const uint64_t* __restrict__ ocert_c0;
  const uint8_t* __restrict__ sig;
  const uint64_t* __restrict__ slot;
  uint64_t slots_per_kes_period, max_kes_evo;
  uint16_t* __restrict__ bits;
  uint8_t* __restrict__ ok_out;
  ge_cached* __restrict__ tabs;          // per-lane tables (LT_ED entries per item)
  int wave_prio;                         // cached verifies: waves at s_setprio <wave_prio> (0 = off)
};

// ------------------------------------------------------------------ KES
// Header mode: t = kp >= c0 ? kp - c0 : 0 (Praos.hs:570), result to bits.
// Plain mode (result != null): t = period[i], result 0 ok / 1 Reject / 2 leaf.
// Items: i in [0, n), or list[0 .. *count) (leaf-key cache partition): k_kes takes
// the misses, k_kes_ck the hits.
struct KesIn {
  const uint8_t* __restrict__ hot_vk;
  const uint8_t* __restrict__ kes_sig;
  const uint64_t* __restrict__ body_off;
  const uint32_t* __restrict__ body_len;
  const uint8_t* __restrict__ body;
  size_t body_bytes_len;
  const uint64_t* __restrict__ slot;
  const uint64_t* __restrict__ ocert_c0;
  uint64_t slots_per_kes_period;
  const uint32_t* __restrict__ period;
  uint16_t* __restrict__ bits;
  uint8_t* __restrict__ result;
  ge_cached* __restrict__ tabs;
  int wave_prio;                         // cached verifies: waves at s_setprio <wave_prio> (0 = off)
};

// ------------------------------------------------------------------ VRF
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
