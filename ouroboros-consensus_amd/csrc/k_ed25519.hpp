// k_ed25519.hpp -- the OCert and Sum6KES per-header inputs and checks around the Ed25519
// verify, shared by k_ed25519.hip and its ILP-4 build for small batches (k_miss4.hip).
#pragma once
#include "kcommon.hpp"

// ------------------------------------------------------------------ OCert (OcertIn: kargs.hpp)
__device__ __forceinline__ void ocert_store(const OcertIn& a, size_t i, bool ok) {
  if (a.ok_out) {
    a.ok_out[i] = ok ? 1 : 0;
    return;
  }
  uint16_t b = ok ? 0 : PRAOS_BIT_OCERT_SIG;
  const uint64_t c0 = a.ocert_c0[i];
  const uint64_t kp = a.slot[i] / a.slots_per_kes_period;     // Praos.hs:596-599
  if (!(c0 <= kp)) b |= PRAOS_BIT_KES_BEFORE_START;            // Praos.hs:567
  if (!(kp < c0 + a.max_kes_evo)) b |= PRAOS_BIT_KES_AFTER_END; // Praos.hs:568
  a.bits[i] = b;
}

__device__ __forceinline__ void ocert_load(const OcertIn& a, size_t i, uint32_t sg[16], uint32_t hram[16],
                                           uint32_t pk[8]) {
  uint32_t hot[8];
  load_words(pk, a.cold_vk + 32 * i, 8);
  load_words(hot, a.hot_vk + 32 * i, 8);
  load_words(sg, a.sig + 64 * i, 16);
  ocert_hram(hram, sg, pk, hot, a.ocert_n[i], a.ocert_c0[i]);
}

// One uncached item (k_ocert; k_ocert4 from the ILP-4 build): the full verify on the lane's tables
__device__ __forceinline__ void ocert_miss_item(const OcertIn& a, size_t i, const ge_niels* btab) {
  uint32_t pk[8], sg[16], hram[16];
  ocert_load(a, i, sg, hram, pk);
  ocert_store(a, i, ed25519_verify_core(pk, sg, sg + 8, hram, btab, lane_tab(a.tabs, i, LT_ED)));
}

// One hit of the cold-key cache (k_ocert_ck; k_ocert_ck4): btab = the radix-2^16 comb, read in place
__device__ __forceinline__ void ocert_hit_item(const OcertIn& a, size_t i, const int32_t* item_entry,
                                               const ge_cached* ktab,
                                               const uint32_t* kinfo,
                                               const ge_niels* btab) {
  const size_t e = (size_t)item_entry[i];
  uint32_t pk[8], sg[16], hram[16];
  ocert_load(a, i, sg, hram, pk);
  ocert_store(a, i, ed25519_verify_cached(sg, sg + 8, hram, kinfo[9 * e], ktab + e * KT_STRIDE, btab));
}

// ------------------------------------------------------------------ KES (KesIn: kargs.hpp)
__device__ __forceinline__ uint64_t kes_t(const KesIn& a, size_t i) {
  if (a.period) return a.period[i];
  const uint64_t kp = a.slot[i] / a.slots_per_kes_period, c0 = a.ocert_c0[i];
  return kp >= c0 ? kp - c0 : 0;
}

// the tail of both prepares: the signature words, the body range check and SHA-512(R || leaf || M)
__device__ __forceinline__ void kes_hram(const KesIn& a, size_t i, const uint8_t* sig,
                                         const uint32_t leaf[8], uint32_t sg[16], uint32_t hram[16], bool& in_range) {
  load_words(sg, sig, 16);
  uint64_t off = a.body_off[i];
  uint32_t len = a.body_len[i];
  in_range = (off & 7) == 0 && off <= a.body_bytes_len && len <= a.body_bytes_len - off;
  if (!in_range) { off = 0; len = 0; }
  uint32_t pre[16];
#pragma unroll
  for (int k = 0; k < 8; k++) { pre[k] = sg[k]; pre[8 + k] = leaf[k]; }
  sha512_stream(hram, pre, 64, a.body + off, len);
}

// Merkle walk + SHA-512(R || leaf || M); returns merkle_ok, in_range, the leaf
// key and the signature words.
__device__ __forceinline__ void kes_prepare(const KesIn& a, size_t i, uint32_t sg[16], uint32_t leaf[8],
                                            uint32_t hram[16], bool& merkle_ok, bool& in_range) {
  const uint8_t* sig = a.kes_sig + 448 * i;
  uint32_t vk[8];
  load_words(vk, a.hot_vk + 32 * i, 8);
  merkle_ok = kes_merkle(leaf, vk, kes_t(a, i), sig);
  kes_hram(a, i, sig, leaf, sg, hram, in_range);
}

// Merkle walk shared per leaf-key cache entry (KES path dedup): the walk reads hot_vk, t and
// the six vk pairs sig[64 .. 448); an item whose bytes equal its entry representative's gets
// the representative's verdict (k_kes_merkle_reps) and selects its leaf as the walk would.
__device__ __forceinline__ bool kes_path_same(const KesIn& a, size_t i, size_t r, uint64_t ti) {
  if (i == r) return true;
  if (kes_t(a, r) != ti) return false;
  const uint4* p = (const uint4*)(a.kes_sig + 448 * i + 64);
  const uint4* q = (const uint4*)(a.kes_sig + 448 * r + 64);
  bool same = true;
#pragma unroll
  for (int k = 0; k < 24; k++) {
    const uint4 x = p[k], y = q[k];
    same &= x.x == y.x && x.y == y.y && x.z == y.z && x.w == y.w;
  }
  const uint4* hp = (const uint4*)(a.hot_vk + 32 * i);
  const uint4* hq = (const uint4*)(a.hot_vk + 32 * r);
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint4 x = hp[k], y = hq[k];
    same &= x.x == y.x && x.y == y.y && x.z == y.z && x.w == y.w;
  }
  return same;
}

// the depth-1 entry kes_merkle ends on (as k_kes_leafkeys)
__device__ __forceinline__ void kes_leaf_select(uint32_t leaf[8], uint64_t t, const uint8_t* __restrict__ sig) {
#pragma unroll
  for (int d = 6; d >= 2; d--) {
    const uint64_t T = 1ull << (d - 1);
    t = t >= T ? t - T : t;
  }
  load_words(leaf, sig + 64 + (t >= 1 ? 32 : 0), 8);
}

// kes_prepare with the path dedup: rep / rep_ok = the item's cache entry's representative and
// its walk verdict (rep_ok null in every lane: every item walks).  The branch is on the wave:
// the hit list is grouped by key, so nearly every wave holds equal paths only and skips the six
// Blake2b compressions altogether; one lane with a path of its own sends its whole wave through
// the walk (a per-lane branch would run both sides for every wave).
__device__ __forceinline__ void kes_prepare_dd(const KesIn& a, size_t i, size_t rep, const uint8_t* rep_ok,
                                               uint32_t sg[16], uint32_t leaf[8], uint32_t hram[16],
                                               bool& merkle_ok, bool& in_range) {
  const uint8_t* sig = a.kes_sig + 448 * i;
  const uint64_t t = kes_t(a, i);
  if (rep_ok && __ballot(!kes_path_same(a, i, rep, t)) == 0) {
    merkle_ok = *rep_ok != 0;
    kes_leaf_select(leaf, t, sig);
  } else {
    uint32_t vk[8];
    load_words(vk, a.hot_vk + 32 * i, 8);
    merkle_ok = kes_merkle(leaf, vk, t, sig);
  }
  kes_hram(a, i, sig, leaf, sg, hram, in_range);
}

__device__ __forceinline__ void kes_store(const KesIn& a, size_t i, bool merkle_ok, bool leaf_ok, bool in_range) {
  if (a.result) {
    a.result[i] = !in_range ? 3 : (!merkle_ok ? 1 : (leaf_ok ? 0 : 2));
    return;
  }
  uint16_t b = 0;
  if (!merkle_ok) b |= PRAOS_BIT_KES_MERKLE;
  else if (!leaf_ok) b |= PRAOS_BIT_KES_LEAF;
  if (!in_range) b |= PRAOS_BIT_INPUT;
  a.bits[i] = b;
}

// One uncached item (k_kes; k_kes4 from the ILP-4 build)
__device__ __forceinline__ void kes_miss_item(const KesIn& a, size_t i, const ge_niels* btab) {
  uint32_t sg[16], leaf[8], hram[16];
  bool merkle_ok, in_range;
  kes_prepare(a, i, sg, leaf, hram, merkle_ok, in_range);
  const bool leaf_ok = ed25519_verify_core(leaf, sg, sg + 8, hram, btab, lane_tab(a.tabs, i, LT_ED));
  kes_store(a, i, merkle_ok, leaf_ok, in_range);
}

// One hit of the leaf-key cache (k_kes_ck; k_kes_ck4, which has no path dedup: rep_ok null)
__device__ __forceinline__ void kes_hit_item(const KesIn& a, size_t i, const int32_t* item_entry,
                                             const ge_cached* ktab, const uint32_t* kinfo,
                                             const ge_niels* btab,
                                             const uint32_t* entry_rep,
                                             const uint8_t* rep_ok) {
  const size_t e = (size_t)item_entry[i];
  uint32_t sg[16], leaf[8], hram[16];
  bool merkle_ok, in_range;
  kes_prepare_dd(a, i, rep_ok ? entry_rep[e] : i, rep_ok ? rep_ok + e : nullptr, sg, leaf, hram, merkle_ok,
                 in_range);
  const bool leaf_ok = ed25519_verify_cached(sg, sg + 8, hram, kinfo[9 * e], ktab + e * KT_STRIDE, btab);
  kes_store(a, i, merkle_ok, leaf_ok, in_range);
}
