// k_miss4.hip -- the uncached OCert and KES verifies (k_ed25519.hip k_ocert / k_kes: a key
// used once in the batch, so no key tables) built with the ILP-4 group formulas
// (PRAOS_ILP4, as k_vrf_v4.hip) at 2 waves per SIMD, optionally at s_setprio 3.  In a small
// batch the misses are a few dozen waves whose full verify chain (decode, 252 doublings,
// encoding) ends the step; the wider interleave shortens each chain.  Identical operations
// and output.
#define PRAOS_ILP4 1
#include "k_ed25519.hpp"

__global__ void __launch_bounds__(NT, 2) k_ocert4(const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                                                  const ge_niels* __restrict__ gbtab, OcertIn a, int prio) {
  const size_t items = *count;
  if ((size_t)blockIdx.x * NT >= items) return;
  __shared__ ge_niels sbtab[BTAB_N];
  const ge_niels* btab = stage_btab<1>(gbtab, sbtab);
  const size_t t = (size_t)blockIdx.x * NT + threadIdx.x;
  if (t >= items) return;
  if (prio) __builtin_amdgcn_s_setprio(3);
  ocert_miss_item(a, list[t], btab);
}

__global__ void __launch_bounds__(NT, 2) k_kes4(const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                                                const ge_niels* __restrict__ gbtab, KesIn a, int prio) {
  const size_t items = *count;
  if ((size_t)blockIdx.x * NT >= items) return;
  __shared__ ge_niels sbtab[BTAB_N];
  const ge_niels* btab = stage_btab<1>(gbtab, sbtab);
  const size_t q = (size_t)blockIdx.x * NT + threadIdx.x;
  if (q >= items) return;
  if (prio) __builtin_amdgcn_s_setprio(3);
  kes_miss_item(a, list[q], btab);
}

// The cached verifies (k_ed25519.hip k_ocert_ck / k_kes_ck, one header per lane) from the same
// ILP-4 build: in a small batch they are the last link of the cached chains
__global__ void __launch_bounds__(NT, 2) k_ocert_ck4(const uint32_t* __restrict__ list,
                                                     const uint32_t* __restrict__ count,
                                                     const int32_t* __restrict__ item_entry,
                                                     const ge_cached* __restrict__ ktab,
                                                     const uint32_t* __restrict__ kinfo,
                                                     const ge_niels* __restrict__ gbtab, OcertIn a) {
  const size_t items = *count;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= items) return;
  ocert_hit_item(a, list[t], item_entry, ktab, kinfo, gbtab);
}

__global__ void __launch_bounds__(NT, 2) k_kes_ck4(const uint32_t* __restrict__ list,
                                                   const uint32_t* __restrict__ count,
                                                   const int32_t* __restrict__ item_entry,
                                                   const ge_cached* __restrict__ ktab,
                                                   const uint32_t* __restrict__ kinfo,
                                                   const ge_niels* __restrict__ gbtab, KesIn a) {
  const size_t items = *count;
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= items) return;
  kes_hit_item(a, list[q], item_entry, ktab, kinfo, gbtab, nullptr, nullptr);
}

// ---- host launchers, called by k_ed25519.hip's only (launch.hpp).  The miss forms take the priority
// from a.wave_prio; the hit forms have none, nor pairing or path dedup.
void launch_ocert4(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const OcertIn& a) {
  hipLaunchKernelGGL(k_ocert4, launch_grid(n), dim3(NT), 0, stream, items.list, items.count, gbtab, a, a.wave_prio);
}
void launch_kes4(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const KesIn& a) {
  hipLaunchKernelGGL(k_kes4, launch_grid(n), dim3(NT), 0, stream, items.list, items.count, gbtab, a, a.wave_prio);
}
void launch_ocert_ck4(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const OcertIn& a) {
  hipLaunchKernelGGL(k_ocert_ck4, launch_grid(n), dim3(NT), 0, stream, h.list, h.count, h.item_entry, h.ktab, h.kinfo,
                     comb, a);
}
void launch_kes_ck4(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const KesIn& a) {
  hipLaunchKernelGGL(k_kes_ck4, launch_grid(n), dim3(NT), 0, stream, h.list, h.count, h.item_entry, h.ktab, h.kinfo,
                     comb, a);
}
