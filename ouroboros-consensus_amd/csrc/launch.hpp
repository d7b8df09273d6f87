// launch.hpp -- host launchers exported by each kernel module (generated
// alongside the kernels; see the bottom of k_*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
// Block size of the kernels without LDS tables (V / U / join of the VRF, the cached-key
// Ed25519 chains).  1-wave blocks for small batches (so that 54k headers = 844 waves spread
// over all 256 CUs instead of 211 four-wave blocks) measured slower (k_vrf_v 2.70 -> 2.98 ms
// at 54k, profiles/r03/timeline_54k_wave_blocks.txt): 4-wave blocks everywhere.
static inline unsigned lat_block(size_t n) { (void)n; return 256u; }
struct ge_niels;
struct ge_cached;
void launch_ocert(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint32_t* list, const uint32_t* count,
                  const ge_niels* gbtab, const uint8_t* cold_vk, const uint8_t* hot_vk, const uint64_t* ocert_n,
                  const uint64_t* ocert_c0, const uint8_t* sig, const uint64_t* slot, uint64_t slots_per_kes_period,
                  uint64_t max_kes_evo, uint16_t* bits, uint8_t* ok_out, ge_cached* tabs);
void launch_ocert_ck(dim3 grid, dim3 block, hipStream_t stream, const uint32_t* list, const uint32_t* count,
                     const int32_t* item_entry, const ge_cached* ktab, const uint32_t* kinfo, const ge_niels* gbtab,
                     const uint8_t* cold_vk, const uint8_t* hot_vk, const uint64_t* ocert_n, const uint64_t* ocert_c0,
                     const uint8_t* sig, const uint64_t* slot, uint64_t slots_per_kes_period, uint64_t max_kes_evo,
                     uint16_t* bits, uint8_t* ok_out, int prio = 0);
void launch_vrf(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint32_t* list, const uint32_t* count,
                const ge_niels* gbtab, const uint8_t* cold_vk, const uint8_t* vrf_vk, const uint8_t* vrf_out,
                const uint8_t* vrf_proof, const uint64_t* slot, const uint32_t* eta0, int eta0_neutral,
                const uint8_t* eta_idx, const uint32_t* pool_hash, const uint32_t* pool_vrf, const int32_t* pool_map,
                uint32_t npools, int check_output, const uint8_t* alpha_in, uint16_t* bits, int32_t* pool_idx,
                int32_t* pool_sorted_idx, uint8_t* beta_out, uint8_t* leader_out, uint8_t* nonce_out, uint8_t* ok_out,
                ge_cached* tabs);
void launch_vrf_ck(dim3 grid, dim3 block, hipStream_t stream, const uint32_t* list, const uint32_t* count,
                   const int32_t* item_entry, const ge_cached* ktab, const uint32_t* kinfo, const ge_niels* gbtab,
                   const uint8_t* cold_vk, const uint8_t* vrf_vk, const uint8_t* vrf_out, const uint8_t* vrf_proof,
                   const uint64_t* slot, const uint32_t* eta0, int eta0_neutral, const uint8_t* eta_idx,
                   const uint32_t* pool_hash, const uint32_t* pool_vrf, const int32_t* pool_map, uint32_t npools,
                   int check_output, const uint8_t* alpha_in, uint16_t* bits, int32_t* pool_idx,
                   int32_t* pool_sorted_idx, uint8_t* beta_out, uint8_t* leader_out, uint8_t* nonce_out,
                   uint8_t* ok_out, ge_cached* tabs);
// pentry / pkey / pmask: the pool-key store probed first (null: none)
void launch_key_insert(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint32_t* list, const uint32_t* count,
                       const uint8_t* keys, uint32_t mask, uint32_t* slot_rep, uint32_t* slot_cnt, int32_t* item_slot,
                       const int32_t* pentry, const uint32_t* pkey, uint32_t pmask, uint32_t* scnt);
// stored entries' hit-list ranges (after the new keys'), from their uses this run
void launch_key_store_ranges(hipStream_t stream, uint32_t entries, const uint32_t* scnt, uint32_t* spos,
                             uint32_t* counters);
// The wide tier of a key cache (k_keys.hip; VRF keys): keys used >= min_uses times (0: tier off),
// at most cap of them; entry_wide / wide_ent: entry <-> wide index; wcnt: [0] wide keys claimed,
// [1] wide hits, [2] ranges handed out; hit: the wide keys' hit list; wtab: WT_STRIDE entries per key;
// wbase: WT_POS entries per key (the position bases, between the two passes of the precompute).
struct KeyWide {
  uint32_t min_uses = 0, cap = 0;
  int32_t* entry_wide = nullptr;
  uint32_t *wide_ent = nullptr, *wcnt = nullptr, *hit = nullptr;
  ge_cached *wtab = nullptr, *wbase = nullptr;
};
void launch_key_assign(dim3 grid, dim3 block, hipStream_t stream, uint32_t cap, const uint32_t* slot_rep,
                       const uint32_t* slot_cnt, uint32_t min_count, uint32_t max_entries, int32_t* slot_entry,
                       uint32_t* entry_rep, uint32_t* entry_pos, uint32_t* counters, const KeyWide& w = KeyWide());
void launch_key_partition(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint32_t* list,
                          const uint32_t* count, const int32_t* item_slot, const int32_t* slot_entry,
                          int32_t* item_entry, uint32_t* entry_pos, uint32_t* hit_list, uint32_t* miss_list,
                          uint32_t* counters, uint32_t* spos, const KeyWide& w = KeyWide());
void launch_ocert_dedup(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* cold, const uint8_t* hot,
                        const uint64_t* on, const uint64_t* oc, const uint8_t* sig, uint32_t mask, uint32_t* slot_rep,
                        uint32_t* item_rep, uint32_t* reps, uint32_t* counters);
void launch_ocert_fanout(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint32_t* item_rep,
                         const uint8_t* ok, const uint64_t* slot, const uint64_t* oc, uint64_t slots_per_kes_period,
                         uint64_t max_kes_evo, uint16_t* bits);
// entries [*base (0 when null), min(counters[0], max_entries)), at most span of them
void launch_key_precompute(int kind, hipStream_t stream, const uint32_t* counters, uint32_t max_entries,
                           const uint32_t* entry_rep, const uint8_t* keys, ge_cached* ktab, uint32_t* kinfo,
                           int wave_prio, const uint32_t* base, uint32_t span,
                           int mode,                       // 1: the chain from the ILP-4 build (k_keys4.hip)
                           const KeyWide& w = KeyWide());
void launch_key_precompute4(int kind, hipStream_t stream, const uint32_t* counters, uint32_t max_entries,
                            const uint32_t* entry_rep, const uint8_t* keys, ge_cached* ktab, uint32_t* kinfo,
                            int wave_prio, const uint32_t* base, uint32_t span);
void launch_pkey_reset(hipStream_t stream, uint32_t* count, int32_t* pentry, uint32_t slots, uint32_t limit, int force);
void launch_pkey_publish(hipStream_t stream, const uint32_t* counters, const uint32_t* base, uint32_t max_entries,
                         const uint32_t* entry_rep, const uint8_t* keys, int32_t* pentry, uint32_t* pkey,
                         uint32_t pmask, uint32_t* count, uint32_t span);
// the cached verifies of a small batch from the ILP-4 build (k_miss4.hip)
void launch_ocert_ck4(hipStream_t stream, size_t n, const uint32_t* list, const uint32_t* count,
                      const int32_t* item_entry, const ge_cached* ktab, const uint32_t* kinfo, const ge_niels* gbtab,
                      const uint8_t* cold_vk, const uint8_t* hot_vk, const uint64_t* ocert_n, const uint64_t* ocert_c0,
                      const uint8_t* sig, const uint64_t* slot, uint64_t slots_per_kes_period, uint64_t max_kes_evo,
                      uint16_t* bits, uint8_t* ok_out);
void launch_kes_ck4(hipStream_t stream, size_t n, const uint32_t* list, const uint32_t* count,
                    const int32_t* item_entry, const ge_cached* ktab, const uint32_t* kinfo, const ge_niels* gbtab,
                    const uint8_t* hot_vk, const uint8_t* kes_sig, const uint64_t* body_off, const uint32_t* body_len,
                    const uint8_t* body, size_t body_bytes_len, const uint64_t* slot, const uint64_t* ocert_c0,
                    uint64_t slots_per_kes_period, uint16_t* bits);
// the uncached verifies of a small batch from the ILP-4 build (k_miss4.hip), list mode only
void launch_ocert4(dim3 grid, dim3 block, hipStream_t stream, const uint32_t* list, const uint32_t* count,
                   const ge_niels* gbtab, const uint8_t* cold_vk, const uint8_t* hot_vk, const uint64_t* ocert_n,
                   const uint64_t* ocert_c0, const uint8_t* sig, const uint64_t* slot, uint64_t slots_per_kes_period,
                   uint64_t max_kes_evo, uint16_t* bits, uint8_t* ok_out, ge_cached* tabs, int prio);
void launch_kes4(dim3 grid, dim3 block, hipStream_t stream, const uint32_t* list, const uint32_t* count,
                 const ge_niels* gbtab, const uint8_t* hot_vk, const uint8_t* kes_sig, const uint64_t* body_off,
                 const uint32_t* body_len, const uint8_t* body, size_t body_bytes_len, const uint64_t* slot,
                 const uint64_t* ocert_c0, uint64_t slots_per_kes_period, uint16_t* bits, ge_cached* tabs, int prio);
void launch_kes(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint32_t* list, const uint32_t* count,
                const ge_niels* gbtab, const uint8_t* hot_vk, const uint8_t* kes_sig, const uint64_t* body_off,
                const uint32_t* body_len, const uint8_t* body, size_t body_bytes_len, const uint64_t* slot,
                const uint64_t* ocert_c0, uint64_t slots_per_kes_period, const uint32_t* period, uint16_t* bits,
                uint8_t* result, ge_cached* tabs);
void launch_kes_ck(dim3 grid, dim3 block, hipStream_t stream, const uint32_t* list, const uint32_t* count,
                   const int32_t* item_entry, const ge_cached* ktab, const uint32_t* kinfo, const ge_niels* gbtab,
                   const uint8_t* hot_vk, const uint8_t* kes_sig, const uint64_t* body_off, const uint32_t* body_len,
                   const uint8_t* body, size_t body_bytes_len, const uint64_t* slot, const uint64_t* ocert_c0,
                   uint64_t slots_per_kes_period, uint16_t* bits,
                   uint32_t pair_min,                       // two headers per lane from pair_min hits on (0: never)
                   const uint32_t* entry_rep,               // with rep_ok (k_kes_merkle_reps): the Merkle path
                   const uint8_t* rep_ok, int prio = 0);                  // dedup per cache entry (null: every item walks)
void launch_kes_merkle_reps(hipStream_t stream, const uint32_t* counters, uint32_t max_entries,
                            const uint32_t* entry_rep, const uint8_t* hot_vk, const uint8_t* kes_sig,
                            const uint64_t* slot, const uint64_t* ocert_c0, uint64_t slots_per_kes_period,
                            uint8_t* rep_ok);
void launch_kes_leafkeys(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* kes_sig,
                         const uint64_t* slot, const uint64_t* ocert_c0, uint64_t slots_per_kes_period,
                         uint8_t* keys);
void launch_init_btab(dim3 grid, dim3 block, hipStream_t stream, ge_niels* btab);
void launch_init_bcomb16(hipStream_t stream, const ge_niels* btab, ge_niels* bcomb16);
void launch_leader(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* leader_in, const int32_t* pool_sorted_idx, const uint32_t* pool_x, const uint32_t* x_item, int f_is_one, int leader_words, const uint16_t* b_ocert, const uint16_t* b_kes, const uint16_t* b_vrf, uint16_t* bits, uint8_t* is_leader, int32_t* iters, const uint16_t* dec_status);
void launch_debug_fe(dim3 grid, dim3 block, hipStream_t stream, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* r);
void launch_debug_sha512(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* prefix, const uint64_t* off, const uint32_t* len, const uint8_t* msg, uint8_t* out);
void launch_debug_blake2b(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* in, uint8_t* out);
void launch_debug_sc_reduce(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* in, uint8_t* out);
void launch_debug_decode(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* in, uint8_t* out, uint8_t* ok);
void launch_debug_smul_base(dim3 grid, dim3 block, hipStream_t stream, size_t n, const ge_niels* gbtab, const uint8_t* s, uint8_t* out);
void launch_debug_h2c(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* pk, const uint8_t* alpha, uint8_t* out);
void launch_synth_pools(dim3 grid, dim3 block, hipStream_t stream, uint32_t npools, const ge_niels* gbtab, const uint32_t* master, uint32_t* cold_seed, uint32_t* cold_pk, uint32_t* vrf_seed, uint32_t* vrf_pk, uint32_t* kes_seed, uint8_t* pool_hash28, uint8_t* pool_vrf32);
void launch_synth_kes_leaves(dim3 grid, dim3 block, hipStream_t stream, uint32_t npools, const ge_niels* gbtab, const uint32_t* kes_seed, uint32_t* leaf_seed, uint32_t* tree);
void launch_synth_kes_tree(dim3 grid, dim3 block, hipStream_t stream, uint32_t npools, uint32_t* tree);
void launch_synth_headers(dim3 grid, dim3 block, hipStream_t stream, size_t n, const ge_niels* gbtab, uint32_t npools, uint32_t nkes, uint64_t first_slot, uint64_t slot_stride, uint64_t slots_per_kes_period, uint32_t blen, uint64_t salt, const uint32_t* eta0, int eta0_neutral, const uint32_t* cold_seed, const uint32_t* cold_pk, const uint32_t* vrf_seed, const uint32_t* vrf_pk, const uint32_t* leaf_seed, const uint32_t* tree, uint8_t* msg_scratch, uint64_t* slot, uint8_t* cold_vk, uint8_t* vrf_vk, uint8_t* vrf_out, uint8_t* vrf_proof, uint8_t* hot_vk, uint64_t* ocert_n, uint64_t* ocert_c0, uint8_t* ocert_sig, uint8_t* kes_sig, uint64_t* body_off, uint32_t* body_len, uint8_t* body_bytes, int tpraos, uint8_t* l_out, uint8_t* l_proof, const uint8_t* body_hash_in, const uint64_t* sched_slot, const uint32_t* sched_pool, uint64_t block_no0, uint32_t* leaf_of);
void launch_synth_link(hipStream_t stream, size_t n, const ge_niels* gbtab, const uint8_t* prev0,
                       const uint32_t* leaf_seed, uint32_t nleaves, uint32_t* lkeys, const uint32_t* tree,
                       const uint32_t* leaf_of, uint8_t* body_bytes, const uint64_t* body_off, uint32_t* body_len,
                       uint8_t* kes_sig, uint8_t* header_hash, uint32_t stride);
void launch_synth_vrf_scalar(dim3 grid, dim3 block, hipStream_t stream, uint32_t npools, const uint32_t* vrf_seed,
                             uint32_t* vrf_x);
void launch_synth_leader_search(dim3 grid, dim3 block, hipStream_t stream, uint64_t first_slot, uint64_t nslots,
                                uint32_t p0, uint32_t pn, const uint32_t* vrf_x, const uint32_t* vrf_pk,
                                const uint32_t* pool_thr, const uint32_t* eta0, int eta0_neutral, int f_is_one,
                                int tpraos, int32_t* leader);
void launch_synth_corrupt(dim3 grid, dim3 block, hipStream_t stream, size_t n, uint32_t per10000, uint64_t salt, uint8_t* ocert_sig, uint8_t* kes_sig, uint8_t* vrf_proof, uint8_t* vrf_out, uint8_t* body_bytes, const uint64_t* body_off, const uint32_t* body_len, uint8_t* corrupted, uint8_t* l_proof, int cbor_body, uint32_t fields, uint8_t* cold_vk, uint8_t* hot_vk, uint64_t* ocert_n, uint64_t* ocert_c0);
// two-stage VRF of the header pipeline (k_vrf.hip): stage V over all n headers into the
// record `mid` (VRF_MID_PLANES x 16 x n bytes); stage F over list[0 .. *count) (or all n when
// list is null), cached (ktab != null: k_vrf_fin) or per-lane U (k_vrf_fin_nc)
void launch_vrf_v(hipStream_t stream, size_t n, const uint8_t* vrf_vk, const uint8_t* vrf_proof, const uint64_t* slot,
                  const uint32_t* eta0, int eta0_neutral, const uint8_t* eta_idx, ge_cached* tabs, void* mid,
                  size_t i0 = 0, size_t i1 = SIZE_MAX,    // headers [i0, min(i1, n)); mid stride n
                  int wave_prio = 0,                       // waves at s_setprio 3
                  int tp_seed = 0,                         // 1 + k: TPraos mkSeed alpha, ucNonce k
                  int ilp4 = 0);                           // 1: the ILP-4 build (k_vrf_v4.hip),
                                                           // 2: the same holding its SIMD alone

// stage V built with the ILP-4 group formulas at 2 waves per SIMD (k_vrf_v4.hip; small batches)
void launch_vrf_v4(hipStream_t stream, size_t n, size_t i0, size_t i1, const uint8_t* vrf_vk,
                   const uint8_t* vrf_proof, const uint64_t* slot, const uint32_t* eta0, int eta0_neutral,
                   const uint8_t* eta_idx, ge_cached* tabs, void* mid, int wave_prio, int tp_seed, int excl);
void launch_vrf_fin(hipStream_t stream, size_t n, const uint32_t* list, const uint32_t* count,
                    const int32_t* item_entry, const ge_cached* ktab, const uint32_t* kinfo, const ge_niels* comb,
                    const ge_niels* gbtab, const uint8_t* cold_vk, const uint8_t* vrf_vk, const uint8_t* vrf_out,
                    const uint8_t* vrf_proof, const uint32_t* pool_hash, const uint32_t* pool_vrf,
                    const int32_t* pool_map, uint32_t npools, int check_output, uint16_t* bits, int32_t* pool_idx,
                    int32_t* pool_sorted_idx, uint8_t* beta_out, uint8_t* leader_out, uint8_t* nonce_out,
                    ge_cached* tabs, const void* mid,
                    const int32_t* entry_wide = nullptr,    // list = a wide hit list, ktab = the wide tables
                    const uint32_t* rec = nullptr);         // cached keys: the entries' pool records (launch_vrf_keyrec)
// three-kernel VRF: stage U (cached: ktab != null, k_vrf_u over the hit list; uncached: k_vrf_u_nc
// over list[0 .. *count) or all n, 8-entry lane tables utabs) and the join over all n
void launch_vrf_u(hipStream_t stream, size_t n, const uint32_t* list, const uint32_t* count, const int32_t* item_entry,
                  const ge_cached* ktab, const uint32_t* kinfo, const ge_niels* comb, const ge_niels* gbtab,
                  const uint8_t* vrf_vk, const uint8_t* vrf_proof, ge_cached* utabs, void* mid,
                  int ilp4 = 0,                            // cached keys: the ILP-4 build (k_vrf_v4.hip k_vrf_u4)
                  int prio = 0,                            // cached keys: waves at s_setprio <prio>
                  const int32_t* entry_wide = nullptr);    // list = a wide hit list, ktab = the wide tables
void launch_vrf_u4(hipStream_t stream, size_t n, const uint32_t* list, const uint32_t* count, const int32_t* item_entry,
                   const ge_cached* ktab, const uint32_t* kinfo, const ge_niels* comb, const uint8_t* vrf_proof,
                   void* mid, int prio = 0);
void launch_vrf_join(hipStream_t stream, size_t n, const uint8_t* cold_vk, const uint8_t* vrf_vk,
                     const uint8_t* vrf_out, const uint8_t* vrf_proof, const uint32_t* pool_hash,
                     const uint32_t* pool_vrf, const int32_t* pool_map, uint32_t npools, int check_output,
                     uint16_t* bits, int32_t* pool_idx, int32_t* pool_sorted_idx, uint8_t* beta_out,
                     uint8_t* leader_out, uint8_t* nonce_out, const void* mid, int wave_prio = 0,
                     int pre = 0,                          // pre: launch_vrf_pool ran before (bits, pool, leader, nonce)
                     const int32_t* rec_entry = nullptr,   // the VRF key cache's item_entry and pool records
                     const uint32_t* rec = nullptr);       // (launch_vrf_keyrec), or null
// the join's pool part ahead of it (k_vrf_stage.hip k_vrf_pool): key bits, pool indices, leader / nonce
void launch_vrf_pool(hipStream_t stream, size_t n, const uint8_t* cold_vk, const uint8_t* vrf_vk,
                     const uint8_t* vrf_out, const uint32_t* pool_hash, const uint32_t* pool_vrf,
                     const int32_t* pool_map, uint32_t npools, uint16_t* bits, int32_t* pool_idx,
                     int32_t* pool_sorted_idx, uint8_t* leader_out, uint8_t* nonce_out,
                     const int32_t* rec_entry = nullptr, const uint32_t* rec = nullptr);   // as launch_vrf_join
// the pool record of each VRF key-cache entry (k_vrf_stage.hip k_vrf_keyrec; VREC_WORDS words per
// entry): the pool part of the entry's representative, which the entry's headers with the same
// cold key take instead of hashing and searching themselves
#define VREC_WORDS 12
void launch_vrf_keyrec(hipStream_t stream, const uint32_t* counters, uint32_t max_entries, const uint32_t* entry_rep,
                       const uint8_t* cold_vk, const uint8_t* vrf_vk, const uint32_t* pool_hash,
                       const uint32_t* pool_vrf, const int32_t* pool_map, uint32_t npools, uint32_t* rec);
// TPraos join of certificate cert (0: eta, 1: leader; k_vrf_stage.hip k_vrf_join_tp), after
// stage V (tp_seed 1 + cert) and U of that certificate into `mid`
void launch_vrf_join_tp(hipStream_t stream, size_t n, int cert, const uint8_t* cold_vk, const uint8_t* vrf_vk,
                        const uint8_t* cert_out, const uint8_t* cert_proof, const uint32_t* pool_hash,
                        const uint32_t* pool_vrf, const int32_t* pool_map, uint32_t npools, int check_output,
                        uint16_t* bits, int32_t* pool_idx, int32_t* pool_sorted_idx, uint8_t* beta_out,
                        uint8_t* nonce_out, const void* mid, const int32_t* ovl_class, const uint32_t* gen);
void launch_vrf_tp(dim3 grid, dim3 block, hipStream_t stream, size_t n, const ge_niels* gbtab, const uint8_t* cold_vk, const uint8_t* vrf_vk, const uint8_t* eta_out, const uint8_t* eta_proof, const uint8_t* l_out, const uint8_t* l_proof, const uint64_t* slot, const uint32_t* eta0, int eta0_neutral, const uint32_t* pool_hash, const uint32_t* pool_vrf, const int32_t* pool_map, uint32_t npools, int check_output, uint16_t* bits, int32_t* pool_idx, int32_t* pool_sorted_idx, uint8_t* beta_eta, uint8_t* beta_l, uint8_t* nonce_out, ge_cached* tabs,
                   const int32_t* ovl_class, const uint32_t* gen, const uint8_t* eta_idx = nullptr);
void launch_decode_praos(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len,
                         const uint64_t* hoff, const uint32_t* hlen, uint64_t* slot, uint8_t* cold_vk, uint8_t* vrf_vk,
                         uint8_t* vrf_out, uint8_t* vrf_proof, uint8_t* hot_vk, uint8_t* ocert_sig, uint8_t* kes_sig,
                         uint64_t* ocert_n, uint64_t* ocert_c0, uint64_t* body_off, uint32_t* body_len,
                         uint8_t* signed_body, uint64_t* block_no, uint8_t* prev_hash, uint8_t* prev_genesis,
                         uint32_t* body_size, uint8_t* body_hash, uint64_t* prot_major, uint64_t* prot_minor,
                         uint8_t* header_hash, uint16_t* status, int allow_tp, uint32_t stride, uint8_t* lead_out = nullptr, uint8_t* lead_proof = nullptr,
                         size_t i0 = 0);   // headers [i0, n); grid covers n - i0
void launch_block_split(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* arena,
                        uint64_t arena_len, uint64_t* off_io, uint32_t* len_io, uint64_t* seg_off, uint32_t* seg_len,
                        uint8_t* nseg, uint8_t* status);
// k_crc32.hip: CRC-32 of n spans; tile_first = exclusive prefix sum of ceil(len / PRAOS_CRC_TILE), n + 1 entries
void launch_crc32(hipStream_t stream, uint32_t n, uint32_t ntiles, const uint8_t* arena, const uint64_t* off,
                  const uint32_t* len, const uint32_t* tile_first, uint32_t* tile_raw, uint32_t* crc);
void launch_seg_hash(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* arena,
                     const uint64_t* seg_off, const uint32_t* seg_len, const uint8_t* nseg, uint8_t* seg_hash);
void launch_block_join(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* nseg,
                       const uint8_t* split_status, const uint16_t* dec_status, const uint16_t* kes_bits,
                       const uint8_t* seg_hash, const uint8_t* body_hash, uint8_t* result, uint8_t* calc_hash);
// k_byron.hip: Byron envelope + header columns (kind: 0 not Byron, 1 EBB, 2 main block, 3 does not decode;
// epoch_out: the header's epoch; spans: PRAOS_BYRON_SPANS u32 columns per block, may be null) and
// verifyBlockIntegrity of Byron blocks (which: PRAOS_BYRON_W_* | PRAOS_BYRON_W_ONE_TX)
#define PRAOS_BYRON_SPANS 28
#define PRAOS_BYRON_W_ONE_TX 0x80u   // which[], host-internal: the block holds exactly one transaction
void launch_byron_split(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len,
                        const uint64_t* blk_off, const uint32_t* blk_len, uint64_t epoch_slots, uint64_t* hoff,
                        uint32_t* hlen, uint64_t* slot, uint64_t* block_no, uint8_t* prev_hash, uint8_t* prev_genesis,
                        uint8_t* header_hash, uint8_t* split_status, uint16_t* dec_status, uint8_t* kind,
                        uint64_t* epoch_out, uint32_t* spans);
void launch_byron_integrity(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* arena,
                            const uint64_t* blk_off, const uint32_t* blk_len, const uint8_t* kind,
                            const uint32_t* spans, uint32_t cfg_pm, const ge_niels* gbtab, ge_cached* tabs,
                            uint8_t* result, uint8_t* which);
// k_txindex.hip: the transaction index of stored blocks.  Row arrays on the device (the
// provisional rows, and the selection of final ones a caller asked for: NULL = not written)
#define PRAOS_BYRON_SPAN_TXP 20   // k_byron.hip's BS_TXP_O; BS_TXP_L follows it
struct praos_txi_dev_rows {
  uint32_t* block;
  uint64_t* body_off;
  uint32_t* body_len;
  uint64_t* wit_off;
  uint32_t* wit_len;
  uint64_t* aux_off;
  uint32_t* aux_len;
  uint32_t* size;
  uint32_t* n_out;
  uint64_t* ex_steps;
  uint8_t* is_valid;
  uint8_t* tx_id;
};
// count: per block the transaction count, PRAOS_TXI_* status and kind, from k_block_split's
// segment spans and (byron != 0) k_byron_split's kind and txPayload span columns.  emit: the row
// spans at first[i] + t, one lane per (segment, block); the row arrays zeroed, is_valid set to ones.  rows: n_out, ex_steps, size per row; bad[i] |= 1
// for a row outside the shapes.  reduce: status and sums per block.  final: the rows of the OK
// blocks at tfirst[i] + t, with tx_id.
void launch_txi_count(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* blk_off,
                      const uint32_t* blk_len, int byron, const uint64_t* seg_off, const uint32_t* seg_len,
                      const uint8_t* nseg, const uint8_t* split_status, const uint8_t* byr_kind, const uint32_t* txp_o,
                      const uint32_t* txp_l, uint32_t* cnt, uint8_t* status, uint8_t* kind);
void launch_txi_emit(hipStream_t stream, size_t n, const uint8_t* arena, const uint64_t* blk_off,
                     const uint64_t* seg_off, const uint32_t* seg_len, const uint32_t* txp_o, const uint32_t* txp_l,
                     const uint8_t* kind, const uint8_t* status, const uint32_t* cnt, const uint32_t* first,
                     const praos_txi_dev_rows* rows);
void launch_txi_rows(hipStream_t stream, size_t nrows, const uint8_t* arena, const uint8_t* kind,
                     const praos_txi_dev_rows* rows, uint32_t* bad);
void launch_txi_reduce(hipStream_t stream, size_t n, const uint32_t* cnt, const uint32_t* first, const uint32_t* bad,
                       const praos_txi_dev_rows* rows, uint8_t* status, uint32_t* n_tx, uint64_t* txs_size,
                       uint64_t* n_out, uint64_t* ex_steps);
void launch_txi_final(hipStream_t stream, size_t nrows, const uint8_t* arena, const uint8_t* status,
                      const uint32_t* first, const uint32_t* tfirst, const praos_txi_dev_rows* rows,
                      const praos_txi_dev_rows* out);
// k_txwit.hip: the key witnesses of the index's final rows.  count: per row the PRAOS_TXW_* status,
// the VKey / bootstrap counts, their sum and the offsets of the two values (blk_kind: the index's
// kind per block).  emit: the witness records at wit_first[row] + j (n_wits = the arrays' length).
// verify: witnesses [w0, w1), lane t on table region t of tabs (LT_ED entries each): ok and the
// key hash [n_wits][28].  tx: the rows' failing witnesses.  blocks: the sums per block over rows
// [tfirst[i], tfirst[i + 1]).
void launch_txw_count(hipStream_t stream, size_t nrows, const uint8_t* arena, uint64_t arena_len,
                      const uint8_t* blk_kind, const uint32_t* row_block, const uint64_t* wit_off,
                      const uint32_t* wit_len, uint8_t* status, uint32_t* n_vkey, uint32_t* n_boot, uint32_t* cnt,
                      uint64_t* v0, uint64_t* v2);
void launch_txw_emit(hipStream_t stream, size_t nrows, const uint8_t* arena, const uint64_t* wit_off,
                     const uint32_t* wit_len, const uint32_t* n_vkey, const uint32_t* n_boot, const uint64_t* v0,
                     const uint64_t* v2, const uint32_t* wit_first, uint64_t n_wits, uint32_t* tx, uint8_t* kind,
                     uint64_t* key_off, uint64_t* sig_off);
void launch_txw_verify(hipStream_t stream, size_t w0, size_t w1, const ge_niels* gbtab, const uint8_t* arena,
                       const uint32_t* tx, const uint8_t* kind, const uint64_t* key_off, const uint64_t* sig_off,
                       const uint8_t* tx_id, uint8_t* ok, uint8_t* key_hash, ge_cached* tabs);
void launch_txw_tx(hipStream_t stream, size_t nrows, const uint32_t* wit_first, const uint8_t* ok, uint32_t* n_bad);
void launch_txw_blocks(hipStream_t stream, size_t n, const uint32_t* tfirst, const uint8_t* status,
                       const uint32_t* cnt, const uint32_t* tx_bad, uint32_t* n_wit, uint32_t* n_bad,
                       uint32_t* n_shape);
// k_pbft.hip: Byron header validation.  decode: one lane per stored header (columns, the verify
// inputs keys / sig / hram, the delegate's key hash dhash [n][28] and its index in dtab -- n_delegs
// x 8 words sorted by the 7 hash words, word 7 the caller's index -- and the list of lanes that
// take the signature verify); sig: uncached verifies over list[0 .. *count); sig_ck: the key
// cache's hits; keyhash: hashVerKey of n 64-byte keys into [n][28].  n sizes the grids.
void launch_pbft_decode(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* hoff,
                        const uint32_t* hlen, const uint8_t* is_ebb, uint64_t epoch_slots, uint32_t pm,
                        const uint32_t* dtab, uint32_t n_delegs, uint64_t* slot, uint64_t* block_no,
                        uint8_t* prev_hash, uint8_t* prev_genesis, uint8_t* header_hash, uint8_t* bits, int32_t* gk_idx,
                        uint8_t* dhash, uint8_t* keys, uint8_t* sig, uint8_t* hram, uint32_t* vlist, uint32_t* vcount);
void launch_pbft_sig(hipStream_t stream, size_t n, const uint32_t* list, const uint32_t* count, const ge_niels* gbtab,
                     const uint8_t* keys, const uint8_t* sig, const uint8_t* hram, uint8_t* bits, ge_cached* tabs);
void launch_pbft_sig_ck(hipStream_t stream, size_t n, const uint32_t* list, const uint32_t* count,
                        const int32_t* item_entry, const ge_cached* ktab, const uint32_t* kinfo, const ge_niels* comb,
                        const uint8_t* keys, const uint8_t* sig, const uint8_t* hram, uint8_t* bits);
void launch_pbft_keyhash(hipStream_t stream, size_t n, const uint8_t* keys64, uint8_t* out28);
// replay: nonce contribution of each header's certified VRF output (k_misc.hip)
void launch_vrf_nonce(hipStream_t stream, size_t n, const uint8_t* vrf_out, int tpraos, uint8_t* nonce_out);
// self-test kernels of the field / group / scalar-multiplication layers (k_selftest.hip; the
// launch_selftest4_* forms come from the ILP-4 build, k_selftest4.hip)
void launch_selftest_fe_multi(hipStream_t stream, int op, size_t n, const uint8_t* in, uint8_t* out);
void launch_selftest_fe(hipStream_t stream, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* r);
void launch_selftest_int(hipStream_t stream, int op, size_t n, const uint8_t* a, const uint8_t* b, const uint8_t* c,
                         uint8_t* out);
void launch_selftest_ge(hipStream_t stream, int op, size_t n, const uint8_t* p, const uint8_t* q, uint8_t* out,
                        const ge_niels* gbtab);
void launch_selftest4_ge(hipStream_t stream, int op, size_t n, const uint8_t* p, const uint8_t* q, uint8_t* out,
                         const ge_niels* gbtab);
void launch_selftest_msm(hipStream_t stream, int variant, size_t n, const uint8_t* P, const uint8_t* Q,
                         const uint8_t* sp, const uint8_t* sq, const uint8_t* sb, const ge_niels* gbtab,
                         const ge_niels* comb, ge_cached* tabs, const ge_cached* ktab, uint8_t* out);
void launch_selftest4_msm(hipStream_t stream, int variant, size_t n, const uint8_t* P, const uint8_t* Q,
                          const uint8_t* sp, const uint8_t* sq, const uint8_t* sb, const ge_niels* gbtab,
                          const ge_niels* comb, ge_cached* tabs, const ge_cached* ktab, uint8_t* out);
// self-test kernels of the stored-byte hashes (k_selftest_hash.hip): praos_debug_hash_bytes kinds
// 0, 1, 3, 4 (kind 2 is launch_seg_hash); the tables are praos_hip.h's
void launch_selftest_hash(hipStream_t stream, int kind, size_t n, const uint8_t* arena, const uint64_t* off,
                          const uint32_t* len, const uint8_t* aux, const uint64_t* parts, uint8_t* out);
// wire headers (k_wire.hip): unwrap + header hash of n wire items (hash may be NULL)
void launch_wire_split(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                       const uint32_t* len, uint32_t n_eras, uint8_t* status, uint8_t* era, uint8_t* kind,
                       uint32_t* hint, uint64_t* ioff, uint32_t* ilen, uint8_t* hash);
// the row set of the wire calls (k_wire.hip; api_internal.hpp RowSet holds the arrays): per-item
// arrays of n entries, item_slot / slot_min say which class an item is in.  set: the hash set over
// (tag, 32-byte key) of the items with flag[i] == 0 and tag[i] < 32 in tag_mask; slot_item /
// slot_min: mask + 1 words each, a power of two >= 2n, zeroed / set to 0xff by the caller.  ident:
// no set, every index below *limit (NULL: n) with flag[i] == flag_ok a class of its own; slot_min:
// n words.  count: item_rep[i] = the lowest item of i's class; blk: one word per block of NT items.
// number: count, then the rows in order of first appearance: *total = the rows; row_off / row_len:
// the representatives' spans ioff / ilen (rows < rows_cap); rep_row: each representative's row;
// item_row: each item's row (0xffffffff: none).  rep: row_item[row] = the row's representative
// (row_item set to 0xff by the caller).  row_kind: row_is_ebb[row] = its kind is 0 (rows < rows_cap).
void launch_hdr_set(hipStream_t stream, size_t n, const uint8_t* flag, const uint8_t* tag, const uint8_t* key,
                    uint32_t tag_mask, uint32_t mask, uint32_t* slot_item, uint32_t* slot_min, uint32_t* item_slot);
void launch_hdr_ident(hipStream_t stream, size_t n, const uint32_t* limit, const uint8_t* flag, uint8_t flag_ok,
                      uint32_t* item_slot, uint32_t* slot_min);
void launch_hdr_count(hipStream_t stream, size_t n, const uint32_t* item_slot, const uint32_t* slot_min,
                      uint32_t* item_rep, uint32_t* blk);
void launch_hdr_number(hipStream_t stream, size_t n, const uint32_t* item_slot, const uint32_t* slot_min,
                       uint32_t* item_rep, uint32_t* blk, uint32_t* total, const uint64_t* ioff, const uint32_t* ilen,
                       uint32_t rows_cap, uint64_t* row_off, uint32_t* row_len, uint32_t* rep_row, uint32_t* item_row);
void launch_hdr_rep(hipStream_t stream, size_t n, const uint32_t* item_slot, const uint32_t* item_rep,
                    const uint32_t* rep_row, uint32_t* row_item);
void launch_hdr_row_kind(hipStream_t stream, size_t n, const uint32_t* item_slot, const uint32_t* item_rep,
                         const uint32_t* rep_row, const uint8_t* kind, uint32_t rows_cap, uint8_t* row_is_ebb);
// wire transactions (k_gentx.hip).  Per-item arrays of n entries (hash may be NULL) and the final
// rows' arrays (n entries each: a call has at most n rows; block: zeros, the row_block of
// launch_txw_count under a one-entry kind table).  split: unwrap, top-level walk, dedup hash.
// rows: provisional rows [0, *total): row_ok, the ExUnits sums, tx_id.
// final: the kept rows' fields at row_final[row]; item_row from provisional to final rows, the
// items of refused rows PRAOS_GTX_SHAPE.
struct praos_gtx_dev_items {
  uint8_t* status;
  uint8_t* era;
  uint8_t* kind;
  uint8_t* is_valid;
  uint64_t* ioff;
  uint32_t* ilen;
  uint64_t* body_off;
  uint32_t* body_len;
  uint64_t* wit_off;
  uint32_t* wit_len;
  uint64_t* aux_off;
  uint32_t* aux_len;
  uint32_t* size;
  uint8_t* hash;
};
struct praos_gtx_dev_rows {
  uint32_t* item;
  uint8_t* era;
  uint64_t* body_off;
  uint32_t* body_len;
  uint64_t* wit_off;
  uint32_t* wit_len;
  uint64_t* aux_off;
  uint32_t* aux_len;
  uint32_t* size;
  uint32_t* in_block_size;
  uint64_t* ex_mem;
  uint64_t* ex_steps;
  uint8_t* is_valid;
  uint8_t* tx_id;
  uint32_t* block;
};
void launch_gtx_split(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                      const uint32_t* len, uint32_t n_eras, const praos_gtx_dev_items* items);
void launch_gtx_rows(hipStream_t stream, size_t n, const uint32_t* total, const uint8_t* arena, const uint32_t* row_item,
                     const praos_gtx_dev_items* items, uint8_t* row_ok, uint64_t* ex_mem, uint64_t* ex_steps,
                     uint8_t* tx_id);
void launch_gtx_final(hipStream_t stream, size_t n, const uint32_t* total, const uint32_t* row_item,
                      const uint8_t* row_ok, const uint32_t* row_final, const uint64_t* ex_mem, const uint64_t* ex_steps,
                      const uint8_t* tx_id, const praos_gtx_dev_items* items, uint32_t* item_row,
                      const praos_gtx_dev_rows* rows);
// wire blocks (k_blockfetch.hip).  unwrap: status, disk tag and inner span of n wire items; hoff /
// hlen: the inner span again, launch_block_split's in / out columns.  key: elig[i] = 0 for an item
// that splits and decodes (1 otherwise) and, key != NULL, the hash set's key (header hash with the
// inner length folded in); *any_byron = 1 when such an item has disk tag 0 or 1.  class: one wave
// per item over launch_hdr_set's item_slot and launch_hdr_count's item_rep: slot2 / min2 for
// launch_hdr_number, a member that differs from its representative in a byte a class of its own.
// rows: the representatives' columns at rep_row (R rows; seg_off / seg_len
// segment-major over R).  bits: a Byron row's bits, which and zero body hash from
// launch_byron_integrity's results (NULL: Byron off).  verdict: PRAOS_BF_* per item, then which[]
// loses its host-internal flag.  span_equal: out[i] = the spans a and b of len[i] bytes are equal.
struct praos_bf_dev_items {
  const uint8_t* tag;
  const uint8_t* kind;            // launch_byron_split's (zeros with Byron off)
  const uint64_t* slot;
  const uint64_t* block_no;
  const uint64_t* hoff;
  const uint32_t* hlen;
  const uint8_t* header_hash;
  const uint8_t* prev_hash;
  const uint8_t* body_hash;       // the header's
  const uint8_t* nseg;
  const uint64_t* seg_off;
  const uint32_t* seg_len;
};
struct praos_bf_dev_rows {
  uint32_t* item;
  uint8_t* tag;
  uint8_t* is_ebb;
  uint64_t* slot;
  uint64_t* block_no;
  uint64_t* hdr_off;
  uint32_t* hdr_len;
  uint8_t* header_hash;
  uint8_t* prev_hash;
  uint8_t* claimed;               // the header's body hash
  uint8_t* nseg;
  uint64_t* seg_off;
  uint32_t* seg_len;
};
void launch_span_equal(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* a_off,
                       const uint64_t* b_off, const uint32_t* len, uint8_t* out);
void launch_bf_unwrap(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                      const uint32_t* len, uint32_t n_eras, uint8_t* status, uint8_t* tag, uint64_t* ioff,
                      uint32_t* ilen, uint64_t* hoff, uint32_t* hlen);
void launch_bf_key(hipStream_t stream, size_t n, const uint8_t* status, const uint8_t* split_status,
                   const uint16_t* dec_status, const uint8_t* tag, const uint32_t* ilen, const uint8_t* header_hash,
                   uint8_t* elig, uint8_t* key, uint32_t* any_byron);
void launch_bf_class(hipStream_t stream, size_t n, const uint8_t* arena, const uint32_t* item_slot,
                     const uint32_t* item_rep, const uint64_t* ioff, const uint32_t* ilen, uint32_t* slot2,
                     uint32_t* min2);
void launch_bf_rows(hipStream_t stream, size_t n, size_t R, const uint32_t* slot2, const uint32_t* rep_row,
                    const praos_bf_dev_items* items, const praos_bf_dev_rows* rows);
void launch_bf_bits(hipStream_t stream, size_t R, const uint8_t* tag, const uint8_t* byr_result,
                    const uint8_t* byr_which, uint8_t* bits, uint8_t* which, uint8_t* body_hash);
void launch_bf_verdict(hipStream_t stream, size_t n, size_t R, int byron_on, const uint8_t* status, const uint8_t* tag,
                       const uint32_t* item_row, const uint32_t* exp_idx, const uint64_t* exp_slot,
                       const uint8_t* exp_hash, const uint64_t* slot, const uint8_t* header_hash, const uint8_t* bits,
                       uint8_t* which, uint8_t* verdict);
