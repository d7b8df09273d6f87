// launch.hpp -- host launchers exported by each kernel module (generated
// alongside the kernels; see the bottom of k_*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "kargs.hpp"
// The launchers of the OCert, KES, VRF, key-cache and PBFT signature kernels take the stream, the
// item count n (they launch ceil(n / 256) blocks of 256: kcommon.hpp launch_grid), the list they run
// over (KeyItems: null list = every i < n; KeyHits: a cache's hits), the tables, and the kernel's
// argument struct (kargs.hpp), which goes to the kernel as it is but for the fields a launcher is
// said to clear.  "reads" names the struct fields the kernels behind a launcher read: a caller may
// leave the others as they are.  ilp4: the kernel's twin from the ILP-4 build (the end of this file).

// OCert.  launch_ocert (k_ocert; ilp4: k_ocert4, list mode only) reads cold_vk, hot_vk, ocert_n,
// ocert_c0, sig, tabs, and ok_out (non-null: the verdict goes there and slot, slots_per_kes_period,
// max_kes_evo, bits are not read); ilp4 also wave_prio (non-zero: waves at s_setprio 3).
// launch_ocert_ck (k_ocert_ck; ilp4: k_ocert_ck4) reads the same but tabs, and wave_prio (2 or 3;
// ilp4: not read).
void launch_ocert(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const OcertIn& a, int ilp4 = 0);
void launch_ocert_ck(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const OcertIn& a,
                     int ilp4 = 0);
// One-kernel VRF (k_vrf), the plain praos_verify_vrf batch: reads vrf_vk, vrf_proof, tabs, alpha_in,
// ok_out, beta_out (null: not written).  With alpha_in null it is the header mode (every field up to
// nonce_out; leader_out / nonce_out / beta_out null: not written), which has no caller.
void launch_vrf(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const VrfIn& a);
// pentry / pkey / pmask: the pool-key store probed first (null: none)
void launch_key_insert(hipStream_t stream, size_t n, KeyItems items, const uint8_t* keys, uint32_t mask,
                       uint32_t* slot_rep, uint32_t* slot_cnt, int32_t* item_slot, const int32_t* pentry,
                       const uint32_t* pkey, uint32_t pmask, uint32_t* scnt);
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
// one lane per hash-set slot (cap of them)
void launch_key_assign(hipStream_t stream, uint32_t cap, const uint32_t* slot_rep, const uint32_t* slot_cnt,
                       uint32_t min_count, uint32_t max_entries, int32_t* slot_entry, uint32_t* entry_rep,
                       uint32_t* entry_pos, uint32_t* counters, const KeyWide& w = KeyWide());
void launch_key_partition(hipStream_t stream, size_t n, KeyItems items, const int32_t* item_slot,
                          const int32_t* slot_entry, int32_t* item_entry, uint32_t* entry_pos, uint32_t* hit_list,
                          uint32_t* miss_list, uint32_t* counters, uint32_t* spos, const KeyWide& w = KeyWide());
void launch_ocert_dedup(hipStream_t stream, size_t n, const uint8_t* cold, const uint8_t* hot,
                        const uint64_t* on, const uint64_t* oc, const uint8_t* sig, uint32_t mask, uint32_t* slot_rep,
                        uint32_t* item_rep, uint32_t* reps, uint32_t* counters);
void launch_ocert_fanout(hipStream_t stream, size_t n, const uint32_t* item_rep,
                         const uint8_t* ok, const uint64_t* slot, const uint64_t* oc, uint64_t slots_per_kes_period,
                         uint64_t max_kes_evo, uint16_t* bits);
// entries [*base (0 when null), min(counters[0], max_entries)), at most span of them
void launch_key_precompute(int kind, hipStream_t stream, const uint32_t* counters, uint32_t max_entries,
                           const uint32_t* entry_rep, const uint8_t* keys, ge_cached* ktab, uint32_t* kinfo,
                           int wave_prio, const uint32_t* base, uint32_t span,
                           int mode,                       // 1: the chain from the ILP-4 build (k_keys4.hip)
                           const KeyWide& w = KeyWide());
void launch_pkey_reset(hipStream_t stream, uint32_t* count, int32_t* pentry, uint32_t slots, uint32_t limit, int force);
void launch_pkey_publish(hipStream_t stream, const uint32_t* counters, const uint32_t* base, uint32_t max_entries,
                         const uint32_t* entry_rep, const uint8_t* keys, int32_t* pentry, uint32_t* pkey,
                         uint32_t pmask, uint32_t* count, uint32_t span);
// KES.  launch_kes (k_kes; ilp4: k_kes4, list mode only) reads hot_vk, kes_sig, body_off, body_len,
// body, body_bytes_len, tabs, period (null: the period from slot, ocert_c0, slots_per_kes_period),
// result (non-null: the verdict goes there, not to bits); ilp4 also wave_prio (non-zero: s_setprio 3).
// launch_kes_ck (k_kes_ck, or k_kes_ck2 when pair_min != 0; ilp4: k_kes_ck4, which ignores pair_min,
// entry_rep / rep_ok and wave_prio) reads the same but tabs, and wave_prio (2 or 3).
// launch_kes_merkle_reps reads hot_vk, kes_sig and the period's fields; launch_kes_leafkeys kes_sig
// and the period's fields.
void launch_kes(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const KesIn& a, int ilp4 = 0);
void launch_kes_ck(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const KesIn& a,
                   uint32_t pair_min,                       // two headers per lane from pair_min hits on (0: never)
                   const uint32_t* entry_rep,               // with rep_ok (k_kes_merkle_reps): the Merkle path
                   const uint8_t* rep_ok,                   // dedup per cache entry (null: every item walks)
                   int ilp4 = 0);
void launch_kes_merkle_reps(hipStream_t stream, const uint32_t* counters, uint32_t max_entries,
                            const uint32_t* entry_rep, const KesIn& a, uint8_t* rep_ok);
void launch_kes_leafkeys(hipStream_t stream, size_t n, const KesIn& a, uint8_t* keys);
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
// The staged VRF of the header pipeline (k_vrf_stage.hip; `mid`: the stage record, VRF_MID_PLANES x
// 16 x n bytes).
// Stage V over headers [i0, min(i1, n)), mid stride n (k_vrf_v; ilp4 1: k_vrf_v4 from the ILP-4 build,
// 2: k_vrf_v4x, the same holding its SIMD alone): reads vrf_vk, vrf_proof, slot, eta0, eta0_neutral,
// eta_idx (null: one nonce), tabs, wave_prio (non-zero: s_setprio 3), tp_seed.
void launch_vrf_v(hipStream_t stream, size_t n, const VrfIn& a, void* mid, size_t i0 = 0, size_t i1 = SIZE_MAX,
                  int ilp4 = 0);
// Two-stage form, stage F = U + join over a list: the uncached keys (k_vrf_fin_nc: per-lane U;
// clears rec) or a cache's hits (k_vrf_fin; entry_wide: k_vrf_fin_w, h = the wide tier's hits and
// tables).  Reads cold_vk, vrf_vk, vrf_out, vrf_proof, the pool fields, check_output, bits, pool_idx,
// pool_sorted_idx, beta_out, leader_out, nonce_out, tabs, and the hits rec (null: no pool records).
// The two tables have one type: gbtab is the fixed-base comb of BCOMB_T tables (the context's btab,
// staged into LDS), comb the radix-2^16 comb (the context's bcomb16, read in place).  The same holds
// for launch_vrf_u, the OCert / KES launchers above and the PBFT ones below.
void launch_vrf_fin(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const VrfIn& a,
                    const void* mid);
void launch_vrf_fin(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const VrfIn& a,
                    const void* mid, const int32_t* entry_wide = nullptr);
// Three-kernel form, stage U over a list: the uncached keys (k_vrf_u_nc, 8-entry lane tables utabs;
// reads vrf_vk, vrf_proof) or a cache's hits (k_vrf_u; ilp4: k_vrf_u4; entry_wide: k_vrf_u_w, no ILP-4
// form; reads vrf_proof, wave_prio 2 or 3) ...
void launch_vrf_u(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const VrfIn& a,
                  ge_cached* utabs, void* mid);
void launch_vrf_u(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const VrfIn& a, void* mid,
                  int ilp4 = 0, const int32_t* entry_wide = nullptr);
// ... and the join over all n (k_vrf_join): reads what the cached stage F reads but tabs, and
// wave_prio (non-zero: s_setprio 3), pre (launch_vrf_pool ran before: bits, pool, leader, nonce are
// there), rec_entry (the VRF key cache's item_entry, or null) and rec; clears rec when rec_entry is null.
void launch_vrf_join(hipStream_t stream, size_t n, const VrfIn& a, const void* mid);
// the join's pool part ahead of it (k_vrf_pool): reads cold_vk, vrf_vk, vrf_out, the pool fields, bits,
// pool_idx, pool_sorted_idx, leader_out, nonce_out, rec_entry, rec (cleared as by the join)
void launch_vrf_pool(hipStream_t stream, size_t n, const VrfIn& a);
// the pool record of each VRF key-cache entry (k_vrf_keyrec; VREC_WORDS words per entry): the pool
// part of the entry's representative, which the entry's headers with the same cold key take instead
// of hashing and searching themselves.  Reads cold_vk, vrf_vk and the pool fields.
#define VREC_WORDS 12
void launch_vrf_keyrec(hipStream_t stream, const uint32_t* counters, uint32_t max_entries, const uint32_t* entry_rep,
                       const VrfIn& a, uint32_t* rec);
// TPraos join of certificate cert (0: eta, 1: leader; k_vrf_join_tp), after stage V (tp_seed 1 + cert)
// and U of that certificate into `mid`: reads cold_vk, vrf_vk, vrf_out / vrf_proof / beta_out (the
// certificate's), the pool fields, check_output, bits, pool_idx, pool_sorted_idx, nonce_out.
void launch_vrf_join_tp(hipStream_t stream, size_t n, int cert, const VrfIn& a, const void* mid,
                        const int32_t* ovl_class, const uint32_t* gen);
// one-kernel TPraos (k_vrf_tp, which takes the columns one by one): a's vrf_out / vrf_proof / beta_out
// are the eta certificate's, l_* the leader certificate's; reads every field up to nonce_out but
// alpha_in and leader_out, and tabs.
void launch_vrf_tp(hipStream_t stream, size_t n, const ge_niels* gbtab, const VrfIn& a, const uint8_t* l_out,
                   const uint8_t* l_proof, uint8_t* beta_l, const int32_t* ovl_class, const uint32_t* gen);
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
void launch_pbft_sig(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const uint8_t* keys,
                     const uint8_t* sig, const uint8_t* hram, uint8_t* bits, ge_cached* tabs);
void launch_pbft_sig_ck(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const uint8_t* keys,
                        const uint8_t* sig, const uint8_t* hram, uint8_t* bits);
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

// ---- between kernel modules only: no host module calls these.  The launchers of the ILP-4 twins
// (k_miss4.hip, k_vrf_v4.hip, k_keys4.hip: the same bodies built with PRAOS_ILP4), which the launchers
// above forward to under their ilp4 / mode argument.
void launch_ocert4(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const OcertIn& a);
void launch_kes4(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const KesIn& a);
void launch_ocert_ck4(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const OcertIn& a);
void launch_kes_ck4(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const KesIn& a);
void launch_vrf_v4(hipStream_t stream, size_t n, size_t i0, size_t i1, const VrfIn& a, void* mid, int excl);
void launch_vrf_u4(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const uint8_t* vrf_proof,
                   void* mid, int prio);
void launch_key_precompute4(int kind, hipStream_t stream, const uint32_t* counters, uint32_t max_entries,
                            const uint32_t* entry_rep, const uint8_t* keys, ge_cached* ktab, uint32_t* kinfo,
                            int wave_prio, const uint32_t* base, uint32_t span);
