#pragma once
// replay_internal.hpp -- entry points of libpraos_hip used by the replay driver
// (praos_replay.hip) for its threaded pipeline, and the few shims the host modules (replay, group,
// candidates, pbft) and the API units share; C++ linkage, not part of the C ABI.
#include "praos_hip.h"
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

// The context for the other host modules (praos_api.hip): its error text; the refusal of a call
// that needs a device (true on a host-only context, with the error text set); the replay call scope
// (first error kept, pool-key store on); and in praos_xfer.hip the group's page-locked ranges
// (praos_group_host_register: pinned once, known to every member) and the staging copy threads onto
// the given CPUs (empty: back to the process's own mask).
void praos_set_error_(praos_ctx* c, const std::string& m);
bool praos_host_only_(praos_ctx* c);
void praos_replay_scope_(praos_ctx* c, bool on);
int praos_ctx_note_registered_(praos_ctx* c, void* p, size_t len, bool add);
void rp_copy_pin(praos_ctx* c, const std::vector<int>& cpus);
// Byron's delegation map (praos_pbft.hip): hashVerKey on the host, and the Bimap's rule (no
// duplicate in either column)
void praos_pbft_key_hash_host_(const uint8_t* keys64, size_t n, uint8_t* out28);
bool praos_pbft_delegs_ok_(const uint8_t* delegs, uint32_t n);

struct praos_span {           // a run of stored bytes in host memory (e.g. an mmapped chunk file)
  const uint8_t* p;
  size_t len;
};

// (praos_stream.hip, down to rp_download_leader but for the ledger views)
// A persistent from-bytes batch with room for n_cap headers over bytes_cap stored bytes, its
// own events and pinned host buffers for the nonce table.
praos_batch* rp_batch_alloc(praos_ctx* c, size_t n_cap, size_t bytes_cap, bool tpraos);
void rp_batch_destroy(praos_ctx* c, praos_batch* b);
bool rp_batch_fits(const praos_batch* b, size_t n, size_t bytes);
// The context keeps the replay's batches between calls (RP_SLOTS of them, freed by praos_close):
// rp_batch_take returns slot k's batch when it fits n headers over `bytes` (else a new one),
// rp_batch_keep hands it back.
constexpr int RP_SLOTS = 4;
praos_batch* rp_batch_take(praos_ctx* c, int k, size_t n, size_t bytes, bool tpraos);
void rp_batch_keep(praos_ctx* c, int k, praos_batch* b);
// the batch's pinned result buffers (bits, pool index: its header capacity each)
void rp_batch_results(praos_batch* b, uint16_t** bits, int32_t** pidx);
// Waits for the batch's last decode and crypto run (a stopped replay leaves queued runs).
void rp_batch_quiesce(praos_batch* b);
// Copy stream: the spans' concatenation (the arena) and the per-header (offset, length) go
// H2D through the pinned staging buffers, then decode and the nonce value of each header's
// certified VRF output (k_vrf_nonce).  Returns once the host side is queued.
int rp_upload_decode(praos_ctx* c, praos_batch* b, size_t n, const praos_span* spans, size_t nspans,
                     const uint64_t* hoff, const uint32_t* hlen);
// D2H of the decoded fields the nonce chain and the fold read, and the nonce values, into the
// batch's pinned area (copy stream; returns when they are in host memory).  d's pointers and
// *nonce stay valid until the batch's next download.
constexpr size_t DEC_H_BYTES = 3 * 8 + 4 * 32 + 4 + 2 + 1;
int rp_download_decoded(praos_ctx* c, praos_batch* b, praos_decoded* d, uint8_t** nonce);
// The crypto run under per-header epoch nonces (etas[eta_idx[i]]), queued after the decode;
// the host arrays are copied before return.
int rp_run(praos_ctx* c, praos_batch* b, const praos_nonce* etas, uint32_t k, const uint8_t* eta_idx);
// Waits for the run and copies its bits and pool indices out (download stream).
int rp_download_results(praos_ctx* c, praos_batch* b, uint16_t* bits, int32_t* pool_idx);
// The pool part of one ledger view (praos_api.hip): host map (hash28 -> caller index) and, when
// built for a device, the tables the VRF join and the leader test read.
struct rp_view;
rp_view* rp_view_make(praos_ctx* c, const praos_pool* pools, uint32_t npools, const praos_params* params,
                      bool device);
void rp_view_free(praos_ctx* c, rp_view* v);
// The device pool tables a context's launches read (praos_set_epoch's, or a view's swapped in by
// the launcher thread: kernels already queued keep the pointers they were launched with).
struct rp_tables {
  uint32_t npools;
  uint32_t *hash, *vrf, *x;
  int32_t* map;
};
rp_tables rp_tables_get(const praos_ctx* c);
void rp_tables_set(praos_ctx* c, const rp_tables& t);
rp_tables rp_view_tables(const rp_view* v);
// praos_validate_headers_nonces / praos_tpraos_validate_headers_nonces with the evolving nonce
// after each header precomputed by the caller's nonce chain (used until the first invalid header);
// view (may be NULL: the context's praos_set_epoch pools) is the ledger view the batch was verified
// under.  (praos_fold.hip)
int rp_fold(praos_ctx* c, const praos_headers* h, const uint8_t* prev_hash, const uint8_t* prev_is_genesis,
            const praos_out* crypto, praos_envelope* env, const praos_epoch_info* ei, praos_chain_state* st,
            const praos_nonce* etas, uint32_t k, const uint8_t* eta_idx, const praos_nonce* evolving_after,
            bool tpraos, const praos_nonce* extra_entropy, uint8_t* verdict, uint16_t* failures, size_t* chain_stop,
            size_t* processed, const rp_view* view, const uint32_t* map = nullptr, bool client = false,
            std::string* err_out = nullptr);
// map: item i reads row map[i] of every per-header input (PRAOS_NO_ROW: an item without a header,
// PRAOS_V_INPUT) and keeps index i for verdict / failures / evolving_after; NULL: row i.  client:
// the ChainSync client's fold (PRAOS_V_DOESNT_FIT before validateHeader; ends at the first
// failure).  err_out: the error text, instead of the context's (folds running side by side).
//
// The context's device (praos_group.hip).  The candidates call (praos_candidates.hip): a device
// buffer of at least `bytes` the context keeps between calls (NULL: allocation failed; its earlier
// contents are gone when it grows; carved by api_internal.hpp's carve_kept), an upload
// of the spans' concatenation into it (copy stream, pinned staging; dst has room for the bytes
// rounded up to 8 plus 16, the pad is zeroed), and the decode of rows [first, n) of a replay
// batch from device span arrays into that arena.
int rp_device(const praos_ctx* c);
uint8_t* rp_scratch(praos_ctx* c, size_t bytes);
int rp_upload_bytes(praos_ctx* c, uint8_t* dst, const praos_span* spans, size_t nspans);
int rp_decode_rows(praos_ctx* c, praos_batch* b, const uint8_t* arena, size_t arena_len, const uint64_t* hoff,
                   const uint32_t* hlen, size_t first, size_t n);
// the leader certificates (output n*64, proof n*80; either may be NULL) of a TPraos batch's rows,
// after its run
int rp_download_leader(praos_ctx* c, praos_batch* b, uint8_t* leader_out, uint8_t* leader_proof);
// The Byron candidates call: praos_verify_pbft_headers' body over n > 0 rows already on the device
// (praos_blocks.hip: spans into an arena with ld64u's pad behind it and two bytes in front of every
// span, is_ebb flags; all final before the call), and the ChainSync client's mode of the PBFT fold
// (praos_pbft.hip): item i reads row map[i] (PRAOS_NO_ROW: PRAOS_V_INPUT) of h and row_is_ebb,
// PRAOS_V_DOESNT_FIT before the envelope, the fold ends at the first failure (*processed = items
// judged).  The caller has checked params, delegs and the state's room; err_out gets the text.
int rp_pbft_verify_rows(praos_ctx* c, size_t n, const uint8_t* arena, size_t arena_len, const uint64_t* hoff,
                        const uint32_t* hlen, const uint8_t* d_is_ebb, const praos_pbft_params* p,
                        const uint8_t* delegs, uint32_t n_delegs, praos_pbft_out* out);
int rp_pbft_fold_client(size_t n, const uint32_t* map, size_t n_rows, const praos_pbft_out* h,
                        const uint8_t* row_is_ebb, const praos_pbft_params* p, const uint8_t* delegs,
                        uint32_t n_delegs, praos_pbft_tip* tip, praos_pbft_state* st, uint8_t* verdict, uint64_t* aux,
                        size_t* chain_stop, size_t* processed, std::string* err_out);
// The replay of praos_replay_immutable[_tpraos|_views] over m contexts (praos_replay.hip): batch k
// is uploaded, decoded and verified on mem[k % m]; the nonce chain and the fold run once, in chain
// order, the fold and the error text on mem[0].  m = 1 is the single-context replay.  views
// (nviews > 0, Praos only): a ledger view per epoch instead of pools / env's limits.
int rp_replay(praos_ctx* const* mem, int m, const char* dir, const praos_pool* pools, uint32_t npools,
              const praos_params* params, const praos_epoch_info* ei, praos_envelope* env, praos_chain_state* st,
              size_t batch_max, uint8_t* verdicts, uint16_t* failures, size_t verdicts_cap,
              praos_replay_stats* stats, bool tpraos, const praos_nonce* extra_entropy,
              const praos_ledger_view* views = nullptr, uint32_t nviews = 0);
