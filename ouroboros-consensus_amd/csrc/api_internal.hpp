#pragma once
// api_internal.hpp -- what the units of the host API share: the context and batch structs, the
// staging pool, the allocation / error helpers, the wire calls' row set and the functions that cross
// unit boundaries (praos_impl).  Included by praos_api / praos_xfer / praos_blocks / praos_stream /
// praos_run / praos_fold / praos_debug / praos_txindex / praos_txwit / praos_gentx / praos_blockfetch /
// praos_candidates only; the other host modules (replay, group, pbft) go through replay_internal.hpp.
#include "praos_hip.h"
#include "launch.hpp"
#include "host_util.hpp"
#include "replay_internal.hpp"
#include "chunk_scan.hpp"
#include "sched.hpp"

static constexpr size_t NT = 256;                  // threads per block of the crypto kernels
static constexpr size_t NIELS_BYTES = 3 * 32;      // sizeof(ge_niels)
static constexpr size_t BTAB_N = 128;              // entries per fixed-base table (scalarmult.hpp)
static constexpr size_t BCOMB_TABLES = 32;         // fixed-base comb: 256^j B, j < 32 (scalarmult.hpp BCOMB_T)
static constexpr size_t C16_TABLES = 16, C16_ENTRIES = 32768;   // radix-2^16 comb (scalarmult.hpp C16_T, C16_N)
static constexpr size_t CACHED_BYTES = 4 * 32;     // sizeof(ge_cached)
static constexpr size_t LT_ED_B = 8 * CACHED_BYTES, LT_VRF_B = 16 * CACHED_BYTES;   // per-lane tables (kcommon.hpp)
static constexpr size_t VRF_MID_BYTES = 28 * 16;    // per-header records of the staged VRF (praos_core.hpp)
static constexpr uint32_t TP_SIGNED_STRIDE = 640;   // max canonical TPraos BHBody: 586 bytes (k_decode.hip)

#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// A small persistent pool of host threads for the staging copies (pageable caller
// memory <-> pinned buffers): one job at a time, each worker takes its share.
class CopyPool {
 public:
  explicit CopyPool(unsigned n) : nt_(n) {
    for (unsigned t = 0; t < nt_; t++) th_.emplace_back([this, t] { loop(t); });
  }
  ~CopyPool() {
    { std::lock_guard<std::mutex> g(m_); stop_ = true; }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  unsigned size() const { return nt_; }
  void run(const std::function<void(unsigned)>& f) {
    std::unique_lock<std::mutex> g(m_);
    job_ = &f;
    pending_ = nt_;
    gen_++;
    cv_.notify_all();
    done_.wait(g, [this] { return pending_ == 0; });
    job_ = nullptr;
  }
  // every worker onto the given CPUs (empty: back to the process's own mask)
  void pin(const std::vector<int>& cpus) {
    cpu_set_t set;
    CPU_ZERO(&set);
    if (cpus.empty()) {
      if (sched_getaffinity(0, sizeof set, &set) != 0) return;
    } else {
      for (int c : cpus) CPU_SET(c, &set);
    }
    run([&](unsigned) { (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set); });
  }
  // dst[0, n) = src[0, n), split over the workers
  void copy(void* dst, const void* src, size_t n) {
    if (n < (1u << 20)) { std::memcpy(dst, src, n); return; }
    run([&](unsigned t) {
      const size_t a = n * t / nt_, b = n * (t + 1) / nt_;
      std::memcpy((uint8_t*)dst + a, (const uint8_t*)src + a, b - a);
    });
  }

 private:
  void loop(unsigned t) {
    uint64_t seen = 0;
    for (;;) {
      const std::function<void(unsigned)>* f;
      {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
        f = job_;
      }
      (*f)(t);
      std::lock_guard<std::mutex> g(m_);
      if (--pending_ == 0) done_.notify_all();
    }
  }
  unsigned nt_;
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  const std::function<void(unsigned)>* job_ = nullptr;
  unsigned pending_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

static constexpr size_t STAGE_PIECE = 16u << 20;    // pinned staging buffers: 2 x 16 MB per context
static constexpr int PIPE_MAX = 8;                  // chunks of the stored-bytes pipeline
static constexpr int PIPE_CALLS = 3;                // submitted stored-bytes calls in flight (pipe[0 .. 3))
static constexpr size_t PIPE_MIN_CHUNK = 49152;     // headers per chunk at least (auto mode)
static constexpr int PIPE_AUTO = 8;                 // chunks in auto mode (round 3, equal chunks: 4 -> 21.9M,
                                                    // 6 -> 23.0M, 8 -> 22.1M headers/s, profiles/r03/e2e_chunks.txt;
                                                    // round 5 with the first chunk at 1/4 of the others: 6 ->
                                                    // 25.3-25.6M, 8 -> 26.4-26.6M, profiles/r05/c8_pipe_head)
struct praos_batch;

// The context's last error.  The replay's worker threads (reader, nonce chain, launcher,
// fold) can fail at the same time, so every assignment takes a lock; while a replay runs
// (first_only) only the first message of the call is kept -- the one that stopped it.
class ErrMsg {
 public:
  ErrMsg& operator=(const std::string& m) {
    std::lock_guard<std::mutex> g(mu_);
    if (!(first_ && held_)) s_ = m;
    held_ = true;
    return *this;
  }
  ErrMsg& operator=(const char* m) { return *this = std::string(m); }
  const char* c_str() {
    std::lock_guard<std::mutex> g(mu_);
    return s_.c_str();
  }
  void first_only(bool on) {
    std::lock_guard<std::mutex> g(mu_);
    first_ = on;
    held_ = false;
  }

 private:
  std::mutex mu_;
  std::string s_;
  bool first_ = false, held_ = false;
};

struct praos_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t side[3] = {nullptr, nullptr, nullptr};   // concurrent crypto kernels
  hipStream_t mside[3] = {nullptr, nullptr, nullptr};  // their key-cache misses (uncached verifies)
  hipEvent_t mdone_ev[3] = {};
  hipStream_t vstream = nullptr;                       // VRF stage V (no key-cache dependence)
  hipStream_t vstream2 = nullptr;                      // the odd chunks' stage V of the stored-bytes pipeline
  hipEvent_t v_ev = nullptr, v2_ev = nullptr;
  hipEvent_t v0_ev = nullptr, v1_ev = nullptr;         // timing of k_vrf_v on its stream (kernel_ms[6])
  hipEvent_t kc0_ev = nullptr, kc1_ev = nullptr;       // timing of k_kes_ck on its stream (kernel_ms[7])
  hipEvent_t u_ev = nullptr;                           // stage U of the uncached VRF keys done
  hipEvent_t vrec_ev = nullptr;                        // the VRF key records are written (k_vrf_keyrec)
  // chunked stored-bytes pipeline (praos_verify_header_bytes): a copy stream, per-chunk
  // events and persistent chunk batches (reused while they are large enough)
  int pipeline = 0;                                    // PRAOS_OPT_PIPELINE (0 = auto)
  hipStream_t cstream = nullptr;
  hipStream_t dstream = nullptr;                       // replay: result downloads (rp_download_results)
  hipStream_t decstream = nullptr;                     // submitted calls: each landed chunk's decode (off the
                                                       // copy stream, whose next upload must not wait for it)
  praos_batch* rp_keep[RP_SLOTS] = {};                 // replay batches kept between calls
  uint8_t* cand_scratch = nullptr;                     // praos_validate_candidates: wire arena, item
  size_t cand_scratch_sz = 0;                          // buffers and hash set, kept between calls
  ge_cached* txw_tabs = nullptr;                       // praos_verify_tx_witnesses: the lane tables of one
  size_t txw_lanes = 0;                                // slice, kept between calls (grown, never shrunk)
  hipEvent_t up_ev[PIPE_MAX] = {}, done_ev[PIPE_MAX] = {};
  praos_batch* pipe[PIPE_MAX] = {};
  // praos_verify_header_bytes_submit: up to PIPE_CALLS calls in flight, on pipe[0 .. PIPE_CALLS) in turn
  struct PipeCall {
    bool active = false;
    praos_out out{};
    praos_decoded* dec = nullptr;
    hipEvent_t ev = nullptr;                           // the call's run has ended (ctx stream)
    uint64_t* off_h = nullptr;                         // pinned: its rebased offsets and lengths (async H2D:
    uint32_t* len_h = nullptr;                         // a pageable copy would wait for the copy stream)
    size_t cap = 0;
  } pcall[PIPE_CALLS];
  int pcall_next = 0;                                  // the slot the next submit takes: the oldest call's
  size_t pipe_n[PIPE_MAX] = {}, pipe_bytes[PIPE_MAX] = {};
  int concurrent = 1;                                  // PRAOS_OPT_CONCURRENT
  int kernels = 7;                                     // PRAOS_OPT_KERNELS
  int keycache = 2;                                    // PRAOS_OPT_KEYCACHE (min uses; 0 = off)
  uint32_t pbft_stats[4] = {0, 0, 0, 0};               // praos_pbft_stats of the last praos_verify_pbft_headers
  uint32_t pbft_raw[5] = {0, 0, 0, 0, 0};              // its download: the cache's counters, the verify count
  int dedup = 1;                                       // PRAOS_OPT_DEDUP
  SchedKnobs knobs;                                    // the schedule's knobs (sched.hpp; read from the
                                                       // environment when the context opens)
  hipEvent_t ev[6] = {};
  hipEvent_t side_ev[4] = {};
  hipEvent_t miss_ev[4] = {};                          // miss lists ready (OCert, KES, VRF), OCert misses done
  float kernel_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool last_from_bytes = false;
  bool v_timed = false;                                // the last run launched k_vrf_v
  bool kes_ck_timed = false;                           // ... and k_kes_ck
  ErrMsg err;
  ge_niels* btab = nullptr;
  ge_niels* bcomb16 = nullptr;                         // radix-2^16 comb of the cached-key chains (48 MB)
  // pool-key store (PRAOS_OPT_POOL_KEYS, k_keys.hip): cold [0] and VRF [1] key entries and
  // tables kept across runs; allocated on first use (256 MB of tables each)
  struct PoolKeyStore {
    uint32_t slots = 0, cap = 0;
    uint32_t *pkey = nullptr, *count = nullptr, *base = nullptr, *entry_rep = nullptr, *entry_pos = nullptr;
    uint32_t* kinfo = nullptr;
    int32_t* pentry = nullptr;
    ge_cached* ktab = nullptr;
    uint32_t *scnt = nullptr, *spos = nullptr;           // per entry: uses this run, start of its hit range
  } pks[2];                                            // [0] cold keys, [1] VRF keys
  int pool_keys = -1;                                  // 1 on, 0 off, -1 on inside praos_replay_immutable*
  bool replaying = false;
  bool pk_reset[2] = {false, false};                   // empty store t before the next run that uses it
  // epoch
  bool have_epoch = false;
  std::vector<praos_pool> epoch_pools;                 // praos_set_epoch's inputs as installed (a call
  praos_params epoch_params{};                         // with the same pools and parameters only swaps eta0)
  praos_params params{};
  uint32_t eta0[8] = {0};
  int eta0_neutral = 1;
  uint32_t npools = 0;
  uint32_t* d_pool_hash = nullptr;   // sorted, 7 words each
  uint32_t* d_pool_vrf = nullptr;    // 8 words
  uint32_t* d_pool_x = nullptr;      // 4 words
  int32_t* d_pool_map = nullptr;     // sorted idx -> caller idx
  uint32_t* d_eta0 = nullptr;
  std::vector<praos_pool> pools;     // caller order
  std::map<std::string, int32_t> pool_by_hash;
  // TPraos overlay schedule (praos_set_overlay): d, ascInv, epochs, genesis delegates
  // sorted by genesis key hash; device table: delegate hash (7 words + 0) | VRF hash (8)
  bool ovl_on = false;
  uint64_t ovl_d_num = 0, ovl_d_den = 1, ovl_asc_inv = 1, ovl_base = 0, ovl_len = 1;
  std::vector<praos_gen_deleg> gen_delegs;
  std::set<std::string> gen_delegate_hashes;
  uint32_t* d_gen = nullptr;
  // caller ranges page-locked with praos_host_register: uploads from them skip the staging
  std::mutex reg_mu;
  std::vector<std::pair<uintptr_t, size_t>> registered;
  // host <-> device staging for large transfers from pageable caller memory
  uint8_t* pin[2] = {nullptr, nullptr};
  uint8_t* zero_h = nullptr;                           // pinned zeros: an arena's tail padding by DMA (a fill
                                                       // kernel on the copy stream could wait behind another
                                                       // stream's kernels on a shared hardware queue)
  hipEvent_t pin_ev[2] = {};
  std::unique_ptr<CopyPool> pool;
  // device buffers of the last freed batch, reused by the next one in allocation
  // order (hipMalloc / hipFree of ~40 buffers cost ~20 ms per 432k batch)
  std::vector<void*> spare;
  std::vector<size_t> spare_sz;
  // host-side repack arena of praos_batch_upload, kept across calls (a fresh 170 MB
  // allocation per 432k batch cost its page faults and its unmapping on every call)
  std::unique_ptr<uint8_t[]> h_arena;
  size_t h_arena_cap = 0;
  std::vector<uint64_t> h_off;
  std::vector<uint32_t> h_len;
};

struct praos_batch {
  size_t n = 0;
  size_t body_bytes_len = 0;
  uint64_t *slot = nullptr, *ocert_n = nullptr, *ocert_c0 = nullptr, *body_off = nullptr;
  uint32_t* body_len = nullptr;
  uint8_t *cold_vk = nullptr, *vrf_vk = nullptr, *vrf_out = nullptr, *vrf_proof = nullptr, *hot_vk = nullptr,
          *ocert_sig = nullptr, *kes_sig = nullptr, *body = nullptr;
  uint16_t* bits = nullptr;
  uint16_t* bits3 = nullptr;   // per-kernel bits: ocert | kes | vrf
  int32_t *pool_idx = nullptr, *pool_sorted = nullptr;
  uint8_t *beta = nullptr, *leader = nullptr, *nonce = nullptr;
  // per-lane point tables of the three crypto kernels (kcommon.hpp lane_tab)
  ge_cached *tab_ocert = nullptr, *tab_kes = nullptr, *tab_vrf = nullptr;
  ge_cached* tab_vrfu = nullptr;   // 8-entry lane tables of stage U on uncached VRF keys
  bool v_done = false;             // stage V already queued on ctx->vstream (stored-bytes pipeline)
  uint8_t* vrf_mid = nullptr;   // stage V -> stage F record of the two-stage VRF
  uint8_t* vrf_mid2 = nullptr;  // TPraos: the leader certificate's record (allocated on first use)
  ge_cached* tab_vrf2 = nullptr; // TPraos: the leader certificate's stage-V lane tables
  size_t vrf_mid2_n = 0;
  // TPraos overlay classes of the batch's slots (praos_set_overlay): device copy sized once
  // per capacity, host arrays kept with the batch (the async upload reads them)
  int32_t* dcls = nullptr;
  size_t dcls_n = 0;
  std::vector<uint64_t> slots_h;
  std::vector<int32_t> cls_h;
  // per-run public-key cache (k_keys.hip): [0] cold keys (OCert), [1] VRF keys, [2] KES leaf keys
  struct KeyCache {
    uint32_t cap = 0, max_entries = 0;
    uint32_t *slot_rep = nullptr, *slot_cnt = nullptr, *entry_rep = nullptr, *entry_pos = nullptr, *kinfo = nullptr;
    int32_t *slot_entry = nullptr, *item_slot = nullptr, *item_entry = nullptr;
    uint32_t *counters = nullptr, *hit = nullptr, *miss = nullptr;   // counters: entries, hits, misses
    ge_cached* ktab = nullptr;
    uint8_t* rep_ok = nullptr;   // KES leaf keys: the Merkle walk verdict of each entry's representative
    uint32_t* vrec = nullptr;    // VRF keys: the pool record of each entry (k_vrf_keyrec, VREC_WORDS words)
    // this run's entry space: the arrays above, or the context's pool-key store
    ge_cached* kt = nullptr;
    uint32_t *ki = nullptr, *erep = nullptr, *epos = nullptr;
    const uint32_t* ebase = nullptr;
    uint32_t emax = 0;
    int store = -1;
    // the wide tier (VRF keys): buffers for wide_alloc keys, allocated when a run first uses it;
    // wide.min_uses = this run's threshold (0: the tier is off and every hit is in `hit`)
    KeyWide wide;
    uint32_t wide_alloc = 0;
  } kc[3];                       // [2] KES leaf keys
  uint8_t* kes_leaf = nullptr;   // n*32: the leaf key of each header's KES signature
  bool kc_used = false;
  // OCert dedup (k_keys.hip k_ocert_dedup): hash set over the 144-byte OCert tuple,
  // representative per item, list of representatives, their verify results
  uint32_t dd_cap = 0;
  uint32_t *dd_slot = nullptr, *dd_item_rep = nullptr, *dd_reps = nullptr, *dd_counters = nullptr;
  uint8_t* dd_ok = nullptr;
  bool dd_used = false;
  // batches from stored bytes (praos_batch_upload_bytes): the arena and the
  // decoded HeaderBody fields beyond the SoA above (k_decode.hip)
  bool from_bytes = false;
  uint32_t signed_stride = PRAOS_SIGNED_STRIDE;   // bytes per signed body (block batches: TP_SIGNED_STRIDE)
  uint8_t* arena = nullptr;
  size_t arena_len = 0;
  uint64_t *hoff = nullptr, *block_no = nullptr, *prot_major = nullptr, *prot_minor = nullptr;
  uint32_t *hlen = nullptr, *body_size = nullptr;
  uint8_t *prev_hash = nullptr, *prev_genesis = nullptr, *body_hash = nullptr, *header_hash = nullptr;
  uint16_t* dec_status = nullptr;
  // block-integrity batches (k_block.hip): stored block spans, segment spans
  // (segment-major [k][i]), per-segment hashes, results
  bool is_block = false;
  // several epoch nonces in one batch (praos_batch_set_nonces): device table of 9-word
  // entries (nonce, neutral flag) and per-header index; host copies for the fold
  uint32_t* eta_tab = nullptr;
  uint8_t* eta_idx = nullptr;
  bool decoded = false;          // praos_batch_decode ran: praos_batch_run skips the decode
  // TPraos header batches from stored bytes (praos_verify_tpraos_header_bytes): the
  // decoded leader certificate and its beta
  bool tp_only = false;
  uint8_t *lead_out = nullptr, *lead_proof = nullptr, *beta_l = nullptr;
  uint64_t *blk_off = nullptr, *seg_off = nullptr;
  uint32_t *blk_len = nullptr, *seg_len = nullptr;
  uint8_t *nseg = nullptr, *split_status = nullptr, *seg_hash = nullptr, *blk_result = nullptr, *blk_hash = nullptr;
  // CRC-32 of the block spans (k_crc32.hip): tile list, per-tile registers, results; kept for re-runs
  uint32_t *crc_first = nullptr, *crc_raw = nullptr, *crc_out = nullptr;
  uint32_t crc_tiles = 0;
  // Byron blocks (k_byron.hip): kind per block, the EBBs' epoch, the main blocks' span table,
  // the failing body comparisons; allocated on first use (byron_buffers)
  uint8_t *byr_kind = nullptr, *byr_which = nullptr;
  uint64_t* byr_epoch = nullptr;
  uint32_t* byr_spans = nullptr;
  std::vector<void*> owned;
  std::vector<size_t> owned_sz;
  praos_ctx* owner = nullptr;
  // replay batches (rp_batch_alloc): capacity, decode / run events, pinned nonce table
  size_t cap_n = 0, cap_bytes = 0;
  hipEvent_t dec_ev = nullptr, run_ev = nullptr;
  uint32_t* eta_h = nullptr;       // pinned: 9-word entries (nonce, neutral flag)
  uint8_t* eidx_h = nullptr;       // pinned: per-header index
  uint16_t* res_bits_h = nullptr;  // pinned: the replay's result downloads (bits, pool index), cap_n each
  int32_t* res_pidx_h = nullptr;
  uint8_t* dec_h = nullptr;        // pinned: the replay's decoded-field downloads (DEC_H_BYTES per header)
};

static constexpr size_t KT_BYTES = 16 * 8 * 4 * 32; // per cached key: 16 tables x 8 cached points
static constexpr size_t WT_BYTES = 22 * 32 * 4 * 32; // per wide key: 22 positions x 32 cached points (WT_STRIDE)
static constexpr uint32_t KC_MAX_ENTRIES = 1u << 20;   // a key used twice already pays for its tables

#define HIPCHK(ctx, x)                                                                    \
  do {                                                                                    \
    if (praos_host_only_(ctx)) return PRAOS_E_STATE;                                      \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      (ctx)->err = std::string(#x) + ": " + hipGetErrorString(e_);                        \
      return PRAOS_E_HIP;                                                                 \
    }                                                                                     \
  } while (0)

static inline unsigned nblocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

template <typename T>
static hipError_t dalloc(praos_batch* b, T** p, size_t bytes) {
  void* q = nullptr;
  size_t sz = bytes ? bytes : 16;
  const size_t k = b->owned.size();
  praos_ctx* c = b->owner;
  hipError_t e = hipSuccess;
  if (c && k < c->spare.size() && c->spare[k] && c->spare_sz[k] >= sz && c->spare_sz[k] <= 2 * sz + 4096) {
    q = c->spare[k];                 // the previous batch's buffer at the same position
    sz = c->spare_sz[k];
    c->spare[k] = nullptr;
  } else {
    e = hipMalloc(&q, sz);
  }
  if (e == hipSuccess) { b->owned.push_back(q); b->owned_sz.push_back(sz); *p = (T*)q; }
  return e;
}

// The pool part of a ledger view (lvPoolDistr): the caller's pools, the map hash28 -> caller
// index (OCert counter slots), and on a device the tables the VRF join and the leader test read
// (hashes sorted, 7 words each | VRF key hashes, 8 | x = -(sigma * c) in Fixed E34, 4 | sorted
// index -> caller index).  praos_set_epoch installs one in the context; the per-epoch replay
// (praos_replay_immutable_views) keeps one per view and swaps its device tables in between batches.
struct rp_view {
  int device = -1;
  uint32_t npools = 0;
  std::vector<praos_pool> pools;
  std::map<std::string, int32_t> by_hash;
  uint32_t *d_hash = nullptr, *d_vrf = nullptr, *d_x = nullptr;
  int32_t* d_map = nullptr;
};

// one device allocation carved into 256-byte aligned parts (praos_txindex / praos_txwit): the
// layout function runs twice, first to measure (base == nullptr) and then over the allocation
struct Carve {
  uint8_t* base = nullptr;
  size_t off = 0;
  template <typename T>
  T* take(size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) & ~(size_t)255;
    return base ? (T*)(base + at) : nullptr;
  }
};

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

template <typename F>
static hipError_t carve_alloc(DevBuf& buf, F&& layout) {
  Carve m;
  layout(m);
  const hipError_t e = hipMalloc(&buf.p, m.off ? m.off : 256);
  if (e != hipSuccess) return e;
  Carve c;
  c.base = (uint8_t*)buf.p;
  layout(c);
  return hipSuccess;
}
// the same over the buffer the context keeps for the candidates calls (rp_scratch: the parts stay
// valid until the next call that carves it); false: no memory
template <typename F>
static bool carve_kept(praos_ctx* c, F&& layout) {
  Carve m;
  layout(m);
  Carve k;
  k.base = rp_scratch(c, m.off);
  if (!k.base) return false;
  layout(k);
  return true;
}

// ---- what the wire calls share (candidates, GenTxs, BlockFetch blocks)
// the items of a call: spans where there are items, bytes where there is a length
static inline bool items_ok(const praos_header_bytes* s) {
  return s && (s->n == 0 || (s->off && s->len)) && (s->bytes_len == 0 || s->bytes);
}
// zeros in the pad behind an arena's bytes (ld64u, arena.hpp), on s: before the bytes go up
static inline hipError_t pad_zero(uint8_t* arena, size_t bytes, hipStream_t s) {
  return hipMemsetAsync(arena + bytes, 0, arena_pad(bytes), s);
}
// the items' offsets and lengths, on s: after the bytes
static inline hipError_t items_upload(const praos_header_bytes& in, uint64_t* d_off, uint32_t* d_len, hipStream_t s) {
  const hipError_t e = hipMemcpyAsync(d_off, in.off, 8 * in.n, hipMemcpyHostToDevice, s);
  return e != hipSuccess ? e : hipMemcpyAsync(d_len, in.len, 4 * in.n, hipMemcpyHostToDevice, s);
}
// the download of an output array the caller may have left NULL
struct Down {
  hipStream_t s;
  hipError_t operator()(void* dst, const void* src, size_t bytes) const {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
  }
};

// The row set: which of n items are the same (tag, 32-byte key), and the row of each distinct one
// in order of first appearance (k_wire.hip's k_hdr_* kernels).  A call lays it out in its Carve,
// then runs reset + set (dedup) or ident, and number.  A copy with other arrays put in numbers
// other classes (BlockFetch: the ones k_bf_class refined) or into other rows (GenTxs' second pass).
struct RowSet {
  size_t n = 0, nb = 0, tab = 0;                 // items, blocks of NT items, the table's slots
  uint32_t *item_slot = nullptr, *item_rep = nullptr, *rep_row = nullptr, *item_row = nullptr, *blk = nullptr,
           *slot_item = nullptr, *slot_min = nullptr;
  void layout(Carve& m, size_t items) {
    n = items;
    nb = (n + NT - 1) / NT;
    for (tab = 2; tab < 2 * n;) tab <<= 1;       // a power of two >= 2n: probing always ends, and
    item_slot = m.take<uint32_t>(4 * n);         // ident's n entries of slot_min fit
    item_rep = m.take<uint32_t>(4 * n);
    rep_row = m.take<uint32_t>(4 * n);
    item_row = m.take<uint32_t>(4 * n);
    blk = m.take<uint32_t>(4 * nb);
    slot_item = m.take<uint32_t>(4 * tab);
    slot_min = m.take<uint32_t>(4 * tab);
  }
  hipError_t reset(hipStream_t s) const {
    const hipError_t e = hipMemsetAsync(slot_item, 0, 4 * tab, s);
    return e != hipSuccess ? e : hipMemsetAsync(slot_min, 0xff, 4 * tab, s);
  }
  // the classes: items with flag 0 and a tag below 32 in tag_mask, by (tag, key)
  void set(hipStream_t s, const uint8_t* flag, const uint8_t* tag, const uint8_t* key, uint32_t tag_mask) const {
    launch_hdr_set(s, n, flag, tag, key, tag_mask, (uint32_t)(tab - 1), slot_item, slot_min, item_slot);
  }
  // ... or every index below *limit (a device word; NULL: n) with flag[i] == flag_ok its own class
  void ident(hipStream_t s, const uint32_t* limit, const uint8_t* flag, uint8_t flag_ok) const {
    launch_hdr_ident(s, n, limit, flag, flag_ok, item_slot, slot_min);
  }
  // item_rep alone: for a caller that refines the classes before it numbers them
  void count(hipStream_t s) const { launch_hdr_count(s, n, item_slot, slot_min, item_rep, blk); }
  // rows in order of first appearance: *total (a device word), rep_row, item_row, and the
  // representatives' spans ioff / ilen compacted into row_off / row_len (n entries)
  void number(hipStream_t s, uint32_t* total, const uint64_t* ioff, const uint32_t* ilen, uint64_t* row_off,
              uint32_t* row_len) const {
    launch_hdr_number(s, n, item_slot, slot_min, item_rep, blk, total, ioff, ilen, (uint32_t)n, row_off, row_len,
                      rep_row, item_row);
  }
};

// The transaction index's device results kept for a pass that follows it (praos_txwit.hip): the
// call's allocations, owned here, and what that pass reads in them.
struct txi_keep {
  void* buf[3] = {nullptr, nullptr, nullptr};
  const uint8_t* kind = nullptr;      // n: k_txindex.hip's kind of each block (3: a Byron main block)
  const uint32_t* tfirst = nullptr;   // n + 1: the final rows' prefix sum (total > 0)
  praos_txi_dev_rows rows{};          // the final rows: block, wit_off, wit_len, tx_id
  size_t total = 0;
  txi_keep() = default;
  txi_keep(const txi_keep&) = delete;
  txi_keep& operator=(const txi_keep&) = delete;
  ~txi_keep() {
    for (void* p : buf)
      if (p) (void)hipFree(p);
  }
};

// The functions that cross the API units' boundaries.
namespace praos_impl {

// praos_txindex.hip: the index over a block batch.  keep != null: rows is ignored, the final rows
// stay on the device (no capacity check, no row download) and the buffers pass to *keep
int txi_run(praos_ctx* c, praos_batch* b, const praos_txi_cfg* cfg, praos_txi_stats* st, praos_txi_rows* rows,
            txi_keep* keep);

// praos_txwit.hip: the witness passes over T device rows (blk_kind[row_block[p]]: k_txindex.hip's
// kind of the row's block; wit span; tx_id [T][32]).  Everything is enqueued on the context's
// stream; the results stay on the device in R, wit_first and the witness count on the host.
struct txw_rows {
  DevBuf buf_t, buf_w;
  uint8_t* st = nullptr;                                  // T: PRAOS_TXW_*
  uint32_t *nv = nullptr, *nb = nullptr, *cnt = nullptr, *txbad = nullptr, *d_wfirst = nullptr;
  uint64_t *v0 = nullptr, *v2 = nullptr;
  uint32_t* tx = nullptr;                                 // W: the witness records
  uint8_t *kind = nullptr, *ok = nullptr, *kh = nullptr;
  uint64_t *koff = nullptr, *soff = nullptr;
  std::vector<uint32_t> wfirst;                           // T + 1
  uint64_t W = 0;
};
int txw_rows_run(praos_ctx* c, const char* who, const uint8_t* arena, uint64_t arena_len, size_t T,
                 const uint8_t* blk_kind, const uint32_t* row_block, const uint64_t* wit_off, const uint32_t* wit_len,
                 const uint8_t* tx_id, uint32_t max_lanes, txw_rows& R);
int txw_rows_down_wits(praos_ctx* c, praos_txw_wits* wits, const txw_rows& R);
// the context's Ed25519 lane tables (txw_tabs) grown to at least `lanes` lanes
int txw_lane_tables(praos_ctx* c, size_t lanes);
// praos_verify_tx_witnesses over a batch of which only n, arena, arena_len, blk_off and blk_len
// are read (praos_blockfetch.hip: the rows of distinct wire blocks as blocks)
int txw_run(praos_ctx* c, praos_batch* b, const praos_txw_cfg* cfg, praos_txw_blocks* bo, praos_txw_txs* txs,
            praos_txw_wits* wits);

// praos_api.hip: the radix-2^16 comb, k_decode_praos over a from-bytes batch, the overlay class
// of a slot
int ensure_bcomb16(praos_ctx* c);
int batch_decode(praos_ctx* c, praos_batch* b);
int32_t overlay_class(const praos_ctx* c, uint64_t slot);
// k_decode_praos of headers [first, upto) into b's columns, from the device spans hoff / hlen into
// arena, on st; the mode and the leader-certificate columns are the batch's
void decode_launch(const praos_batch* b, hipStream_t st, const uint8_t* arena, size_t arena_len, const uint64_t* hoff,
                   const uint32_t* hlen, size_t first, size_t upto);
// device buffers of a from-bytes batch of n headers over an arena of bytes_len bytes
// (owner == nullptr: fresh allocations, not taken from / given back to the spare list)
praos_batch* bytes_batch_alloc(praos_ctx* c, size_t n, size_t bytes_len, bool tpraos, praos_ctx* owner);
// arena upload of a from-bytes batch (zero padding for ld64u, then the bytes), on the ctx stream
int arena_upload(praos_ctx* c, praos_batch* b, const uint8_t* bytes, size_t bytes_len);

// praos_xfer.hip: the pinned staging buffers and the copies through them (h2d / d2h: on the ctx
// stream; d2h_on and d2h return when the bytes are in dst)
bool stage_init(praos_ctx* c);
hipError_t zero_pad(praos_ctx* c, uint8_t* dst, size_t pad, hipStream_t st);
hipError_t h2d_on(praos_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st);
hipError_t d2h_on(praos_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st);
hipError_t h2d(praos_ctx* c, void* dst, const void* src, size_t bytes);
hipError_t d2h(praos_ctx* c, void* dst, const void* src, size_t bytes);
hipError_t h2d_gather(praos_ctx* c, uint8_t* dst, const praos_span* sp, size_t ns, size_t total, hipStream_t st);

// praos_stream.hip: what praos_close frees of the batches and calls the context keeps (the replay's
// batches, the candidates' scratch, the pipeline's batches, events and pinned offsets)
void stream_close(praos_ctx* c);

// The columns a call downloads, each as f(host pointer, device pointer, bytes); a column the caller
// left NULL is skipped, the first error ends the walk.  Outputs of a run:
template <typename F>
static hipError_t out_cols(const praos_out& o, const praos_batch& b, F&& f) {
  const struct { void* h; const void* d; size_t w; } col[] = {
      {o.bits, b.bits, 2}, {o.pool_idx, b.pool_idx, 4}, {o.beta, b.beta, 64}, {o.leader, b.leader, 32},
      {o.nonce, b.nonce, 32}};
  hipError_t e = hipSuccess;
  for (const auto& x : col)
    if (x.h && e == hipSuccess) e = f(x.h, x.d, x.w * b.n);
  return e;
}
// ... and the decoded fields of a from-bytes batch:
template <typename F>
static hipError_t decoded_cols(const praos_decoded& d, const praos_batch& b, F&& f) {
  const struct { void* h; const void* d; size_t w; } col[] = {
      {d.status, b.dec_status, 2},   {d.block_no, b.block_no, 8},     {d.slot, b.slot, 8},
      {d.prev_hash, b.prev_hash, 32}, {d.prev_is_genesis, b.prev_genesis, 1}, {d.cold_vk, b.cold_vk, 32},
      {d.vrf_vk, b.vrf_vk, 32},      {d.vrf_out, b.vrf_out, 64},      {d.vrf_proof, b.vrf_proof, 80},
      {d.body_size, b.body_size, 4}, {d.body_hash, b.body_hash, 32},  {d.hot_vk, b.hot_vk, 32},
      {d.ocert_n, b.ocert_n, 8},     {d.ocert_c0, b.ocert_c0, 8},     {d.ocert_sig, b.ocert_sig, 64},
      {d.prot_major, b.prot_major, 8}, {d.prot_minor, b.prot_minor, 8}, {d.kes_sig, b.kes_sig, 448},
      {d.signed_len, b.body_len, 4}, {d.signed_body, b.body, b.signed_stride}, {d.header_hash, b.header_hash, 32}};
  hipError_t e = hipSuccess;
  for (const auto& x : col)
    if (x.h && e == hipSuccess) e = f(x.h, x.d, x.w * b.n);
  return e;
}

// A batch that a one-shot call borrows as the owner of its device allocations: on scope exit the
// ctx stream is drained and the buffers go to the context's spare list (praos_batch_free).
struct ScratchBatch {
  praos_ctx* c;
  praos_batch* b;
  ScratchBatch(praos_ctx* c_, praos_batch* b_) : c(c_), b(b_) {}          // adopts an uploaded batch
  ScratchBatch(praos_ctx* c_, size_t n) : c(c_), b(new praos_batch()) {
    b->owner = c;
    b->n = n;
  }
  ScratchBatch(const ScratchBatch&) = delete;
  ScratchBatch& operator=(const ScratchBatch&) = delete;
  ~ScratchBatch() {
    (void)hipStreamSynchronize(c->stream);
    praos_batch_free(c, b);
  }
};

// the device's nonce table: 9 words per entry (nonce, neutral flag)
static inline void pack_nonce_table(const praos_nonce* etas, uint32_t k, uint32_t* out36) {
  std::memset(out36, 0, 36 * (size_t)k);
  for (uint32_t e = 0; e < k; e++) {
    if (!etas[e].neutral) std::memcpy(out36 + 9 * e, etas[e].hash, 32);
    out36[9 * e + 8] = etas[e].neutral ? 1u : 0u;
  }
}

// A key cache's lists after kc_lists, as the launchers take them (kargs.hpp): the misses, the hits
// against this run's entry space, and the wide tier's hits against its tables
static inline KeyItems key_misses(const praos_batch::KeyCache& k) { return {k.miss, k.counters + 2}; }
static inline KeyHits key_hits(const praos_batch::KeyCache& k) {
  return {k.hit, k.counters + 1, k.item_entry, k.kt, k.ki};
}
static inline KeyHits key_wide_hits(const praos_batch::KeyCache& k) {
  return {k.wide.hit, k.wide.wcnt + 1, k.item_entry, k.wide.wtab, k.ki};
}

// The KES kernels' arguments of an uploaded batch in header mode (the period from the slot), verdicts
// to bits; and stage V's part of the VRF arguments (batch_run_impl fills in the rest)
static inline KesIn batch_kes_in(const praos_batch* b, uint64_t slots_per_kes_period, uint16_t* bits) {
  KesIn a{};
  a.hot_vk = b->hot_vk;
  a.kes_sig = b->kes_sig;
  a.body_off = b->body_off;
  a.body_len = b->body_len;
  a.body = b->body;
  a.body_bytes_len = b->body_bytes_len;
  a.slot = b->slot;
  a.ocert_c0 = b->ocert_c0;
  a.slots_per_kes_period = slots_per_kes_period;
  a.bits = bits;
  a.tabs = b->tab_kes;
  return a;
}
static inline VrfIn batch_vrf_v_in(const praos_ctx* c, const praos_batch* b) {
  VrfIn a{};
  a.vrf_vk = b->vrf_vk;
  a.vrf_proof = b->vrf_proof;
  a.slot = b->slot;
  a.eta0 = b->eta_tab ? b->eta_tab : c->d_eta0;
  a.eta0_neutral = c->eta0_neutral;
  a.eta_idx = b->eta_idx;
  a.tabs = b->tab_vrf;
  return a;
}

// praos_run.hip: the key-cache prepass (hash set, entries, hit / miss lists), the entries' key
// tables, and the crypto step's stream scheduler
int kc_lists(praos_ctx* c, praos_batch* b, const RunPlan& P, praos_batch::KeyCache& k, size_t n, const uint8_t* keys,
             hipStream_t st, KeyItems items, int which);
void kc_precompute(praos_ctx* c, const RunPlan& P, praos_batch::KeyCache& k, const uint8_t* keys, int kind,
                   hipStream_t st, size_t n);
RunShape run_shape(const praos_ctx* c, size_t n, bool tp_only, bool v_done);   // the context's options + the batch
int batch_run_impl(praos_ctx* c, praos_batch* b);

}  // namespace praos_impl
