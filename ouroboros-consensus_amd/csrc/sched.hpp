#pragma once
// sched.hpp -- the schedule of a batch run as values: the knobs (SchedKnobs) with their environment
// names and size cut-offs, what a run knows before it queues anything (RunShape), and every decision
// the crypto step takes from the two (RunPlan, plan_run).  Plain C++17, no HIP: the host modules
// include it through api_internal.hpp, and tests/test_sched_plan.py compiles it with g++ alone.
// This file is the source of the knob table in DESIGN ("The schedule as a value"): a default, an
// auto rule or a cut-off changes here first.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

// Batches below this many headers (a strong-scaling shard of an epoch over 8 GPUs is 54k) leave
// most wave slots empty and run latency-bound (PRAOS_VRF_PRIO = -1 raises stage V there)
static constexpr size_t SMALL_BATCH = 80000;
// the Praos VRF runs as three kernels (V | U | join) below this many headers and as two stages
// (V | U + join) from it on (PRAOS_VRF3 -1).  Equal to WIDE_BATCH today, but a cut-off of its own
static constexpr size_t VRF3_BATCH = 300000;
static constexpr size_t WIDE_BATCH = 300000;           // the VRF key cache's wide tier: batches from this size on
static constexpr uint32_t WIDE_MIN_USES = 43;          // ... and keys with this many uses: the break-even of
                                                       // W_KEY_VRF_WIDE against W_VRF_F_CK_WIDE (tools/workmodel.py)
// below this many headers the key precomputes run at raised wave priority (PRAOS_KEY_PRIO -1):
// they head the cached chains (profiles/r04/bb: 96k 3.66 -> 3.57 ms, 108k 4.14 -> 3.83, 160k
// 5.19 -> 4.88, 300k 8.83 -> 8.67; 432k within noise)
static constexpr size_t KEY_PRIO_BATCH = 400000;
// below this many headers stage V, the uncached verifies and the key precompute come from their
// ILP-4 builds (k_vrf_v4 / k_miss4 / k_keys4): a step's chains are latency-bound there
// (profiles/r04/y: 96k 4.06 -> 3.64 ms, 108k 4.25 -> 4.10, 112k 4.39 -> 4.15; equal at 120k,
// slower at 128k)
static constexpr size_t ILP4_BATCH = 120000;
// from this many headers on the KES Merkle walk runs once per leaf-key entry (PRAOS_KES_DEDUP -1).
// Medians of alternating runs, ms per step without / with it, beside the other cuts of DESIGN
// section 24: 432k 9.907 -> 9.847 (eight runs each, every run with it below every run without);
// 300k 7.170 -> 7.231 and 160k 4.058 -> 4.117 (four each): slower, the step there is not bound
// by the instruction count; the KES-only configs[3] 9.355 -> 9.413, inside its spread
// (profiles/r08_perkey_ab.json)
static constexpr size_t KES_DEDUP_BATCH = 400000;
// Byron header batches (praos_verify_pbft_headers) below this many headers verify uncached: the
// delegate keys' precompute chain (250 doublings, then the table pass) is pure latency there.
// Measured on an MI355X (tools/pbft_bench.py: 7 delegates in turn, a freshly opened context per
// variant and pass, medians of 9 runs, cached / uncached ms end to end): 16,384 2.07 / 1.83,
// 32,768 2.38 / 2.16, 65,536 3.16 / 2.73, 98,304 4.17 / 3.95, 131,072 4.98 / 4.67, 163,840 6.03 /
// 6.04, 216,000 7.51 / 7.94: the medians cross at about 163,840.  With 7 keys the cache's insert
// and partition passes serialise on 7 hash slots (0.66 + 0.62 ms at 216,000, kernel trace), which
// is what moves the crossing this far out.
static constexpr size_t PBFT_CK_MIN = 163840;
// below this many headers the KES leaf keys are not cached (every KES check uncached, from the
// ILP-4 build, beside stage V): a 54k-header shard's stage V and uncached KES waves fit in one
// round of wave slots (2 per SIMD), and the leaf-key chain -- lists, precompute, tables, k_kes_ck,
// the step's longest after stage V + join -- is gone (54k 2.44-2.49 -> 2.29-2.37 ms; at 64k the
// waves no longer fit and it is slower, 2.53 -> 3.05; 80k 2.97 -> 3.47; 108k 3.41 -> 4.59;
// profiles/r06/i_kes_nocache).  PRAOS_OPT_KES_NOCACHE / PRAOS_KES_NOCACHE=<headers> override it
// (0: always cached).
static constexpr size_t KES_NOCACHE_BATCH = 58000;
// below this many headers (the 1/8-epoch shard of a 432k epoch is 54k) stage V's join runs on the
// main stream after it waits for U itself (PRAOS_V_MAIN 2) and the uncached verifies keep normal
// wave priority
static constexpr size_t SHARD_SMALL = 60000;
// k_kes_ck takes two headers per lane from this many hits on when the KES pass runs alone
// (PRAOS_KES_PAIR -1)
static constexpr uint32_t KES_PAIR_ALONE = 196608;
static constexpr int VRF_WIDE_CAP = 4096, VRF_WIDE_CAP_MAX = 1 << 16;   // wide keys per batch: default, most

struct SchedKnobs {
  int tp_staged = 1;                                  // TPraos VRF through the staged kernels + VRF key cache
                                                       // (PRAOS_TP_STAGED=0: the one-kernel k_vrf_tp)
  int vrf_prio = 0;                                   // stage V and join waves at s_setprio 3 (PRAOS_VRF_PRIO 1 / 0;
                                                       // -1: batches below SMALL_BATCH headers).  Off: with the
                                                       // uncached verifies raised instead a 54k-header step takes
                                                       // 2.83 ms against 3.16 (profiles/r04/i, r04/j)
  int vrf_ilp4 = (int)ILP4_BATCH;                    // stage V from the ILP-4 build (k_vrf_v4.hip): PRAOS_VRF_ILP4
                                                       // 1 always, 0 never, N > 1: batches below N headers
                                                       // (profiles/r04/b: V alone 1.71 -> 1.51 ms at 54k; alone
                                                       // at 108k the step was slower, 4.25 -> 4.37, but with the
                                                       // ILP-4 uncached verifies and precompute beside it faster,
                                                       // profiles/r04/y)
  int v_excl = 0;                                      // the ILP-4 stage V holding its SIMDs alone (k_vrf_v4x):
                                                       // PRAOS_V_EXCL (54k: 3.30 -> 3.46 ms, off)
  int miss4 = -1;                                      // uncached OCert / KES verifies from the ILP-4 build
                                                       // (k_miss4.hip): PRAOS_MISS4 1 / 0, -1 below ILP4_BATCH
                                                       // (54k: 3.33 -> 3.09 ms; 108k: 4.26 -> 4.66, so not there)
  int miss_prio = -1;                                  // ... at s_setprio 3: PRAOS_MISS_PRIO 1 / 0, -1 with miss4
                                                       // from SHARD_SMALL headers on (below it, beside the GCD
                                                       // inversion's shorter join, normal priority with
                                                       // v_main 1 was faster: profiles/r06/s_retune)
  long kes_pair = -1;                                  // k_kes_ck two headers per lane from this many hits on
                                                       // (PRAOS_KES_PAIR, 0 = never; -1: from 196,608 when the
                                                       // KES pass runs alone -- beside the OCert / VRF passes
                                                       // the paired kernel has 4 % fewer VALU instructions
                                                       // (0.983 G -> 0.941 G per 432k step) and the step is
                                                       // longer, 9.847 -> 10.113 ms, medians of eight
                                                       // alternating runs, profiles/r08_perkey_ab.json; its
                                                       // waves are twice as long and spill 176 bytes per lane)
  int kes_dedup = -1;                                  // KES Merkle path dedup per leaf-key entry (PRAOS_KES_DEDUP
                                                       // 1 / 0): the representatives walk once, a wave of
                                                       // k_kes_ck whose paths all equal theirs skips the walk;
                                                       // -1: from KES_DEDUP_BATCH headers on
  int vrf_perkey = 1;                                  // pool record per VRF key-cache entry (k_vrf_keyrec): a
                                                       // wave of the cached stage F / the join whose cold keys
                                                       // all equal their records' skips the two Blake2b and the
                                                       // pool search (PRAOS_VRF_PERKEY 1 / 0)
  int v_main = -1;                                     // stage V on the main stream (PRAOS_V_MAIN; 0 off): no
                                                       // cross-stream wait between the previous run's end and V;
                                                       // the join after U and V on the VRF stream (3), or on the
                                                       // main stream after a wait for U (1; 2: U's two streams
                                                       // waited for separately).  54k headers (C5 1/8 shard):
                                                       // 2.354-2.380 ms off, 2.284-2.330 (1), 2.315-2.332 (2),
                                                       // 2.267-2.297 (3); 108k: 3.418-3.443 off, 3.36-3.42 on
                                                       // (profiles/r06/k_vmain); -1: 2 below ILP4_BATCH
                                                       // headers, 3 from it (with the GCD inversion, mode 1 +
                                                       // normal-priority misses below SHARD_SMALL: 54k
                                                       // 2.18-2.22 -> 2.17-2.19 ms, 40k 2.19-2.21 -> 2.08; then
                                                       // mode 2 over mode 1 at 54k 2.16-2.19 -> 2.15, 40k equal
                                                       // or 2 % faster; over mode 3 at 80k 2.78-2.80 -> 2.76,
                                                       // 108k 3.24-3.26 -> 3.21-3.22, 216k 5.63-5.70 -> 5.70-5.71;
                                                       // profiles/r06/s_retune)
  int pre_join = -1;                                   // the join's pool part (lookup, key hash, leader / nonce
                                                       // values) as k_vrf_pool on the VRF miss stream before the
                                                       // uncached U, off the chain after stage V (PRAOS_PRE_JOIN
                                                       // 1 / 0, -1 below SMALL_BATCH)
  // PRAOS_VRF_KEYS_FIRST: the three-kernel Praos VRF's key lists, uncached U and key precompute +
  // cached U queued ahead of the OCert and KES passes when the streams run concurrently: after
  // stage V, the VRF key chain -- lists, precompute, tables, U, join -- is a small batch's longest
  // (profiles/r04/i: its lists started 0.33 ms into a 54k-header step, behind the OCert and KES
  // lists).  54k: 2.80 -> 2.85 ms, 108k 4.24 -> 4.27: off, profiles/r04/k
  int vrf_keys_first = 0;
  int key4 = -1;                                       // key precompute from the ILP-4 build (k_keys4.hip):
                                                       // PRAOS_KEY4 1 / 0, -1 below ILP4_BATCH (54k: 2.78-2.84
                                                       // -> 2.76-2.77 ms; 108k 4.17 -> 4.21, profiles/r04/n)
  // (round 5 also measured a key precompute with four lanes per key, DPP quad broadcasts: inside a
  // step its chains were about as long as the ILP-4 build's and its four lanes per key took issue
  // slots from the rest, 54k 2.72-2.75 -> 2.84-2.88 ms, 108k 3.79-3.84 -> 4.00,
  // profiles/r05/c11_keyq_nobranch; removed in round 6)
  int u4 = -1;                                         // cached stage U from the ILP-4 build (PRAOS_U4 1 / 0,
                                                       // -1 below ILP4_BATCH; 54k 2.79 -> 2.75 ms, 108k 3.87-3.92
                                                       // -> 3.81-3.83, profiles/r04/hh)
  int ck4 = 0;                                         // cached OCert / KES verifies from the ILP-4 build
                                                       // (PRAOS_CK4 1 / 0, -1 below ILP4_BATCH)
  int vrf3 = -1;                                       // VRF as V | U | join (1), V | U + join (0), -1 auto:
                                                       // the three-kernel form below VRF3_BATCH headers (latency)
  // wide tier of the VRF key cache (praos_set_vrf_wide / PRAOS_VRF_WIDE): a key with this many uses
  // in the batch gets positional tables (k_keys.hip); 0 off; -1 auto: WIDE_MIN_USES, the modelled
  // break-even, in batches from WIDE_BATCH headers on (below it the longer key precompute is on the
  // step's critical path and few keys reach the threshold)
  int vrf_wide = -1;
  // (with a wide tier the tables' chain -- decode, chunk bases, position bases, tables -- is longer
  // than stage V leaves room for in a large batch, and the U chains wait for it: raised wave
  // priority, as in a small batch; 432k 10.24 -> 10.09 ms, profiles/r07_wide_ab.json)
  int wide_prio = 1;                                   // the VRF key precompute at raised wave priority when it
                                                       // builds wide tables (PRAOS_WIDE_PRIO 1 / 0)
  int vrf_wide_cap = VRF_WIDE_CAP;                     // wide keys per batch at most (PRAOS_VRF_WIDE_CAP)
  int stream_chunk_v = 1;                              // submitted calls: stage V per landed chunk (1) or in the
                                                       // run over the whole batch (0); PRAOS_STREAM_CHUNK_V.  C5,
                                                       // 432k headers, three calls in flight: 13.2-13.4 ms per
                                                       // call (1) against 15.3-17.6 (0), profiles/r06/l_stream
  size_t pbft_ck_min = PBFT_CK_MIN;                    // PRAOS_PBFT_CK_MIN (see PBFT_CK_MIN)
  size_t kes_nocache = KES_NOCACHE_BATCH;              // PRAOS_KES_NOCACHE (see KES_NOCACHE_BATCH)
  int kc_min[3] = {0, 0, 0};                           // per cache (cold, VRF, KES leaf) min uses overriding
                                                       // keycache when > 0 (PRAOS_KC_MIN="c,v,k")
  // (round 5 measured the cached chains' last kernels -- cached U, the join, the cached OCert /
  // KES verifies -- at s_setprio 2 / 3 below ILP4_BATCH: U shortened (54k 0.71 -> 0.43 ms) but
  // stage V stretched past it and the step with it, 54k 2.74-2.76 -> 2.89-2.95 ms,
  // profiles/r05/c14_ckprio; the option was removed in round 6)
  int key_wave_prio = -1;                              // key precompute waves at s_setprio 3 (PRAOS_KEY_PRIO 1 / 0;
                                                       // -1: batches below KEY_PRIO_BATCH headers)
  // (round 6 measured key hints for the stored-bytes pipeline -- each header's cold, VRF and KES
  // leaf keys read on the host while the chunks upload, the key stores filled from them on the
  // side streams before the last chunk lands -- bit-exact and slower, 432k e2e 15.7 -> 18.4 ms:
  // the fill shares the GPU with the chunks' stage V and the tail stays throughput-bound;
  // profiles/r06/h_e2e_hints.  Removed.)
  // (round 5 measured a per-chunk key prefill in the stored-bytes pipeline -- the landed chunks'
  // cold, KES leaf and VRF keys stored and their tables built while later chunks upload -- in two
  // forms, both slower: the GPU is busy with the chunks' stage V during the upload, so the
  // prefill only moves work there, and a key first seen in the last chunk still needs a
  // latency-bound chain after it lands (432k, 8 chunks: 16.3-16.4 -> 18.2-18.5 ms,
  // profiles/r05/c12_prefill_v3; 16.9 -> 19.2 ms, c7_e2e_timeline_pf{0,1}.txt).  Removed in round 6.)
  // stored-bytes pipeline: the first chunk's size in percent of the others' (PRAOS_PIPE_HEAD):
  // nothing runs on the GPU until it has landed and been decoded
  int pipe_head = 25;                                  // (432k headers, 8 chunks: 100 -> 16.9-17.0 ms,
                                                       // 50 -> 16.5, 25 -> 16.3-16.4, 12 -> 16.2-16.4)
  // (round 6 measured the KES checks queued while later chunks upload, in two forms, both slower:
  // uncached per landed chunk, 432k e2e 15.5-16.0 -> 18.2-18.9 ms; with the leaf-key cache over 1,
  // 2 or 4 groups of landed chunks, 15.8 / 17.0 / 18.2-18.7 ms: the GPU runs the chunks' stage V
  // during the upload, so the KES work there only stretches V; profiles/r06/g_e2e_kes.  Removed.)
  int pipe_tail = 100;                                 // ... and the last chunk's (PRAOS_PIPE_TAIL): the run after it
                                                       // waits for its decode, but a smaller one leaves more of the
                                                       // batch's stage V after the upload (432k, 8 chunks: 100 ->
                                                       // 16.4-16.7 ms, 50 -> 17.1-17.3, 25 -> 18.5-18.8;
                                                       // profiles/r05/c16_pipe_tail)
};

// praos_set_vrf_wide's clamps (PRAOS_VRF_WIDE / PRAOS_VRF_WIDE_CAP take one argument each)
static inline int sched_clamp_vrf_wide(int min_uses) { return min_uses < 0 ? -1 : min_uses; }
static inline int sched_clamp_vrf_wide_cap(int max_keys) {
  return max_keys < 1 ? VRF_WIDE_CAP : std::min(max_keys, VRF_WIDE_CAP_MAX);
}

// How an environment variable's text becomes its knob
enum SchedEnvKind {
  ENV_INT,        // atoi
  ENV_BOOL,       // atoi != 0 (PRAOS_VRF3=2 is 1: the variable cannot ask for auto)
  ENV_LONG,       // atol
  ENV_SIZE,       // atoll, a number of headers
  ENV_PERCENT,    // atoi clamped to 5 .. 100
  ENV_INT3,       // "%d,%d,%d"; fields the text leaves out keep their values
  ENV_WIDE,       // atoi through sched_clamp_vrf_wide
  ENV_WIDE_CAP    // atoi through sched_clamp_vrf_wide_cap
};
struct SchedEnv {
  const char* name;
  SchedEnvKind kind;
  size_t field;   // offsetof(SchedKnobs, ...)
};
#define SCHED_ENV(name, kind, f) {name, kind, offsetof(SchedKnobs, f)}
static const SchedEnv SCHED_ENV_TABLE[] = {
    SCHED_ENV("PRAOS_KEY_PRIO", ENV_INT, key_wave_prio),
    SCHED_ENV("PRAOS_VRF3", ENV_BOOL, vrf3),
    SCHED_ENV("PRAOS_VRF_PRIO", ENV_INT, vrf_prio),
    SCHED_ENV("PRAOS_VRF_ILP4", ENV_INT, vrf_ilp4),
    SCHED_ENV("PRAOS_V_EXCL", ENV_INT, v_excl),
    SCHED_ENV("PRAOS_MISS4", ENV_INT, miss4),
    SCHED_ENV("PRAOS_KEY4", ENV_INT, key4),
    SCHED_ENV("PRAOS_U4", ENV_INT, u4),
    SCHED_ENV("PRAOS_CK4", ENV_INT, ck4),
    SCHED_ENV("PRAOS_KES_DEDUP", ENV_INT, kes_dedup),
    SCHED_ENV("PRAOS_VRF_PERKEY", ENV_INT, vrf_perkey),
    SCHED_ENV("PRAOS_VRF_KEYS_FIRST", ENV_INT, vrf_keys_first),
    SCHED_ENV("PRAOS_VRF_WIDE", ENV_WIDE, vrf_wide),
    SCHED_ENV("PRAOS_WIDE_PRIO", ENV_INT, wide_prio),
    SCHED_ENV("PRAOS_VRF_WIDE_CAP", ENV_WIDE_CAP, vrf_wide_cap),
    SCHED_ENV("PRAOS_PRE_JOIN", ENV_INT, pre_join),
    SCHED_ENV("PRAOS_V_MAIN", ENV_INT, v_main),
    SCHED_ENV("PRAOS_STREAM_CHUNK_V", ENV_INT, stream_chunk_v),
    SCHED_ENV("PRAOS_KES_NOCACHE", ENV_SIZE, kes_nocache),
    SCHED_ENV("PRAOS_PBFT_CK_MIN", ENV_SIZE, pbft_ck_min),
    SCHED_ENV("PRAOS_MISS_PRIO", ENV_INT, miss_prio),
    SCHED_ENV("PRAOS_KES_PAIR", ENV_LONG, kes_pair),
    SCHED_ENV("PRAOS_KC_MIN", ENV_INT3, kc_min),
    SCHED_ENV("PRAOS_TP_STAGED", ENV_BOOL, tp_staged),
    SCHED_ENV("PRAOS_PIPE_HEAD", ENV_PERCENT, pipe_head),
    SCHED_ENV("PRAOS_PIPE_TAIL", ENV_PERCENT, pipe_tail),
};
#undef SCHED_ENV

// every variable of the table that is set overrides its knob (read once, when a context opens)
static inline void sched_knobs_from_env(SchedKnobs& k) {
  for (const SchedEnv& v : SCHED_ENV_TABLE) {
    const char* e = std::getenv(v.name);
    if (!e) continue;
    void* f = (char*)&k + v.field;
    switch (v.kind) {
      case ENV_INT: *(int*)f = std::atoi(e); break;
      case ENV_BOOL: *(int*)f = std::atoi(e) != 0; break;
      case ENV_LONG: *(long*)f = std::atol(e); break;
      case ENV_SIZE: *(size_t*)f = (size_t)std::atoll(e); break;
      case ENV_PERCENT: *(int*)f = std::max(5, std::min(100, std::atoi(e))); break;
      case ENV_INT3: (void)std::sscanf(e, "%d,%d,%d", (int*)f, (int*)f + 1, (int*)f + 2); break;
      case ENV_WIDE: *(int*)f = sched_clamp_vrf_wide(std::atoi(e)); break;
      case ENV_WIDE_CAP: *(int*)f = sched_clamp_vrf_wide_cap(std::atoi(e)); break;
    }
  }
}

// What a run knows before it queues anything: the batch and the caller's options
struct RunShape {
  size_t n = 0;
  int concurrent = 1;      // PRAOS_OPT_CONCURRENT
  int kernels = 7;         // PRAOS_OPT_KERNELS
  int keycache = 2;        // PRAOS_OPT_KEYCACHE
  int dedup = 1;           // PRAOS_OPT_DEDUP
  bool tp_only = false;    // a TPraos batch
  bool v_done = false;     // stage V already queued chunk by chunk (stored-bytes pipeline)
  int pool_keys = -1;      // PRAOS_OPT_POOL_KEYS
  bool replaying = false;  // inside praos_replay_immutable*
};

// Every decision of a run's schedule (batch_run_impl, kc_lists, kc_precompute read nothing else)
struct RunPlan {
  bool kc = false;              // the key caches are on
  bool dedup = false;           // the OCert pass runs over the distinct OCert tuples
  bool pk_on = false;           // the cold and VRF key caches run on the pool-key store, if it can be allocated
  bool do_ocert = false, do_kes = false, do_vrf = false;   // PRAOS_OPT_KERNELS bits 1, 2, 4
  bool tp_staged = false;       // TPraos VRF: the staged kernels (else the one-kernel k_vrf_tp)
  bool vrf3 = false;            // Praos VRF: V | U | join (else V | U + join)
  // the three-kernel Praos VRF with stage V and the join on the main stream (the step's critical
  // path then crosses streams once, U -> join, instead of at ev[0] -> V, V -> join and join ->
  // leader); vm_mode: see SchedKnobs::v_main
  int vm_mode = 0;
  bool v_main = false;
  bool v_first = false;         // stage V queued ahead of the key passes
  int wprio_v = 0;              // stage V and join waves at raised priority
  bool pre_join = false;        // k_vrf_pool ahead of the uncached U
  bool vrf_keys_first = false;  // the VRF key chain ahead of the OCert and KES passes
  int v_ilp4 = 0;               // stage V: 0 plain, 1 the ILP-4 build, 2 the same holding its SIMDs alone
  bool ck4 = false, miss4 = false, u4 = false, key4 = false;   // the ILP-4 builds of the other kernels
  int miss_prio = 0;            // the ILP-4 uncached verifies at raised priority
  bool kes_dd = false;          // KES Merkle path dedup
  uint32_t kes_pair_min = 0;    // k_kes_ck two headers per lane from this many hits on (0: never)
  bool kes_ck4 = false;         // the cached KES verifies from the ILP-4 build
  // min uses of a key for an entry in cache t (cold, VRF, KES leaf): in the batch's own entry space,
  // and on the pool-key store (every new key is cached: it recurs in the runs that follow).  Whether
  // the store could be allocated is a runtime fact: kc_lists picks
  int min_uses[3] = {0, 0, 0};
  int min_uses_store[3] = {0, 0, 0};
  uint32_t wide_min = 0;        // the wide tier's min uses (VRF cache, off the store only); 0: off
  int vrf_wide_cap = VRF_WIDE_CAP;
  int key_prio = 0;             // key precompute at raised wave priority: without a wide tier (cold, KES
  int key_prio_wide = 0;        // leaf, VRF) and when it builds wide tables (VRF)
  int vrf_perkey = 0;           // pool records of the VRF cache's entries (if the batch has their buffer)
};

// stage V's build for a batch of n headers (the stored-bytes pipeline queues stage V itself)
static inline int sched_v_ilp4(const SchedKnobs& k, size_t n) {
  const bool on = k.vrf_ilp4 == 1 || (k.vrf_ilp4 > 1 && n < (size_t)k.vrf_ilp4);
  return on ? (k.v_excl ? 2 : 1) : 0;
}

static inline RunPlan plan_run(const SchedKnobs& k, const RunShape& s) {
  const size_t n = s.n;
  const auto below = [n](int knob, size_t cut) { return knob > 0 || (knob < 0 && n < cut); };
  RunPlan p;
  p.kc = s.keycache > 0 && n >= 2;
  p.dedup = s.dedup && n >= 2;
  p.pk_on = s.keycache > 0 && (s.pool_keys > 0 || (s.pool_keys < 0 && s.replaying));
  p.do_ocert = (s.kernels & 1) != 0;
  p.do_kes = (s.kernels & 2) != 0;
  p.do_vrf = (s.kernels & 4) != 0;
  p.tp_staged = p.do_vrf && s.tp_only && k.tp_staged;
  p.vrf3 = p.do_vrf && !s.tp_only && below(k.vrf3, VRF3_BATCH);
  p.vm_mode = k.v_main >= 0 ? k.v_main : (n < ILP4_BATCH ? 2 : 3);
  p.v_main = p.vm_mode > 0 && s.concurrent && p.do_vrf && !s.tp_only && !s.v_done && p.vrf3;
  p.v_first = s.concurrent && p.do_vrf && (p.tp_staged || (!s.tp_only && !s.v_done));
  p.wprio_v = below(k.vrf_prio, SMALL_BATCH);
  p.pre_join = p.vrf3 && p.kc && below(k.pre_join, SMALL_BATCH);
  p.vrf_keys_first = p.vrf3 && p.kc && s.concurrent && k.vrf_keys_first;
  p.v_ilp4 = sched_v_ilp4(k, n);
  p.ck4 = below(k.ck4, ILP4_BATCH);
  p.miss4 = below(k.miss4, ILP4_BATCH);
  p.u4 = below(k.u4, ILP4_BATCH);
  p.key4 = below(k.key4, ILP4_BATCH);
  p.miss_prio = k.miss_prio >= 0 ? k.miss_prio : (n < SHARD_SMALL ? 0 : 1);
  p.kes_dd = k.kes_dedup > 0 || (k.kes_dedup < 0 && n >= KES_DEDUP_BATCH);
  p.kes_pair_min = k.kes_pair >= 0 ? (uint32_t)k.kes_pair : ((s.kernels & 5) ? 0u : KES_PAIR_ALONE);
  p.kes_ck4 = p.ck4 && !p.kes_pair_min && !p.kes_dd;
  for (int t = 0; t < 3; t++) {
    p.min_uses[t] = k.kc_min[t] > 0 ? k.kc_min[t] : s.keycache;
    // small batches: no KES leaf key is cached (every item a miss, KES_NOCACHE_BATCH)
    if (t == 2 && k.kc_min[2] <= 0 && n < k.kes_nocache) p.min_uses[t] = INT32_MAX;
    p.min_uses_store[t] = t < 2 ? 1 : p.min_uses[t];
  }
  p.wide_min = k.vrf_wide > 0 ? (uint32_t)k.vrf_wide : (k.vrf_wide < 0 && n >= WIDE_BATCH ? WIDE_MIN_USES : 0u);
  p.vrf_wide_cap = k.vrf_wide_cap;
  p.key_prio = k.key_wave_prio > 0 || (k.key_wave_prio < 0 && n < KEY_PRIO_BATCH);
  p.key_prio_wide = k.key_wave_prio > 0 || (k.key_wave_prio < 0 && (n < KEY_PRIO_BATCH || k.wide_prio));
  p.vrf_perkey = k.vrf_perkey;
  return p;
}
