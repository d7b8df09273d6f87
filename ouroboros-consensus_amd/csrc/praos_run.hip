// praos_run.hip -- the crypto step of a batch (praos_batch_run): the key-cache passes and the
// scheduler that spreads the OCert, KES and VRF chains over the context's streams.
// Every decision of the schedule is taken once, by plan_run (sched.hpp); the passes read the plan.
#include "api_internal.hpp"

using namespace praos_impl;

extern "C" {

int praos_batch_run(praos_ctx* c, praos_batch* b) {
  if (!c || !b) return PRAOS_E_ARG;
  if (!c->have_epoch) return PRAOS_E_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  if (b->n == 0) return PRAOS_OK;
  const int r = batch_run_impl(c, b);
  if (r != PRAOS_OK && c->concurrent) {
    // work already queued on the side streams must be ordered before anything the ctx
    // stream runs next (praos_batch_free hands this batch's buffers to the next upload)
    for (int k = 0; k < 3; k++) {
      if (hipEventRecord(c->side_ev[k], c->side[k]) != hipSuccess ||
          hipStreamWaitEvent(c->stream, c->side_ev[k], 0) != hipSuccess)
        (void)hipStreamSynchronize(c->side[k]);
      if (hipEventRecord(c->mdone_ev[k], c->mside[k]) != hipSuccess ||
          hipStreamWaitEvent(c->stream, c->mdone_ev[k], 0) != hipSuccess)
        (void)hipStreamSynchronize(c->mside[k]);
    }
    if (hipEventRecord(c->v_ev, c->vstream) != hipSuccess || hipStreamWaitEvent(c->stream, c->v_ev, 0) != hipSuccess)
      (void)hipStreamSynchronize(c->vstream);
    if (hipEventRecord(c->v2_ev, c->vstream2) != hipSuccess || hipStreamWaitEvent(c->stream, c->v2_ev, 0) != hipSuccess)
      (void)hipStreamSynchronize(c->vstream2);
  }
  return r;
}

}  // extern "C"

namespace praos_impl {

// key cache prepass over items [0, n) (or list[0 .. *count)): hash set, entries, hit/miss lists
// the pool-key store t (cold 0, VRF 1): 32,768 slots, 16,384 entries.  Allocated on first use
// and initialised on st, the stream every later use of store t is ordered after (the cache's
// own stream; the context's other streams join it at the end of a run): no device-wide sync.
static bool ensure_pks(praos_ctx* c, int t, hipStream_t st) {
  praos_ctx::PoolKeyStore& s = c->pks[t];
  if (s.ktab) return true;
  praos_ctx::PoolKeyStore z;
  z.slots = 1u << 15;
  z.cap = 1u << 14;
  bool ok = hipMalloc(&z.pkey, 32 * (size_t)z.slots) == hipSuccess;
  ok = ok && hipMalloc(&z.pentry, 4 * (size_t)z.slots) == hipSuccess;
  ok = ok && hipMalloc(&z.count, 8) == hipSuccess;
  ok = ok && hipMalloc(&z.base, 8) == hipSuccess;
  ok = ok && hipMalloc(&z.entry_rep, 4 * (size_t)z.cap) == hipSuccess;
  ok = ok && hipMalloc(&z.entry_pos, 4 * (size_t)z.cap) == hipSuccess;
  ok = ok && hipMalloc(&z.kinfo, 36 * (size_t)z.cap) == hipSuccess;
  ok = ok && hipMalloc(&z.ktab, KT_BYTES * (size_t)z.cap) == hipSuccess;
  ok = ok && hipMalloc(&z.scnt, 4 * (size_t)z.cap) == hipSuccess;
  ok = ok && hipMalloc(&z.spos, 4 * (size_t)z.cap) == hipSuccess;
  ok = ok && hipMemsetAsync(z.pentry, 0xff, 4 * (size_t)z.slots, st) == hipSuccess;
  ok = ok && hipMemsetAsync(z.count, 0, 8, st) == hipSuccess;
  ok = ok && hipMemsetAsync(z.base, 0, 8, st) == hipSuccess;
  if (!ok) {
    (void)hipStreamSynchronize(st);              // (the memsets queued so far) before the frees
    for (void* q : {(void*)z.pkey, (void*)z.count, (void*)z.base, (void*)z.entry_rep, (void*)z.entry_pos,
                    (void*)z.kinfo, (void*)z.pentry, (void*)z.ktab, (void*)z.scnt, (void*)z.spos})
      (void)hipFree(q);
    return false;
  }
  s = z;
  return true;
}

int kc_lists(praos_ctx* c, praos_batch* b, const RunPlan& P, praos_batch::KeyCache& k, size_t n, const uint8_t* keys,
             hipStream_t st, KeyItems items, int which) {
  int min_uses = P.min_uses[which];
  k.kt = k.ktab; k.ki = k.kinfo; k.erep = k.entry_rep; k.epos = k.entry_pos; k.emax = k.max_entries;
  k.ebase = nullptr; k.store = -1;
  HIPCHK(c, hipMemsetAsync(k.slot_rep, 0, 4 * (size_t)k.cap, st));
  HIPCHK(c, hipMemsetAsync(k.slot_cnt, 0, 4 * (size_t)k.cap, st));
  HIPCHK(c, hipMemsetAsync(k.counters, 0, 16, st));
  praos_ctx::PoolKeyStore* ps = nullptr;
  if (P.pk_on && which < 2 && ensure_pks(c, which, st)) {
    // pool keys: entries continue the store's, every new key is cached (it recurs in the runs
    // that follow); a store more than 3/4 full (decided on the device, from the count the last
    // run left: no host read of a count still in flight) or one asked to be emptied is emptied
    ps = &c->pks[which];
    launch_pkey_reset(st, ps->count, ps->pentry, ps->slots, ps->cap / 4 * 3, c->pk_reset[which] ? 1 : 0);
    c->pk_reset[which] = false;
    HIPCHK(c, hipMemsetAsync(ps->scnt, 0, 4 * (size_t)ps->cap, st));
    HIPCHK(c, hipMemcpyAsync(k.counters, ps->count, 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(ps->base, ps->count, 4, hipMemcpyDeviceToDevice, st));
    k.kt = ps->ktab; k.ki = ps->kinfo; k.erep = ps->entry_rep; k.epos = ps->entry_pos; k.emax = ps->cap;
    k.ebase = ps->base; k.store = which;
    min_uses = P.min_uses_store[which];
  }
  // wide tier: VRF keys of this batch's own cache (the pool-key store's entries stay in the chunk tier)
  k.wide.min_uses = 0;
  if (which == 1 && !ps && P.wide_min > 0) {
    const uint32_t wmin = std::max(P.wide_min, (uint32_t)std::max(min_uses, 1));
    const uint32_t need = (uint32_t)std::min<size_t>((size_t)std::max(P.vrf_wide_cap, 1), n / wmin + 1);
    // allocated by the first run that uses the tier, for the batch's capacity, and kept; a later run
    // that needs more keys allocates a larger set (the smaller one stays owned until the batch is freed)
    if (k.wide_alloc < need) {
      const size_t cap_n = std::max(n, b->cap_n);
      const uint32_t wcap = (uint32_t)std::min<size_t>((size_t)std::max(P.vrf_wide_cap, 1), cap_n / wmin + 1);
      KeyWide w;
      if (dalloc(b, &w.entry_wide, 4 * (size_t)k.max_entries) != hipSuccess ||
          dalloc(b, &w.wide_ent, 4 * (size_t)wcap) != hipSuccess || dalloc(b, &w.wcnt, 16) != hipSuccess ||
          dalloc(b, &w.hit, 4 * cap_n) != hipSuccess ||
          dalloc(b, (uint8_t**)&w.wtab, WT_BYTES * (size_t)wcap) != hipSuccess ||
          dalloc(b, (uint8_t**)&w.wbase, WT_BYTES / 32 * (size_t)wcap) != hipSuccess)
        return PRAOS_E_OOM;
      k.wide = w;
      k.wide_alloc = wcap;
    }
    k.wide.min_uses = wmin;
    k.wide.cap = need;
    HIPCHK(c, hipMemsetAsync(k.wide.wcnt, 0, 16, st));
  }
  launch_key_insert(st, n, items, keys, k.cap - 1, k.slot_rep, k.slot_cnt, k.item_slot, ps ? ps->pentry : nullptr,
                    ps ? ps->pkey : nullptr, ps ? ps->slots - 1 : 0u, ps ? ps->scnt : nullptr);
  launch_key_assign(st, k.cap, k.slot_rep, k.slot_cnt, (uint32_t)min_uses, k.emax, k.slot_entry, k.erep, k.epos,
                    k.counters, k.wide);
  if (ps) launch_key_store_ranges(st, ps->cap, ps->scnt, ps->spos, k.counters);
  launch_key_partition(st, n, items, k.item_slot, k.slot_entry, k.item_entry, k.epos, k.hit, k.miss, k.counters,
                       ps ? ps->spos : nullptr, k.wide);
  return PRAOS_OK;
}
void kc_precompute(praos_ctx* c, const RunPlan& P, praos_batch::KeyCache& k, const uint8_t* keys, int kind,
                   hipStream_t st, size_t n) {
  const int prio = k.wide.min_uses != 0 ? P.key_prio_wide : P.key_prio;
  const int mode = P.key4 ? 1 : 0;                                 // 1: the ILP-4 build (k_keys4.hip)
  if (k.store < 0) {
    launch_key_precompute(kind, st, k.counters, k.max_entries, k.entry_rep, keys, k.ktab, k.kinfo, prio, nullptr,
                          k.max_entries, mode, k.wide);
    return;
  }
  praos_ctx::PoolKeyStore& ps = c->pks[k.store];
  const uint32_t span = (uint32_t)std::min<size_t>(n, ps.cap);   // new entries of this run, at most
  launch_key_precompute(kind, st, k.counters, ps.cap, ps.entry_rep, keys, ps.ktab, ps.kinfo, prio, ps.base, span,
                        mode);
  launch_pkey_publish(st, k.counters, ps.base, ps.cap, ps.entry_rep, keys, ps.pentry, ps.pkey, ps.slots - 1, ps.count,
                      span);
}

// One run of the crypto step: the plan, the streams it resolves to (a serial run: the context's
// stream for every one of them) and what the passes below hand each other.
// The three crypto chains are independent; run concurrently they fill each other's tail waves (one
// launch of 432k headers is ~3.3 rounds of resident waves).  Each writes its own bit array;
// k_leader joins and combines.
// Each miss list goes to its own stream as soon as its partition is known, so the uncached
// verifies run during the latency-bound key precompute, beside each other, instead of trailing the
// cached chains (miss_ev[t]: the partition of cache t is done).
struct Run {
  praos_ctx* c;
  praos_batch* b;
  size_t n;
  RunPlan P;
  hipStream_t so, sk, sv;       // the OCert, KES and VRF chains
  hipStream_t sm_[3];           // the misses of cache t (cold, KES leaf, VRF keys)
  hipStream_t sV;               // Praos stage V
  hipStream_t sVk[2];           // staged TPraos: stage V of the two certificates
  uint16_t *bo, *bk, *bv;       // the chains' bit arrays
  // the kernels' arguments over the whole batch (header mode, verdicts to bo / bk / bv, every
  // per-launch field zero); a pass changes a copy where a launch differs
  OcertIn ocert;
  KesIn kes;
  VrfIn vrf;
  int32_t* dcls = nullptr;      // TPraos overlay classes (praos_set_overlay)
  bool v_queued = false, vrf_keys_queued = false;
  // pool records of the VRF key cache's entries (k_vrf_keyrec), set once this run's lists are queued;
  // not for the pool-key store's entries (their representatives are headers of earlier runs)
  const uint32_t* vrec = nullptr;
};

static int to_main(Run& r, int t, hipStream_t st) {
  praos_ctx* c = r.c;
  if (st == r.sm_[t]) return PRAOS_OK;
  HIPCHK(c, hipEventRecord(c->miss_ev[t], st));
  HIPCHK(c, hipStreamWaitEvent(r.sm_[t], c->miss_ev[t], 0));
  return PRAOS_OK;
}

// Stage V of the VRF needs nothing but the decoded header (no key table, no list), and it is
// the longest chain of the step: with concurrent streams it is queued first (RunPlan::v_first), so
// its waves are dispatched before the key-cache passes' (queued after it, it started ~0.3 ms into a
// 54k-header step, behind a dozen list kernels on the other streams)
static int queue_stage_v(Run& r) {
  praos_ctx* c = r.c;
  praos_batch* b = r.b;
  const size_t n = r.n;
  const RunPlan& P = r.P;
  VrfIn a = r.vrf;
  a.wave_prio = P.wprio_v;
  if (P.tp_staged) {
    // the two certificates' stage V side by side (own lane tables, mkSeed alphas): a batch
    // below ~300k headers leaves most wave slots empty with one V at a time
    const uint8_t* proof[2] = {b->vrf_proof, b->lead_proof};
    uint8_t* mid[2] = {b->vrf_mid, b->vrf_mid2};
    ge_cached* vtab[2] = {b->tab_vrf, b->tab_vrf2};
    for (int k = 0; k < 2; k++) {
      if (r.sVk[k] != c->stream) HIPCHK(c, hipStreamWaitEvent(r.sVk[k], c->ev[0], 0));
      if (k == 0) HIPCHK(c, hipEventRecord(c->v0_ev, r.sVk[0]));
      a.vrf_proof = proof[k];
      a.tabs = vtab[k];
      a.tp_seed = 1 + k;
      launch_vrf_v(r.sVk[k], n, a, mid[k], 0, SIZE_MAX, P.v_ilp4);
    }
    HIPCHK(c, hipEventRecord(c->v1_ev, r.sVk[0]));
    HIPCHK(c, hipEventRecord(c->v_ev, r.sVk[0]));
    HIPCHK(c, hipEventRecord(c->v2_ev, r.sVk[1]));
  } else {
    if (r.sV != c->stream) HIPCHK(c, hipStreamWaitEvent(r.sV, c->ev[0], 0));
    HIPCHK(c, hipEventRecord(c->v0_ev, r.sV));
    launch_vrf_v(r.sV, n, a, b->vrf_mid, 0, SIZE_MAX, P.v_ilp4);
    HIPCHK(c, hipEventRecord(c->v1_ev, r.sV));
  }
  c->v_timed = true;
  r.v_queued = true;
  return PRAOS_OK;
}

static void queue_vrec(Run& r, praos_batch::KeyCache& k) {
  if (!r.P.vrf_perkey || k.store >= 0 || !k.vrec) return;
  launch_vrf_keyrec(r.sm_[2], k.counters, k.max_entries, k.entry_rep, r.vrf, k.vrec);
  r.vrec = k.vrec;
}

// The VRF key chain of the three-kernel Praos VRF (one certificate) and of staged TPraos (two):
// key lists -> U of the uncached keys on the miss stream (u_ev) -> key precompute -> U of the
// cached keys, then of the wide tier's, per certificate.  Praos only: the entries' pool records
// and, under pre_join, k_vrf_pool head the miss stream; with v_main mode 2 the main stream waits
// for u_ev itself, before the join (the plan has neither pre_join nor v_main for a TPraos batch).
static int vrf_key_chain(Run& r, int ncert, const uint8_t* const proof[], uint8_t* const mid[], bool praos) {
  praos_ctx* c = r.c;
  praos_batch* b = r.b;
  const size_t n = r.n;
  const RunPlan& P = r.P;
  hipStream_t sv = r.sv, sm = r.sm_[2];
  praos_batch::KeyCache& k = b->kc[1];
  int rc = kc_lists(c, b, P, k, n, b->vrf_vk, sv, KeyItems{}, 1);
  if (rc == PRAOS_OK) rc = to_main(r, 2, sv);
  if (rc != PRAOS_OK) return rc;
  if (praos) {
    // (the records head the miss stream: the join and k_vrf_pool follow them there or wait for u_ev)
    queue_vrec(r, k);
    if (P.pre_join) {
      VrfIn a = r.vrf;
      a.rec_entry = r.vrec ? k.item_entry : nullptr;
      a.rec = r.vrec;
      launch_vrf_pool(sm, n, a);
    }
  }
  VrfIn a = r.vrf;                               // (stage U reads the key and the certificate's proof)
  for (int q = 0; q < ncert; q++) {
    a.vrf_proof = proof[q];
    launch_vrf_u(sm, n, key_misses(k), c->btab, a, b->tab_vrfu, mid[q]);
  }
  if (sm != sv) HIPCHK(c, hipEventRecord(c->u_ev, sm));
  kc_precompute(c, P, k, b->vrf_vk, 1, sv, n);
  for (int q = 0; q < ncert; q++) {
    a.vrf_proof = proof[q];
    launch_vrf_u(sv, n, key_hits(k), c->bcomb16, a, mid[q], P.u4);
    if (k.wide.min_uses) launch_vrf_u(sv, n, key_wide_hits(k), c->bcomb16, a, mid[q], 0, k.wide.entry_wide);
  }
  if (sm != sv && !(praos && P.v_main && P.vm_mode == 2)) HIPCHK(c, hipStreamWaitEvent(sv, c->u_ev, 0));
  r.vrf_keys_queued = true;
  return PRAOS_OK;
}

static int praos_vrf_keys(Run& r) {
  const uint8_t* proof[1] = {r.b->vrf_proof};
  uint8_t* mid[1] = {r.b->vrf_mid};
  return vrf_key_chain(r, 1, proof, mid, true);
}

// OCert: dedup, key cache, hits, misses, fanout
static int pass_ocert(Run& r) {
  praos_ctx* c = r.c;
  praos_batch* b = r.b;
  const size_t n = r.n;
  const RunPlan& P = r.P;
  hipStream_t so = r.so, sm = r.sm_[0];
  // With dedup the pass runs over the distinct OCert tuples only (their representatives: the
  // items), writes their verdicts to ok_out, and the verdicts fan out to every header carrying
  // them; without it the pass runs over every header (null list, null ok_out) and that is all.
  const bool dedup = P.dedup;
  const KeyItems items = dedup ? KeyItems{b->dd_reps, b->dd_counters} : KeyItems{};
  OcertIn a = r.ocert;
  a.ok_out = dedup ? b->dd_ok : nullptr;
  if (dedup) {
    b->dd_used = true;
    HIPCHK(c, hipMemsetAsync(b->dd_slot, 0, 4 * (size_t)b->dd_cap, so));
    HIPCHK(c, hipMemsetAsync(b->dd_counters, 0, 16, so));
    launch_ocert_dedup(so, n, b->cold_vk, b->hot_vk, b->ocert_n, b->ocert_c0, b->ocert_sig, b->dd_cap - 1, b->dd_slot,
                       b->dd_item_rep, b->dd_reps, b->dd_counters);
  }
  if (P.kc) {
    praos_batch::KeyCache& k = b->kc[0];
    int rc = kc_lists(c, b, P, k, n, b->cold_vk, so, items, 0);
    if (rc == PRAOS_OK) rc = to_main(r, 0, so);
    if (rc != PRAOS_OK) return rc;
    kc_precompute(c, P, k, b->cold_vk, 0, so, n);
    launch_ocert_ck(so, n, key_hits(k), c->bcomb16, a, P.ck4);
    // the misses go to their stream after the hit chain's launches are queued
    OcertIn miss = a;
    miss.wave_prio = P.miss_prio;                // (the ILP-4 form's; k_ocert has no priority)
    launch_ocert(sm, n, key_misses(k), c->btab, miss, P.miss4);
  } else {
    launch_ocert(so, n, items, c->btab, a);
  }
  if (dedup) {
    // the fanout reads dd_ok of the misses (main stream) and of the hits (this stream)
    if (P.kc && so != sm) {
      (void)hipEventRecord(c->miss_ev[3], sm);
      (void)hipStreamWaitEvent(so, c->miss_ev[3], 0);
    }
    launch_ocert_fanout(so, n, b->dd_item_rep, b->dd_ok, b->slot, b->ocert_c0, a.slots_per_kes_period, a.max_kes_evo,
                        r.bo);
  }
  return PRAOS_OK;
}

// KES: leaf keys, key cache, misses, Merkle representatives, precompute, hits
static int pass_kes(Run& r) {
  praos_ctx* c = r.c;
  praos_batch* b = r.b;
  const size_t n = r.n;
  const RunPlan& P = r.P;
  hipStream_t sk = r.sk, sm = r.sm_[1];
  if (!P.kc) {
    launch_kes(sk, n, KeyItems{}, c->btab, r.kes);
    return PRAOS_OK;
  }
  // leaf-key cache: the Ed25519 key a Sum6KES signature ends on repeats for every
  // header a pool signs in one KES period
  praos_batch::KeyCache& k = b->kc[2];
  launch_kes_leafkeys(sk, n, r.kes, b->kes_leaf);
  // (the lists of the KES pass run over every header)
  int rc = kc_lists(c, b, P, k, n, b->kes_leaf, sk, KeyItems{}, 2);
  if (rc == PRAOS_OK) rc = to_main(r, 1, sk);
  if (rc != PRAOS_OK) return rc;
  KesIn miss = r.kes;
  miss.wave_prio = P.miss_prio;                  // (the ILP-4 form's; k_kes has no priority)
  launch_kes(sm, n, key_misses(k), c->btab, miss, P.miss4);
  // Merkle path dedup: a pool's headers of one KES period carry the same hot key, period and
  // six vk pairs, so each cache entry's representative walks once and equal paths reuse it.
  // The walks stay on the KES stream ahead of the key precompute: on the miss stream, on a
  // stream of their own or behind the misses, with k_kes_ck waiting for their event, the 432k
  // step was 0.06-0.09 ms longer (profiles/r08_perkey_ab.json, kes_walks_placement)
  if (P.kes_dd) launch_kes_merkle_reps(sk, k.counters, k.max_entries, k.entry_rep, r.kes, k.rep_ok);
  kc_precompute(c, P, k, b->kes_leaf, 0, sk, n);
  HIPCHK(c, hipEventRecord(c->kc0_ev, sk));
  launch_kes_ck(sk, n, key_hits(k), c->bcomb16, r.kes, P.kes_pair_min, P.kes_dd ? k.entry_rep : nullptr,
                P.kes_dd ? k.rep_ok : nullptr, P.kes_ck4);
  HIPCHK(c, hipEventRecord(c->kc1_ev, sk));
  c->kes_ck_timed = true;
  return PRAOS_OK;
}

// after stage V (and, stored-bytes pipeline, the odd chunks' on vstream2)
static int after_v(Run& r, hipStream_t st) {
  praos_ctx* c = r.c;
  if (st != r.sV) HIPCHK(c, hipStreamWaitEvent(st, c->v_ev, 0));
  if (r.b->v_done) HIPCHK(c, hipStreamWaitEvent(st, c->v2_ev, 0));
  return PRAOS_OK;
}

// stage F (U + join): over a list of uncached keys, or over a cache's hits (against the key tables,
// or the wide tier's), with the entries' pool records when the run has them
static void vrf_fin_nc(Run& r, hipStream_t st, KeyItems items) {
  launch_vrf_fin(st, r.n, items, r.c->btab, r.vrf, r.b->vrf_mid);
}
static void vrf_fin(Run& r, hipStream_t st, const praos_batch::KeyCache& k, bool wide = false) {
  VrfIn a = r.vrf;
  a.rec = r.vrec;
  launch_vrf_fin(st, r.n, wide ? key_wide_hits(k) : key_hits(k), r.c->bcomb16, a, r.b->vrf_mid,
                 wide ? k.wide.entry_wide : nullptr);
}

static void vrf_join(Run& r, hipStream_t st) {
  VrfIn a = r.vrf;
  a.wave_prio = r.P.wprio_v;
  a.pre = r.P.pre_join ? 1 : 0;
  a.rec_entry = r.vrec && r.P.kc ? r.b->kc[1].item_entry : nullptr;
  a.rec = r.vrec;
  launch_vrf_join(st, r.n, a, r.b->vrf_mid);
}

// Praos VRF, two stages (k_vrf_stage.hip): V over every header on its own stream, from ev[0] on
// (it needs no key); then either U beside it and the join after both (three kernels, RunPlan::vrf3,
// with v_main's three placements of the join), or F = U + join after it -- the hits on sv once
// their key tables exist, the misses on their miss stream (per-lane U)
static int pass_vrf_praos(Run& r) {
  praos_ctx* c = r.c;
  praos_batch* b = r.b;
  const RunPlan& P = r.P;
  hipStream_t sv = r.sv, sm = r.sm_[2];
  int rc;
  // (stored-bytes pipeline: stage V was queued chunk by chunk on vstream while the later
  // chunks were still uploading; b->v_done)
  if (!b->v_done && !r.v_queued && (rc = queue_stage_v(r)) != PRAOS_OK) return rc;
  HIPCHK(c, hipEventRecord(c->v_ev, r.sV));
  if (b->v_done) HIPCHK(c, hipEventRecord(c->v2_ev, c->vstream2));
  if (P.vrf3) {
    // three kernels: U runs beside V (uncached keys at once on the miss stream, cached keys
    // once their tables exist), the join after both
    if (P.kc) {
      if (!r.vrf_keys_queued && (rc = praos_vrf_keys(r)) != PRAOS_OK) return rc;
    } else {
      launch_vrf_u(sv, r.n, KeyItems{}, c->btab, r.vrf, b->tab_vrfu, b->vrf_mid);
    }
    if (P.v_main && P.vm_mode == 3) {  // V on the main stream, the join on the VRF stream after U
      HIPCHK(c, hipEventRecord(c->v_ev, c->stream));
      HIPCHK(c, hipStreamWaitEvent(sv, c->v_ev, 0));
      vrf_join(r, sv);
    } else if (P.v_main) {             // V is on the main stream: the join follows it there, after U
      if (P.vm_mode == 2 && P.kc) HIPCHK(c, hipStreamWaitEvent(c->stream, c->u_ev, 0));
      HIPCHK(c, hipEventRecord(c->side_ev[2], sv));
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->side_ev[2], 0));
      vrf_join(r, c->stream);
    } else {
      if ((rc = after_v(r, sv)) != PRAOS_OK) return rc;
      vrf_join(r, sv);
    }
  } else if (P.kc) {
    praos_batch::KeyCache& k = b->kc[1];
    rc = kc_lists(c, b, P, k, r.n, b->vrf_vk, sv, KeyItems{}, 1);
    if (rc == PRAOS_OK) rc = to_main(r, 2, sv);
    if (rc != PRAOS_OK) return rc;
    // the entries' pool records: on the miss stream ahead of its wait for stage V, off the chain
    // lists -> precompute -> tables that the cached F waits for; sv joins them after its tables
    queue_vrec(r, k);
    const bool vrec_wait = r.vrec && sm != sv;
    if (vrec_wait) HIPCHK(c, hipEventRecord(c->vrec_ev, sm));
    if ((rc = after_v(r, sm)) != PRAOS_OK) return rc;
    vrf_fin_nc(r, sm, key_misses(k));
    kc_precompute(c, P, k, b->vrf_vk, 1, sv, r.n);
    if (k.wide.min_uses && sm != sv) {
      // two hit lists, and this is the step's tail: the chunk tier's few waves run beside the wide
      // tier's on the miss stream (which waited for stage V above) once the tables exist, instead
      // of trailing them as a launch of their own (432k: 10.106 -> 10.041 ms, medians of six
      // alternating runs, lower in every pair; profiles/r07_wide_ab.json)
      HIPCHK(c, hipEventRecord(c->u_ev, sv));
      HIPCHK(c, hipStreamWaitEvent(sm, c->u_ev, 0));
      vrf_fin(r, sm, k);
      if ((rc = after_v(r, sv)) != PRAOS_OK) return rc;
      if (vrec_wait) HIPCHK(c, hipStreamWaitEvent(sv, c->vrec_ev, 0));
      vrf_fin(r, sv, k, true);
    } else {
      if ((rc = after_v(r, sv)) != PRAOS_OK) return rc;
      if (vrec_wait) HIPCHK(c, hipStreamWaitEvent(sv, c->vrec_ev, 0));
      if (k.wide.min_uses) vrf_fin(r, sv, k, true);
      vrf_fin(r, sv, k);
    }
  } else {
    if ((rc = after_v(r, sv)) != PRAOS_OK) return rc;
    vrf_fin_nc(r, sv, KeyItems{});
  }
  return PRAOS_OK;
}

// TPraos VRF (b->tp_only): the two-certificate k_vrf_tp, or staged -- stage V of both certificates
// (mkSeed alphas) on the V streams from ev[0] on (queue_stage_v), U of both against the VRF key
// cache (misses on the miss stream at once, hits after the key tables), then the two joins in
// order on the VRF stream
static int pass_vrf_tpraos(Run& r) {
  praos_ctx* c = r.c;
  praos_batch* b = r.b;
  const size_t n = r.n;
  hipStream_t sv = r.sv;
  if (!r.P.tp_staged) {
    launch_vrf_tp(sv, n, c->btab, r.vrf, b->lead_out, b->lead_proof, b->beta_l, r.dcls, c->d_gen);
    return PRAOS_OK;
  }
  int rc;
  if (!r.v_queued && (rc = queue_stage_v(r)) != PRAOS_OK) return rc;
  const uint8_t* proof[2] = {b->vrf_proof, b->lead_proof};
  const uint8_t* outv[2] = {b->vrf_out, b->lead_out};
  uint8_t* mid[2] = {b->vrf_mid, b->vrf_mid2};
  uint8_t* beta[2] = {b->beta, b->beta_l};
  if (r.P.kc) {
    if ((rc = vrf_key_chain(r, 2, proof, mid, false)) != PRAOS_OK) return rc;
  } else {
    VrfIn a = r.vrf;
    for (int q = 0; q < 2; q++) {
      a.vrf_proof = proof[q];
      launch_vrf_u(sv, n, KeyItems{}, c->btab, a, b->tab_vrfu, mid[q]);
    }
  }
  if (sv != r.sVk[0]) HIPCHK(c, hipStreamWaitEvent(sv, c->v_ev, 0));
  if (sv != r.sVk[1]) HIPCHK(c, hipStreamWaitEvent(sv, c->v2_ev, 0));
  VrfIn a = r.vrf;
  for (int q = 0; q < 2; q++) {
    a.vrf_out = outv[q];
    a.vrf_proof = proof[q];
    a.beta_out = beta[q];
    launch_vrf_join_tp(sv, n, q, a, mid[q], r.dcls, c->d_gen);
  }
  return PRAOS_OK;
}

// TPraos overlay classes (praos_set_overlay) from the host slots, uploaded on the main stream
static int overlay_classes(Run& r) {
  praos_ctx* c = r.c;
  praos_batch* b = r.b;
  const size_t n = r.n;
  // the slots come from the decode on this stream; the sync also retires the previous
  // run's upload of cls_h before it is rewritten
  b->slots_h.resize(n);
  b->cls_h.resize(n);
  HIPCHK(c, hipMemcpyAsync(b->slots_h.data(), b->slot, 8 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n; i++) b->cls_h[i] = overlay_class(c, b->slots_h[i]);
  if (!b->dcls || b->dcls_n < n) {
    const size_t cap = std::max(n, b->cap_n);
    if (dalloc(b, &b->dcls, 4 * cap) != hipSuccess) return PRAOS_E_OOM;
    b->dcls_n = cap;
  }
  r.dcls = b->dcls;
  HIPCHK(c, hipMemcpyAsync(r.dcls, b->cls_h.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
  return PRAOS_OK;
}

RunShape run_shape(const praos_ctx* c, size_t n, bool tp_only, bool v_done) {
  RunShape s;
  s.n = n;
  s.concurrent = c->concurrent;
  s.kernels = c->kernels;
  s.keycache = c->keycache;
  s.dedup = c->dedup;
  s.tp_only = tp_only;
  s.v_done = v_done;
  s.pool_keys = c->pool_keys;
  s.replaying = c->replaying;
  return s;
}

int batch_run_impl(praos_ctx* c, praos_batch* b) {
  const size_t n = b->n;
  const RunPlan P = plan_run(c->knobs, run_shape(c, n, b->tp_only, b->v_done));
  Run r{c, b, n, P};
  r.bo = b->bits3;
  r.bk = b->bits3 + n;
  r.bv = b->bits3 + 2 * n;
  {
    const praos_params& pp = c->params;
    OcertIn& o = r.ocert;
    o = OcertIn{};
    o.cold_vk = b->cold_vk;
    o.hot_vk = b->hot_vk;
    o.ocert_n = b->ocert_n;
    o.ocert_c0 = b->ocert_c0;
    o.sig = b->ocert_sig;
    o.slot = b->slot;
    o.slots_per_kes_period = pp.slots_per_kes_period;
    o.max_kes_evo = pp.max_kes_evo;
    o.bits = r.bo;
    o.tabs = b->tab_ocert;
    r.kes = batch_kes_in(b, pp.slots_per_kes_period, r.bk);
    VrfIn& v = r.vrf;
    v = batch_vrf_v_in(c, b);
    v.cold_vk = b->cold_vk;
    v.vrf_out = b->vrf_out;
    v.pool_hash = c->d_pool_hash;
    v.pool_vrf = c->d_pool_vrf;
    v.pool_map = c->d_pool_map;
    v.npools = c->npools;
    v.check_output = (int)pp.vrf_check_output;
    v.bits = r.bv;
    v.pool_idx = b->pool_idx;
    v.pool_sorted_idx = b->pool_sorted;
    v.beta_out = b->beta;
    v.leader_out = b->leader;
    v.nonce_out = b->nonce;
  }
  const bool conc = c->concurrent != 0;
  r.so = conc ? c->side[0] : c->stream;
  r.sk = conc ? c->side[1] : c->stream;
  r.sv = conc ? c->side[2] : c->stream;
  for (int t = 0; t < 3; t++) r.sm_[t] = conc ? c->mside[t] : c->stream;
  r.sV = P.v_main ? c->stream : (conc || b->v_done) ? c->vstream : c->stream;
  r.sVk[0] = conc ? c->vstream : c->stream;
  r.sVk[1] = conc ? c->vstream2 : c->stream;
  c->last_from_bytes = b->from_bytes;
  c->v_timed = false;
  c->kes_ck_timed = false;
  int rc;
  if (b->from_bytes) {
    // stored bytes -> SoA (k_decode.hip); the crypto kernels read its output
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
    if (!b->decoded) {
      const int rd = batch_decode(c, b);
      if (rd != PRAOS_OK) { c->err = "decode launch failed"; return rd; }
    }
  }
  // the comb is read by the cached chains: built before ev[0]
  if (P.kc && (rc = ensure_bcomb16(c)) != PRAOS_OK) return rc;
  // TPraos (b->tp_only): the same OCert and KES passes (dedup, key caches, side streams); the
  // VRF pass is the two-certificate one (overlay classes from the host slots when
  // praos_set_overlay is on) and the leader test takes the certified L output, 2^512 bound
  if (b->tp_only && c->ovl_on && (rc = overlay_classes(r)) != PRAOS_OK) return rc;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if (conc)
    for (int k = 0; k < 3; k++) HIPCHK(c, hipStreamWaitEvent(c->side[k], c->ev[0], 0));
  if (P.tp_staged) {
    const size_t cap = std::max(n, b->cap_n);
    if (!b->vrf_mid2 || b->vrf_mid2_n < n) {
      if (dalloc(b, &b->vrf_mid2, VRF_MID_BYTES * cap) != hipSuccess ||
          dalloc(b, (uint8_t**)&b->tab_vrf2, LT_VRF_B * cap) != hipSuccess)
        return PRAOS_E_OOM;
      b->vrf_mid2_n = cap;
    }
  }
  // (serial runs keep the OCert | KES | VRF order: their per-stream spans are measured in turn)
  if (P.v_first && (rc = queue_stage_v(r)) != PRAOS_OK) return rc;
  b->kc_used = P.kc;
  if (P.vrf_keys_first && (rc = praos_vrf_keys(r)) != PRAOS_OK) return rc;
  b->dd_used = false;
  if (P.do_ocert) {
    if ((rc = pass_ocert(r)) != PRAOS_OK) return rc;
  } else {
    HIPCHK(c, hipMemsetAsync(r.bo, 0, 2 * n, r.so));
  }
  HIPCHK(c, hipEventRecord(c->side_ev[0], r.so));
  if (P.do_kes) {
    if ((rc = pass_kes(r)) != PRAOS_OK) return rc;
  } else {
    HIPCHK(c, hipMemsetAsync(r.bk, 0, 2 * n, r.sk));
  }
  HIPCHK(c, hipEventRecord(c->side_ev[1], r.sk));
  if (P.do_vrf) {
    if ((rc = b->tp_only ? pass_vrf_tpraos(r) : pass_vrf_praos(r)) != PRAOS_OK) return rc;
  } else {
    HIPCHK(c, hipMemsetAsync(r.bv, 0, 2 * n, r.sv));
    HIPCHK(c, hipMemsetAsync(b->pool_sorted, 0xff, 4 * n, r.sv));   // no pool -> leader kernel skips
  }
  HIPCHK(c, hipEventRecord(c->side_ev[2], r.sv));
  if (conc) {
    // (v_main: the VRF stream and its miss stream -- u_ev -- were waited for before the join)
    const bool sv_done = P.v_main && P.vm_mode != 3;
    for (int k = 0; k < 3; k++)
      if (!(sv_done && k == 2)) HIPCHK(c, hipStreamWaitEvent(c->stream, c->side_ev[k], 0));
    for (int k = 0; k < 3; k++) {
      if (sv_done && k == 2) continue;
      HIPCHK(c, hipEventRecord(c->mdone_ev[k], c->mside[k]));
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->mdone_ev[k], 0));
    }
  }
  launch_leader(dim3(nblocks(n, NT)), dim3(NT), c->stream, n, b->tp_only ? b->lead_out : b->leader, b->pool_sorted,
                c->d_pool_x, (const uint32_t*)nullptr, (int)c->params.f_is_one, b->tp_only ? 16 : 8, r.bo, r.bk, r.bv, b->bits,
                (uint8_t*)nullptr, (int32_t*)nullptr, b->from_bytes ? b->dec_status : (const uint16_t*)nullptr);
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  HIPCHK(c, hipGetLastError());
  return PRAOS_OK;
}

}  // namespace praos_impl

