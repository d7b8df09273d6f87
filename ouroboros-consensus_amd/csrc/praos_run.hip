// praos_run.hip -- the crypto step of a batch (praos_batch_run): the key-cache passes and the
// scheduler that spreads the OCert, KES and VRF chains over the context's streams.
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

int kc_lists(praos_ctx* c, praos_batch* b, praos_batch::KeyCache& k, size_t n, const uint8_t* keys,
             hipStream_t st, const uint32_t* list, const uint32_t* count, int which) {
  int min_uses = c->kc_min[which] > 0 ? c->kc_min[which] : c->keycache;
  // small batches: no KES leaf key is cached (every item a miss, KES_NOCACHE_BATCH); the batch size
  // is the caller's n (the lists of the KES pass run over every header)
  if (which == 2 && c->kc_min[2] <= 0 && n < c->kes_nocache) min_uses = INT32_MAX;
  const dim3 g(nblocks(n, NT)), blk(NT);
  k.kt = k.ktab; k.ki = k.kinfo; k.erep = k.entry_rep; k.epos = k.entry_pos; k.emax = k.max_entries;
  k.ebase = nullptr; k.store = -1;
  HIPCHK(c, hipMemsetAsync(k.slot_rep, 0, 4 * (size_t)k.cap, st));
  HIPCHK(c, hipMemsetAsync(k.slot_cnt, 0, 4 * (size_t)k.cap, st));
  HIPCHK(c, hipMemsetAsync(k.counters, 0, 16, st));
  praos_ctx::PoolKeyStore* ps = nullptr;
  if (c->pk_on && which < 2 && ensure_pks(c, which, st)) {
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
    min_uses = 1;
  }
  // wide tier: VRF keys of this batch's own cache (the pool-key store's entries stay in the chunk tier)
  k.wide.min_uses = 0;
  if (which == 1 && !ps && c->wide_min(n) > 0) {
    const uint32_t wmin = std::max(c->wide_min(n), (uint32_t)std::max(min_uses, 1));
    const uint32_t need = (uint32_t)std::min<size_t>((size_t)std::max(c->vrf_wide_cap, 1), n / wmin + 1);
    // allocated by the first run that uses the tier, for the batch's capacity, and kept; a later run
    // that needs more keys allocates a larger set (the smaller one stays owned until the batch is freed)
    if (k.wide_alloc < need) {
      const size_t cap_n = std::max(n, b->cap_n);
      const uint32_t wcap = (uint32_t)std::min<size_t>((size_t)std::max(c->vrf_wide_cap, 1), cap_n / wmin + 1);
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
  launch_key_insert(g, blk, st, n, list, count, keys, k.cap - 1, k.slot_rep, k.slot_cnt, k.item_slot,
                    ps ? ps->pentry : nullptr, ps ? ps->pkey : nullptr, ps ? ps->slots - 1 : 0u,
                    ps ? ps->scnt : nullptr);
  launch_key_assign(dim3(nblocks(k.cap, NT)), blk, st, k.cap, k.slot_rep, k.slot_cnt, (uint32_t)min_uses,
                    k.emax, k.slot_entry, k.erep, k.epos, k.counters, k.wide);
  if (ps) launch_key_store_ranges(st, ps->cap, ps->scnt, ps->spos, k.counters);
  launch_key_partition(g, blk, st, n, list, count, k.item_slot, k.slot_entry, k.item_entry, k.epos, k.hit, k.miss,
                       k.counters, ps ? ps->spos : nullptr, k.wide);
  return PRAOS_OK;
}
void kc_precompute(praos_ctx* c, praos_batch::KeyCache& k, const uint8_t* keys, int kind, hipStream_t st, size_t n) {
  // (with a wide tier the tables' chain -- decode, chunk bases, position bases, tables -- is longer
  // than stage V leaves room for in a large batch, and the U chains wait for it: raised wave
  // priority, as in a small batch; 432k 10.24 -> 10.09 ms, profiles/r07_wide_ab.json)
  const bool wide = k.wide.min_uses != 0;
  const int prio = c->key_wave_prio > 0 || (c->key_wave_prio < 0 && (n < KEY_PRIO_BATCH || (wide && c->wide_prio)));
  if (k.store < 0) {
    launch_key_precompute(kind, st, k.counters, k.max_entries, k.entry_rep, keys, k.ktab, k.kinfo, prio, nullptr,
                          k.max_entries, c->key_mode(n), k.wide);
    return;
  }
  praos_ctx::PoolKeyStore& ps = c->pks[k.store];
  const uint32_t span = (uint32_t)std::min<size_t>(n, ps.cap);   // new entries of this run, at most
  launch_key_precompute(kind, st, k.counters, ps.cap, ps.entry_rep, keys, ps.ktab, ps.kinfo, prio, ps.base, span,
                        c->key_mode(n));
  launch_pkey_publish(st, k.counters, ps.base, ps.cap, ps.entry_rep, keys, ps.pentry, ps.pkey, ps.slots - 1, ps.count,
                      span);
}

int batch_run_impl(praos_ctx* c, praos_batch* b) {
  const size_t n = b->n;
  const praos_params& P = c->params;
  uint16_t* bo = b->bits3;
  uint16_t* bk = b->bits3 + n;
  uint16_t* bv = b->bits3 + 2 * n;
  const dim3 g(nblocks(n, NT)), blk(NT);
  const dim3 gl(nblocks(n, lat_block(n))), bl(lat_block(n));     // kernels without LDS tables
  // The three crypto kernels are independent; run concurrently they fill each
  // other's tail waves (one launch of 432k headers is ~3.3 rounds of resident
  // waves).  Each writes its own bit array; k_leader joins and combines.
  hipStream_t so = c->concurrent ? c->side[0] : c->stream;
  hipStream_t sk = c->concurrent ? c->side[1] : c->stream;
  hipStream_t sv = c->concurrent ? c->side[2] : c->stream;
  c->last_from_bytes = b->from_bytes;
  c->v_timed = false;
  c->kes_ck_timed = false;
  c->pk_on = c->keycache > 0 && (c->pool_keys > 0 || (c->pool_keys < 0 && c->replaying));
  if (b->from_bytes) {
    // stored bytes -> SoA (k_decode.hip); the crypto kernels read its output
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
    if (!b->decoded) {
      const int rd = batch_decode(c, b);
      if (rd != PRAOS_OK) { c->err = "decode launch failed"; return rd; }
    }
  }
  if (c->keycache > 0 && n >= 2) {     // the comb is read by the cached chains: built before ev[0]
    const int rc = ensure_bcomb16(c);
    if (rc != PRAOS_OK) return rc;
  }
  // TPraos (b->tp_only): the same OCert and KES passes (dedup, key caches, side streams); the
  // VRF pass is the two-certificate k_vrf_tp (overlay classes from the host slots when
  // praos_set_overlay is on) and the leader test takes the certified L output, 2^512 bound
  int32_t* dcls = nullptr;
  if (b->tp_only && c->ovl_on) {
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
    dcls = b->dcls;
    HIPCHK(c, hipMemcpyAsync(dcls, b->cls_h.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if (c->concurrent)
    for (int k = 0; k < 3; k++) HIPCHK(c, hipStreamWaitEvent(c->side[k], c->ev[0], 0));
  // Stage V of the VRF needs nothing but the decoded header (no key table, no list), and it is
  // the longest chain of the step: with concurrent streams it is queued first, so its waves
  // are dispatched before the key-cache passes' (queued after it, it started ~0.3 ms into a
  // 54k-header step, behind a dozen list kernels on the other streams)
  const bool do_vrf = (c->kernels & 4) != 0;
  const bool tp_staged = do_vrf && b->tp_only && c->tp_staged;
  // PRAOS_V_MAIN: the three-kernel Praos VRF with stage V and the join on the main stream (the
  // step's critical path then crosses streams once, U -> join, instead of at ev[0] -> V, V -> join
  // and join -> leader)
  const int vm_mode = c->vmain_mode(n);
  const bool v_main = vm_mode > 0 && c->concurrent && do_vrf && !b->tp_only && !b->v_done &&
                      (c->vrf3 > 0 || (c->vrf3 < 0 && n < 300000));
  const int wprio_v = c->vrf_prio > 0 || (c->vrf_prio < 0 && n < SMALL_BATCH);
  bool v_queued = false;
  if (tp_staged) {
    const size_t cap = std::max(n, b->cap_n);
    if (!b->vrf_mid2 || b->vrf_mid2_n < n) {
      if (dalloc(b, &b->vrf_mid2, VRF_MID_BYTES * cap) != hipSuccess ||
          dalloc(b, (uint8_t**)&b->tab_vrf2, LT_VRF_B * cap) != hipSuccess)
        return PRAOS_E_OOM;
      b->vrf_mid2_n = cap;
    }
  }
  auto queue_stage_v = [&]() -> int {
    const uint32_t* eta = b->eta_tab ? b->eta_tab : c->d_eta0;
    if (tp_staged) {
      // the two certificates' stage V side by side (own lane tables, mkSeed alphas): a batch
      // below ~300k headers leaves most wave slots empty with one V at a time
      hipStream_t sVk[2] = {c->concurrent ? c->vstream : c->stream, c->concurrent ? c->vstream2 : c->stream};
      const uint8_t* proof[2] = {b->vrf_proof, b->lead_proof};
      uint8_t* mid[2] = {b->vrf_mid, b->vrf_mid2};
      ge_cached* vtab[2] = {b->tab_vrf, b->tab_vrf2};
      for (int k = 0; k < 2; k++) {
        if (sVk[k] != c->stream) HIPCHK(c, hipStreamWaitEvent(sVk[k], c->ev[0], 0));
        if (k == 0) HIPCHK(c, hipEventRecord(c->v0_ev, sVk[0]));
        launch_vrf_v(sVk[k], n, b->vrf_vk, proof[k], b->slot, eta, c->eta0_neutral, b->eta_idx, vtab[k], mid[k], 0,
                     SIZE_MAX, wprio_v, 1 + k, c->v_ilp4(n));
      }
      HIPCHK(c, hipEventRecord(c->v1_ev, sVk[0]));
      HIPCHK(c, hipEventRecord(c->v_ev, sVk[0]));
      HIPCHK(c, hipEventRecord(c->v2_ev, sVk[1]));
    } else {
      hipStream_t sV = c->concurrent && !v_main ? c->vstream : c->stream;
      if (sV != c->stream) HIPCHK(c, hipStreamWaitEvent(sV, c->ev[0], 0));
      HIPCHK(c, hipEventRecord(c->v0_ev, sV));
      launch_vrf_v(sV, n, b->vrf_vk, b->vrf_proof, b->slot, eta, c->eta0_neutral, b->eta_idx, b->tab_vrf,
                   b->vrf_mid, 0, SIZE_MAX, wprio_v, 0, c->v_ilp4(n));
      HIPCHK(c, hipEventRecord(c->v1_ev, sV));
    }
    c->v_timed = true;
    v_queued = true;
    return PRAOS_OK;
  };
  // (serial runs keep the OCert | KES | VRF order: their per-stream spans are measured in turn)
  if (c->concurrent && do_vrf && (tp_staged || (!b->tp_only && !b->v_done))) {
    const int r = queue_stage_v();
    if (r != PRAOS_OK) return r;
  }
  const bool kc = c->keycache > 0 && n >= 2;
  b->kc_used = kc;
  // key cache prepass on the kernel's own stream: hash set, entries, hit/miss lists, tables
  // (items: all n, or list[0 .. *count) when list != null)
  // Each miss list goes to its own stream as soon as its partition is known, so the
  // uncached verifies run during the latency-bound key precompute, beside each other,
  // instead of trailing the cached chains (miss_ev[t]: the partition of cache t is done).
  hipStream_t sm_[3] = {c->concurrent ? c->mside[0] : c->stream, c->concurrent ? c->mside[1] : c->stream,
                        c->concurrent ? c->mside[2] : c->stream};
  auto to_main = [&](int t, hipStream_t st) -> int {
    if (st == sm_[t]) return PRAOS_OK;
    HIPCHK(c, hipEventRecord(c->miss_ev[t], st));
    HIPCHK(c, hipStreamWaitEvent(sm_[t], c->miss_ev[t], 0));
    return PRAOS_OK;
  };
  auto keycache_lists = [&](praos_batch::KeyCache& k, const uint8_t* keys, hipStream_t st,
                            const uint32_t* list = nullptr, const uint32_t* count = nullptr) -> int {
    return kc_lists(c, b, k, n, keys, st, list, count, (int)(&k - b->kc));
  };
  auto keycache_precompute = [&](praos_batch::KeyCache& k, const uint8_t* keys, int kind, hipStream_t st) {
    kc_precompute(c, k, keys, kind, st, n);
  };
  // Praos VRF in three kernels (below 300k headers): the VRF key lists, the uncached U and the
  // key precompute + cached U are queued ahead of the OCert and KES passes when the streams
  // run concurrently (PRAOS_VRF_KEYS_FIRST): after stage V, the VRF key chain -- lists,
  // precompute, tables, U, join -- is a small batch's longest (profiles/r04/i: its lists
  // started 0.33 ms into a 54k-header step, behind the OCert and KES lists)
  const bool vrf3 = do_vrf && !b->tp_only && (c->vrf3 > 0 || (c->vrf3 < 0 && n < 300000));
  bool vrf_keys_queued = false;
  // pool records of the VRF key cache's entries (k_vrf_keyrec), set once this run's lists are queued;
  // not for the pool-key store's entries (their representatives are headers of earlier runs)
  const uint32_t* vrec = nullptr;
  auto queue_vrec = [&](praos_batch::KeyCache& k) {
    if (!c->vrf_perkey || k.store >= 0 || !k.vrec) return;
    launch_vrf_keyrec(sm_[2], k.counters, k.max_entries, k.entry_rep, b->cold_vk, b->vrf_vk, c->d_pool_hash,
                      c->d_pool_vrf, c->d_pool_map, c->npools, k.vrec);
    vrec = k.vrec;
  };
  const bool pre_join = vrf3 && kc && (c->pre_join > 0 || (c->pre_join < 0 && n < SMALL_BATCH));
  auto vrf_keys = [&]() -> int {
    praos_batch::KeyCache& k = b->kc[1];
    int r = keycache_lists(k, b->vrf_vk, sv);
    if (r == PRAOS_OK) r = to_main(2, sv);
    if (r != PRAOS_OK) return r;
    // (the records head the miss stream: the join and k_vrf_pool follow them there or wait for u_ev)
    queue_vrec(k);
    if (pre_join)
      launch_vrf_pool(sm_[2], n, b->cold_vk, b->vrf_vk, b->vrf_out, c->d_pool_hash, c->d_pool_vrf, c->d_pool_map,
                      c->npools, bv, b->pool_idx, b->pool_sorted, b->leader, b->nonce, vrec ? k.item_entry : nullptr,
                      vrec);
    launch_vrf_u(sm_[2], n, k.miss, k.counters + 2, nullptr, nullptr, nullptr, c->bcomb16, c->btab, b->vrf_vk,
                 b->vrf_proof, b->tab_vrfu, b->vrf_mid);
    if (sm_[2] != sv) HIPCHK(c, hipEventRecord(c->u_ev, sm_[2]));
    keycache_precompute(k, b->vrf_vk, 1, sv);
    launch_vrf_u(sv, n, k.hit, k.counters + 1, k.item_entry, k.kt, k.ki, c->bcomb16, c->btab, b->vrf_vk,
                 b->vrf_proof, b->tab_vrfu, b->vrf_mid, c->use_u4(n), 0);
    if (k.wide.min_uses)
      launch_vrf_u(sv, n, k.wide.hit, k.wide.wcnt + 1, k.item_entry, k.wide.wtab, k.ki, c->bcomb16, c->btab,
                   b->vrf_vk, b->vrf_proof, b->tab_vrfu, b->vrf_mid, 0, 0, k.wide.entry_wide);
    // (v_main 2: the main stream waits for u_ev itself, before the join)
    if (sm_[2] != sv && !(v_main && vm_mode == 2)) HIPCHK(c, hipStreamWaitEvent(sv, c->u_ev, 0));
    vrf_keys_queued = true;
    return PRAOS_OK;
  };
  if (vrf3 && kc && c->concurrent && c->vrf_keys_first) {
    const int r = vrf_keys();
    if (r != PRAOS_OK) return r;
  }
  b->dd_used = false;
  if (c->kernels & 1) {
    // With dedup the pass runs over the distinct OCert tuples only (their representatives: list /
    // count), writes their verdicts to ok_out, and the verdicts fan out to every header carrying
    // them; without it the pass runs over every header (null list, null ok_out) and that is all.
    const bool dedup = c->dedup && n >= 2;
    const uint32_t* const list = dedup ? b->dd_reps : nullptr;
    const uint32_t* const count = dedup ? b->dd_counters : nullptr;
    uint8_t* const ok_out = dedup ? b->dd_ok : nullptr;
    if (dedup) {
      b->dd_used = true;
      HIPCHK(c, hipMemsetAsync(b->dd_slot, 0, 4 * (size_t)b->dd_cap, so));
      HIPCHK(c, hipMemsetAsync(b->dd_counters, 0, 16, so));
      launch_ocert_dedup(g, blk, so, n, b->cold_vk, b->hot_vk, b->ocert_n, b->ocert_c0, b->ocert_sig, b->dd_cap - 1,
                         b->dd_slot, b->dd_item_rep, b->dd_reps, b->dd_counters);
    }
    if (kc) {
      praos_batch::KeyCache& k = b->kc[0];
      int r = keycache_lists(k, b->cold_vk, so, list, count);
      if (r == PRAOS_OK) r = to_main(0, so);
      if (r != PRAOS_OK) return r;
      keycache_precompute(k, b->cold_vk, 0, so);
      if (c->use_ck4(n))
        launch_ocert_ck4(so, n, k.hit, k.counters + 1, k.item_entry, k.kt, k.ki, c->bcomb16, b->cold_vk, b->hot_vk,
                         b->ocert_n, b->ocert_c0, b->ocert_sig, b->slot, P.slots_per_kes_period, P.max_kes_evo, bo,
                         ok_out);
      else
        launch_ocert_ck(gl, bl, so, k.hit, k.counters + 1, k.item_entry, k.kt, k.ki, c->bcomb16, b->cold_vk,
                        b->hot_vk, b->ocert_n, b->ocert_c0, b->ocert_sig, b->slot, P.slots_per_kes_period,
                        P.max_kes_evo, bo, ok_out, 0);
      // the misses go to their stream after the hit chain's launches are queued
      if (c->use_miss4(n))
        launch_ocert4(g, blk, sm_[0], k.miss, k.counters + 2, c->btab, b->cold_vk, b->hot_vk, b->ocert_n,
                      b->ocert_c0, b->ocert_sig, b->slot, P.slots_per_kes_period, P.max_kes_evo, bo, ok_out,
                      b->tab_ocert, c->miss_prio_for(n));
      else
        launch_ocert(g, blk, sm_[0], n, k.miss, k.counters + 2, c->btab, b->cold_vk, b->hot_vk, b->ocert_n,
                     b->ocert_c0, b->ocert_sig, b->slot, P.slots_per_kes_period, P.max_kes_evo, bo, ok_out,
                     b->tab_ocert);
    } else {
      launch_ocert(g, blk, so, n, list, count, c->btab, b->cold_vk, b->hot_vk, b->ocert_n, b->ocert_c0,
                   b->ocert_sig, b->slot, P.slots_per_kes_period, P.max_kes_evo, bo, ok_out, b->tab_ocert);
    }
    if (dedup) {
      // the fanout reads dd_ok of the misses (main stream) and of the hits (this stream)
      if (kc && so != sm_[0]) {
        (void)hipEventRecord(c->miss_ev[3], sm_[0]);
        (void)hipStreamWaitEvent(so, c->miss_ev[3], 0);
      }
      launch_ocert_fanout(g, blk, so, n, b->dd_item_rep, b->dd_ok, b->slot, b->ocert_c0, P.slots_per_kes_period,
                          P.max_kes_evo, bo);
    }
  } else {
    HIPCHK(c, hipMemsetAsync(bo, 0, 2 * n, so));
  }
  HIPCHK(c, hipEventRecord(c->side_ev[0], so));
  if (c->kernels & 2) {
    if (kc) {
      // leaf-key cache: the Ed25519 key a Sum6KES signature ends on repeats for every
      // header a pool signs in one KES period
      praos_batch::KeyCache& k = b->kc[2];
      launch_kes_leafkeys(g, blk, sk, n, b->kes_sig, b->slot, b->ocert_c0, P.slots_per_kes_period, b->kes_leaf);
      int r = keycache_lists(k, b->kes_leaf, sk);
      if (r == PRAOS_OK) r = to_main(1, sk);
      if (r != PRAOS_OK) return r;
      // Merkle path dedup: a pool's headers of one KES period carry the same hot key, period and
      // six vk pairs, so each cache entry's representative walks once and equal paths reuse it.
      // The walks stay on the KES stream ahead of the key precompute: on the miss stream, on a
      // stream of their own or behind the misses, with k_kes_ck waiting for their event, the 432k
      // step was 0.06-0.09 ms longer (profiles/r08_perkey_ab.json, kes_walks_placement)
      const bool kes_dd = c->use_kes_dedup(n);
      if (c->use_miss4(n))
        launch_kes4(g, blk, sm_[1], k.miss, k.counters + 2, c->btab, b->hot_vk, b->kes_sig, b->body_off, b->body_len,
                    b->body, b->body_bytes_len, b->slot, b->ocert_c0, P.slots_per_kes_period, bk, b->tab_kes,
                    c->miss_prio_for(n));
      else
        launch_kes(g, blk, sm_[1], n, k.miss, k.counters + 2, c->btab, b->hot_vk, b->kes_sig, b->body_off,
                   b->body_len, b->body, b->body_bytes_len, b->slot, b->ocert_c0, P.slots_per_kes_period,
                   (const uint32_t*)nullptr, bk, (uint8_t*)nullptr, b->tab_kes);
      if (kes_dd)
        launch_kes_merkle_reps(sk, k.counters, k.max_entries, k.entry_rep, b->hot_vk, b->kes_sig, b->slot,
                               b->ocert_c0, P.slots_per_kes_period, k.rep_ok);
      keycache_precompute(k, b->kes_leaf, 0, sk);
      HIPCHK(c, hipEventRecord(c->kc0_ev, sk));
      if (c->use_ck4(n) && !c->kes_pair_min() && !kes_dd)
        launch_kes_ck4(sk, n, k.hit, k.counters + 1, k.item_entry, k.kt, k.ki, c->bcomb16, b->hot_vk, b->kes_sig,
                       b->body_off, b->body_len, b->body, b->body_bytes_len, b->slot, b->ocert_c0,
                       P.slots_per_kes_period, bk);
      else
        launch_kes_ck(gl, bl, sk, k.hit, k.counters + 1, k.item_entry, k.kt, k.ki, c->bcomb16, b->hot_vk, b->kes_sig,
                      b->body_off, b->body_len, b->body, b->body_bytes_len, b->slot, b->ocert_c0,
                      P.slots_per_kes_period, bk, c->kes_pair_min(), kes_dd ? k.entry_rep : nullptr,
                      kes_dd ? k.rep_ok : nullptr, 0);
      HIPCHK(c, hipEventRecord(c->kc1_ev, sk));
      c->kes_ck_timed = true;
    } else {
      launch_kes(g, blk, sk, n, (const uint32_t*)nullptr, (const uint32_t*)nullptr, c->btab, b->hot_vk, b->kes_sig,
                 b->body_off, b->body_len, b->body, b->body_bytes_len, b->slot, b->ocert_c0, P.slots_per_kes_period,
                 (const uint32_t*)nullptr, bk, (uint8_t*)nullptr, b->tab_kes);
    }
  } else
    HIPCHK(c, hipMemsetAsync(bk, 0, 2 * n, sk));
  HIPCHK(c, hipEventRecord(c->side_ev[1], sk));
  if (tp_staged) {
    // TPraos, staged: stage V of both certificates (mkSeed alphas) on the V streams from ev[0]
    // on (queue_stage_v), U of both against the VRF key cache (misses on the miss stream at
    // once, hits after the key tables), then the two joins in order on the VRF stream
    if (!v_queued) {
      const int r = queue_stage_v();
      if (r != PRAOS_OK) return r;
    }
    const uint8_t* proof[2] = {b->vrf_proof, b->lead_proof};
    const uint8_t* outv[2] = {b->vrf_out, b->lead_out};
    uint8_t* mid[2] = {b->vrf_mid, b->vrf_mid2};
    uint8_t* beta[2] = {b->beta, b->beta_l};
    hipStream_t sVk[2] = {c->concurrent ? c->vstream : c->stream, c->concurrent ? c->vstream2 : c->stream};
    if (kc) {
      praos_batch::KeyCache& k = b->kc[1];
      int r = keycache_lists(k, b->vrf_vk, sv);
      if (r == PRAOS_OK) r = to_main(2, sv);
      if (r != PRAOS_OK) return r;
      for (int q = 0; q < 2; q++)
        launch_vrf_u(sm_[2], n, k.miss, k.counters + 2, nullptr, nullptr, nullptr, c->bcomb16, c->btab, b->vrf_vk,
                     proof[q], b->tab_vrfu, mid[q]);
      if (sm_[2] != sv) HIPCHK(c, hipEventRecord(c->u_ev, sm_[2]));
      keycache_precompute(k, b->vrf_vk, 1, sv);
      for (int q = 0; q < 2; q++) {
        launch_vrf_u(sv, n, k.hit, k.counters + 1, k.item_entry, k.kt, k.ki, c->bcomb16, c->btab, b->vrf_vk,
                     proof[q], b->tab_vrfu, mid[q], c->use_u4(n));
        if (k.wide.min_uses)
          launch_vrf_u(sv, n, k.wide.hit, k.wide.wcnt + 1, k.item_entry, k.wide.wtab, k.ki, c->bcomb16, c->btab,
                       b->vrf_vk, proof[q], b->tab_vrfu, mid[q], 0, 0, k.wide.entry_wide);
      }
      if (sm_[2] != sv) HIPCHK(c, hipStreamWaitEvent(sv, c->u_ev, 0));
    } else {
      for (int q = 0; q < 2; q++)
        launch_vrf_u(sv, n, nullptr, nullptr, nullptr, nullptr, nullptr, c->bcomb16, c->btab, b->vrf_vk, proof[q],
                     b->tab_vrfu, mid[q]);
    }
    if (sv != sVk[0]) HIPCHK(c, hipStreamWaitEvent(sv, c->v_ev, 0));
    if (sv != sVk[1]) HIPCHK(c, hipStreamWaitEvent(sv, c->v2_ev, 0));
    for (int q = 0; q < 2; q++)
      launch_vrf_join_tp(sv, n, q, b->cold_vk, b->vrf_vk, outv[q], proof[q], c->d_pool_hash, c->d_pool_vrf,
                         c->d_pool_map, c->npools, (int)P.vrf_check_output, bv, b->pool_idx, b->pool_sorted, beta[q],
                         b->nonce, mid[q], dcls, c->d_gen);
  } else if (do_vrf && b->tp_only) {
    launch_vrf_tp(g, blk, sv, n, c->btab, b->cold_vk, b->vrf_vk, b->vrf_out, b->vrf_proof, b->lead_out, b->lead_proof,
                  b->slot, b->eta_tab ? b->eta_tab : c->d_eta0, c->eta0_neutral, c->d_pool_hash, c->d_pool_vrf,
                  c->d_pool_map, c->npools, (int)P.vrf_check_output, bv, b->pool_idx, b->pool_sorted, b->beta, b->beta_l,
                  b->nonce, b->tab_vrf, dcls, c->d_gen, b->eta_idx);
  } else if (do_vrf) {
    // two stages (k_vrf_stage.hip): V over every header on its own stream, from ev[0] on (it
    // needs no key); F after it -- the hits on sv once their key tables exist, the misses
    // on their miss stream (per-lane U)
    const uint32_t* eta = b->eta_tab ? b->eta_tab : c->d_eta0;
    // (stored-bytes pipeline: stage V was queued chunk by chunk on vstream while the later
    // chunks were still uploading; b->v_done)
    hipStream_t sV = v_main ? c->stream : (c->concurrent || b->v_done) ? c->vstream : c->stream;
    const int wprio = wprio_v;
    if (!b->v_done && !v_queued) {
      const int r = queue_stage_v();
      if (r != PRAOS_OK) return r;
    }
    HIPCHK(c, hipEventRecord(c->v_ev, sV));
    if (b->v_done) HIPCHK(c, hipEventRecord(c->v2_ev, c->vstream2));
    auto after_v = [&](hipStream_t st) -> int {
      if (st != sV) HIPCHK(c, hipStreamWaitEvent(st, c->v_ev, 0));
      if (b->v_done) HIPCHK(c, hipStreamWaitEvent(st, c->v2_ev, 0));
      return PRAOS_OK;
    };
    auto fin = [&](hipStream_t st, const uint32_t* list, const uint32_t* count, const praos_batch::KeyCache* k,
                   bool wide = false) {
      launch_vrf_fin(st, n, list, count, k ? k->item_entry : nullptr, k ? (wide ? k->wide.wtab : k->kt) : nullptr,
                     k ? k->ki : nullptr, c->bcomb16, c->btab, b->cold_vk, b->vrf_vk, b->vrf_out, b->vrf_proof,
                     c->d_pool_hash, c->d_pool_vrf, c->d_pool_map, c->npools, (int)P.vrf_check_output, bv, b->pool_idx,
                     b->pool_sorted, b->beta, b->leader, b->nonce, b->tab_vrf, b->vrf_mid,
                     wide ? k->wide.entry_wide : nullptr, k ? vrec : nullptr);
    };
    auto stage_u = [&](hipStream_t st, const uint32_t* list, const uint32_t* count, const praos_batch::KeyCache* k) {
      launch_vrf_u(st, n, list, count, k ? k->item_entry : nullptr, k ? k->kt : nullptr, k ? k->ki : nullptr,
                   c->bcomb16, c->btab, b->vrf_vk, b->vrf_proof, b->tab_vrfu, b->vrf_mid);
    };
    auto join = [&](hipStream_t st) {
      launch_vrf_join(st, n, b->cold_vk, b->vrf_vk, b->vrf_out, b->vrf_proof, c->d_pool_hash, c->d_pool_vrf,
                      c->d_pool_map, c->npools, (int)P.vrf_check_output, bv, b->pool_idx, b->pool_sorted, b->beta,
                      b->leader, b->nonce, b->vrf_mid, wprio, pre_join ? 1 : 0,
                      vrec && kc ? b->kc[1].item_entry : nullptr, vrec);
    };
    if (vrf3) {
      // three kernels: U runs beside V (uncached keys at once on the miss stream, cached keys
      // once their tables exist), the join after both
      int r;
      if (kc) {
        if (!vrf_keys_queued && (r = vrf_keys()) != PRAOS_OK) return r;
      } else {
        stage_u(sv, nullptr, nullptr, nullptr);
      }
      if (v_main && vm_mode == 3) {  // V on the main stream, the join on the VRF stream after U
        HIPCHK(c, hipEventRecord(c->v_ev, c->stream));
        HIPCHK(c, hipStreamWaitEvent(sv, c->v_ev, 0));
        join(sv);
      } else if (v_main) {             // V is on the main stream: the join follows it there, after U
        if (vm_mode == 2 && kc) HIPCHK(c, hipStreamWaitEvent(c->stream, c->u_ev, 0));
        HIPCHK(c, hipEventRecord(c->side_ev[2], sv));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->side_ev[2], 0));
        join(c->stream);
      } else {
        if ((r = after_v(sv)) != PRAOS_OK) return r;
        join(sv);
      }
    } else if (kc) {
      praos_batch::KeyCache& k = b->kc[1];
      int r = keycache_lists(k, b->vrf_vk, sv);
      if (r == PRAOS_OK) r = to_main(2, sv);
      if (r != PRAOS_OK) return r;
      // the entries' pool records: on the miss stream ahead of its wait for stage V, off the chain
      // lists -> precompute -> tables that the cached F waits for; sv joins them after its tables
      queue_vrec(k);
      const bool vrec_wait = vrec && sm_[2] != sv;
      if (vrec_wait) HIPCHK(c, hipEventRecord(c->vrec_ev, sm_[2]));
      if ((r = after_v(sm_[2])) != PRAOS_OK) return r;
      fin(sm_[2], k.miss, k.counters + 2, nullptr);
      keycache_precompute(k, b->vrf_vk, 1, sv);
      if (k.wide.min_uses && sm_[2] != sv) {
        // two hit lists, and this is the step's tail: the chunk tier's few waves run beside the wide
        // tier's on the miss stream (which waited for stage V above) once the tables exist, instead
        // of trailing them as a launch of their own (432k: 10.106 -> 10.041 ms, medians of six
        // alternating runs, lower in every pair; profiles/r07_wide_ab.json)
        HIPCHK(c, hipEventRecord(c->u_ev, sv));
        HIPCHK(c, hipStreamWaitEvent(sm_[2], c->u_ev, 0));
        fin(sm_[2], k.hit, k.counters + 1, &k);
        if ((r = after_v(sv)) != PRAOS_OK) return r;
        if (vrec_wait) HIPCHK(c, hipStreamWaitEvent(sv, c->vrec_ev, 0));
        fin(sv, k.wide.hit, k.wide.wcnt + 1, &k, true);
      } else {
        if ((r = after_v(sv)) != PRAOS_OK) return r;
        if (vrec_wait) HIPCHK(c, hipStreamWaitEvent(sv, c->vrec_ev, 0));
        if (k.wide.min_uses) fin(sv, k.wide.hit, k.wide.wcnt + 1, &k, true);
        fin(sv, k.hit, k.counters + 1, &k);
      }
    } else {
      const int r = after_v(sv);
      if (r != PRAOS_OK) return r;
      fin(sv, nullptr, nullptr, nullptr);
    }
  }
  else {
    HIPCHK(c, hipMemsetAsync(bv, 0, 2 * n, sv));
    HIPCHK(c, hipMemsetAsync(b->pool_sorted, 0xff, 4 * n, sv));   // no pool -> leader kernel skips
  }
  HIPCHK(c, hipEventRecord(c->side_ev[2], sv));
  if (c->concurrent) {
    // (v_main: the VRF stream and its miss stream -- u_ev -- were waited for before the join)
    const bool sv_done = v_main && vm_mode != 3;
    for (int k = 0; k < 3; k++)
      if (!(sv_done && k == 2)) HIPCHK(c, hipStreamWaitEvent(c->stream, c->side_ev[k], 0));
    for (int k = 0; k < 3; k++) {
      if (sv_done && k == 2) continue;
      HIPCHK(c, hipEventRecord(c->mdone_ev[k], c->mside[k]));
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->mdone_ev[k], 0));
    }
  }
  launch_leader(g, blk, c->stream, n, b->tp_only ? b->lead_out : b->leader, b->pool_sorted, c->d_pool_x,
                (const uint32_t*)nullptr, (int)P.f_is_one, b->tp_only ? 16 : 8, bo, bk, bv, b->bits, (uint8_t*)nullptr,
                (int32_t*)nullptr, b->from_bytes ? b->dec_status : (const uint16_t*)nullptr);
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  HIPCHK(c, hipGetLastError());
  return PRAOS_OK;
}

}  // namespace praos_impl
