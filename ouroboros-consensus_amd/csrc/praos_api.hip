// praos_api.hip -- host side of libpraos_hip: the context, the epoch's tables, batches and their
// uploads / downloads, and the Praos and TPraos verify calls that compose them.  The transfers are
// praos_xfer.hip, block, Byron and chunk validation praos_blocks.hip, the batches a context keeps
// between calls (the replay's entry points, the stored-bytes pipeline) praos_stream.hip, the crypto
// step's scheduler praos_run.hip, the sequential part of Praos.updateChainDepState praos_fold.hip,
// generator and debug entry points praos_debug.hip; they share praos_ctx / praos_batch through
// api_internal.hpp.  The kernels sit in the k_* modules behind launch.hpp (no relocatable device
// code).
#include "api_internal.hpp"

using namespace praos_impl;

static void free_spare(praos_ctx* c) {
  for (void* p : c->spare)
    if (p) (void)hipFree(p);
  c->spare.clear();
  c->spare_sz.clear();
}

extern "C" {

int praos_abi_version(void) { return PRAOS_ABI_VERSION; }

const char* praos_last_error(praos_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }

// streams and events of a context (praos_open, and the pipeline's second engine)
static bool open_streams(praos_ctx* c) {
  if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    c->stream = nullptr;
    return false;
  }
  for (auto& e : c->ev) (void)hipEventCreate(&e);
  for (auto& e : c->side_ev) (void)hipEventCreate(&e);
  for (auto& e : c->miss_ev) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
  for (auto& e : c->mdone_ev) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
  (void)hipEventCreateWithFlags(&c->v_ev, hipEventDisableTiming);
  (void)hipEventCreateWithFlags(&c->v2_ev, hipEventDisableTiming);
  (void)hipEventCreate(&c->v0_ev);
  (void)hipEventCreateWithFlags(&c->u_ev, hipEventDisableTiming);
  (void)hipEventCreateWithFlags(&c->vrec_ev, hipEventDisableTiming);
  sched_knobs_from_env(c->knobs);                     // the schedule's knobs: sched.hpp's table
  if (const char* e = std::getenv("PRAOS_POOL_KEYS")) (void)praos_set_option(c, PRAOS_OPT_POOL_KEYS, std::atoi(e));
  (void)hipEventCreate(&c->v1_ev);
  (void)hipEventCreate(&c->kc0_ev);
  (void)hipEventCreate(&c->kc1_ev);
  for (auto& e : c->up_ev) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
  for (auto& e : c->done_ev) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
  for (auto& p : c->pcall) (void)hipEventCreateWithFlags(&p.ev, hipEventDisableTiming);
  // side streams: [0] OCert, [1] KES, [2] VRF.  The VRF stream (the longest chain of
  // work) gets the device's greatest priority, so its waves dispatch first and the
  // KES / OCert / miss kernels fill the remaining slots and its tail (C5: 15.8 ->
  // 14.3 ms per 432k-header step, round-2 A/B).  PRAOS_SIDE_PRIO = three
  // digits overriding that (1 = greatest, 0 = default priority), an A/B knob.
  {
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    const char* pe = std::getenv("PRAOS_SIDE_PRIO");
    if (!pe || std::strlen(pe) != 3) pe = "001";
    for (int k = 0; k < 3; k++) {
      const bool hi = pe && std::strlen(pe) == 3 && pe[k] == '1';
      (void)hipStreamCreateWithPriority(&c->side[k], hipStreamNonBlocking, hi ? greatest : least);
      // each kind's misses get a stream of their own at the same priority: a handful of
      // uncached verifies is one full-length chain of latency, and three of them in a
      // row on one stream were the critical path of small batches (54k headers: k_kes
      // 2.1 ms -> k_vrf 3.4 ms -> k_ocert 1.6 ms, profiles/r03b/timeline.txt)
      (void)hipStreamCreateWithPriority(&c->mside[k], hipStreamNonBlocking, hi ? greatest : least);
    }
    // the VRF's stage V is the longest chain of a batch and starts at once: greatest priority
    // (PRAOS_V_PRIO=0: least, an A/B knob)
    const char* vp = std::getenv("PRAOS_V_PRIO");
    const int vprio = (vp && std::atoi(vp) == 0) ? least : greatest;
    (void)hipStreamCreateWithPriority(&c->vstream, hipStreamNonBlocking, vprio);
    (void)hipStreamCreateWithPriority(&c->vstream2, hipStreamNonBlocking, vprio);
    // the copy stream (uploads; the replay's decode): PRAOS_CSTREAM_PRIO=1 at the greatest priority
    const char* cp = std::getenv("PRAOS_CSTREAM_PRIO");
    // (the copy / decode / download streams on hardware queues of their own -- CU-masked streams,
    // every CU enabled -- or GPU_MAX_HW_QUEUES=16 were measured for the streaming form: no gain,
    // 13.2-13.4 -> 13.5-13.7 ms per call, profiles/r06/l_stream)
    (void)hipStreamCreateWithPriority(&c->cstream, hipStreamNonBlocking, (cp && std::atoi(cp) == 1) ? greatest : least);
    (void)hipStreamCreateWithFlags(&c->dstream, hipStreamNonBlocking);
    (void)hipStreamCreateWithFlags(&c->decstream, hipStreamNonBlocking);
  }
  return true;
}

praos_ctx* praos_open(int device) {
  if (device == PRAOS_HOST_ONLY) {
    praos_ctx* c = new praos_ctx();
    c->device = -1;
    return c;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    fprintf(stderr, "praos_open: no HIP device %d (count %d)\n", device, ndev);
    return nullptr;
  }
  praos_ctx* c = new praos_ctx();
  c->device = device;
  if (!open_streams(c)) {
    praos_close(c);
    return nullptr;
  }
  if (hipMalloc(&c->btab, BCOMB_TABLES * BTAB_N * NIELS_BYTES) != hipSuccess) {
    c->btab = nullptr;
    praos_close(c);
    return nullptr;
  }
  // (the check below reads the thread's last error: drop one that an earlier call of this thread
  // left, such as an argument check on a host-only context)
  (void)hipGetLastError();
  launch_init_btab(dim3(BCOMB_TABLES * BTAB_N / 256), dim3(256), c->stream, c->btab);
  if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) {
    fprintf(stderr, "praos_open: init kernel failed\n");
    praos_close(c);
    return nullptr;
  }
  return c;
}

}  // extern "C"

namespace praos_impl {

// The radix-2^16 comb of the cached-key chains (48 MB, scalarmult.hpp C16_T x C16_N):
// built on the first run that uses a key cache, on the ctx stream (the kernels that
// read it are ordered after it), then kept for the context's lifetime.
int ensure_bcomb16(praos_ctx* c) {
  if (c->bcomb16) return PRAOS_OK;
  ge_niels* t = nullptr;
  if (hipMalloc(&t, C16_TABLES * C16_ENTRIES * NIELS_BYTES) != hipSuccess) {
    c->err = "praos: radix-2^16 comb allocation (48 MB) failed";
    return PRAOS_E_OOM;
  }
  launch_init_bcomb16(c->stream, c->btab, t);
  if (hipGetLastError() != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(t);
    c->err = "praos: comb init launch failed";
    return PRAOS_E_HIP;
  }
  c->bcomb16 = t;
  return PRAOS_OK;
}

void decode_launch(const praos_batch* b, hipStream_t st, const uint8_t* arena, size_t arena_len, const uint64_t* hoff,
                   const uint32_t* hlen, size_t first, size_t upto) {
  launch_decode_praos(dim3(nblocks(upto - first, NT)), dim3(NT), st, upto, arena, arena_len, hoff, hlen,
                      b->slot, b->cold_vk, b->vrf_vk, b->vrf_out, b->vrf_proof, b->hot_vk, b->ocert_sig, b->kes_sig,
                      b->ocert_n, b->ocert_c0, b->body_off, b->body_len, b->body, b->block_no, b->prev_hash,
                      b->prev_genesis, b->body_size, b->body_hash, b->prot_major, b->prot_minor, b->header_hash,
                      b->dec_status, b->is_block ? 1 : (b->tp_only ? 2 : 0), b->signed_stride, b->lead_out,
                      b->lead_proof, first);
}

// k_decode_praos over a from-bytes batch, on the ctx stream
int batch_decode(praos_ctx* c, praos_batch* b) {
  if (b->n == 0) return PRAOS_OK;
  decode_launch(b, c->stream, b->arena, b->arena_len, b->hoff, b->hlen, 0, b->n);
  return hipGetLastError() == hipSuccess ? PRAOS_OK : PRAOS_E_HIP;
}

int32_t overlay_class(const praos_ctx* c, uint64_t slot) {
  if (!c->ovl_on || slot < c->ovl_base) return -1;
  const uint64_t first = c->ovl_base + (slot - c->ovl_base) / c->ovl_len * c->ovl_len;
  const unsigned __int128 x = slot - first;
  auto step = [&](unsigned __int128 v) {             // ceiling (v * d), v * d_num < 2^128
    const unsigned __int128 num = v * c->ovl_d_num;
    return (num + c->ovl_d_den - 1) / c->ovl_d_den;
  };
  const unsigned __int128 position = step(x);
  if (!(position < step(x + 1))) return -1;
  if (position % c->ovl_asc_inv != 0) return -2;
  return (int32_t)((position / c->ovl_asc_inv) % c->gen_delegs.size());
}

}  // namespace praos_impl

extern "C" {

static void free_epoch(praos_ctx* c) {
  (void)hipFree(c->d_pool_hash); (void)hipFree(c->d_pool_vrf); (void)hipFree(c->d_pool_x);
  (void)hipFree(c->d_pool_map); (void)hipFree(c->d_eta0);
  c->d_pool_hash = nullptr; c->d_pool_vrf = nullptr; c->d_pool_x = nullptr; c->d_pool_map = nullptr; c->d_eta0 = nullptr;
}

void praos_close(praos_ctx* c) {
  if (!c) return;
  if (c->device < 0) { delete c; return; }
  (void)hipSetDevice(c->device);
  (void)praos_verify_drain(c);                 // submitted calls' outputs are written before the close
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  free_epoch(c);
  (void)hipFree(c->d_gen);
  (void)hipFree(c->btab);
  (void)hipFree(c->bcomb16);
  (void)hipFree(c->txw_tabs);
  for (auto& ps : c->pks) {
    for (void* q : {(void*)ps.pkey, (void*)ps.count, (void*)ps.base, (void*)ps.entry_rep, (void*)ps.entry_pos,
                    (void*)ps.kinfo, (void*)ps.pentry, (void*)ps.ktab, (void*)ps.scnt, (void*)ps.spos})
      (void)hipFree(q);
  }
  free_spare(c);
  c->pool.reset();
  for (int k = 0; k < 2; k++) {
    if (c->pin[k]) (void)hipHostFree(c->pin[k]);
    if (c->pin_ev[k]) (void)hipEventDestroy(c->pin_ev[k]);
  }
  if (c->zero_h) (void)hipHostFree(c->zero_h);
  for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : c->side_ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : c->miss_ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : c->mdone_ev) if (e) (void)hipEventDestroy(e);
  for (auto& st : c->side) if (st) (void)hipStreamDestroy(st);
  for (auto& st : c->mside) if (st) (void)hipStreamDestroy(st);
  if (c->vstream) (void)hipStreamDestroy(c->vstream);
  if (c->vstream2) (void)hipStreamDestroy(c->vstream2);
  if (c->v2_ev) (void)hipEventDestroy(c->v2_ev);
  if (c->v_ev) (void)hipEventDestroy(c->v_ev);
  if (c->v0_ev) (void)hipEventDestroy(c->v0_ev);
  if (c->u_ev) (void)hipEventDestroy(c->u_ev);
  if (c->vrec_ev) (void)hipEventDestroy(c->vrec_ev);
  if (c->v1_ev) (void)hipEventDestroy(c->v1_ev);
  if (c->kc0_ev) (void)hipEventDestroy(c->kc0_ev);
  if (c->kc1_ev) (void)hipEventDestroy(c->kc1_ev);
  if (c->cstream) (void)hipStreamSynchronize(c->cstream);
  stream_close(c);                             // the kept batches, the pipeline's batches and events
  if (c->cstream) (void)hipStreamDestroy(c->cstream);
  if (c->dstream) (void)hipStreamDestroy(c->dstream);
  if (c->decstream) (void)hipStreamDestroy(c->decstream);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

}  // extern "C"

static void pool_tables_free(rp_view* v) {
  if (!v || v->device < 0) return;
  (void)hipFree(v->d_hash); (void)hipFree(v->d_vrf); (void)hipFree(v->d_x); (void)hipFree(v->d_map);
  v->d_hash = v->d_vrf = v->d_x = nullptr;
  v->d_map = nullptr;
}

// Builds v's host map and, for device >= 0, its device tables (on the current device).  On
// failure nothing is left allocated and err says why.
static int pool_tables_build(rp_view* v, int device, const praos_pool* pools, uint32_t npools,
                             const praos_params* params, std::string* err) {
  std::vector<int32_t> order(npools);
  for (uint32_t i = 0; i < npools; i++) order[i] = (int32_t)i;
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    return std::memcmp(pools[a].hash28, pools[b].hash28, 28) < 0;
  });
  std::vector<uint32_t> h(7 * (size_t)std::max(1u, npools)), vr(8 * (size_t)std::max(1u, npools)),
      x(4 * (size_t)std::max(1u, npools));
  std::map<std::string, int32_t> by_hash;
  for (uint32_t s = 0; s < npools; s++) {
    const praos_pool& p = pools[order[s]];
    std::memcpy(&h[7 * s], p.hash28, 28);
    std::memcpy(&vr[8 * s], p.vrf_hash32, 32);
    uint8_t xr[16];
    if (!praos_host::leader_x_raw(xr, p.sigma_fp, params->c_raw)) {
      *err = "sigma * activeSlotLog out of range (x_raw > 16 * 10^34)";
      return PRAOS_E_ARG;
    }
    std::memcpy(&x[4 * s], xr, 16);
    by_hash[std::string((const char*)p.hash28, 28)] = order[s];
  }
  v->device = device;
  if (device >= 0) {
    bool ok = hipMalloc(&v->d_hash, h.size() * 4) == hipSuccess && hipMalloc(&v->d_vrf, vr.size() * 4) == hipSuccess &&
              hipMalloc(&v->d_x, x.size() * 4) == hipSuccess &&
              hipMalloc(&v->d_map, std::max<size_t>(1, npools) * 4) == hipSuccess;
    ok = ok && hipMemcpy(v->d_hash, h.data(), h.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(v->d_vrf, vr.data(), vr.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(v->d_x, x.data(), x.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         (!npools || hipMemcpy(v->d_map, order.data(), npools * 4, hipMemcpyHostToDevice) == hipSuccess);
    if (!ok) {
      pool_tables_free(v);
      *err = "pool tables: device allocation / copy failed";
      return PRAOS_E_OOM;
    }
  }
  v->npools = npools;
  v->pools.assign(pools, pools + npools);
  v->by_hash.swap(by_hash);
  return PRAOS_OK;
}

rp_view* rp_view_make(praos_ctx* c, const praos_pool* pools, uint32_t npools, const praos_params* params,
                      bool device) {
  if (!c || !params || (npools && !pools)) return nullptr;
  if (device && c->device < 0) return nullptr;
  if (device) (void)hipSetDevice(c->device);
  rp_view* v = new rp_view;
  std::string err;
  if (pool_tables_build(v, device ? c->device : -1, pools, npools, params, &err) != PRAOS_OK) {
    c->err = err;
    delete v;
    return nullptr;
  }
  return v;
}

void rp_view_free(praos_ctx* c, rp_view* v) {
  if (!v) return;
  if (c && v->device >= 0) (void)hipSetDevice(v->device);
  pool_tables_free(v);
  delete v;
}

rp_tables rp_tables_get(const praos_ctx* c) {
  return {c->npools, c->d_pool_hash, c->d_pool_vrf, c->d_pool_x, c->d_pool_map};
}

void rp_tables_set(praos_ctx* c, const rp_tables& t) {
  c->npools = t.npools;
  c->d_pool_hash = t.hash; c->d_pool_vrf = t.vrf; c->d_pool_x = t.x; c->d_pool_map = t.map;
}

rp_tables rp_view_tables(const rp_view* v) { return {v->npools, v->d_hash, v->d_vrf, v->d_x, v->d_map}; }

extern "C" {

int praos_set_epoch(praos_ctx* c, const uint8_t eta0[32], const praos_pool* pools, uint32_t npools,
                    const praos_params* params) {
  if (!c || !params || (npools && !pools) || params->slots_per_kes_period == 0) return PRAOS_E_ARG;
  // The installed ledger view again (a replay call per batch of epochs, db-analyser's per-epoch
  // calls under an unchanged PoolDistr): only the epoch nonce changes.  The memcmp over the
  // caller's structs sees every byte of them, so neither may have padding (uninitialised padding
  // would make equal views compare unequal and take the slow path):
  static_assert(sizeof(praos_params) == sizeof(praos_params::slots_per_kes_period) + sizeof(praos_params::max_kes_evo) +
                                            sizeof(praos_params::f_is_one) + sizeof(praos_params::vrf_check_output) +
                                            sizeof(praos_params::c_raw),
                "praos_params has padding: praos_set_epoch compares it with memcmp");
  static_assert(sizeof(praos_pool) == sizeof(praos_pool::hash28) + sizeof(praos_pool::vrf_hash32) +
                                          sizeof(praos_pool::sigma_fp),
                "praos_pool has padding: praos_set_epoch compares it with memcmp");
  if (c->have_epoch && c->device >= 0 && npools == c->epoch_pools.size() &&
      std::memcmp(params, &c->epoch_params, sizeof *params) == 0 &&
      (npools == 0 || std::memcmp(pools, c->epoch_pools.data(), npools * sizeof *pools) == 0)) {
    if ((eta0 == nullptr) == c->eta0_neutral && (eta0 == nullptr || std::memcmp(eta0, c->eta0, 32) == 0))
      return PRAOS_OK;                            // the same nonce too: nothing to change
  }
  if (std::any_of(std::begin(c->pcall), std::end(c->pcall), [](const praos_ctx::PipeCall& p) { return p.active; })) {
    // submitted calls (praos_verify_header_bytes_submit) read the installed view and nonce until
    // they end: their outputs first
    const int r = praos_verify_drain(c);
    if (r != PRAOS_OK) return r;
  }
  if (c->have_epoch && c->device >= 0 && npools == c->epoch_pools.size() &&
      std::memcmp(params, &c->epoch_params, sizeof *params) == 0 &&
      (npools == 0 || std::memcmp(pools, c->epoch_pools.data(), npools * sizeof *pools) == 0)) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // no run in flight reads the old nonce
    uint32_t e0[8] = {0};
    if (eta0) std::memcpy(e0, eta0, 32);
    HIPCHK(c, hipMemcpy(c->d_eta0, e0, 32, hipMemcpyHostToDevice));
    c->eta0_neutral = eta0 == nullptr;
    std::memset(c->eta0, 0, 32);
    if (eta0) std::memcpy(c->eta0, eta0, 32);
    return PRAOS_OK;
  }
  // Validate and build every table first; the context is only touched once all of it
  // succeeded (a failed call leaves NO epoch: runs return PRAOS_E_STATE until the next
  // successful praos_set_epoch).
  if (c->device >= 0) {
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipStreamSynchronize(c->stream);      // no run in flight reads the old tables
    free_epoch(c);
  }
  c->have_epoch = false;
  c->npools = 0;
  c->pools.clear();
  c->pool_by_hash.clear();
  rp_view v;
  std::string err;
  int r = pool_tables_build(&v, c->device, pools, npools, params, &err);
  if (r != PRAOS_OK) { c->err = err; return r; }
  if (c->device >= 0) {
    uint32_t e0[8] = {0};
    if (eta0) std::memcpy(e0, eta0, 32);
    if (hipMalloc(&c->d_eta0, 32) != hipSuccess ||
        hipMemcpy(c->d_eta0, e0, 32, hipMemcpyHostToDevice) != hipSuccess) {
      pool_tables_free(&v);
      (void)hipFree(c->d_eta0);
      c->d_eta0 = nullptr;
      c->err = "praos_set_epoch: device allocation / copy failed";
      return PRAOS_E_OOM;
    }
    c->d_pool_hash = v.d_hash; c->d_pool_vrf = v.d_vrf; c->d_pool_x = v.d_x; c->d_pool_map = v.d_map;
  }
  c->params = *params;
  c->eta0_neutral = eta0 == nullptr;
  std::memset(c->eta0, 0, 32);
  if (eta0) std::memcpy(c->eta0, eta0, 32);
  c->npools = npools;
  c->pools.swap(v.pools);
  c->pool_by_hash.swap(v.by_hash);
  c->epoch_pools.assign(pools, pools + npools);
  c->epoch_params = *params;
  c->have_epoch = true;
  return PRAOS_OK;
}

void praos_batch_free(praos_ctx* c, praos_batch* b) {
  if (!b) return;
  if (c && c->device >= 0 && b->owner == c) {
    // keep the buffers for the next batch (its kernels are ordered after this one's on
    // the ctx stream, so no wait is needed); drop the older spares it did not take
    (void)hipSetDevice(c->device);
    free_spare(c);
    c->spare.swap(b->owned);
    c->spare_sz.swap(b->owned_sz);
    delete b;
    return;
  }
  if (c) (void)hipSetDevice(c->device);
  for (void* p : b->owned) (void)hipFree(p);
  delete b;
}

// one public-key cache (k_keys.hip) for batches of up to n items
static bool alloc_keycache(praos_batch* b, praos_batch::KeyCache& k, size_t n, bool vrf = false) {
  bool ok = true;
  k.cap = 256;
  while (k.cap < 2 * n) k.cap <<= 1;
  k.max_entries = (uint32_t)std::min<size_t>(n / 2 + 1, KC_MAX_ENTRIES);
  ok &= dalloc(b, &k.slot_rep, 4 * (size_t)k.cap) == hipSuccess;
  ok &= dalloc(b, &k.slot_cnt, 4 * (size_t)k.cap) == hipSuccess;
  ok &= dalloc(b, &k.slot_entry, 4 * (size_t)k.cap) == hipSuccess;
  ok &= dalloc(b, &k.item_slot, 4 * n) == hipSuccess;
  ok &= dalloc(b, &k.item_entry, 4 * n) == hipSuccess;
  ok &= dalloc(b, &k.hit, 4 * n) == hipSuccess;
  ok &= dalloc(b, &k.miss, 4 * n) == hipSuccess;
  ok &= dalloc(b, &k.counters, 16) == hipSuccess;
  ok &= dalloc(b, &k.entry_rep, 4 * (size_t)k.max_entries) == hipSuccess;
  ok &= dalloc(b, &k.entry_pos, 4 * (size_t)k.max_entries) == hipSuccess;
  ok &= dalloc(b, &k.kinfo, 36 * (size_t)k.max_entries) == hipSuccess;
  ok &= dalloc(b, (uint8_t**)&k.ktab, KT_BYTES * k.max_entries) == hipSuccess;
  ok &= dalloc(b, &k.rep_ok, (size_t)k.max_entries) == hipSuccess;
  if (vrf) ok &= dalloc(b, &k.vrec, 4 * (size_t)VREC_WORDS * k.max_entries) == hipSuccess;
  return ok;
}

// device buffers of a batch: header SoA, body arena, outputs, key caches
static bool alloc_soa(praos_batch* b, size_t n, size_t body_arena_bytes) {
  bool ok = true;
  ok &= dalloc(b, &b->slot, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->ocert_n, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->ocert_c0, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->body_off, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->body_len, 4 * n) == hipSuccess;
  ok &= dalloc(b, &b->cold_vk, 32 * n) == hipSuccess;
  ok &= dalloc(b, &b->vrf_vk, 32 * n) == hipSuccess;
  ok &= dalloc(b, &b->vrf_out, 64 * n) == hipSuccess;
  ok &= dalloc(b, &b->vrf_proof, 80 * n) == hipSuccess;
  ok &= dalloc(b, &b->hot_vk, 32 * n) == hipSuccess;
  ok &= dalloc(b, &b->ocert_sig, 64 * n) == hipSuccess;
  ok &= dalloc(b, &b->kes_sig, 448 * n) == hipSuccess;
  ok &= dalloc(b, &b->body, body_arena_bytes) == hipSuccess;
  ok &= dalloc(b, &b->bits, 2 * n) == hipSuccess;
  ok &= dalloc(b, &b->bits3, 6 * n) == hipSuccess;
  ok &= dalloc(b, &b->pool_idx, 4 * n) == hipSuccess;
  ok &= dalloc(b, &b->pool_sorted, 4 * n) == hipSuccess;
  ok &= dalloc(b, &b->beta, 64 * n) == hipSuccess;
  ok &= dalloc(b, &b->leader, 32 * n) == hipSuccess;
  ok &= dalloc(b, &b->nonce, 32 * n) == hipSuccess;
  ok &= dalloc(b, (uint8_t**)&b->tab_ocert, LT_ED_B * n) == hipSuccess;
  ok &= dalloc(b, (uint8_t**)&b->tab_kes, LT_ED_B * n) == hipSuccess;
  ok &= dalloc(b, (uint8_t**)&b->tab_vrf, LT_VRF_B * n) == hipSuccess;
  ok &= dalloc(b, (uint8_t**)&b->tab_vrfu, LT_ED_B * n) == hipSuccess;
  ok &= dalloc(b, &b->vrf_mid, VRF_MID_BYTES * n) == hipSuccess;
  ok &= dalloc(b, &b->kes_leaf, 32 * n) == hipSuccess;
  b->dd_cap = 256;
  while (b->dd_cap < 2 * n) b->dd_cap <<= 1;
  ok &= dalloc(b, &b->dd_slot, 4 * (size_t)b->dd_cap) == hipSuccess;
  ok &= dalloc(b, &b->dd_item_rep, 4 * n) == hipSuccess;
  ok &= dalloc(b, &b->dd_reps, 4 * n) == hipSuccess;
  ok &= dalloc(b, &b->dd_counters, 16) == hipSuccess;
  ok &= dalloc(b, &b->dd_ok, n) == hipSuccess;
  for (auto& k : b->kc) ok &= alloc_keycache(b, k, n, &k == &b->kc[1]);
  return ok;
}

praos_batch* praos_batch_upload(praos_ctx* c, const praos_headers* h) {
  if (!c || !h) return nullptr;
  if (hipSetDevice(c->device) != hipSuccess) return nullptr;
  praos_batch* b = new praos_batch();
  b->owner = c;
  const size_t n = h->n;
  b->n = n;
  // repack bodies 8-byte aligned (the SHA-512 feeder reads 64-bit words)
  std::vector<uint64_t>& off = c->h_off;
  off.resize(n);
  size_t total = 0;
  bool bad_range = false;
  for (size_t i = 0; i < n; i++) {
    off[i] = total;
    if (h->body_off[i] > h->body_bytes_len || h->body_len[i] > h->body_bytes_len - h->body_off[i]) bad_range = true;
    total += (h->body_len[i] + 7) & ~(size_t)7;
  }
  auto tr0 = std::chrono::steady_clock::now();
  if (c->h_arena_cap < total + 16) {
    c->h_arena.reset(new uint8_t[total + 16]);
    c->h_arena_cap = total + 16;
  }
  uint8_t* const arena = c->h_arena.get();
  std::vector<uint32_t>& len = c->h_len;
  len.resize(n);
  auto repack = [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; i++) {
      const bool ok = h->body_off[i] <= h->body_bytes_len && h->body_len[i] <= h->body_bytes_len - h->body_off[i];
      len[i] = ok ? h->body_len[i] : 0xffffffffu;  // marks out-of-range (kernel flags PRAOS_BIT_INPUT)
      const size_t pad = ((size_t)h->body_len[i] + 7) & ~(size_t)7;
      uint8_t* d = arena + off[i];
      if (ok) std::memcpy(d, h->body_bytes + h->body_off[i], h->body_len[i]);
      if (pad > (ok ? (size_t)h->body_len[i] : 0)) std::memset(d + (ok ? h->body_len[i] : 0), 0, pad - (ok ? h->body_len[i] : 0));
    }
  };
  if (n >= 65536 && stage_init(c)) {
    const unsigned nt = c->pool->size();
    c->pool->run([&](unsigned t) { repack(n * t / nt, n * (t + 1) / nt); });
  } else {
    repack(0, n);
  }
  std::memset(arena + total, 0, 16);
  if (std::getenv("PRAOS_TRACE_UPLOAD"))
    fprintf(stderr, "upload: repack %.2f ms\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count());
  (void)bad_range;
  b->body_bytes_len = total;
  static const bool trace = std::getenv("PRAOS_TRACE_UPLOAD") != nullptr;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto t0 = now();
  bool ok = alloc_soa(b, n, total + 16);
  if (!ok) { c->err = "device allocation failed"; praos_batch_free(c, b); return nullptr; }
  if (trace) fprintf(stderr, "upload: alloc %.2f ms\n", std::chrono::duration<double, std::milli>(now() - t0).count());
  auto up = [&](void* d, const void* s, size_t bytes) {
    auto t = now();
    if (bytes) ok &= h2d(c, d, s, bytes) == hipSuccess;
    if (trace) fprintf(stderr, "upload: %zu bytes %.2f ms\n", bytes, std::chrono::duration<double, std::milli>(now() - t).count());
  };
  up(b->slot, h->slot, 8 * n);
  up(b->ocert_n, h->ocert_n, 8 * n);
  up(b->ocert_c0, h->ocert_c0, 8 * n);
  up(b->body_off, off.data(), 8 * n);
  up(b->body_len, len.data(), 4 * n);
  up(b->cold_vk, h->cold_vk, 32 * n);
  up(b->vrf_vk, h->vrf_vk, 32 * n);
  up(b->vrf_out, h->vrf_out, 64 * n);
  up(b->vrf_proof, h->vrf_proof, 80 * n);
  up(b->hot_vk, h->hot_vk, 32 * n);
  up(b->ocert_sig, h->ocert_sig, 64 * n);
  up(b->kes_sig, h->kes_sig, 448 * n);
  up(b->body, arena, total + 16);
  auto ts = now();
  ok &= hipStreamSynchronize(c->stream) == hipSuccess;
  if (trace) fprintf(stderr, "upload: final sync %.2f ms, from the repack %.2f ms\n",
                     std::chrono::duration<double, std::milli>(now() - ts).count(),
                     std::chrono::duration<double, std::milli>(now() - tr0).count());
  if (!ok) { c->err = "upload failed"; praos_batch_free(c, b); return nullptr; }
  return b;
}

static praos_batch* upload_bytes_impl(praos_ctx* c, const praos_header_bytes* in, bool tpraos);

praos_batch* praos_batch_upload_bytes(praos_ctx* c, const praos_header_bytes* in) {
  return upload_bytes_impl(c, in, false);
}

}  // extern "C"

namespace praos_impl {

// device buffers of a from-bytes batch of n headers over an arena of bytes_len bytes
// (owner == nullptr: fresh allocations, not taken from / given back to the spare list)
praos_batch* bytes_batch_alloc(praos_ctx* c, size_t n, size_t bytes_len, bool tpraos, praos_ctx* owner) {
  praos_batch* b = new praos_batch();
  b->owner = owner;
  b->n = n;
  b->from_bytes = true;
  b->arena_len = bytes_len;
  b->tp_only = tpraos;
  b->signed_stride = tpraos ? TP_SIGNED_STRIDE : PRAOS_SIGNED_STRIDE;
  b->body_bytes_len = (size_t)b->signed_stride * n;
  bool ok = alloc_soa(b, n, b->body_bytes_len + 16);
  if (tpraos) {
    ok &= dalloc(b, &b->lead_out, 64 * n) == hipSuccess;
    ok &= dalloc(b, &b->lead_proof, 80 * n) == hipSuccess;
    ok &= dalloc(b, &b->beta_l, 64 * n) == hipSuccess;
  }
  ok &= dalloc(b, &b->arena, arena_room(bytes_len)) == hipSuccess;
  ok &= dalloc(b, &b->hoff, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->hlen, 4 * n) == hipSuccess;
  ok &= dalloc(b, &b->block_no, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->prot_major, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->prot_minor, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->body_size, 4 * n) == hipSuccess;
  ok &= dalloc(b, &b->prev_hash, 32 * n) == hipSuccess;
  ok &= dalloc(b, &b->prev_genesis, n) == hipSuccess;
  ok &= dalloc(b, &b->body_hash, 32 * n) == hipSuccess;
  ok &= dalloc(b, &b->header_hash, 32 * n) == hipSuccess;
  ok &= dalloc(b, &b->dec_status, 2 * n) == hipSuccess;
  if (!ok) {
    c->err = "device allocation failed";
    for (void* p : b->owned) (void)hipFree(p);
    delete b;
    return nullptr;
  }
  return b;
}

// arena upload of a from-bytes batch (zero padding for ld64u, then the bytes), on the ctx stream
int arena_upload(praos_ctx* c, praos_batch* b, const uint8_t* bytes, size_t bytes_len) {
  HIPCHK(c, hipMemsetAsync(b->arena + bytes_len, 0, arena_pad(bytes_len), c->stream));
  if (bytes_len) HIPCHK(c, h2d(c, b->arena, bytes, bytes_len));
  return PRAOS_OK;
}

}  // namespace praos_impl

extern "C" {

static praos_batch* upload_bytes_impl(praos_ctx* c, const praos_header_bytes* in, bool tpraos) {
  if (!c || !in || (in->n && (!in->off || !in->len || (!in->bytes && in->bytes_len)))) return nullptr;
  if (praos_host_only_(c) || hipSetDevice(c->device) != hipSuccess) return nullptr;
  const size_t n = in->n;
  praos_batch* b = bytes_batch_alloc(c, n, in->bytes_len, tpraos, c);
  if (!b) return nullptr;
  bool ok = arena_upload(c, b, in->bytes, in->bytes_len) == PRAOS_OK;
  if (n) {
    ok &= hipMemcpyAsync(b->hoff, in->off, 8 * n, hipMemcpyHostToDevice, c->stream) == hipSuccess;
    ok &= hipMemcpyAsync(b->hlen, in->len, 4 * n, hipMemcpyHostToDevice, c->stream) == hipSuccess;
  }
  ok &= hipStreamSynchronize(c->stream) == hipSuccess;
  if (!ok) { c->err = "upload failed"; praos_batch_free(c, b); return nullptr; }
  return b;
}

int praos_batch_stats(praos_ctx* c, praos_batch* b, uint32_t out[9]) {
  if (!c || !b || !out) return PRAOS_E_ARG;
  for (int k = 0; k < 9; k++) out[k] = 0;
  if (!b->kc_used) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int t = 0; t < 3; t++) {
    uint32_t cnt[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpy(cnt, b->kc[t].counters, 16, hipMemcpyDeviceToHost));
    out[3 * t] = std::min(cnt[0], b->kc[t].emax ? b->kc[t].emax : b->kc[t].max_entries);
    out[3 * t + 1] = cnt[1];
    out[3 * t + 2] = cnt[2];
    if (b->kc[t].wide.min_uses) {      // the wide tier's hits are hits too
      uint32_t w[4] = {0, 0, 0, 0};
      HIPCHK(c, hipMemcpy(w, b->kc[t].wide.wcnt, 16, hipMemcpyDeviceToHost));
      out[3 * t + 1] += w[1];
    }
  }
  return PRAOS_OK;
}

int praos_batch_wide_stats(praos_ctx* c, praos_batch* b, uint32_t out[2]) {
  if (!c || !b || !out) return PRAOS_E_ARG;
  out[0] = out[1] = 0;
  const praos_batch::KeyCache& k = b->kc[1];
  if (!b->kc_used || !k.wide.min_uses) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  uint32_t w[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpy(w, k.wide.wcnt, 16, hipMemcpyDeviceToHost));
  out[0] = std::min(w[0], k.wide.cap);
  out[1] = w[1];
  return PRAOS_OK;
}

int praos_batch_dedup_stats(praos_ctx* c, praos_batch* b, uint32_t out[2]) {
  if (!c || !b || !out) return PRAOS_E_ARG;
  out[0] = 0;
  out[1] = (uint32_t)b->n;
  if (!b->dd_used) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, b->dd_counters, 4, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_set_option(praos_ctx* c, int opt, int value) {
  if (!c) return PRAOS_E_ARG;
  if (opt == PRAOS_OPT_CONCURRENT) { c->concurrent = value != 0; return PRAOS_OK; }
  if (opt == PRAOS_OPT_KERNELS) { c->kernels = value & 7; return PRAOS_OK; }
  if (opt == PRAOS_OPT_KEYCACHE) { c->keycache = value < 0 ? 0 : value; return PRAOS_OK; }
  if (opt == PRAOS_OPT_DEDUP) { c->dedup = value != 0; return PRAOS_OK; }
  if (opt == PRAOS_OPT_PIPELINE) { c->pipeline = value < 0 ? 0 : std::min(value, PIPE_MAX); return PRAOS_OK; }
  if (opt == PRAOS_OPT_KES_PAIR) { c->knobs.kes_pair = value < 0 ? -1 : value; return PRAOS_OK; }
  if (opt == PRAOS_OPT_KES_NOCACHE) { c->knobs.kes_nocache = value < 0 ? KES_NOCACHE_BATCH : (size_t)value; return PRAOS_OK; }
  if (opt == PRAOS_OPT_POOL_KEYS) {
    c->pool_keys = value < 0 ? -1 : (value != 0);
    if (value == 2) c->pk_reset[0] = c->pk_reset[1] = true;
    return PRAOS_OK;
  }
  return PRAOS_E_ARG;
}

int praos_set_vrf_wide(praos_ctx* c, int min_uses, int max_keys) {
  if (!c) return PRAOS_E_ARG;
  c->knobs.vrf_wide = sched_clamp_vrf_wide(min_uses);
  c->knobs.vrf_wide_cap = sched_clamp_vrf_wide_cap(max_keys);
  return PRAOS_OK;
}

int praos_batch_sync(praos_ctx* c) {
  if (!c) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // per-kernel: from the common start event to each kernel's end event (with
  // concurrent streams these overlap; which = 4 is the whole run)
  float t[3] = {0, 0, 0};
  for (int k = 0; k < 3; k++) (void)hipEventElapsedTime(&t[k], c->ev[0], c->side_ev[k]);
  if (c->concurrent) {
    for (int k = 0; k < 3; k++) c->kernel_ms[k] = t[k];
  } else {
    c->kernel_ms[0] = t[0];
    c->kernel_ms[1] = t[1] - t[0];
    c->kernel_ms[2] = t[2] - t[1];
  }
  float all = 0, dec = 0;
  (void)hipEventElapsedTime(&all, c->ev[0], c->ev[4]);
  if (c->last_from_bytes) (void)hipEventElapsedTime(&dec, c->ev[5], c->ev[0]);
  c->kernel_ms[3] = all - (c->concurrent ? std::max(t[0], std::max(t[1], t[2])) : t[2]);
  c->kernel_ms[4] = all + dec;
  c->kernel_ms[5] = dec;
  c->kernel_ms[6] = 0;
  if (c->v_timed) (void)hipEventElapsedTime(&c->kernel_ms[6], c->v0_ev, c->v1_ev);
  c->kernel_ms[7] = 0;
  if (c->kes_ck_timed) (void)hipEventElapsedTime(&c->kernel_ms[7], c->kc0_ev, c->kc1_ev);
  return PRAOS_OK;
}

float praos_batch_kernel_ms(praos_ctx* c, int which) {
  if (!c || which < 0 || which > 7) return -1.f;
  return c->kernel_ms[which];
}

int praos_batch_download(praos_ctx* c, praos_batch* b, praos_out* out) {
  if (!c || !b || !out || !out->bits) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (b->n == 0) return PRAOS_OK;
  HIPCHK(c, out_cols(*out, *b, [&](void* dst, const void* src, size_t bytes) { return d2h(c, dst, src, bytes); }));
  return PRAOS_OK;
}

int praos_verify_headers(praos_ctx* c, const praos_headers* h, praos_out* out) {
  if (!c || !h || !out || !out->bits) return PRAOS_E_ARG;
  if (!c->have_epoch) return PRAOS_E_STATE;
  if (h->n == 0) return PRAOS_OK;
  praos_batch* b = praos_batch_upload(c, h);
  if (!b) return PRAOS_E_OOM;
  int r = praos_batch_run(c, b);
  if (r == PRAOS_OK) r = praos_batch_sync(c);
  if (r == PRAOS_OK) r = praos_batch_download(c, b, out);
  praos_batch_free(c, b);
  return r;
}

int praos_batch_decode(praos_ctx* c, praos_batch* b) {
  if (!c || !b || !b->from_bytes) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const int r = batch_decode(c, b);
  if (r != PRAOS_OK) { c->err = "decode launch failed"; return r; }
  b->decoded = true;
  return PRAOS_OK;
}

int praos_batch_set_nonces(praos_ctx* c, praos_batch* b, const praos_nonce* etas, uint32_t k, const uint8_t* eta_idx) {
  if (!c || !b || (b->n && (!etas || !eta_idx)) || k == 0 || k > 256) return PRAOS_E_ARG;
  for (size_t i = 0; i < b->n; i++)
    if (eta_idx[i] >= k) { c->err = "eta_idx out of range"; return PRAOS_E_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<uint32_t> tab(9 * (size_t)k);
  pack_nonce_table(etas, k, tab.data());
  if (!b->eta_tab) {
    if (dalloc(b, &b->eta_tab, 9 * 4 * 256) != hipSuccess || dalloc(b, &b->eta_idx, std::max<size_t>(b->n, 1)) != hipSuccess) {
      c->err = "device allocation failed";
      return PRAOS_E_OOM;
    }
  }
  HIPCHK(c, hipMemcpyAsync(b->eta_tab, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice, c->stream));
  if (b->n) HIPCHK(c, hipMemcpyAsync(b->eta_idx, eta_idx, b->n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PRAOS_OK;
}

int praos_batch_download_decoded(praos_ctx* c, praos_batch* b, praos_decoded* d) {
  if (!c || !b || !d || !b->from_bytes) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (b->n == 0) return PRAOS_OK;
  HIPCHK(c, decoded_cols(*d, *b, [&](void* dst, const void* src, size_t bytes) { return d2h(c, dst, src, bytes); }));
  return PRAOS_OK;
}

int praos_decode_headers(praos_ctx* c, const praos_header_bytes* in, praos_decoded* out) {
  if (!c || !in || !out) return PRAOS_E_ARG;
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  if (in->n == 0) return PRAOS_OK;
  praos_batch* b = praos_batch_upload_bytes(c, in);
  if (!b) return PRAOS_E_OOM;
  int r = batch_decode(c, b);
  if (r == PRAOS_OK) r = praos_batch_download_decoded(c, b, out);
  praos_batch_free(c, b);
  return r;
}

}  // extern "C"

// ---- the context for the other host modules (replay, group, candidates, pbft): the shims that
// replay_internal.hpp declares
// error text for the other host modules of the library (praos_replay.hip)
void praos_set_error_(praos_ctx* c, const std::string& m) { if (c) c->err = m; }
// the refusal of a call that needs a device
bool praos_host_only_(praos_ctx* c) {
  if (c->device >= 0) return false;
  c->err = "host-only context: no HIP device";
  return true;
}
void praos_replay_scope_(praos_ctx* c, bool on) {
  if (!c) return;
  c->err.first_only(on);
  c->replaying = on;                                   // (set for the length of a replay call)
}

extern "C" {

// ---- TPraos overlay schedule (cardano-protocol-tpraos Rules/Overlay.hs, restated):
//   isOverlaySlot firstSlotNo d slot = step s < step (s + 1), step x = ceiling (x * d),
//     s = slot - firstSlotNo;
//   classifyOverlaySlot: position = ceiling (s * d); active iff position mod ascInv == 0,
//     ascInv = floor (1 / activeSlotVal f); genesis key = Set.elemAt ((position div ascInv)
//     mod |gkeys|) gkeys (ascending byte order of the 28-byte key hashes).
int praos_set_overlay(praos_ctx* c, const praos_overlay* ov) {
  if (!c) return PRAOS_E_ARG;
  if (!ov) {
    c->ovl_on = false;
    c->gen_delegs.clear();
    c->gen_delegate_hashes.clear();
    return PRAOS_OK;
  }
  // d = 0 keeps the genesis delegates for the OCERT counter rule only (currentIssueNo)
  if (ov->d_den == 0 || ov->d_num > ov->d_den || ov->asc_num == 0 || ov->asc_den == 0 || ov->asc_num > ov->asc_den ||
      ov->epoch_length == 0 || (ov->n_gen_delegs && !ov->gen_delegs) || (ov->d_num && ov->n_gen_delegs == 0))
    return PRAOS_E_ARG;
  std::vector<praos_gen_deleg> g(ov->gen_delegs, ov->gen_delegs + ov->n_gen_delegs);
  std::sort(g.begin(), g.end(), [](const praos_gen_deleg& a, const praos_gen_deleg& b) {
    return std::memcmp(a.genesis_hash28, b.genesis_hash28, 28) < 0;
  });
  for (size_t k = 1; k < g.size(); k++)
    if (std::memcmp(g[k - 1].genesis_hash28, g[k].genesis_hash28, 28) == 0) return PRAOS_E_ARG;   // a Map
  if (c->device >= 0 && ov->d_num) {
    std::vector<uint32_t> t(16 * g.size(), 0);
    for (size_t k = 0; k < g.size(); k++) {
      std::memcpy(&t[16 * k], g[k].delegate_hash28, 28);
      std::memcpy(&t[16 * k + 8], g[k].vrf_hash32, 32);
    }
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(c->d_gen);
    c->d_gen = nullptr;
    c->ovl_on = false;
    HIPCHK(c, hipMalloc(&c->d_gen, 4 * t.size()));
    HIPCHK(c, hipMemcpy(c->d_gen, t.data(), 4 * t.size(), hipMemcpyHostToDevice));
  }
  c->ovl_d_num = ov->d_num;
  c->ovl_d_den = ov->d_den;
  c->ovl_asc_inv = ov->asc_den / ov->asc_num;          // floor (1 / f), >= 1
  c->ovl_base = ov->epoch_base_slot;
  c->ovl_len = ov->epoch_length;
  c->gen_delegs.swap(g);
  c->gen_delegate_hashes.clear();
  for (const auto& e : c->gen_delegs) c->gen_delegate_hashes.insert(std::string((const char*)e.delegate_hash28, 28));
  c->ovl_on = ov->d_num != 0;
  return PRAOS_OK;
}

int praos_overlay_classify(praos_ctx* c, size_t n, const uint64_t* slots, int32_t* cls) {
  if (!c || (n && (!slots || !cls))) return PRAOS_E_ARG;
  for (size_t i = 0; i < n; i++) cls[i] = overlay_class(c, slots[i]);
  return PRAOS_OK;
}

static int tpraos_download(praos_ctx* c, praos_batch* b, const uint8_t* dbeta_l, praos_tpraos_out* out) {
  const size_t n = b->n;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, d2h(c, out->bits, b->bits, 2 * n));
  if (out->pool_idx) HIPCHK(c, d2h(c, out->pool_idx, b->pool_idx, 4 * n));
  if (out->beta_eta) HIPCHK(c, d2h(c, out->beta_eta, b->beta, 64 * n));
  if (out->beta_leader) HIPCHK(c, d2h(c, out->beta_leader, dbeta_l, 64 * n));
  if (out->nonce) HIPCHK(c, d2h(c, out->nonce, b->nonce, 32 * n));
  return PRAOS_OK;
}

int praos_verify_tpraos_headers(praos_ctx* c, const praos_tpraos_headers* th, praos_tpraos_out* out) {
  if (!c || !th || !out || !out->bits || !th->leader_out || !th->leader_proof) return PRAOS_E_ARG;
  if (!c->have_epoch) return PRAOS_E_STATE;
  const size_t n = th->h.n;
  if (n == 0) return PRAOS_OK;
  praos_batch* b = praos_batch_upload(c, &th->h);
  if (!b) return PRAOS_E_OOM;
  ScratchBatch scratch(c, b);
  uint8_t *dlout = nullptr, *dlproof = nullptr, *dbeta_l = nullptr;
  if (dalloc(b, &dlout, 64 * n) != hipSuccess || dalloc(b, &dlproof, 80 * n) != hipSuccess ||
      dalloc(b, &dbeta_l, 64 * n) != hipSuccess)
    return PRAOS_E_OOM;
  HIPCHK(c, hipMemcpy(dlout, th->leader_out, 64 * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dlproof, th->leader_proof, 80 * n, hipMemcpyHostToDevice));
  b->tp_only = true;
  b->lead_out = dlout;
  b->lead_proof = dlproof;
  b->beta_l = dbeta_l;
  const int r = praos_batch_run(c, b);
  return r == PRAOS_OK ? tpraos_download(c, b, dbeta_l, out) : r;
}

praos_batch* praos_batch_upload_tpraos_bytes(praos_ctx* c, const praos_header_bytes* in) {
  return upload_bytes_impl(c, in, true);
}

int praos_batch_download_tpraos(praos_ctx* c, praos_batch* b, praos_tpraos_out* out) {
  if (!c || !b || !out || !out->bits || !b->tp_only) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (b->n == 0) return PRAOS_OK;
  return tpraos_download(c, b, b->beta_l, out);
}

int praos_verify_tpraos_header_bytes(praos_ctx* c, const praos_header_bytes* in, praos_tpraos_out* out,
                                     praos_decoded* dec, uint8_t* leader_out, uint8_t* leader_proof) {
  if (!c || !in || !out || !out->bits) return PRAOS_E_ARG;
  if (!c->have_epoch) return PRAOS_E_STATE;
  const size_t n = in->n;
  if (n == 0) return PRAOS_OK;
  praos_batch* b = upload_bytes_impl(c, in, true);
  if (!b) return PRAOS_E_OOM;
  ScratchBatch scratch(c, b);
  int r = praos_batch_run(c, b);             // decode, then the TPraos passes
  if (r == PRAOS_OK) r = tpraos_download(c, b, b->beta_l, out);
  if (r == PRAOS_OK && dec) r = praos_batch_download_decoded(c, b, dec);
  if (r == PRAOS_OK && leader_out) HIPCHK(c, d2h(c, leader_out, b->lead_out, 64 * n));
  if (r == PRAOS_OK && leader_proof) HIPCHK(c, d2h(c, leader_proof, b->lead_proof, 80 * n));
  return r;
}

}  // extern "C"
