// praos_api.hip -- host side of libpraos_hip: the context, the epoch's tables, batches and their
// uploads / downloads, block, Byron and chunk validation, the replay's entry points and the
// stored-bytes pipeline.  The crypto step's scheduler is praos_run.hip, the sequential part of
// Praos.updateChainDepState praos_fold.hip, generator and debug entry points praos_debug.hip; they
// share praos_ctx / praos_batch through api_internal.hpp.  The kernels sit in the k_* modules
// behind launch.hpp (no relocatable device code).
#include "api_internal.hpp"

using namespace praos_impl;

static void free_spare(praos_ctx* c) {
  for (void* p : c->spare)
    if (p) (void)hipFree(p);
  c->spare.clear();
  c->spare_sz.clear();
}

// Large H2D / D2H copies through two pinned buffers: the host threads fill (drain) one
// piece while the DMA engine moves the other, so pageable caller memory moves at PCIe
// speed instead of through the runtime's own pageable path.  Small copies go direct.
// the arena's zero padding after its last byte (< 64 bytes), copied from pinned zeros on st
static hipError_t zero_pad(praos_ctx* c, uint8_t* dst, size_t pad, hipStream_t st) {
  if (!c->zero_h) {
    if (hipHostMalloc((void**)&c->zero_h, 64, hipHostMallocDefault) != hipSuccess) return hipErrorOutOfMemory;
    std::memset(c->zero_h, 0, 64);
  }
  return hipMemcpyAsync(dst, c->zero_h, pad, hipMemcpyHostToDevice, st);
}

static bool stage_init(praos_ctx* c) {
  if (c->pin[0]) return true;
  for (int k = 0; k < 2; k++) {
    if (hipHostMalloc((void**)&c->pin[k], STAGE_PIECE, hipHostMallocDefault) != hipSuccess) return false;
    if (hipEventCreateWithFlags(&c->pin_ev[k], hipEventDisableTiming) != hipSuccess) return false;
  }
  const unsigned hw = std::thread::hardware_concurrency();
  unsigned nt = std::max(1u, std::min(16u, hw ? hw : 1u));      // the box's CPU share per GPU
  if (const char* e = std::getenv("PRAOS_COPY_THREADS")) nt = (unsigned)std::max(1, std::min(64, std::atoi(e)));
  c->pool.reset(new CopyPool(nt));
  return true;
}

static bool is_registered(praos_ctx* c, const void* p, size_t len) {
  std::lock_guard<std::mutex> g(c->reg_mu);
  const uintptr_t a = (uintptr_t)p;
  for (const auto& r : c->registered)
    if (a >= r.first && len <= r.second && a - r.first <= r.second - len) return true;
  return false;
}

static hipError_t h2d_on(praos_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (bytes < (4u << 20) || is_registered(c, src, bytes) || !stage_init(c))
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);   // registered memory: direct DMA
  for (size_t off = 0, k = 0; off < bytes; off += STAGE_PIECE, k++) {
    const size_t len = std::min(STAGE_PIECE, bytes - off);
    hipError_t e = hipEventSynchronize(c->pin_ev[k & 1]);    // the DMA that last used this buffer
    if (e != hipSuccess) return e;
    c->pool->copy(c->pin[k & 1], (const uint8_t*)src + off, len);
    e = hipMemcpyAsync((uint8_t*)dst + off, c->pin[k & 1], len, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(c->pin_ev[k & 1], st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// D2H on stream st, whose producers the caller has ordered before (an event wait); returns
// when the bytes are in dst
static hipError_t d2h_on(praos_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (bytes < (4u << 20) || is_registered(c, dst, bytes) || !stage_init(c)) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
  }
  const size_t np = (bytes + STAGE_PIECE - 1) / STAGE_PIECE;
  hipError_t e = hipSuccess;
  for (size_t k = 0; k <= np && e == hipSuccess; k++) {
    if (k < np) {
      const size_t off = k * STAGE_PIECE, len = std::min(STAGE_PIECE, bytes - off);
      e = hipEventSynchronize(c->pin_ev[k & 1]);
      if (e == hipSuccess) e = hipMemcpyAsync(c->pin[k & 1], (const uint8_t*)src + off, len, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipEventRecord(c->pin_ev[k & 1], st);
    }
    if (e == hipSuccess && k > 0) {
      const size_t j = k - 1, off = j * STAGE_PIECE, len = std::min(STAGE_PIECE, bytes - off);
      e = hipEventSynchronize(c->pin_ev[j & 1]);
      if (e == hipSuccess) c->pool->copy((uint8_t*)dst + off, c->pin[j & 1], len);
    }
  }
  return e;
}

static hipError_t h2d(praos_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes < (4u << 20) || !stage_init(c)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
  for (size_t off = 0, k = 0; off < bytes; off += STAGE_PIECE, k++) {
    const size_t len = std::min(STAGE_PIECE, bytes - off);
    hipError_t e = hipEventSynchronize(c->pin_ev[k & 1]);    // the DMA that last read this buffer
    if (e != hipSuccess) return e;
    c->pool->copy(c->pin[k & 1], (const uint8_t*)src + off, len);
    e = hipMemcpyAsync((uint8_t*)dst + off, c->pin[k & 1], len, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipEventRecord(c->pin_ev[k & 1], c->stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// blocking: the stream is drained first (the producer kernels), then piecewise
static hipError_t d2h(praos_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes < (4u << 20) || !stage_init(c)) return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  hipError_t e = hipStreamSynchronize(c->stream);
  const size_t np = (bytes + STAGE_PIECE - 1) / STAGE_PIECE;
  for (size_t k = 0; k <= np && e == hipSuccess; k++) {
    if (k < np) {     // start piece k, then drain piece k - 1 while it moves
      const size_t off = k * STAGE_PIECE, len = std::min(STAGE_PIECE, bytes - off);
      e = hipMemcpyAsync(c->pin[k & 1], (const uint8_t*)src + off, len, hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipEventRecord(c->pin_ev[k & 1], c->stream);
    }
    if (e == hipSuccess && k > 0) {
      const size_t j = k - 1, off = j * STAGE_PIECE, len = std::min(STAGE_PIECE, bytes - off);
      e = hipEventSynchronize(c->pin_ev[j & 1]);
      if (e == hipSuccess) c->pool->copy((uint8_t*)dst + off, c->pin[j & 1], len);
    }
  }
  return e;
}

extern "C" {

int praos_abi_version(void) { return PRAOS_ABI_VERSION; }

int praos_host_register(praos_ctx* c, void* p, size_t len) {
  if (!c || !p || len == 0) return PRAOS_E_ARG;
  if (c->device < 0) return PRAOS_E_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipHostRegister(p, len, hipHostRegisterDefault));
  std::lock_guard<std::mutex> g(c->reg_mu);
  c->registered.emplace_back((uintptr_t)p, len);
  return PRAOS_OK;
}

int praos_host_unregister(praos_ctx* c, void* p) {
  if (!c || !p) return PRAOS_E_ARG;
  {
    std::lock_guard<std::mutex> g(c->reg_mu);
    auto it = std::find_if(c->registered.begin(), c->registered.end(),
                           [&](const std::pair<uintptr_t, size_t>& r) { return r.first == (uintptr_t)p; });
    if (it == c->registered.end()) return PRAOS_E_ARG;
    c->registered.erase(it);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipHostUnregister(p));
  return PRAOS_OK;
}

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

// k_decode_praos over a from-bytes batch, on the ctx stream
int batch_decode(praos_ctx* c, praos_batch* b) {
  if (b->n == 0) return PRAOS_OK;
  launch_decode_praos(dim3(nblocks(b->n, NT)), dim3(NT), c->stream, b->n, b->arena, b->arena_len, b->hoff, b->hlen,
                      b->slot, b->cold_vk, b->vrf_vk, b->vrf_out, b->vrf_proof, b->hot_vk, b->ocert_sig, b->kes_sig,
                      b->ocert_n, b->ocert_c0, b->body_off, b->body_len, b->body, b->block_no, b->prev_hash,
                      b->prev_genesis, b->body_size, b->body_hash, b->prot_major, b->prot_minor, b->header_hash,
                      b->dec_status, b->is_block ? 1 : (b->tp_only ? 2 : 0), b->signed_stride, b->lead_out,
                      b->lead_proof);
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
  for (int k = 0; k < RP_SLOTS; k++) rp_batch_destroy(c, c->rp_keep[k]);
  if (c->cand_scratch) (void)hipFree(c->cand_scratch);
  for (int k = 0; k < PIPE_MAX; k++) {
    if (c->pipe[k]) {
      for (void* p : c->pipe[k]->owned) (void)hipFree(p);
      delete c->pipe[k];
    }
    if (c->up_ev[k]) (void)hipEventDestroy(c->up_ev[k]);
    if (c->done_ev[k]) (void)hipEventDestroy(c->done_ev[k]);
  }
  for (auto& p : c->pcall) {
    if (p.ev) (void)hipEventDestroy(p.ev);
    if (p.off_h) (void)hipHostFree(p.off_h);
    if (p.len_h) (void)hipHostFree(p.len_h);
  }
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

// device buffers of a from-bytes batch of n headers over an arena of bytes_len bytes
// (owner == nullptr: fresh allocations, not taken from / given back to the spare list)
static praos_batch* bytes_batch_alloc(praos_ctx* c, size_t n, size_t bytes_len, bool tpraos, praos_ctx* owner) {
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
  ok &= dalloc(b, &b->arena, ((bytes_len + 7) & ~(size_t)7) + 16) == hipSuccess;  // +16: ld64u pad
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

static praos_batch* upload_bytes_impl(praos_ctx* c, const praos_header_bytes* in, bool tpraos) {
  if (!c || !in || (in->n && (!in->off || !in->len || (!in->bytes && in->bytes_len)))) return nullptr;
  if (c->device < 0) { c->err = "host-only context: no HIP device"; return nullptr; }
  if (hipSetDevice(c->device) != hipSuccess) return nullptr;
  praos_batch* b = new praos_batch();
  b->owner = c;
  const size_t n = in->n;
  b->n = n;
  b->from_bytes = true;
  b->arena_len = in->bytes_len;
  b->tp_only = tpraos;
  b->signed_stride = tpraos ? TP_SIGNED_STRIDE : PRAOS_SIGNED_STRIDE;
  b->body_bytes_len = (size_t)b->signed_stride * n;
  bool ok = alloc_soa(b, n, b->body_bytes_len + 16);
  if (tpraos) {
    ok &= dalloc(b, &b->lead_out, 64 * n) == hipSuccess;
    ok &= dalloc(b, &b->lead_proof, 80 * n) == hipSuccess;
    ok &= dalloc(b, &b->beta_l, 64 * n) == hipSuccess;
  }
  ok &= dalloc(b, &b->arena, ((in->bytes_len + 7) & ~(size_t)7) + 16) == hipSuccess;  // +16: ld64u pad
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
  if (!ok) { c->err = "device allocation failed"; praos_batch_free(c, b); return nullptr; }
  const size_t pad = ((in->bytes_len + 7) & ~(size_t)7) + 16 - in->bytes_len;
  ok &= hipMemsetAsync(b->arena + in->bytes_len, 0, pad, c->stream) == hipSuccess;
  if (in->bytes_len)
    ok &= h2d(c, b->arena, in->bytes, in->bytes_len) == hipSuccess;
  if (n) {
    ok &= hipMemcpyAsync(b->hoff, in->off, 8 * n, hipMemcpyHostToDevice, c->stream) == hipSuccess;
    ok &= hipMemcpyAsync(b->hlen, in->len, 4 * n, hipMemcpyHostToDevice, c->stream) == hipSuccess;
  }
  ok &= hipStreamSynchronize(c->stream) == hipSuccess;
  if (!ok) { c->err = "upload failed"; praos_batch_free(c, b); return nullptr; }
  return b;
}

static int tpraos_download(praos_ctx* c, praos_batch* b, const uint8_t* dbeta_l, praos_tpraos_out* out);

// ---- block-integrity batch (k_block.hip + k_decode + k_kes header mode)
// the buffers a block batch has beyond a from-bytes batch
static bool block_batch_buffers(praos_batch* b) {
  const size_t n = b->n;
  b->is_block = true;
  bool ok = dalloc(b, &b->blk_off, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->blk_len, 4 * n) == hipSuccess;
  ok &= dalloc(b, &b->seg_off, 8 * 4 * n) == hipSuccess;
  ok &= dalloc(b, &b->seg_len, 4 * 4 * n) == hipSuccess;
  ok &= dalloc(b, &b->nseg, n) == hipSuccess;
  ok &= dalloc(b, &b->split_status, n) == hipSuccess;
  ok &= dalloc(b, &b->seg_hash, 32 * 4 * n) == hipSuccess;
  ok &= dalloc(b, &b->blk_result, n) == hipSuccess;
  ok &= dalloc(b, &b->blk_hash, 32 * n) == hipSuccess;
  // TPraos BHBody signed bodies are up to 586 bytes: a wider stride than header batches
  b->signed_stride = TP_SIGNED_STRIDE;
  b->body_bytes_len = (size_t)TP_SIGNED_STRIDE * n;
  ok &= dalloc(b, &b->body, b->body_bytes_len + 16) == hipSuccess;
  return ok;
}

praos_batch* praos_block_batch_upload(praos_ctx* c, const praos_header_bytes* blocks) {
  praos_batch* b = praos_batch_upload_bytes(c, blocks);
  if (!b) return nullptr;
  const size_t n = b->n;
  bool ok = block_batch_buffers(b);
  if (!ok) { c->err = "device allocation failed"; praos_batch_free(c, b); return nullptr; }
  // the uploaded spans are whole blocks; k_block_split rewrites hoff/hlen to the header spans
  if (n) {
    ok &= hipMemcpyAsync(b->blk_off, b->hoff, 8 * n, hipMemcpyDeviceToDevice, c->stream) == hipSuccess;
    ok &= hipMemcpyAsync(b->blk_len, b->hlen, 4 * n, hipMemcpyDeviceToDevice, c->stream) == hipSuccess;
  }
  ok &= hipStreamSynchronize(c->stream) == hipSuccess;
  if (!ok) { c->err = "upload failed"; praos_batch_free(c, b); return nullptr; }
  return b;
}

int praos_block_batch_run(praos_ctx* c, praos_batch* b, uint64_t slots_per_kes_period) {
  if (!c || !b || !b->is_block || slots_per_kes_period == 0) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = b->n;
  if (n == 0) return PRAOS_OK;
  const dim3 g(nblocks(n, NT)), blk(NT);
  uint16_t* bk = b->bits3 + n;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  HIPCHK(c, hipMemcpyAsync(b->hoff, b->blk_off, 8 * n, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b->hlen, b->blk_len, 4 * n, hipMemcpyDeviceToDevice, c->stream));
  (void)hipGetLastError();   // clear a stale error of an earlier, already-reported runtime call
  launch_block_split(g, blk, c->stream, n, b->arena, b->arena_len, b->hoff, b->hlen, b->seg_off, b->seg_len, b->nseg,
                     b->split_status);
  HIPCHK(c, hipGetLastError());
  const int rd = batch_decode(c, b);
  if (rd != PRAOS_OK) { c->err = "decode launch failed"; return rd; }
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  // segment hashes on a side stream, concurrent with the KES verify
  HIPCHK(c, hipStreamWaitEvent(c->side[0], c->ev[1], 0));
  launch_seg_hash(dim3(nblocks(4 * n, NT)), blk, c->side[0], n, b->arena, b->seg_off, b->seg_len, b->nseg,
                  b->seg_hash);
  HIPCHK(c, hipEventRecord(c->side_ev[0], c->side[0]));
  launch_kes(g, blk, c->stream, n, (const uint32_t*)nullptr, (const uint32_t*)nullptr, c->btab, b->hot_vk, b->kes_sig, b->body_off, b->body_len, b->body,
             b->body_bytes_len, b->slot, b->ocert_c0, slots_per_kes_period, (const uint32_t*)nullptr, bk,
             (uint8_t*)nullptr, b->tab_kes);
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->side_ev[0], 0));
  launch_block_join(g, blk, c->stream, n, b->nseg, b->split_status, b->dec_status, bk, b->seg_hash, b->body_hash,
                    b->blk_result, b->blk_hash);
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  HIPCHK(c, hipGetLastError());
  return PRAOS_OK;
}

int praos_block_batch_download(praos_ctx* c, praos_batch* b, uint8_t* result, uint8_t* body_hash) {
  if (!c || !b || !b->is_block || (b->n && !result)) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (b->n == 0) return PRAOS_OK;
  HIPCHK(c, hipMemcpy(result, b->blk_result, b->n, hipMemcpyDeviceToHost));
  if (body_hash) HIPCHK(c, hipMemcpy(body_hash, b->blk_hash, 32 * b->n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_verify_block_integrity(praos_ctx* c, const praos_header_bytes* blocks, uint64_t slots_per_kes_period,
                                 uint8_t* result, uint8_t* body_hash) {
  if (!c || !blocks || (blocks->n && !result) || slots_per_kes_period == 0) return PRAOS_E_ARG;
  if (c->device < 0) { c->err = "host-only context: no HIP device"; return PRAOS_E_STATE; }
  if (blocks->n == 0) return PRAOS_OK;
  praos_batch* b = praos_block_batch_upload(c, blocks);
  if (!b) return PRAOS_E_OOM;
  int r = praos_block_batch_run(c, b, slots_per_kes_period);
  if (r == PRAOS_OK) r = praos_block_batch_download(c, b, result, body_hash);
  praos_batch_free(c, b);
  return r;
}

// ---- ImmutableDB chunk validation: CRC-32 (k_crc32.hip) and parseChunkFile as one call
// CRC-32 of n spans of d_arena on stream st; the buffers belong to batch b.  len_h: the
// spans' lengths on the host (the tile list is their prefix sum).
static int crc_spans(praos_ctx* c, praos_batch* b, hipStream_t st, size_t n, const uint32_t* len_h,
                     const uint8_t* d_arena, const uint64_t* d_off, const uint32_t* d_len, uint32_t** d_crc) {
  if (!b->crc_out) {   // a batch's spans do not change: the tile list is built once
    std::vector<uint32_t> first(n + 1);
    uint64_t tiles = 0;
    for (size_t i = 0; i < n; i++) {
      first[i] = (uint32_t)tiles;
      tiles += ((uint64_t)len_h[i] + PRAOS_CRC_TILE - 1) / PRAOS_CRC_TILE;
      if (tiles > 0x7fffffffu) { c->err = "too many CRC tiles"; return PRAOS_E_ARG; }
    }
    first[n] = (uint32_t)tiles;
    bool ok = dalloc(b, &b->crc_first, 4 * (n + 1)) == hipSuccess;
    ok &= dalloc(b, &b->crc_raw, 4 * (size_t)tiles) == hipSuccess;
    uint32_t* out = nullptr;
    ok &= dalloc(b, &out, 4 * n) == hipSuccess;
    if (!ok) { c->err = "device allocation failed"; return PRAOS_E_OOM; }
    HIPCHK(c, hipMemcpy(b->crc_first, first.data(), 4 * (n + 1), hipMemcpyHostToDevice));
    b->crc_tiles = (uint32_t)tiles;
    b->crc_out = out;
  }
  (void)hipGetLastError();
  launch_crc32(st, (uint32_t)n, b->crc_tiles, d_arena, d_off, d_len, b->crc_first, b->crc_raw, b->crc_out);
  HIPCHK(c, hipGetLastError());
  *d_crc = b->crc_out;
  return PRAOS_OK;
}

// arena upload of a from-bytes batch (zero padding for ld64u, then the bytes), on the ctx stream
static int arena_upload(praos_ctx* c, praos_batch* b, const uint8_t* bytes, size_t bytes_len) {
  const size_t pad = ((bytes_len + 7) & ~(size_t)7) + 16 - bytes_len;
  HIPCHK(c, hipMemsetAsync(b->arena + bytes_len, 0, pad, c->stream));
  if (bytes_len) HIPCHK(c, h2d(c, b->arena, bytes, bytes_len));
  return PRAOS_OK;
}

int praos_crc32(praos_ctx* c, const praos_header_bytes* s, uint32_t* crc) {
  if (!c || !s || (s->n && (!s->off || !s->len || !crc)) || (!s->bytes && s->bytes_len) || s->n > 0x7fffffffu)
    return PRAOS_E_ARG;
  for (size_t i = 0; i < s->n; i++)
    if (s->off[i] > s->bytes_len || s->len[i] > s->bytes_len - s->off[i]) {
      c->err = "praos_crc32: span " + std::to_string(i) + " outside the arena";
      return PRAOS_E_ARG;
    }
  if (c->device < 0) { c->err = "host-only context: no HIP device"; return PRAOS_E_STATE; }
  if (s->n == 0) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = s->n;
  praos_batch* b = new praos_batch();
  b->owner = c;
  b->n = n;
  b->arena_len = s->bytes_len;
  auto run = [&]() -> int {
    bool ok = dalloc(b, &b->arena, ((s->bytes_len + 7) & ~(size_t)7) + 16) == hipSuccess;
    ok &= dalloc(b, &b->hoff, 8 * n) == hipSuccess;
    ok &= dalloc(b, &b->hlen, 4 * n) == hipSuccess;
    if (!ok) { c->err = "device allocation failed"; return PRAOS_E_OOM; }
    int r = arena_upload(c, b, s->bytes, s->bytes_len);
    if (r != PRAOS_OK) return r;
    HIPCHK(c, hipMemcpyAsync(b->hoff, s->off, 8 * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b->hlen, s->len, 4 * n, hipMemcpyHostToDevice, c->stream));
    uint32_t* d_crc = nullptr;
    r = crc_spans(c, b, c->stream, n, s->len, b->arena, b->hoff, b->hlen, &d_crc);
    if (r != PRAOS_OK) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(crc, d_crc, 4 * n, hipMemcpyDeviceToHost));
    return PRAOS_OK;
  };
  const int r = run();
  (void)hipStreamSynchronize(c->stream);
  praos_batch_free(c, b);
  return r;
}

int praos_block_batch_crc32(praos_ctx* c, praos_batch* b, uint32_t* crc) {
  if (!c || !b || !b->is_block || (b->n && !crc) || b->n > 0x7fffffffu) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = b->n;
  if (n == 0) return PRAOS_OK;
  std::vector<uint32_t> len;
  if (!b->crc_out) {
    len.resize(n);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(len.data(), b->blk_len, 4 * n, hipMemcpyDeviceToHost));
    std::vector<uint64_t> off(n);
    HIPCHK(c, hipMemcpy(off.data(), b->blk_off, 8 * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++)   // the kernel does not range-check: nothing is launched on a bad span
      if (off[i] > b->arena_len || len[i] > b->arena_len - off[i]) {
        c->err = "praos_block_batch_crc32: span " + std::to_string(i) + " outside the arena";
        return PRAOS_E_ARG;
      }
  }
  uint32_t* d_crc = nullptr;
  const int r = crc_spans(c, b, c->stream, n, len.data(), b->arena, b->blk_off, b->blk_len, &d_crc);
  if (r != PRAOS_OK) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(crc, d_crc, 4 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

namespace {
// per-block columns of pass A, on the host
struct ChunkCols {
  std::vector<uint64_t> off, hoff, slot, block_no;
  std::vector<uint32_t> len, hlen, crc;
  std::vector<uint16_t> dec;
  std::vector<uint8_t> split, gen, prev, hh, kind;   // kind: k_byron_split's (0 unless Byron is on)
  std::vector<uint64_t> epoch;
  void resize(size_t n) {
    kind.resize(n); epoch.resize(n);
    off.resize(n); hoff.resize(n); slot.resize(n); block_no.resize(n); len.resize(n); hlen.resize(n);
    crc.resize(n); dec.resize(n); split.resize(n); gen.resize(n); prev.resize(32 * n); hh.resize(32 * n);
  }
};
void put_be(uint8_t* p, uint64_t v, int nbytes) {
  for (int k = 0; k < nbytes; k++) p[k] = (uint8_t)(v >> (8 * (nbytes - 1 - k)));
}
}  // namespace

// a block batch of n blocks over the arena of `arena_of` (no upload), or over a fresh arena
static praos_batch* chunk_batch(praos_ctx* c, size_t n, size_t bytes_len, const praos_batch* arena_of) {
  praos_batch* b = bytes_batch_alloc(c, n, arena_of ? 0 : bytes_len, false, c);
  if (!b) return nullptr;
  if (!block_batch_buffers(b)) { c->err = "device allocation failed"; praos_batch_free(c, b); return nullptr; }
  if (arena_of) { b->arena = arena_of->arena; b->arena_len = arena_of->arena_len; }
  return b;
}

// pass A over blocks [base, base + b->n) of col (off / len filled in): CRC on a side stream
// beside split + decode on the ctx stream, then the columns come back
// the Byron buffers of a block batch (after every other allocation, so a batch without Byron
// allocates as it always did)
static bool byron_buffers(praos_batch* b) {
  if (b->byr_kind) return true;
  const size_t n = b->n;
  bool ok = dalloc(b, &b->byr_kind, n) == hipSuccess;
  ok &= dalloc(b, &b->byr_which, n) == hipSuccess;
  ok &= dalloc(b, &b->byr_epoch, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->byr_spans, 4 * (size_t)PRAOS_BYRON_SPANS * n) == hipSuccess;
  return ok;
}

static void byron_split(praos_ctx* c, praos_batch* b, uint64_t es, bool spans) {
  launch_byron_split(dim3(nblocks(b->n, NT)), dim3(NT), c->stream, b->n, b->arena, b->arena_len, b->blk_off, b->blk_len,
                     es, b->hoff, b->hlen, b->slot, b->block_no, b->prev_hash, b->prev_genesis, b->header_hash,
                     b->split_status, b->dec_status, b->byr_kind, b->byr_epoch, spans ? b->byr_spans : nullptr);
}

// verifyBlockIntegrity of the Byron blocks of a block batch (blk_off / blk_len set), on the ctx stream
static int byron_integrity_run(praos_ctx* c, praos_batch* b, uint64_t es, uint32_t pm, uint8_t* result, uint8_t* which) {
  const size_t n = b->n;
  if (n == 0) return PRAOS_OK;
  if (!byron_buffers(b)) { c->err = "device allocation failed"; return PRAOS_E_OOM; }
  (void)hipGetLastError();
  byron_split(c, b, es, true);
  HIPCHK(c, hipGetLastError());
  launch_byron_integrity(dim3(nblocks(n, NT)), dim3(NT), c->stream, n, b->arena, b->blk_off, b->blk_len, b->byr_kind,
                         b->byr_spans, pm, c->btab, b->tab_kes, b->blk_result, b->byr_which);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(result, b->blk_result, n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(which, b->byr_which, n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_verify_byron_integrity(praos_ctx* c, const praos_header_bytes* blocks, uint64_t epoch_slots,
                                 uint32_t protocol_magic, uint8_t* result, uint8_t* which) {
  if (!c || !blocks || (blocks->n && !result) || epoch_slots == 0) return PRAOS_E_ARG;
  if (c->device < 0) { c->err = "host-only context: no HIP device"; return PRAOS_E_STATE; }
  if (blocks->n == 0) return PRAOS_OK;
  praos_batch* b = praos_block_batch_upload(c, blocks);
  if (!b) return PRAOS_E_OOM;
  std::vector<uint8_t> w(blocks->n);
  const int r = byron_integrity_run(c, b, epoch_slots, protocol_magic, result, w.data());
  if (r == PRAOS_OK && which)
    for (size_t i = 0; i < blocks->n; i++) which[i] = w[i] & (uint8_t)~PRAOS_BYRON_W_ONE_TX;
  (void)hipStreamSynchronize(c->stream);
  praos_batch_free(c, b);
  return r;
}

// ---- Byron header validation, the device half (k_pbft.hip; the fold is praos_pbft.hip)

int praos_byron_key_hash(praos_ctx* c, const uint8_t* keys64, size_t n, uint8_t* out28) {
  if (!c || (n && (!keys64 || !out28))) return PRAOS_E_ARG;
  if (n == 0) return PRAOS_OK;
  if (c->device < 0) {
    praos_pbft_key_hash_host_(keys64, n, out28);
    return PRAOS_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  praos_batch* b = new praos_batch();
  b->owner = c;
  b->n = n;
  auto run = [&]() -> int {
    uint8_t *dk = nullptr, *dh = nullptr;
    if (dalloc(b, &dk, 64 * n) != hipSuccess || dalloc(b, &dh, 28 * n) != hipSuccess) {
      c->err = "device allocation failed";
      return PRAOS_E_OOM;
    }
    HIPCHK(c, h2d(c, dk, keys64, 64 * n));
    launch_pbft_keyhash(c->stream, n, dk, dh);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out28, dh, 28 * n, hipMemcpyDeviceToHost));
    return PRAOS_OK;
  };
  const int r = run();
  (void)hipStreamSynchronize(c->stream);
  praos_batch_free(c, b);
  return r;
}

}  // extern "C"

// the delegation table for the device: sorted by the delegate hash's 7 little-endian words
// (word 0 first, k_pbft.hip hash_cmp), word 7 = the caller's index
static std::vector<std::array<uint32_t, 8>> pbft_deleg_table(const uint8_t* delegs, uint32_t n_delegs) {
  std::vector<std::array<uint32_t, 8>> tab(n_delegs);
  for (uint32_t k = 0; k < n_delegs; k++) {
    std::memcpy(tab[k].data(), delegs + 56 * (size_t)k + 28, 28);
    tab[k][7] = k;
  }
  std::sort(tab.begin(), tab.end(), [](const std::array<uint32_t, 8>& x, const std::array<uint32_t, 8>& y) {
    return std::lexicographical_compare(x.begin(), x.begin() + 7, y.begin(), y.begin() + 7);
  });
  return tab;
}

// The body of praos_verify_pbft_headers over device-resident inputs: n header spans (hoff, hlen)
// into an arena of alen bytes (ld64u's pad behind it; the two bytes in front of every span inside
// it) and their is_ebb flags, all final in the order of the context's stream.  The working buffers
// go to b, which the caller frees.  The cached / uncached choice and praos_pbft_stats are over
// these n headers.
static int pbft_verify_dev(praos_ctx* c, praos_batch* b, size_t n, const uint8_t* arena, size_t alen,
                           const uint64_t* hoff, const uint32_t* hlen, const uint8_t* d_ebb,
                           const praos_pbft_params* p, const uint8_t* delegs, uint32_t n_delegs, praos_pbft_out* out) {
  const std::vector<std::array<uint32_t, 8>> tab = pbft_deleg_table(delegs, n_delegs);
  const bool cached = c->keycache > 0 && n >= c->knobs.pbft_ck_min;
  uint8_t *d_bits = nullptr, *d_dhash = nullptr, *d_keys = nullptr, *d_sig = nullptr, *d_hram = nullptr;
  uint32_t *d_tab = nullptr, *d_vlist = nullptr, *d_vcount = nullptr;
  int32_t* d_gk = nullptr;
  bool ok = dalloc(b, &d_tab, 32 * (size_t)n_delegs) == hipSuccess;
  ok &= dalloc(b, &b->slot, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->block_no, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->prev_hash, 32 * n) == hipSuccess;
  ok &= dalloc(b, &b->prev_genesis, n) == hipSuccess;
  ok &= dalloc(b, &b->header_hash, 32 * n) == hipSuccess;
  ok &= dalloc(b, &d_bits, n) == hipSuccess;
  ok &= dalloc(b, &d_gk, 4 * n) == hipSuccess;
  ok &= dalloc(b, &d_dhash, 28 * n) == hipSuccess;
  ok &= dalloc(b, &d_keys, 32 * n) == hipSuccess;
  ok &= dalloc(b, &d_sig, 64 * n) == hipSuccess;
  ok &= dalloc(b, &d_hram, 64 * n) == hipSuccess;
  ok &= dalloc(b, &d_vlist, 4 * n) == hipSuccess;
  ok &= dalloc(b, &d_vcount, 16) == hipSuccess;
  ok &= dalloc(b, (uint8_t**)&b->tab_ocert, LT_ED_B * n) == hipSuccess;
  praos_batch::KeyCache& k = b->kc[0];
  if (cached) {
    // the delegate keys of a batch are few (7 on mainnet): a small entry space, the keys
    // past it verify uncached
    k.cap = 256;
    while (k.cap < 2 * n) k.cap <<= 1;
    k.max_entries = (uint32_t)std::min<size_t>(n / 2 + 1, 1024);
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
  }
  if (!ok) { c->err = "device allocation failed"; return PRAOS_E_OOM; }
  if (cached) {
    const int r = ensure_bcomb16(c);
    if (r != PRAOS_OK) return r;
  }
  hipStream_t st = c->stream;
  if (n_delegs) HIPCHK(c, hipMemcpyAsync(d_tab, tab.data(), 32 * (size_t)n_delegs, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(d_vcount, 0, 16, st));
  (void)hipGetLastError();
  launch_pbft_decode(st, n, arena, alen, hoff, hlen, d_ebb, p->epoch_slots, p->protocol_magic, d_tab, n_delegs,
                     b->slot, b->block_no, b->prev_hash, b->prev_genesis, b->header_hash, d_bits, d_gk, d_dhash, d_keys,
                     d_sig, d_hram, d_vlist, d_vcount);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[0], st));             // the decode's columns are final here
  // (an ILP-4 build of this kernel, as the OCert misses have below ILP4_BATCH, measured level
  // with it -- 21,600 headers 2.152 ms against the ILP-4 build's 2.175, 65,536 2.878 against
  // 2.960 -- and was not kept)
  auto sig_nc = [&](const uint32_t* list, const uint32_t* count) {   // uncached verifies over a list
    launch_pbft_sig(st, n, list, count, c->btab, d_keys, d_sig, d_hram, d_bits, b->tab_ocert);
  };
  if (cached) {
    RunShape shape = run_shape(c, n, false, false);
    shape.pool_keys = 0;                               // the batch's own entries, not the pool-key store
    const RunPlan P = plan_run(c->knobs, shape);
    const int r = kc_lists(c, b, P, k, n, d_keys, st, d_vlist, d_vcount, 0);
    if (r == PRAOS_OK) kc_precompute(c, P, k, d_keys, 0, st, n);
    if (r != PRAOS_OK) return r;
    launch_pbft_sig_ck(st, n, k.hit, k.counters + 1, k.item_entry, k.kt, k.ki, c->bcomb16, d_keys, d_sig, d_hram,
                       d_bits);
    sig_nc(k.miss, k.counters + 2);
  } else {
    sig_nc(d_vlist, d_vcount);
  }
  HIPCHK(c, hipGetLastError());
  // every column but the bits comes back on the download stream while the verifies run
  hipStream_t ds = c->dstream;
  HIPCHK(c, hipStreamWaitEvent(ds, c->ev[0], 0));
  // (large columns through the pinned staging buffers; the small ones queued, one wait for all)
  auto col = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    if (bytes >= (4u << 20)) return d2h_on(c, dst, src, bytes, ds);
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ds);
  };
  HIPCHK(c, col(out->prev_hash, b->prev_hash, 32 * n));
  HIPCHK(c, col(out->header_hash, b->header_hash, 32 * n));
  if (out->delegate_hash) HIPCHK(c, col(out->delegate_hash, d_dhash, 28 * n));
  HIPCHK(c, col(out->slot, b->slot, 8 * n));
  HIPCHK(c, col(out->block_no, b->block_no, 8 * n));
  HIPCHK(c, col(out->gk_idx, d_gk, 4 * n));
  HIPCHK(c, col(out->prev_is_genesis, b->prev_genesis, n));
  std::memset(c->pbft_raw, 0, sizeof c->pbft_raw);
  if (cached) HIPCHK(c, hipMemcpyAsync(c->pbft_raw, k.counters, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(c->pbft_raw + 4, d_vcount, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(ds));
  HIPCHK(c, hipStreamSynchronize(st));
  c->pbft_stats[0] = cached ? 1 : 0;
  c->pbft_stats[1] = cached ? std::min(c->pbft_raw[0], k.max_entries) : 0;
  c->pbft_stats[2] = cached ? c->pbft_raw[1] : 0;
  c->pbft_stats[3] = cached ? c->pbft_raw[2] : c->pbft_raw[4];
  HIPCHK(c, hipMemcpy(out->bits, d_bits, n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

// The candidates call's way in (praos_candidates.hip): n > 0 rows whose spans, flags and arena
// are already on the device and final (the caller has synchronised the stream that wrote them);
// out has every column but delegate_hash.
int rp_pbft_verify_rows(praos_ctx* c, size_t n, const uint8_t* arena, size_t arena_len, const uint64_t* hoff,
                        const uint32_t* hlen, const uint8_t* d_is_ebb, const praos_pbft_params* p,
                        const uint8_t* delegs, uint32_t n_delegs, praos_pbft_out* out) {
  HIPCHK(c, hipSetDevice(c->device));
  praos_batch* b = new praos_batch();
  b->owner = c;
  b->n = n;
  const int r = pbft_verify_dev(c, b, n, arena, arena_len, hoff, hlen, d_is_ebb, p, delegs, n_delegs, out);
  (void)hipStreamSynchronize(c->stream);
  praos_batch_free(c, b);
  return r;
}

extern "C" {

int praos_verify_pbft_headers(praos_ctx* c, const praos_header_bytes* in, const uint8_t* is_ebb,
                              const praos_pbft_params* p, const uint8_t* delegs, uint32_t n_delegs,
                              praos_pbft_out* out) {
  if (!c || !in || !p || !out || p->epoch_slots == 0 || (n_delegs && !delegs) || in->n > 0x7fffffffu ||
      (!in->bytes && in->bytes_len))
    return PRAOS_E_ARG;
  const size_t n = in->n;
  if (n && (!in->off || !in->len || !is_ebb || !out->bits || !out->gk_idx || !out->slot || !out->block_no ||
            !out->prev_hash || !out->prev_is_genesis || !out->header_hash))
    return PRAOS_E_ARG;
  for (size_t i = 0; i < n; i++)   // nothing is launched on a bad span
    if (in->off[i] > in->bytes_len || in->len[i] > in->bytes_len - in->off[i]) {
      c->err = "praos_verify_pbft_headers: span " + std::to_string(i) + " outside the arena";
      return PRAOS_E_ARG;
    }
  if (!praos_pbft_delegs_ok_(delegs, n_delegs)) {
    c->err = "pbft: duplicate hash in the delegation map";
    return PRAOS_E_ARG;
  }
  if (c->device < 0) { c->err = "host-only context: no HIP device"; return PRAOS_E_STATE; }
  if (n == 0) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // the arena behind 8 zero bytes: the header hash reads the two bytes before a header (its
  // 82 0k prefix replaces them), and a header may start at offset 0 of the caller's arena
  constexpr size_t FRONT = 8;
  std::vector<uint64_t> off(n);
  for (size_t i = 0; i < n; i++) off[i] = in->off[i] + FRONT;
  const size_t alen = FRONT + in->bytes_len;
  praos_batch* b = new praos_batch();
  b->owner = c;
  b->n = n;
  auto run = [&]() -> int {
    uint8_t* d_ebb = nullptr;
    bool ok = dalloc(b, &b->arena, ((alen + 7) & ~(size_t)7) + 16) == hipSuccess;
    ok &= dalloc(b, &b->hoff, 8 * n) == hipSuccess;
    ok &= dalloc(b, &b->hlen, 4 * n) == hipSuccess;
    ok &= dalloc(b, &d_ebb, n) == hipSuccess;
    if (!ok) { c->err = "device allocation failed"; return PRAOS_E_OOM; }
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemsetAsync(b->arena, 0, FRONT, st));
    HIPCHK(c, hipMemsetAsync(b->arena + alen, 0, ((alen + 7) & ~(size_t)7) + 16 - alen, st));
    if (in->bytes_len) HIPCHK(c, h2d(c, b->arena + FRONT, in->bytes, in->bytes_len));
    HIPCHK(c, hipMemcpyAsync(b->hoff, off.data(), 8 * n, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(b->hlen, in->len, 4 * n, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_ebb, is_ebb, n, hipMemcpyHostToDevice, st));
    return pbft_verify_dev(c, b, n, b->arena, alen, b->hoff, b->hlen, d_ebb, p, delegs, n_delegs, out);
  };
  const int r = run();
  (void)hipStreamSynchronize(c->stream);
  praos_batch_free(c, b);
  return r;
}

int praos_pbft_stats(praos_ctx* c, uint32_t out[4]) {
  if (!c || !out) return PRAOS_E_ARG;
  std::memcpy(out, c->pbft_stats, sizeof c->pbft_stats);
  return PRAOS_OK;
}

// es: byron_epoch_slots (0: Byron off, pass A exactly as before)
static int chunk_pass_a(praos_ctx* c, praos_batch* b, size_t base, ChunkCols& col, uint64_t es) {
  const size_t n = b->n;
  if (n == 0) return PRAOS_OK;
  const dim3 g(nblocks(n, NT)), blk(NT);
  HIPCHK(c, hipMemcpyAsync(b->blk_off, col.off.data() + base, 8 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b->blk_len, col.len.data() + base, 4 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b->hoff, b->blk_off, 8 * n, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b->hlen, b->blk_len, 4 * n, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->side[0], c->ev[0], 0));
  uint32_t* d_crc = nullptr;
  int r = crc_spans(c, b, c->side[0], n, col.len.data() + base, b->arena, b->blk_off, b->blk_len, &d_crc);
  if (r != PRAOS_OK) return r;
  HIPCHK(c, hipEventRecord(c->side_ev[0], c->side[0]));
  launch_block_split(g, blk, c->stream, n, b->arena, b->arena_len, b->hoff, b->hlen, b->seg_off, b->seg_len, b->nseg,
                     b->split_status);
  HIPCHK(c, hipGetLastError());
  r = batch_decode(c, b);
  if (r != PRAOS_OK) { c->err = "decode launch failed"; return r; }
  if (es) {   // Byron lanes get their columns from k_byron_split; the others keep the decode's
    if (!byron_buffers(b)) { c->err = "device allocation failed"; return PRAOS_E_OOM; }
    byron_split(c, b, es, false);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->side_ev[0], 0));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (es) {
    HIPCHK(c, hipMemcpy(col.kind.data() + base, b->byr_kind, n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(col.epoch.data() + base, b->byr_epoch, 8 * n, hipMemcpyDeviceToHost));
  }
  HIPCHK(c, hipMemcpy(col.crc.data() + base, d_crc, 4 * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(col.split.data() + base, b->split_status, n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(col.dec.data() + base, b->dec_status, 2 * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(col.hoff.data() + base, b->hoff, 8 * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(col.hlen.data() + base, b->hlen, 4 * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(col.slot.data() + base, b->slot, 8 * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(col.block_no.data() + base, b->block_no, 8 * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(col.gen.data() + base, b->prev_genesis, n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(col.prev.data() + 32 * base, b->prev_hash, 32 * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(col.hh.data() + 32 * base, b->header_hash, 32 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_validate_chunk(praos_ctx* c, const praos_chunk* ch, uint64_t spkp, praos_chunk_result* res,
                         praos_chunk_out* out) {
  const praos_chunk_cfg cfg{spkp, 0, 0, 0};
  return praos_validate_chunk_cfg(c, ch, &cfg, res, out, nullptr);
}

int praos_validate_chunk_cfg(praos_ctx* c, const praos_chunk* ch, const praos_chunk_cfg* cfg, praos_chunk_result* res,
                             praos_chunk_out* out, uint8_t* is_ebb) {
  if (!cfg) return PRAOS_E_ARG;
  const uint64_t spkp = cfg->slots_per_kes_period, es = cfg->byron_epoch_slots;
  if (!c || !ch || !res || !out || spkp == 0 || (!ch->bytes && ch->bytes_len) ||
      (ch->n_expected && !ch->expected_crc) || ch->bytes_len > 0xffffffffu)
    return PRAOS_E_ARG;
  if (c->device < 0) { c->err = "host-only context: no HIP device"; return PRAOS_E_STATE; }
  const uint64_t L = ch->bytes_len;
  const size_t m = ch->n_expected;
  std::memset(res, 0, sizeof *res);
  res->truncate_at = L;
  res->rescanned_from = L;
  if (L == 0) { res->rescanned_from = 0; return PRAOS_OK; }
  HIPCHK(c, hipSetDevice(c->device));
  // the leading offsets that can be candidates at all: off[0] == 0, ascending, inside the file
  size_t k = 0;
  if (ch->block_off)
    while (k < m && ch->block_off[k] < L && (k == 0 ? ch->block_off[0] == 0 : ch->block_off[k] > ch->block_off[k - 1]))
      k++;
  const bool all = m > 0 && k == m;
  const size_t ncand = all ? m : (k ? k - 1 : 0);
  ChunkCols col;
  col.resize(ncand);
  for (size_t j = 0; j < ncand; j++) {
    col.off[j] = ch->block_off[j];
    col.len[j] = (uint32_t)((j + 1 < m ? ch->block_off[j + 1] : L) - ch->block_off[j]);
  }
  praos_batch *b1 = nullptr, *b2 = nullptr, *b3 = nullptr, *b4 = nullptr;
  std::vector<uint8_t> verdict, whichv;
  std::vector<size_t> sub;
  size_t nblk = 0;           // blocks with columns
  bool bad_tail = false;     // the item after them is not well-formed
  auto run = [&]() -> int {
    uint64_t rs = all ? L : (k ? ch->block_off[k - 1] : 0);
    bool rescan = !all;
    size_t keep = ncand;
    if (ncand) {
      b1 = chunk_batch(c, ncand, L, nullptr);
      if (!b1) return PRAOS_E_OOM;
      int r = arena_upload(c, b1, ch->bytes, L);
      if (r == PRAOS_OK) r = chunk_pass_a(c, b1, 0, col, es);
      if (r != PRAOS_OK) return r;
      for (size_t j = 0; j < ncand; j++)
        if (col.split[j]) { keep = j; rs = col.off[j]; rescan = true; break; }
    }
    nblk = keep;
    if (rescan) {
      // the host finds the true boundaries from rs on; the device passes run on them
      res->rescanned_from = rs;
      std::vector<uint64_t> o;
      uint64_t pos = rs;
      while (pos < L) {
        const int64_t e = chunk_scan::chunk_item_end(ch->bytes, pos, L);
        if (e < 0) { bad_tail = true; break; }
        o.push_back(pos);
        pos = (uint64_t)e;
      }
      const uint64_t stop = pos;
      nblk = keep + o.size();
      col.resize(nblk + (bad_tail ? 1 : 0));
      for (size_t j = 0; j < o.size(); j++) {
        col.off[keep + j] = o[j];
        col.len[keep + j] = (uint32_t)((j + 1 < o.size() ? o[j + 1] : stop) - o[j]);
      }
      if (bad_tail) col.off[nblk] = stop;
      if (!o.empty()) {
        b2 = chunk_batch(c, o.size(), L, b1);
        if (!b2) return PRAOS_E_OOM;
        int r = b1 ? PRAOS_OK : arena_upload(c, b2, ch->bytes, L);
        if (r == PRAOS_OK) r = chunk_pass_a(c, b2, keep, col, es);
        if (r != PRAOS_OK) return r;
      }
    }
    // the first block that does not decode ends the parse; so does the first prev-hash mismatch,
    // where a corrupt block still comes first
    size_t E = nblk;
    for (size_t i = 0; i < nblk; i++)
      if (col.split[i] || (col.dec[i] & PRAOS_DEC_FAILED)) { E = i; break; }
    auto mismatch = [&](size_t i) {
      return i > 0 && (col.gen[i] || std::memcmp(&col.prev[32 * i], &col.hh[32 * (i - 1)], 32) != 0);
    };
    auto trusted = [&](size_t i) { return i < m && col.crc[i] == ch->expected_crc[i]; };
    size_t M = E;
    for (size_t i = 0; i < E; i++)
      if (mismatch(i)) { M = i; break; }
    for (size_t i = 0; i < E && i <= M; i++)
      if (!trusted(i)) sub.push_back(i);
    // pass B: verifyBlockIntegrity of the untrusted blocks, over the same device arena; the
    // Shelley-based ones and the Byron ones (col.kind 1 / 2) as a batch each
    verdict.assign(sub.size(), 0);
    whichv.assign(sub.size(), 0);
    for (int byr = 0; byr < 2; byr++) {
      std::vector<size_t> pos;   // positions in sub
      for (size_t j = 0; j < sub.size(); j++)
        if ((col.kind[sub[j]] != 0) == (byr != 0)) pos.push_back(j);
      if (pos.empty()) continue;
      praos_batch* arena_b = b1 ? b1 : b2;
      praos_batch* bb = chunk_batch(c, pos.size(), L, arena_b);
      if (!bb) return PRAOS_E_OOM;
      (byr ? b4 : b3) = bb;
      std::vector<uint64_t> so(pos.size());
      std::vector<uint32_t> sl(pos.size());
      std::vector<uint8_t> v(pos.size()), w(pos.size());
      for (size_t j = 0; j < pos.size(); j++) { so[j] = col.off[sub[pos[j]]]; sl[j] = col.len[sub[pos[j]]]; }
      HIPCHK(c, hipMemcpy(bb->blk_off, so.data(), 8 * so.size(), hipMemcpyHostToDevice));
      HIPCHK(c, hipMemcpy(bb->blk_len, sl.data(), 4 * sl.size(), hipMemcpyHostToDevice));
      int r;
      if (byr) {
        r = byron_integrity_run(c, bb, es, cfg->byron_protocol_magic, v.data(), w.data());
      } else {
        r = praos_block_batch_run(c, bb, spkp);
        if (r == PRAOS_OK) r = praos_block_batch_download(c, bb, v.data(), nullptr);
      }
      if (r != PRAOS_OK) return r;
      for (size_t j = 0; j < pos.size(); j++) { verdict[pos[j]] = v[j]; whichv[pos[j]] = w[j]; }
    }
    // fold in file order: read, then corrupt, then mismatch
    size_t y = 0, q = 0;
    for (size_t i = 0; i < nblk + (bad_tail ? 1 : 0); i++) {
      if (i == E || i == nblk) {
        const bool byron = i < nblk && chunk_scan::chunk_item_end(ch->bytes, col.off[i], L) == (int64_t)(col.off[i] + col.len[i]) &&
                           chunk_scan::is_byron_item(ch->bytes, col.off[i], L);
        res->outcome = byron && !es ? PRAOS_CHUNK_UNSUPPORTED : PRAOS_CHUNK_ERR_READ;
        res->truncate_at = col.off[i];
        break;
      }
      if (!trusted(i)) {
        res->checked++;
        const uint8_t v = verdict[q], w = whichv[q];
        q++;
        // only the Merkle root of a block with n /= 1 transactions fails: no reference file pins
        // that rule, so the reference decides
        if (col.kind[i] == 2 && v == PRAOS_BLK_BODY_HASH && w == PRAOS_BYRON_W_ROOT) {
          res->outcome = PRAOS_CHUNK_UNSUPPORTED;
          res->truncate_at = col.off[i];
          break;
        }
        if (v) {
          res->outcome = PRAOS_CHUNK_ERR_CORRUPT;
          res->integrity_bits = v;
          res->truncate_at = col.off[i];
          res->err_slot = col.slot[i];
          std::memcpy(res->err_hash, &col.hh[32 * i], 32);
          break;
        }
      }
      if (mismatch(i)) {
        res->outcome = PRAOS_CHUNK_ERR_HASH_MISMATCH;
        res->truncate_at = col.off[i];
        res->err_slot = col.slot[i];
        std::memcpy(res->err_hash, &col.hh[32 * i], 32);
        std::memcpy(res->expected_prev, &col.hh[32 * (i - 1)], 32);
        std::memcpy(res->actual_prev, &col.prev[32 * i], 32);
        res->actual_prev_is_genesis = col.gen[i];
        break;
      }
      y++;
    }
    res->blocks = y;
    if (y > out->cap) { c->err = "praos_validate_chunk: out->cap too small"; return PRAOS_E_ARG; }
    if (y && (!out->entries || !out->block_no || !out->prev_hash || !out->prev_is_genesis || !out->integrity))
      return PRAOS_E_ARG;
    for (size_t i = 0; i < y; i++) {
      uint8_t* e = out->entries + PRAOS_CHUNK_ENTRY_SIZE * i;
      put_be(e, col.off[i], 8);
      put_be(e + 8, col.hoff[i] - col.off[i], 2);
      put_be(e + 10, col.hlen[i], 2);
      put_be(e + 12, col.crc[i], 4);
      std::memcpy(e + 16, &col.hh[32 * i], 32);
      put_be(e + 48, col.kind[i] == 1 ? col.epoch[i] : col.slot[i], 8);   // blockOrEBB: an EBB's epoch number
      if (is_ebb) is_ebb[i] = col.kind[i] == 1;
      out->block_no[i] = col.block_no[i];
      std::memcpy(out->prev_hash + 32 * i, &col.prev[32 * i], 32);
      out->prev_is_genesis[i] = col.gen[i];
      out->integrity[i] = trusted(i) ? -1 : 0;
    }
    return PRAOS_OK;
  };
  const int r = run();
  (void)hipStreamSynchronize(c->side[0]);
  (void)hipStreamSynchronize(c->stream);
  // the batches that borrow the arena go first
  praos_batch_free(c, b4);
  praos_batch_free(c, b3);
  praos_batch_free(c, b2 && b1 ? b2 : nullptr);
  praos_batch_free(c, b1 ? b1 : b2);
  return r;
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
  const size_t n = b->n;
  if (n == 0) return PRAOS_OK;
  HIPCHK(c, d2h(c, out->bits, b->bits, 2 * n));
  if (out->pool_idx) HIPCHK(c, d2h(c, out->pool_idx, b->pool_idx, 4 * n));
  if (out->beta) HIPCHK(c, d2h(c, out->beta, b->beta, 64 * n));
  if (out->leader) HIPCHK(c, d2h(c, out->leader, b->leader, 32 * n));
  if (out->nonce) HIPCHK(c, d2h(c, out->nonce, b->nonce, 32 * n));
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
  std::vector<uint32_t> tab(9 * (size_t)k, 0);
  for (uint32_t e = 0; e < k; e++) {
    if (!etas[e].neutral) std::memcpy(&tab[9 * e], etas[e].hash, 32);
    tab[9 * e + 8] = etas[e].neutral ? 1u : 0u;
  }
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
  const size_t n = b->n;
  if (n == 0) return PRAOS_OK;
  auto dn = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return dst ? d2h(c, dst, src, bytes) : hipSuccess;
  };
  HIPCHK(c, dn(d->status, b->dec_status, 2 * n));
  HIPCHK(c, dn(d->block_no, b->block_no, 8 * n));
  HIPCHK(c, dn(d->slot, b->slot, 8 * n));
  HIPCHK(c, dn(d->prev_hash, b->prev_hash, 32 * n));
  HIPCHK(c, dn(d->prev_is_genesis, b->prev_genesis, n));
  HIPCHK(c, dn(d->cold_vk, b->cold_vk, 32 * n));
  HIPCHK(c, dn(d->vrf_vk, b->vrf_vk, 32 * n));
  HIPCHK(c, dn(d->vrf_out, b->vrf_out, 64 * n));
  HIPCHK(c, dn(d->vrf_proof, b->vrf_proof, 80 * n));
  HIPCHK(c, dn(d->body_size, b->body_size, 4 * n));
  HIPCHK(c, dn(d->body_hash, b->body_hash, 32 * n));
  HIPCHK(c, dn(d->hot_vk, b->hot_vk, 32 * n));
  HIPCHK(c, dn(d->ocert_n, b->ocert_n, 8 * n));
  HIPCHK(c, dn(d->ocert_c0, b->ocert_c0, 8 * n));
  HIPCHK(c, dn(d->ocert_sig, b->ocert_sig, 64 * n));
  HIPCHK(c, dn(d->prot_major, b->prot_major, 8 * n));
  HIPCHK(c, dn(d->prot_minor, b->prot_minor, 8 * n));
  HIPCHK(c, dn(d->kes_sig, b->kes_sig, 448 * n));
  HIPCHK(c, dn(d->signed_len, b->body_len, 4 * n));
  HIPCHK(c, dn(d->signed_body, b->body, (size_t)b->signed_stride * n));
  HIPCHK(c, dn(d->header_hash, b->header_hash, 32 * n));
  return PRAOS_OK;
}

int praos_decode_headers(praos_ctx* c, const praos_header_bytes* in, praos_decoded* out) {
  if (!c || !in || !out) return PRAOS_E_ARG;
  if (c->device < 0) { c->err = "host-only context: no HIP device"; return PRAOS_E_STATE; }
  if (in->n == 0) return PRAOS_OK;
  praos_batch* b = praos_batch_upload_bytes(c, in);
  if (!b) return PRAOS_E_OOM;
  int r = batch_decode(c, b);
  if (r == PRAOS_OK) r = praos_batch_download_decoded(c, b, out);
  praos_batch_free(c, b);
  return r;
}

}  // extern "C"

// ---------------------------------------------------------------- replay pipeline (internal, C++ linkage)
// A batch the context keeps between calls (the replay's RP_SLOTS batches, the stored-bytes
// pipeline's batch) goes through here every time it is taken for another run: every per-run field
// back to the state of a fresh batch, so nothing one call set (its header count, "decoded",
// "stage V queued", the key-cache / dedup use of its last run, the nonce table's use) can reach
// the next call, whichever entry point made either.  Buffers, capacities and events stay.
static void batch_reuse_reset(praos_batch* b) {
  b->n = 0;
  b->arena_len = 0;
  b->body_bytes_len = 0;
  b->decoded = false;
  b->v_done = false;
  b->kc_used = false;
  b->dd_used = false;
  for (auto& k : b->kc) {            // this run's entry space (set again by the run's key lists)
    k.kt = nullptr; k.ki = nullptr; k.erep = nullptr; k.epos = nullptr; k.ebase = nullptr;
    k.emax = 0; k.store = -1;
  }
}

praos_batch* rp_batch_alloc(praos_ctx* c, size_t n_cap, size_t bytes_cap, bool tpraos) {
  if (!c || c->device < 0) return nullptr;
  (void)hipSetDevice(c->device);
  praos_batch* b = bytes_batch_alloc(c, std::max<size_t>(n_cap, 1), std::max<size_t>(bytes_cap, 8), tpraos, nullptr);
  if (!b) return nullptr;
  b->cap_n = std::max<size_t>(n_cap, 1);
  b->cap_bytes = std::max<size_t>(bytes_cap, 8);
  bool ok = dalloc(b, &b->eta_tab, 9 * 4 * 256) == hipSuccess && dalloc(b, &b->eta_idx, b->cap_n) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&b->dec_ev, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&b->run_ev, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventRecord(b->run_ev, c->stream) == hipSuccess;     // recorded once: waits on it are defined
  ok = ok && hipHostMalloc((void**)&b->eta_h, 9 * 4 * 256, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&b->eidx_h, b->cap_n, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&b->res_bits_h, 2 * b->cap_n, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&b->res_pidx_h, 4 * b->cap_n, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&b->dec_h, DEC_H_BYTES * b->cap_n, hipHostMallocDefault) == hipSuccess;
  if (!ok) { rp_batch_destroy(c, b); return nullptr; }
  return b;
}

// the batch's pinned result buffers (kept with it between calls: no page-locking per call)
void rp_batch_results(praos_batch* b, uint16_t** bits, int32_t** pidx) {
  *bits = b->res_bits_h;
  *pidx = b->res_pidx_h;
}

void rp_batch_destroy(praos_ctx* c, praos_batch* b) {
  if (!b) return;
  if (c) (void)hipSetDevice(c->device);
  if (b->dec_ev) (void)hipEventSynchronize(b->dec_ev);
  if (b->run_ev) (void)hipEventSynchronize(b->run_ev);
  if (b->dec_ev) (void)hipEventDestroy(b->dec_ev);
  if (b->run_ev) (void)hipEventDestroy(b->run_ev);
  if (b->eta_h) (void)hipHostFree(b->eta_h);
  if (b->eidx_h) (void)hipHostFree(b->eidx_h);
  if (b->res_bits_h) (void)hipHostFree(b->res_bits_h);
  if (b->res_pidx_h) (void)hipHostFree(b->res_pidx_h);
  if (b->dec_h) (void)hipHostFree(b->dec_h);
  for (void* p : b->owned) (void)hipFree(p);
  delete b;
}

bool rp_batch_fits(const praos_batch* b, size_t n, size_t bytes) { return b && n <= b->cap_n && bytes <= b->cap_bytes; }

praos_batch* rp_batch_take(praos_ctx* c, int k, size_t n, size_t bytes, bool tpraos) {
  if (!c || k < 0 || k >= RP_SLOTS) return nullptr;
  praos_batch* b = c->rp_keep[k];
  c->rp_keep[k] = nullptr;
  if (b && rp_batch_fits(b, n, bytes) && b->tp_only == tpraos) {
    batch_reuse_reset(b);
    return b;
  }
  rp_batch_destroy(c, b);
  return rp_batch_alloc(c, n + n / 8 + 64, bytes + bytes / 8 + 4096, tpraos);
}

void rp_batch_quiesce(praos_batch* b) {
  if (!b) return;
  if (b->dec_ev) (void)hipEventSynchronize(b->dec_ev);
  if (b->run_ev) (void)hipEventSynchronize(b->run_ev);
}

void rp_batch_keep(praos_ctx* c, int k, praos_batch* b) {
  if (!c || k < 0 || k >= RP_SLOTS) { rp_batch_destroy(c, b); return; }
  if (c->rp_keep[k] && c->rp_keep[k] != b) rp_batch_destroy(c, c->rp_keep[k]);
  c->rp_keep[k] = b;
}

// H2D of the concatenation of spans through the two pinned staging buffers: the pool's
// threads gather each 16 MB piece (many small spans or a few large ones) while the DMA
// engine moves the previous piece
static hipError_t h2d_gather(praos_ctx* c, uint8_t* dst, const praos_span* sp, size_t ns, size_t total,
                             hipStream_t st) {
  if (!stage_init(c)) return hipErrorOutOfMemory;
  std::vector<size_t> pre(ns + 1, 0);
  for (size_t j = 0; j < ns; j++) pre[j + 1] = pre[j] + sp[j].len;
  for (size_t off = 0, k = 0; off < total; off += STAGE_PIECE, k++) {
    const size_t len = std::min(STAGE_PIECE, total - off);
    hipError_t e = hipEventSynchronize(c->pin_ev[k & 1]);    // the DMA that last read this buffer
    if (e != hipSuccess) return e;
    uint8_t* pin = c->pin[k & 1];
    const unsigned nt = c->pool->size();
    c->pool->run([&](unsigned t) {
      size_t a = off + len * t / nt;
      const size_t b_ = off + len * (t + 1) / nt;
      size_t j = (size_t)(std::upper_bound(pre.begin(), pre.end(), a) - pre.begin()) - 1;
      while (a < b_ && j < ns) {
        const size_t in = a - pre[j], m = std::min(b_ - a, sp[j].len - in);
        std::memcpy(pin + (a - off), sp[j].p + in, m);
        a += m;
        j++;
      }
    });
    e = hipMemcpyAsync(dst + off, pin, len, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(c->pin_ev[k & 1], st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int rp_upload_decode(praos_ctx* c, praos_batch* b, size_t n, const praos_span* spans, size_t nspans,
                     const uint64_t* hoff, const uint32_t* hlen) {
  size_t bytes = 0;
  for (size_t j = 0; j < nspans; j++) bytes += spans[j].len;
  if (!c || !b || !rp_batch_fits(b, n, bytes) || (n && (!hoff || !hlen))) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  // the batch's previous crypto run (ctx stream) reads the buffers rewritten below
  HIPCHK(c, hipStreamWaitEvent(c->cstream, b->run_ev, 0));
  b->n = n;
  b->arena_len = bytes;
  b->body_bytes_len = (size_t)b->signed_stride * n;
  b->decoded = true;                               // praos_batch_run skips the decode
  const size_t pad = ((bytes + 7) & ~(size_t)7) + 16 - bytes;
  HIPCHK(c, zero_pad(c, b->arena + bytes, pad, c->cstream));
  if (bytes) HIPCHK(c, h2d_gather(c, b->arena, spans, nspans, bytes, c->cstream));
  if (n) {
    HIPCHK(c, h2d_on(c, b->hoff, hoff, 8 * n, c->cstream));
    HIPCHK(c, h2d_on(c, b->hlen, hlen, 4 * n, c->cstream));
    launch_decode_praos(dim3(nblocks(n, NT)), dim3(NT), c->cstream, n, b->arena, bytes, b->hoff, b->hlen, b->slot,
                        b->cold_vk, b->vrf_vk, b->vrf_out, b->vrf_proof, b->hot_vk, b->ocert_sig, b->kes_sig,
                        b->ocert_n, b->ocert_c0, b->body_off, b->body_len, b->body, b->block_no, b->prev_hash,
                        b->prev_genesis, b->body_size, b->body_hash, b->prot_major, b->prot_minor, b->header_hash,
                        b->dec_status, b->tp_only ? 2 : 0, b->signed_stride, b->lead_out, b->lead_proof);
    launch_vrf_nonce(c->cstream, n, b->vrf_out, b->tp_only ? 1 : 0, b->nonce);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipEventRecord(b->dec_ev, c->cstream));
  return PRAOS_OK;
}

// The decoded fields into the batch's pinned area (direct DMA, one sync: ten pageable copies
// with a sync each took ~2-3 ms of the replay's per-batch decode stage); d's pointers and
// *nonce point into it until the batch's next download
int rp_download_decoded(praos_ctx* c, praos_batch* b, praos_decoded* d, uint8_t** nonce) {
  if (!c || !b || !d || !nonce || !b->dec_h) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = b->n;
  uint8_t* h = b->dec_h;                          // 8-byte fields first, then 32-byte, 4, 2, 1
  *d = praos_decoded{};
  d->block_no = (uint64_t*)h; h += 8 * n;
  d->slot = (uint64_t*)h; h += 8 * n;
  d->ocert_n = (uint64_t*)h; h += 8 * n;
  d->prev_hash = h; h += 32 * n;
  d->cold_vk = h; h += 32 * n;
  d->header_hash = h; h += 32 * n;
  *nonce = h; h += 32 * n;
  d->body_size = (uint32_t*)h; h += 4 * n;
  d->status = (uint16_t*)h; h += 2 * n;
  d->prev_is_genesis = h;
  if (n == 0) return PRAOS_OK;
  auto dn = [&](void* dst, const void* src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->cstream);
  };
  HIPCHK(c, dn(d->block_no, b->block_no, 8 * n));
  HIPCHK(c, dn(d->slot, b->slot, 8 * n));
  HIPCHK(c, dn(d->ocert_n, b->ocert_n, 8 * n));
  HIPCHK(c, dn(d->prev_hash, b->prev_hash, 32 * n));
  HIPCHK(c, dn(d->cold_vk, b->cold_vk, 32 * n));
  HIPCHK(c, dn(d->header_hash, b->header_hash, 32 * n));
  HIPCHK(c, dn(*nonce, b->nonce, 32 * n));
  HIPCHK(c, dn(d->body_size, b->body_size, 4 * n));
  HIPCHK(c, dn(d->status, b->dec_status, 2 * n));
  HIPCHK(c, dn(d->prev_is_genesis, b->prev_genesis, n));
  HIPCHK(c, hipStreamSynchronize(c->cstream));
  return PRAOS_OK;
}

int rp_run(praos_ctx* c, praos_batch* b, const praos_nonce* etas, uint32_t k, const uint8_t* eta_idx) {
  if (!c || !b || (b->n && (!etas || !eta_idx)) || k == 0 || k > 256) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  for (uint32_t e = 0; e < k; e++) {
    std::memset(b->eta_h + 9 * e, 0, 36);
    if (!etas[e].neutral) std::memcpy(b->eta_h + 9 * e, etas[e].hash, 32);
    b->eta_h[9 * e + 8] = etas[e].neutral ? 1u : 0u;
  }
  std::memcpy(b->eidx_h, eta_idx, b->n);
  // the pinned host buffers are reused by the next batch on this slot only after this run
  HIPCHK(c, hipStreamWaitEvent(c->stream, b->dec_ev, 0));
  HIPCHK(c, hipMemcpyAsync(b->eta_tab, b->eta_h, 36 * (size_t)k, hipMemcpyHostToDevice, c->stream));
  if (b->n) HIPCHK(c, hipMemcpyAsync(b->eta_idx, b->eidx_h, b->n, hipMemcpyHostToDevice, c->stream));
  const int r = praos_batch_run(c, b);
  if (r != PRAOS_OK) return r;
  HIPCHK(c, hipEventRecord(b->run_ev, c->stream));
  return PRAOS_OK;
}

int rp_download_results(praos_ctx* c, praos_batch* b, uint16_t* bits, int32_t* pool_idx) {
  if (!c || !b || !bits) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamWaitEvent(c->dstream, b->run_ev, 0));
  if (b->n) {
    HIPCHK(c, hipMemcpyAsync(bits, b->bits, 2 * b->n, hipMemcpyDeviceToHost, c->dstream));
    if (pool_idx) HIPCHK(c, hipMemcpyAsync(pool_idx, b->pool_idx, 4 * b->n, hipMemcpyDeviceToHost, c->dstream));
  }
  HIPCHK(c, hipStreamSynchronize(c->dstream));
  return PRAOS_OK;
}

// ---- the candidates call (praos_candidates.hip): the wire arena, the item buffers and the hash
// set live in one device buffer the context keeps between calls (like its replay batches); the
// header dedup writes the distinct headers' spans there, and the decode of a replay batch reads
// arena and spans from it, over those rows only
int rp_device(const praos_ctx* c) { return c ? c->device : -1; }
hipStream_t rp_copy_stream(praos_ctx* c) { return c->cstream; }
bool rp_have_epoch(const praos_ctx* c) { return c && c->have_epoch; }

uint8_t* rp_scratch(praos_ctx* c, size_t bytes) {
  if (!c || c->device < 0) return nullptr;
  if (c->cand_scratch && c->cand_scratch_sz >= bytes) return c->cand_scratch;
  (void)hipSetDevice(c->device);
  if (c->cand_scratch) (void)hipFree(c->cand_scratch);
  c->cand_scratch = nullptr;
  c->cand_scratch_sz = 0;
  const size_t sz = bytes + bytes / 8 + 4096;
  if (hipMalloc((void**)&c->cand_scratch, sz) != hipSuccess) { c->cand_scratch = nullptr; return nullptr; }
  c->cand_scratch_sz = sz;
  return c->cand_scratch;
}

// the spans' concatenation to dst (room for the bytes rounded up to 8, plus 16: ld64u's pad, zeroed)
// through the pinned staging buffers, on the copy stream
int rp_upload_bytes(praos_ctx* c, uint8_t* dst, const praos_span* spans, size_t nspans) {
  size_t bytes = 0;
  for (size_t j = 0; j < nspans; j++) bytes += spans[j].len;
  if (!c || !dst) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t pad = ((bytes + 7) & ~(size_t)7) + 16 - bytes;
  HIPCHK(c, zero_pad(c, dst + bytes, pad, c->cstream));
  if (bytes) HIPCHK(c, h2d_gather(c, dst, spans, nspans, bytes, c->cstream));
  return PRAOS_OK;
}

// k_decode_praos and k_vrf_nonce over rows [first, n) of a replay batch, from the device span arrays
// hoff / hlen into arena (copy stream); the batch then holds n rows
int rp_decode_rows(praos_ctx* c, praos_batch* b, const uint8_t* arena, size_t arena_len, const uint64_t* hoff,
                   const uint32_t* hlen, size_t first, size_t n) {
  if (!c || !b || !arena || !hoff || !hlen || first > n || n > b->cap_n) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (first == 0) HIPCHK(c, hipStreamWaitEvent(c->cstream, b->run_ev, 0));   // the batch's previous run reads the rows
  b->n = n;
  b->arena_len = 0;
  b->body_bytes_len = (size_t)b->signed_stride * n;
  b->decoded = true;
  if (n > first) {
    launch_decode_praos(dim3(nblocks(n - first, NT)), dim3(NT), c->cstream, n, arena, arena_len, hoff, hlen,
                        b->slot, b->cold_vk, b->vrf_vk, b->vrf_out, b->vrf_proof, b->hot_vk, b->ocert_sig, b->kes_sig,
                        b->ocert_n, b->ocert_c0, b->body_off, b->body_len, b->body, b->block_no, b->prev_hash,
                        b->prev_genesis, b->body_size, b->body_hash, b->prot_major, b->prot_minor, b->header_hash,
                        b->dec_status, b->tp_only ? 2 : 0, b->signed_stride, b->lead_out, b->lead_proof, first);
    launch_vrf_nonce(c->cstream, n - first, b->vrf_out + 64 * first, b->tp_only ? 1 : 0, b->nonce + 32 * first);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipEventRecord(b->dec_ev, c->cstream));
  return PRAOS_OK;
}

int rp_download_leader(praos_ctx* c, praos_batch* b, uint8_t* leader_out, uint8_t* leader_proof) {
  if (!c || !b || !b->tp_only) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (b->n == 0 || (!leader_out && !leader_proof)) return PRAOS_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (leader_out) HIPCHK(c, d2h(c, leader_out, b->lead_out, 64 * b->n));
  if (leader_proof) HIPCHK(c, d2h(c, leader_proof, b->lead_proof, 80 * b->n));
  return PRAOS_OK;
}

extern "C" {

// Stored-bytes verification with the upload in K chunks (contiguous runs of headers) and
// the batch's largest kernel run under it: chunk k's bytes move H2D on the copy stream
// (pinned staging, host threads) while, on the GPU, chunk k-1 is decoded (ctx stream) and
// its VRF stage V (H, Gamma, V = [s]H - [c]Gamma: over half of a header's work, and it needs
// nothing but the header) runs on vstream.  After the last chunk the rest of the batch --
// key caches, OCert, KES, U, the join, the leader test -- runs once over the whole batch, as
// praos_batch_run does (full-batch key caches, no small-batch tails).  One batch for the whole
// input, kept in the context (device buffers allocated once for a given size).
//
// async (praos_verify_header_bytes_submit): the call on pipe[slot], queued and not waited for:
// each chunk is decoded on the copy stream right after its upload (on the ctx stream the decode
// would queue behind the previous call's run), the run's end is recorded in pcall[slot].ev and the
// outputs come back in pipe_finish.  The next call's uploads, decodes and stage V then overlap this
// call's key chains, as back-to-back resident runs overlap.
static int verify_bytes_pipelined(praos_ctx* c, const praos_header_bytes* in, praos_out* out, praos_decoded* dec,
                                  int K, int slot = 0, bool async = false) {
  const auto t_entry = std::chrono::steady_clock::now();
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = in->n;
  // the arena span of the in-range headers, and offsets rebased to it
  uint64_t base = UINT64_MAX, end = 0;
  for (size_t i = 0; i < n; i++) {
    if (in->off[i] > in->bytes_len || in->len[i] > in->bytes_len - in->off[i]) continue;
    base = std::min<uint64_t>(base, in->off[i]);
    end = std::max<uint64_t>(end, in->off[i] + in->len[i]);
  }
  if (base == UINT64_MAX) base = end = 0;
  praos_ctx::PipeCall& pc = c->pcall[slot];
  if (pc.cap < n) {                     // (the slot's previous call has finished: its H2D is done)
    if (pc.off_h) (void)hipHostFree(pc.off_h);
    if (pc.len_h) (void)hipHostFree(pc.len_h);
    pc.off_h = nullptr;
    pc.len_h = nullptr;
    pc.cap = 0;
    const size_t cap = n + n / 8 + 64;
    if (hipHostMalloc((void**)&pc.off_h, 8 * cap, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&pc.len_h, 4 * cap, hipHostMallocDefault) != hipSuccess) {
      c->err = "pinned offsets";
      return PRAOS_E_OOM;
    }
    pc.cap = cap;
  }
  uint64_t* off = pc.off_h;
  std::memcpy(pc.len_h, in->len, 4 * n);
  for (size_t i = 0; i < n; i++) {   // a span outside the caller's arena stays outside
    const bool in_range = in->off[i] <= in->bytes_len && in->len[i] <= in->bytes_len - in->off[i];
    off[i] = in_range ? in->off[i] - base : UINT64_MAX / 2;
  }
  // chunk k = headers [lo_k, hi_k) and the byte range [b0_k, b1_k) of the arena its headers
  // need (relative to base); chunk k's upload covers what earlier chunks did not
  std::vector<size_t> lo(K + 1);
  std::vector<uint64_t> need(K);
  {
    // weights: head / 100 for chunk 0, tail / 100 for chunk K-1, 1 for the others
    std::vector<size_t> w(K, 100);
    w[0] = (size_t)c->knobs.pipe_head;
    if (K > 2) w[K - 1] = (size_t)c->knobs.pipe_tail;
    size_t W = 0, acc = 0;
    for (int k = 0; k < K; k++) W += w[k];
    lo[0] = 0;
    for (int k = 1; k <= K; k++) { acc += w[k - 1]; lo[k] = n * acc / W; }
  }
  uint64_t hw = 0;
  for (int k = 0; k < K; k++) {
    for (size_t i = lo[k]; i < lo[k + 1]; i++)
      if (off[i] != UINT64_MAX / 2) hw = std::max<uint64_t>(hw, off[i] + in->len[i]);
    need[k] = hw;                                 // bytes [0, need[k]) cover chunks 0..k
  }
  const uint64_t bytes = end - base;
  if (!c->pipe[slot] || c->pipe_n[slot] < n || c->pipe_bytes[slot] < bytes) {
    if (c->pipe[slot]) {
      HIPCHK(c, hipDeviceSynchronize());
      for (void* q : c->pipe[slot]->owned) (void)hipFree(q);
      delete c->pipe[slot];
      c->pipe[slot] = nullptr;
    }
    const size_t mc = n + n / 8 + 64, bc = bytes + bytes / 8 + 4096;   // headroom for the next call
    c->pipe[slot] = bytes_batch_alloc(c, mc, bc, false, nullptr);
    if (!c->pipe[slot]) return PRAOS_E_OOM;
    c->pipe_n[slot] = mc;
    c->pipe_bytes[slot] = bc;
  }
  praos_batch* b = c->pipe[slot];
  batch_reuse_reset(b);
  b->n = n;
  b->arena_len = bytes;
  b->body_bytes_len = (size_t)b->signed_stride * n;
  const size_t pad = ((bytes + 7) & ~(size_t)7) + 16 - bytes;
  HIPCHK(c, zero_pad(c, b->arena + bytes, pad, c->cstream));
  HIPCHK(c, hipMemcpyAsync(b->hoff, off, 8 * n, hipMemcpyHostToDevice, c->cstream));
  HIPCHK(c, hipMemcpyAsync(b->hlen, pc.len_h, 4 * n, hipMemcpyHostToDevice, c->cstream));
  if (c->keycache > 0 && n >= 2) {               // the comb the cached chains read (built once)
    const int rc = ensure_bcomb16(c);
    if (rc != PRAOS_OK) return rc;
  }
  const uint32_t* eta = b->eta_tab ? b->eta_tab : c->d_eta0;
  // stage V chunk by chunk under the upload, or (submitted calls, PRAOS_STREAM_CHUNK_V=0) in the
  // run over the whole batch
  const bool vrf = (c->kernels & 4) != 0 && (!async || c->knobs.stream_chunk_v);
  uint64_t sent = 0;
  for (int k = 0; k < K; k++) {
    if (need[k] > sent) {
      HIPCHK(c, h2d_on(c, b->arena + sent, in->bytes + base + sent, need[k] - sent, c->cstream));
      sent = need[k];
    }
    hipStream_t sd = async ? c->decstream : c->stream;    // the chunk's decode
    HIPCHK(c, hipEventRecord(c->up_ev[k], c->cstream));
    HIPCHK(c, hipStreamWaitEvent(sd, c->up_ev[k], 0));
    const size_t m = lo[k + 1] - lo[k];
    if (m) {
      launch_decode_praos(dim3(nblocks(m, NT)), dim3(NT), sd, lo[k + 1], b->arena, bytes, b->hoff, b->hlen,
                          b->slot, b->cold_vk, b->vrf_vk, b->vrf_out, b->vrf_proof, b->hot_vk, b->ocert_sig,
                          b->kes_sig, b->ocert_n, b->ocert_c0, b->body_off, b->body_len, b->body, b->block_no,
                          b->prev_hash, b->prev_genesis, b->body_size, b->body_hash, b->prot_major, b->prot_minor,
                          b->header_hash, b->dec_status, 0, b->signed_stride, nullptr, nullptr, lo[k]);
      HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->done_ev[k], sd));
    if (m && vrf) {
      // the chunks' stage V alternate between two streams: on one they would queue behind
      // each other (a chunk's V alone is latency-bound)
      hipStream_t sv = (k & 1) ? c->vstream2 : c->vstream;
      HIPCHK(c, hipStreamWaitEvent(sv, c->done_ev[k], 0));
      launch_vrf_v(sv, n, b->vrf_vk, b->vrf_proof, b->slot, eta, c->eta0_neutral, b->eta_idx, b->tab_vrf,
                   b->vrf_mid, lo[k], lo[k + 1], 0, 0, sched_v_ilp4(c->knobs, n));
      HIPCHK(c, hipGetLastError());
    }
  }
  if (async) HIPCHK(c, hipStreamWaitEvent(c->stream, c->done_ev[K - 1], 0));   // every chunk decoded
  const auto t_chunks = std::chrono::steady_clock::now();
  b->decoded = true;
  b->v_done = vrf;
  int r = praos_batch_run(c, b);
  if (async && std::getenv("PRAOS_SUBMIT_TRACE"))
    std::fprintf(stderr, "submit: chunks queued %.3f ms after entry, run queued %.3f ms\n",
                 std::chrono::duration<double, std::milli>(t_chunks - t_entry).count(),
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_chunks).count());
  b->decoded = false;                // (the downloads below still read b->n; the next call resets
  b->v_done = false;                 // every per-run field when it takes the batch: batch_reuse_reset)
  if (async) {
    if (r != PRAOS_OK) {             // nothing of this call is left running when it reports an error
      (void)hipDeviceSynchronize();
      return r;
    }
    praos_ctx::PipeCall& p = c->pcall[slot];
    HIPCHK(c, hipEventRecord(p.ev, c->stream));
    p.out = *out;
    p.dec = dec;
    p.active = true;
    return PRAOS_OK;
  }
  // the VRF outputs (pool index, beta, leader and nonce values: 132 of the 134 bytes per
  // header) are final once the VRF stream and its miss stream are done: they come back while KES
  // still runs.  (The two-stage VRF writes the uncached keys' outputs, and with a wide tier the
  // chunk tier's, on the miss stream, which the VRF stream does not wait for: mdone_ev[2], recorded
  // at the end of the run, covers them.  Without this wait a small batch forced to the two-stage
  // form lost the race: tests/test_gpu_group.py::test_large_batch_plan_equals_default)
  if (r == PRAOS_OK && c->concurrent) {
    HIPCHK(c, hipStreamWaitEvent(c->cstream, c->side_ev[2], 0));
    HIPCHK(c, hipStreamWaitEvent(c->cstream, c->mdone_ev[2], 0));
    auto dn = [&](void* dst, const void* src, size_t nb) -> hipError_t {
      return dst && nb ? d2h_on(c, dst, src, nb, c->cstream) : hipSuccess;
    };
    HIPCHK(c, dn(out->pool_idx, b->pool_idx, 4 * n));
    HIPCHK(c, dn(out->beta, b->beta, 64 * n));
    HIPCHK(c, dn(out->leader, b->leader, 32 * n));
    HIPCHK(c, dn(out->nonce, b->nonce, 32 * n));
    if (r == PRAOS_OK) r = praos_batch_sync(c);
    if (r == PRAOS_OK) HIPCHK(c, d2h(c, out->bits, b->bits, 2 * n));
  } else {
    if (r == PRAOS_OK) r = praos_batch_sync(c);
    if (r == PRAOS_OK) r = praos_batch_download(c, b, out);
  }
  if (r == PRAOS_OK && dec) r = praos_batch_download_decoded(c, b, dec);
  (void)hipStreamSynchronize(c->cstream);
  (void)hipStreamSynchronize(c->vstream);
  (void)hipStreamSynchronize(c->vstream2);
  return r;
}

// the outputs of submitted call `slot` (waits for its run): on the download stream, which the
// calls queued after it do not use
static int pipe_finish(praos_ctx* c, int slot) {
  praos_ctx::PipeCall& p = c->pcall[slot];
  if (!p.active) return PRAOS_OK;
  p.active = false;
  HIPCHK(c, hipSetDevice(c->device));
  const praos_batch* b = c->pipe[slot];
  const size_t n = b->n;
  HIPCHK(c, hipStreamWaitEvent(c->dstream, p.ev, 0));
  auto dn = [&](void* dst, const void* src, size_t nb) -> hipError_t {
    return dst && nb ? d2h_on(c, dst, src, nb, c->dstream) : hipSuccess;
  };
  HIPCHK(c, dn(p.out.bits, b->bits, 2 * n));
  HIPCHK(c, dn(p.out.pool_idx, b->pool_idx, 4 * n));
  HIPCHK(c, dn(p.out.beta, b->beta, 64 * n));
  HIPCHK(c, dn(p.out.leader, b->leader, 32 * n));
  HIPCHK(c, dn(p.out.nonce, b->nonce, 32 * n));
  if (praos_decoded* d = p.dec) {
    HIPCHK(c, dn(d->status, b->dec_status, 2 * n));
    HIPCHK(c, dn(d->block_no, b->block_no, 8 * n));
    HIPCHK(c, dn(d->slot, b->slot, 8 * n));
    HIPCHK(c, dn(d->prev_hash, b->prev_hash, 32 * n));
    HIPCHK(c, dn(d->prev_is_genesis, b->prev_genesis, n));
    HIPCHK(c, dn(d->cold_vk, b->cold_vk, 32 * n));
    HIPCHK(c, dn(d->vrf_vk, b->vrf_vk, 32 * n));
    HIPCHK(c, dn(d->vrf_out, b->vrf_out, 64 * n));
    HIPCHK(c, dn(d->vrf_proof, b->vrf_proof, 80 * n));
    HIPCHK(c, dn(d->body_size, b->body_size, 4 * n));
    HIPCHK(c, dn(d->body_hash, b->body_hash, 32 * n));
    HIPCHK(c, dn(d->hot_vk, b->hot_vk, 32 * n));
    HIPCHK(c, dn(d->ocert_n, b->ocert_n, 8 * n));
    HIPCHK(c, dn(d->ocert_c0, b->ocert_c0, 8 * n));
    HIPCHK(c, dn(d->ocert_sig, b->ocert_sig, 64 * n));
    HIPCHK(c, dn(d->prot_major, b->prot_major, 8 * n));
    HIPCHK(c, dn(d->prot_minor, b->prot_minor, 8 * n));
    HIPCHK(c, dn(d->header_hash, b->header_hash, 32 * n));
    HIPCHK(c, dn(d->kes_sig, b->kes_sig, 448 * n));
    HIPCHK(c, dn(d->signed_body, b->body, (size_t)b->signed_stride * n));
    HIPCHK(c, dn(d->signed_len, b->body_len, 4 * n));
  }
  HIPCHK(c, hipStreamSynchronize(c->dstream));
  return PRAOS_OK;
}

int praos_verify_drain(praos_ctx* c) {
  if (!c) return PRAOS_E_ARG;
  if (c->device < 0) return PRAOS_OK;
  int r = PRAOS_OK;
  for (int j = 0; j < PIPE_CALLS; j++) {       // oldest first: the slot the next submit reuses
    const int rj = pipe_finish(c, (c->pcall_next + j) % PIPE_CALLS);
    if (r == PRAOS_OK) r = rj;
  }
  return r;
}

int praos_verify_header_bytes_submit(praos_ctx* c, const praos_header_bytes* in, praos_out* out, praos_decoded* dec) {
  if (!c || !in || !out || !out->bits) return PRAOS_E_ARG;
  if (!c->have_epoch) return PRAOS_E_STATE;
  if (in->n && (!in->off || !in->len || (!in->bytes && in->bytes_len))) return PRAOS_E_ARG;
  int K = c->pipeline;
  if (K == 0) K = (int)std::min<size_t>(PIPE_AUTO, in->n / PIPE_MIN_CHUNK);
  K = std::min<int>(K, (int)std::min<size_t>(PIPE_MAX, in->n));
  if (in->n == 0 || K < 2 || c->device < 0) {  // too small to pipeline: the blocking call, in order
    const int r = praos_verify_drain(c);
    return r != PRAOS_OK ? r : praos_verify_header_bytes(c, in, out, dec);
  }
  const int slot = c->pcall_next;
  const auto t0 = std::chrono::steady_clock::now();
  int r = pipe_finish(c, slot);                // PIPE_CALLS in flight: the oldest one's outputs first
  if (r != PRAOS_OK) return r;
  if (std::getenv("PRAOS_SUBMIT_TRACE"))
    std::fprintf(stderr, "submit: finish of the oldest call %.3f ms\n",
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  r = verify_bytes_pipelined(c, in, out, dec, K, slot, true);
  if (r == PRAOS_OK) c->pcall_next = (slot + 1) % PIPE_CALLS;
  return r;
}

int praos_verify_header_bytes(praos_ctx* c, const praos_header_bytes* in, praos_out* out, praos_decoded* dec) {
  if (!c || !in || !out || !out->bits) return PRAOS_E_ARG;
  if (!c->have_epoch) return PRAOS_E_STATE;
  if (in->n == 0) return PRAOS_OK;
  if (in->n && (!in->off || !in->len || (!in->bytes && in->bytes_len))) return PRAOS_E_ARG;
  {
    const int rd = praos_verify_drain(c);     // submitted calls use pipe[0 .. PIPE_CALLS): finished first
    if (rd != PRAOS_OK) return rd;
  }
  {
    // chunked pipeline (PRAOS_OPT_PIPELINE: chunks; 0 = auto: up to PIPE_AUTO chunks of >= PIPE_MIN_CHUNK)
    int K = c->pipeline;
    if (K == 0) K = (int)std::min<size_t>(PIPE_AUTO, in->n / PIPE_MIN_CHUNK);
    K = std::min<int>(K, (int)std::min<size_t>(PIPE_MAX, in->n));
    if (K >= 2 && c->device >= 0) return verify_bytes_pipelined(c, in, out, dec, K);
  }
  praos_batch* b = praos_batch_upload_bytes(c, in);
  if (!b) return PRAOS_E_OOM;
  int r = praos_batch_run(c, b);
  if (r == PRAOS_OK) r = praos_batch_sync(c);
  if (r == PRAOS_OK) r = praos_batch_download(c, b, out);
  if (r == PRAOS_OK && dec) r = praos_batch_download_decoded(c, b, dec);
  praos_batch_free(c, b);
  return r;
}

}  // extern "C"

// ---- the context for the other host modules (replay, group, candidates, pbft): the shims that
// replay_internal.hpp declares
// the staging copy threads of a context onto the given CPUs (the replay's thread placement)
void rp_copy_pin(praos_ctx* c, const std::vector<int>& cpus) {
  if (c && c->device >= 0 && stage_init(c)) c->pool->pin(cpus);
}

// error text for the other host modules of the library (praos_replay.hip)
void praos_set_error_(praos_ctx* c, const std::string& m) { if (c) c->err = m; }
// the group's page-locked ranges (praos_group_host_register: pinned once, known to every member)
int praos_ctx_note_registered_(praos_ctx* c, void* p, size_t len, bool add) {
  if (!c) return PRAOS_E_ARG;
  std::lock_guard<std::mutex> g(c->reg_mu);
  if (add) {
    c->registered.emplace_back((uintptr_t)p, len);
    return PRAOS_OK;
  }
  auto it = std::find_if(c->registered.begin(), c->registered.end(),
                         [&](const std::pair<uintptr_t, size_t>& r) { return r.first == (uintptr_t)p; });
  if (it == c->registered.end()) return PRAOS_E_ARG;
  c->registered.erase(it);
  return PRAOS_OK;
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
  uint8_t *dlout = nullptr, *dlproof = nullptr, *dbeta_l = nullptr;
  int rc = PRAOS_OK;
  if (dalloc(b, &dlout, 64 * n) != hipSuccess || dalloc(b, &dlproof, 80 * n) != hipSuccess ||
      dalloc(b, &dbeta_l, 64 * n) != hipSuccess) {
    praos_batch_free(c, b);
    return PRAOS_E_OOM;
  }
  auto body = [&]() -> int {
    HIPCHK(c, hipMemcpy(dlout, th->leader_out, 64 * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dlproof, th->leader_proof, 80 * n, hipMemcpyHostToDevice));
    b->tp_only = true;
    b->lead_out = dlout;
    b->lead_proof = dlproof;
    b->beta_l = dbeta_l;
    const int r = praos_batch_run(c, b);
    return r == PRAOS_OK ? tpraos_download(c, b, dbeta_l, out) : r;
  };
  rc = body();
  praos_batch_free(c, b);
  return rc;
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
  auto body = [&]() -> int {
    int r = praos_batch_run(c, b);             // decode, then the TPraos passes
    if (r == PRAOS_OK) r = tpraos_download(c, b, b->beta_l, out);
    if (r == PRAOS_OK && dec) r = praos_batch_download_decoded(c, b, dec);
    if (r == PRAOS_OK && leader_out) HIPCHK(c, d2h(c, leader_out, b->lead_out, 64 * n));
    if (r == PRAOS_OK && leader_proof) HIPCHK(c, d2h(c, leader_proof, b->lead_proof, 80 * n));
    return r;
  };
  const int rc = body();
  praos_batch_free(c, b);
  return rc;
}

}  // extern "C"
