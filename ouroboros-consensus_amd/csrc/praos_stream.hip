// praos_stream.hip -- the batches a context keeps between calls: the replay's RP_SLOTS batches with
// the rp_* entry points that replay_internal.hpp declares for the replay, the group and the
// candidates call, and the stored-bytes pipeline (praos_verify_header_bytes, its submitted form and
// praos_verify_drain) with its batches, events and pinned offsets.
#include "api_internal.hpp"

using namespace praos_impl;

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
  HIPCHK(c, zero_pad(c, b->arena + bytes, arena_pad(bytes), c->cstream));
  if (bytes) HIPCHK(c, h2d_gather(c, b->arena, spans, nspans, bytes, c->cstream));
  if (n) {
    HIPCHK(c, h2d_on(c, b->hoff, hoff, 8 * n, c->cstream));
    HIPCHK(c, h2d_on(c, b->hlen, hlen, 4 * n, c->cstream));
    decode_launch(b, c->cstream, b->arena, bytes, b->hoff, b->hlen, 0, n);
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
  pack_nonce_table(etas, k, b->eta_h);
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
  HIPCHK(c, zero_pad(c, dst + bytes, arena_pad(bytes), c->cstream));
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
    decode_launch(b, c->cstream, arena, arena_len, hoff, hlen, first, n);
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

// the device buffers of a kept pipeline batch (its owner is null: not the spare list's)
static void pipe_batch_free(praos_ctx* c, int slot) {
  if (!c->pipe[slot]) return;
  for (void* q : c->pipe[slot]->owned) (void)hipFree(q);
  delete c->pipe[slot];
  c->pipe[slot] = nullptr;
}

void praos_impl::stream_close(praos_ctx* c) {
  for (int k = 0; k < RP_SLOTS; k++) rp_batch_destroy(c, c->rp_keep[k]);
  if (c->cand_scratch) (void)hipFree(c->cand_scratch);
  for (int k = 0; k < PIPE_MAX; k++) {
    pipe_batch_free(c, k);
    if (c->up_ev[k]) (void)hipEventDestroy(c->up_ev[k]);
    if (c->done_ev[k]) (void)hipEventDestroy(c->done_ev[k]);
  }
  for (auto& p : c->pcall) {
    if (p.ev) (void)hipEventDestroy(p.ev);
    if (p.off_h) (void)hipHostFree(p.off_h);
    if (p.len_h) (void)hipHostFree(p.len_h);
  }
}

// chunked pipeline (PRAOS_OPT_PIPELINE: chunks; 0 = auto: up to PIPE_AUTO chunks of >= PIPE_MIN_CHUNK);
// below 2 the input is too small to pipeline
static int pipe_chunks(const praos_ctx* c, size_t n) {
  int K = c->pipeline;
  if (K == 0) K = (int)std::min<size_t>(PIPE_AUTO, n / PIPE_MIN_CHUNK);
  return std::min<int>(K, (int)std::min<size_t>(PIPE_MAX, n));
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
      pipe_batch_free(c, slot);
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
  HIPCHK(c, zero_pad(c, b->arena + bytes, arena_pad(bytes), c->cstream));
  HIPCHK(c, hipMemcpyAsync(b->hoff, off, 8 * n, hipMemcpyHostToDevice, c->cstream));
  HIPCHK(c, hipMemcpyAsync(b->hlen, pc.len_h, 4 * n, hipMemcpyHostToDevice, c->cstream));
  if (c->keycache > 0 && n >= 2) {               // the comb the cached chains read (built once)
    const int rc = ensure_bcomb16(c);
    if (rc != PRAOS_OK) return rc;
  }
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
      decode_launch(b, sd, b->arena, bytes, b->hoff, b->hlen, lo[k], lo[k + 1]);
      HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->done_ev[k], sd));
    if (m && vrf) {
      // the chunks' stage V alternate between two streams: on one they would queue behind
      // each other (a chunk's V alone is latency-bound)
      hipStream_t sv = (k & 1) ? c->vstream2 : c->vstream;
      HIPCHK(c, hipStreamWaitEvent(sv, c->done_ev[k], 0));
      launch_vrf_v(sv, n, batch_vrf_v_in(c, b), b->vrf_mid, lo[k], lo[k + 1], sched_v_ilp4(c->knobs, n));
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
    praos_out early = *out;          // every output column but the bits
    early.bits = nullptr;
    HIPCHK(c, out_cols(early, *b, [&](void* dst, const void* src, size_t nb) {
      return d2h_on(c, dst, src, nb, c->cstream);
    }));
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
  HIPCHK(c, hipStreamWaitEvent(c->dstream, p.ev, 0));
  auto dn = [&](void* dst, const void* src, size_t nb) -> hipError_t {
    return nb ? d2h_on(c, dst, src, nb, c->dstream) : hipSuccess;
  };
  HIPCHK(c, out_cols(p.out, *b, dn));
  if (p.dec) HIPCHK(c, decoded_cols(*p.dec, *b, dn));
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
  const int K = pipe_chunks(c, in->n);
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
  const int K = pipe_chunks(c, in->n);
  if (K >= 2 && c->device >= 0) return verify_bytes_pipelined(c, in, out, dec, K);
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
