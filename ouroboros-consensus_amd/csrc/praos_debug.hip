// praos_debug.hip -- single-primitive batches, the header generator, the leader schedule and the
// praos_debug_* entry points the tests drive.
#include "api_internal.hpp"

using namespace praos_impl;

// ---------------------------------------------------------------- single-primitive batches
namespace {
struct Scratch {
  praos_ctx* c;
  std::vector<void*> ptrs;
  bool ok = true;
  explicit Scratch(praos_ctx* cc) : c(cc) {}
  ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
  template <typename T>
  T* up(const T* src, size_t bytes) {
    void* d = nullptr;
    if (hipMalloc(&d, bytes ? bytes : 16) != hipSuccess) { ok = false; return nullptr; }
    ptrs.push_back(d);
    if (src && bytes && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return (T*)d;
  }
  template <typename T>
  T* zeros(size_t bytes) {
    T* d = up<T>(nullptr, bytes);
    // on the ctx stream: a null-stream hipMemset is not ordered with the (non-blocking)
    // stream the kernel runs on and could land after the kernel's writes
    if (d && hipMemsetAsync(d, 0, bytes ? bytes : 16, c->stream) != hipSuccess) ok = false;
    return d;
  }
};
}  // namespace
extern "C" {

int praos_verify_ocert(praos_ctx* c, size_t n, const uint8_t* cold_vk, const uint8_t* hot_vk, const uint64_t* ocert_n,
                       const uint64_t* ocert_c0, const uint8_t* sig, uint8_t* ok) {
  if (!c || (n && (!cold_vk || !hot_vk || !ocert_n || !ocert_c0 || !sig || !ok))) return PRAOS_E_ARG;
  if (n == 0) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto dv = s.up(cold_vk, 32 * n);
  auto dh = s.up(hot_vk, 32 * n);
  auto dn = s.up(ocert_n, 8 * n);
  auto dc = s.up(ocert_c0, 8 * n);
  auto ds = s.up(sig, 64 * n);
  auto dok = s.zeros<uint8_t>(n);
  auto dtab = s.up<ge_cached>(nullptr, LT_ED_B * n);
  if (!s.ok) { c->err = "alloc/copy"; return PRAOS_E_OOM; }
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  OcertIn a{};                                   // plain mode: the verdicts to ok_out, no period checks
  a.cold_vk = dv;
  a.hot_vk = dh;
  a.ocert_n = dn;
  a.ocert_c0 = dc;
  a.sig = ds;
  a.slots_per_kes_period = 1;
  a.ok_out = dok;
  a.tabs = dtab;
  launch_ocert(c->stream, n, KeyItems{}, c->btab, a);
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  (void)hipEventElapsedTime(&c->kernel_ms[0], c->ev[0], c->ev[1]);
  HIPCHK(c, hipMemcpy(ok, dok, n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_verify_kes(praos_ctx* c, size_t n, const uint8_t* vk, const uint32_t* period, const uint8_t* sig,
                     const uint64_t* msg_off, const uint32_t* msg_len, const uint8_t* msg_bytes, size_t msg_bytes_len,
                     uint8_t* result) {
  if (!c || (n && (!vk || !period || !sig || !msg_off || !msg_len || !result))) return PRAOS_E_ARG;
  if (n == 0) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<uint64_t> off(n);
  std::vector<uint32_t> len(n);
  size_t total = 0;
  for (size_t i = 0; i < n; i++) { off[i] = total; total += (msg_len[i] + 7) & ~(size_t)7; }
  std::vector<uint8_t> arena(total + 16, 0);
  for (size_t i = 0; i < n; i++) {
    const bool okr = msg_off[i] <= msg_bytes_len && msg_len[i] <= msg_bytes_len - msg_off[i];
    len[i] = okr ? msg_len[i] : 0xffffffffu;
    if (okr && msg_len[i]) std::memcpy(arena.data() + off[i], msg_bytes + msg_off[i], msg_len[i]);
  }
  Scratch s(c);
  auto dvk = s.up(vk, 32 * n);
  auto dp = s.up(period, 4 * n);
  auto dsig = s.up(sig, 448 * n);
  auto doff = s.up(off.data(), 8 * n);
  auto dlen = s.up(len.data(), 4 * n);
  auto dmsg = s.up(arena.data(), arena.size());
  auto dres = s.zeros<uint8_t>(n);
  auto dtab = s.up<ge_cached>(nullptr, LT_ED_B * n);
  if (!s.ok) { c->err = "alloc/copy"; return PRAOS_E_OOM; }
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  KesIn a{};                                     // plain mode: the caller's periods, the verdicts to result
  a.hot_vk = dvk;
  a.kes_sig = dsig;
  a.body_off = doff;
  a.body_len = dlen;
  a.body = dmsg;
  a.body_bytes_len = total;
  a.slots_per_kes_period = 1;
  a.period = dp;
  a.result = dres;
  a.tabs = dtab;
  launch_kes(c->stream, n, KeyItems{}, c->btab, a);
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  (void)hipEventElapsedTime(&c->kernel_ms[1], c->ev[0], c->ev[1]);
  HIPCHK(c, hipMemcpy(result, dres, n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_verify_vrf(praos_ctx* c, size_t n, const uint8_t* vk, const uint8_t* proof, const uint8_t* alpha,
                     uint8_t* ok, uint8_t* beta) {
  if (!c || (n && (!vk || !proof || !alpha || !ok))) return PRAOS_E_ARG;
  if (n == 0) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto dvk = s.up(vk, 32 * n);
  auto dpr = s.up(proof, 80 * n);
  auto dal = s.up(alpha, 32 * n);
  auto dok = s.zeros<uint8_t>(n);
  auto dbeta = s.zeros<uint8_t>(64 * n);
  auto dtab = s.up<ge_cached>(nullptr, LT_VRF_B * n);
  if (!s.ok) { c->err = "alloc/copy"; return PRAOS_E_OOM; }
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  VrfIn a{};                                     // plain mode: the caller's alphas, ok and beta only
  a.vrf_vk = dvk;
  a.vrf_proof = dpr;
  a.eta0_neutral = 1;
  a.alpha_in = dal;
  a.beta_out = dbeta;
  a.ok_out = dok;
  a.tabs = dtab;
  launch_vrf(c->stream, n, KeyItems{}, c->btab, a);
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  (void)hipEventElapsedTime(&c->kernel_ms[2], c->ev[0], c->ev[1]);
  HIPCHK(c, hipMemcpy(ok, dok, n, hipMemcpyDeviceToHost));
  if (beta) HIPCHK(c, hipMemcpy(beta, dbeta, 64 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_check_leader(praos_ctx* c, size_t n, const uint8_t* leader, const uint8_t* sigma_fp,
                       const praos_params* params, uint8_t* is_leader) {
  if (!c || !params || (n && (!leader || !sigma_fp || !is_leader))) return PRAOS_E_ARG;
  if (n == 0) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<uint32_t> x(4 * n);
  for (size_t i = 0; i < n; i++) {
    uint8_t xr[16];
    if (!praos_host::leader_x_raw(xr, sigma_fp + 16 * i, params->c_raw)) { c->err = "x out of range"; return PRAOS_E_ARG; }
    std::memcpy(&x[4 * i], xr, 16);
  }
  Scratch s(c);
  auto dl = s.up(leader, 32 * n);
  auto dx = s.up(x.data(), 16 * n);
  auto dres = s.zeros<uint8_t>(n);
  if (!s.ok) { c->err = "alloc/copy"; return PRAOS_E_OOM; }
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  launch_leader(dim3(nblocks(n, NT)), dim3(NT), c->stream, n, dl, (const int32_t*)nullptr,
                (const uint32_t*)nullptr, dx, (int)params->f_is_one, 8, (const uint16_t*)nullptr,
                (const uint16_t*)nullptr, (const uint16_t*)nullptr, (uint16_t*)nullptr, dres, (int32_t*)nullptr, (const uint16_t*)nullptr);
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  (void)hipEventElapsedTime(&c->kernel_ms[3], c->ev[0], c->ev[1]);
  HIPCHK(c, hipMemcpy(is_leader, dres, n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

// ---------------------------------------------------------------- generator
}  // extern "C"
static int synthesize_impl(praos_ctx* c, const praos_synth_params* sp, const praos_params* params,
                           const uint8_t eta0[32], praos_pool* pools_out, uint64_t* slot, uint8_t* cold_vk,
                           uint8_t* vrf_vk, uint8_t* vrf_out, uint8_t* vrf_proof, uint8_t* hot_vk, uint64_t* ocert_n,
                           uint64_t* ocert_c0, uint8_t* ocert_sig, uint8_t* kes_sig, uint64_t* body_off,
                           uint32_t* body_len, uint8_t* body_bytes, uint8_t* corrupted, int tpraos,
                           uint8_t* leader_out, uint8_t* leader_proof) {
  if (!c || !sp || !params || sp->npools == 0 || params->slots_per_kes_period == 0) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = sp->n, np = sp->npools;
  // body_len 0: genuine CBOR bodies, PRAOS_SIGNED_STRIDE (Praos HeaderBody) or
  // TP_SIGNED_STRIDE (TPraos BHBody) bytes per header
  const size_t bstride = sp->body_len ? (((size_t)sp->body_len + 7) & ~(size_t)7)
                                      : (size_t)(tpraos ? TP_SIGNED_STRIDE : PRAOS_SIGNED_STRIDE);
  Scratch s(c);
  uint32_t master[8], e0[8] = {0};
  std::memcpy(master, sp->seed, 32);
  if (eta0) std::memcpy(e0, eta0, 32);
  auto dmaster = s.up(master, 32);
  auto de0 = s.up(e0, 32);
  auto cold_seed = s.zeros<uint32_t>(32 * np);
  auto cold_pk = s.zeros<uint32_t>(32 * np);
  auto vrf_seed = s.zeros<uint32_t>(32 * np);
  auto vrf_pk = s.zeros<uint32_t>(32 * np);
  auto kes_seed = s.zeros<uint32_t>(32 * np);
  auto ph = s.zeros<uint8_t>(28 * np);
  auto pv = s.zeros<uint8_t>(32 * np);
  const size_t nk = sp->nkes ? std::min<size_t>(sp->nkes, np) : np;
  auto leaf_seed = s.zeros<uint32_t>(32 * nk * 64);
  auto tree = s.zeros<uint32_t>(32 * nk * 128);
  auto scratch = s.zeros<uint8_t>(48 * n);
  auto dslot = s.zeros<uint64_t>(8 * n);
  auto dcold = s.zeros<uint8_t>(32 * n);
  auto dvrfvk = s.zeros<uint8_t>(32 * n);
  auto dvout = s.zeros<uint8_t>(64 * n);
  auto dproof = s.zeros<uint8_t>(80 * n);
  auto dhot = s.zeros<uint8_t>(32 * n);
  auto dn = s.zeros<uint64_t>(8 * n);
  auto dc0 = s.zeros<uint64_t>(8 * n);
  auto dosig = s.zeros<uint8_t>(64 * n);
  auto dksig = s.zeros<uint8_t>(448 * n);
  auto doff = s.zeros<uint64_t>(8 * n);
  auto dlen = s.zeros<uint32_t>(4 * n);
  auto dbody = s.zeros<uint8_t>(bstride * n + 8);
  auto dcor = s.zeros<uint8_t>(n);
  auto dlout = s.zeros<uint8_t>(tpraos ? 64 * n : 16);
  auto dlproof = s.zeros<uint8_t>(tpraos ? 80 * n : 16);
  const uint8_t* dbh = sp->body_hash ? s.up(sp->body_hash, 32 * n) : nullptr;   // caller's hbBodyHash values
  if ((sp->sched_slot == nullptr) != (sp->sched_pool == nullptr)) return PRAOS_E_ARG;
  if (sp->sched_pool)
    for (size_t i = 0; i < n; i++)
      if (sp->sched_pool[i] >= np) { c->err = "sched_pool out of range"; return PRAOS_E_ARG; }
  const uint64_t* dss = sp->sched_slot ? s.up(sp->sched_slot, 8 * n) : nullptr;
  const uint32_t* dsp = sp->sched_pool ? s.up(sp->sched_pool, 4 * n) : nullptr;
  const bool link = sp->link_prev != 0;
  if (link && sp->body_len != 0) { c->err = "link_prev needs CBOR bodies (body_len 0)"; return PRAOS_E_ARG; }
  auto dleaf = s.zeros<uint32_t>(4 * n);
  auto dprev0 = link && sp->prev0 ? s.up(sp->prev0, 32) : nullptr;
  auto dlkeys = s.zeros<uint32_t>(link ? 4 * 24 * (size_t)nk * 64 : 16);   // per KES leaf: a, r, R (k_synth_link_keys)
  auto dhh = s.zeros<uint8_t>(link ? 32 * n : 16);
  if (!s.ok) { c->err = "alloc"; return PRAOS_E_OOM; }
  uint64_t salt = 0;
  std::memcpy(&salt, sp->seed, 8);
  launch_synth_pools(dim3(nblocks(np, NT)), dim3(NT), c->stream, (uint32_t)np, c->btab, dmaster,
                     cold_seed, cold_pk, vrf_seed, vrf_pk, kes_seed, ph, pv);
  launch_synth_kes_leaves(dim3(nblocks(nk * 64, NT)), dim3(NT), c->stream, (uint32_t)nk, c->btab,
                     kes_seed, leaf_seed, tree);
  launch_synth_kes_tree(dim3(nblocks(nk, 64)), dim3(64), c->stream, (uint32_t)nk, tree);
  if (n) {
    launch_synth_headers(dim3(nblocks(n, NT)), dim3(NT), c->stream, n, c->btab, (uint32_t)np,
                       (uint32_t)nk, sp->first_slot, sp->slot_stride, params->slots_per_kes_period, sp->body_len, salt, de0,
                       eta0 ? 0 : 1, cold_seed, cold_pk, vrf_seed, vrf_pk, leaf_seed, tree, scratch, dslot, dcold,
                       dvrfvk, dvout, dproof, dhot, dn, dc0, dosig, dksig, doff, dlen, dbody, tpraos, dlout, dlproof,
                       sp->body_len == 0 ? dbh : nullptr, dss, dsp, sp->block_no0, dleaf);
    if (link)
      launch_synth_link(c->stream, n, c->btab, dprev0, leaf_seed, (uint32_t)(nk * 64), dlkeys, tree, dleaf, dbody, doff,
                        dlen, dksig, dhh, (uint32_t)bstride);
    launch_synth_corrupt(dim3(nblocks(n, 256)), dim3(256), c->stream, n, sp->corrupt_per_10000,
                       salt, dosig, dksig, dproof, dvout, dbody, doff, dlen, dcor, tpraos ? dlproof : nullptr,
                       sp->body_len == 0 ? (tpraos ? 2 : 1) : 0, sp->corrupt_fields ? sp->corrupt_fields : 0x1fu, dcold, dhot, dn,
                       dc0);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<uint8_t> hh(28 * np), vv(32 * np);
  HIPCHK(c, hipMemcpy(hh.data(), ph, 28 * np, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(vv.data(), pv, 32 * np, hipMemcpyDeviceToHost));
  if (pools_out)
    for (size_t p = 0; p < np; p++) {
      std::memcpy(pools_out[p].hash28, &hh[28 * p], 28);
      std::memcpy(pools_out[p].vrf_hash32, &vv[32 * p], 32);
    }
  if (n) {
    auto dn2h = [&](void* h, const void* d, size_t bytes) -> int {
      if (h) HIPCHK(c, hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
      return PRAOS_OK;
    };
    int r = PRAOS_OK;
    r |= dn2h(slot, dslot, 8 * n); r |= dn2h(cold_vk, dcold, 32 * n); r |= dn2h(vrf_vk, dvrfvk, 32 * n);
    r |= dn2h(vrf_out, dvout, 64 * n); r |= dn2h(vrf_proof, dproof, 80 * n); r |= dn2h(hot_vk, dhot, 32 * n);
    r |= dn2h(ocert_n, dn, 8 * n); r |= dn2h(ocert_c0, dc0, 8 * n); r |= dn2h(ocert_sig, dosig, 64 * n);
    r |= dn2h(kes_sig, dksig, 448 * n); r |= dn2h(body_off, doff, 8 * n); r |= dn2h(body_len, dlen, 4 * n);
    r |= dn2h(body_bytes, dbody, bstride * n + 8); r |= dn2h(corrupted, dcor, n);
    if (tpraos) { r |= dn2h(leader_out, dlout, 64 * n); r |= dn2h(leader_proof, dlproof, 80 * n); }
    if (link) r |= dn2h(sp->header_hash, dhh, 32 * n);
    if (r != PRAOS_OK) return PRAOS_E_HIP;
  }
  return PRAOS_OK;
}
extern "C" {

int praos_synthesize(praos_ctx* c, const praos_synth_params* sp, const praos_params* params, const uint8_t eta0[32],
                     praos_pool* pools_out, uint64_t* slot, uint8_t* cold_vk, uint8_t* vrf_vk, uint8_t* vrf_out,
                     uint8_t* vrf_proof, uint8_t* hot_vk, uint64_t* ocert_n, uint64_t* ocert_c0, uint8_t* ocert_sig,
                     uint8_t* kes_sig, uint64_t* body_off, uint32_t* body_len, uint8_t* body_bytes,
                     uint8_t* corrupted) {
  return synthesize_impl(c, sp, params, eta0, pools_out, slot, cold_vk, vrf_vk, vrf_out, vrf_proof, hot_vk, ocert_n,
                         ocert_c0, ocert_sig, kes_sig, body_off, body_len, body_bytes, corrupted, 0, nullptr, nullptr);
}

int praos_synthesize_tpraos(praos_ctx* c, const praos_synth_params* sp, const praos_params* params,
                            const uint8_t eta0[32], praos_pool* pools_out, uint64_t* slot, uint8_t* cold_vk,
                            uint8_t* vrf_vk, uint8_t* vrf_out, uint8_t* vrf_proof, uint8_t* hot_vk, uint64_t* ocert_n,
                            uint64_t* ocert_c0, uint8_t* ocert_sig, uint8_t* kes_sig, uint64_t* body_off,
                            uint32_t* body_len, uint8_t* body_bytes, uint8_t* leader_out, uint8_t* leader_proof,
                            uint8_t* corrupted) {
  if (!leader_out || !leader_proof) return PRAOS_E_ARG;
  return synthesize_impl(c, sp, params, eta0, pools_out, slot, cold_vk, vrf_vk, vrf_out, vrf_proof, hot_vk, ocert_n,
                         ocert_c0, ocert_sig, kes_sig, body_off, body_len, body_bytes, corrupted, 1, leader_out,
                         leader_proof);
}

int praos_leader_schedule(praos_ctx* c, const uint8_t seed[32], uint32_t npools, const uint8_t* sigma_fp,
                          const praos_params* params, const uint8_t eta0[32], uint64_t first_slot, uint64_t nslots,
                          int tpraos, int32_t* leader) {
  if (!c || !seed || npools == 0 || !sigma_fp || !params || (nslots && !leader)) return PRAOS_E_ARG;
  if (nslots > (1ull << 32)) { c->err = "nslots > 2^32: split the range"; return PRAOS_E_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  if (nslots == 0) return PRAOS_OK;
  std::vector<uint32_t> thr(4 * (size_t)npools);
  for (uint32_t p = 0; p < npools; p++)
    if (!praos_host::leader_x_raw((uint8_t*)&thr[4 * p], sigma_fp + 16 * (size_t)p, params->c_raw)) {
      c->err = "sigma * activeSlotLog out of range";
      return PRAOS_E_ARG;
    }
  Scratch s(c);
  uint32_t master[8], e0[8] = {0};
  std::memcpy(master, seed, 32);
  if (eta0) std::memcpy(e0, eta0, 32);
  const size_t np = npools;
  auto dmaster = s.up(master, 32);
  auto de0 = s.up(e0, 32);
  auto cold_seed = s.zeros<uint32_t>(32 * np);
  auto cold_pk = s.zeros<uint32_t>(32 * np);
  auto vrf_seed = s.zeros<uint32_t>(32 * np);
  auto vrf_pk = s.zeros<uint32_t>(32 * np);
  auto kes_seed = s.zeros<uint32_t>(32 * np);
  auto vrf_x = s.zeros<uint32_t>(32 * np);
  auto ph = s.zeros<uint8_t>(28 * np);
  auto pv = s.zeros<uint8_t>(32 * np);
  auto dthr = s.up(thr.data(), 16 * np);
  auto dlead = s.up<int32_t>(nullptr, 4 * nslots);
  if (!s.ok) { c->err = "alloc"; return PRAOS_E_OOM; }
  launch_synth_pools(dim3(nblocks(np, NT)), dim3(NT), c->stream, (uint32_t)np, c->btab, dmaster, cold_seed, cold_pk,
                     vrf_seed, vrf_pk, kes_seed, ph, pv);
  launch_synth_vrf_scalar(dim3(nblocks(np, 64)), dim3(64), c->stream, (uint32_t)np, vrf_seed, vrf_x);
  HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)dlead, 0x7fffffff, nslots, c->stream));
  // pool chunks in forger order; a slot led by an earlier chunk is skipped by later ones
  constexpr uint32_t CH = 32;
  for (uint32_t p0 = 0; p0 < npools; p0 += CH) {
    const uint32_t pn = std::min(CH, npools - p0);
    const uint64_t lanes = nslots * pn;
    if (lanes / NT + 1 > 0x7fffffffull) { c->err = "range too large"; return PRAOS_E_ARG; }
    launch_synth_leader_search(dim3((unsigned)((lanes + NT - 1) / NT)), dim3(NT), c->stream, first_slot, nslots, p0,
                               pn, vrf_x, vrf_pk, dthr, de0, eta0 ? 0 : 1, (int)params->f_is_one, tpraos, dlead);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(leader, dlead, 4 * nslots, hipMemcpyDeviceToHost));
  for (uint64_t k = 0; k < nslots; k++)
    if (leader[k] == 0x7fffffff) leader[k] = -1;
  return PRAOS_OK;
}

// ---------------------------------------------------------------- debug entry points
int praos_debug_fe(praos_ctx* c, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* r) {
  if (!c || !a || !r) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto da = s.up(a, 32 * n);
  auto db = s.up(b ? b : a, 32 * n);
  auto dr = s.zeros<uint8_t>(32 * n);
  if (!s.ok) return PRAOS_E_OOM;
  if (op >= 9 && op <= 14) launch_selftest_fe(c->stream, op, n, da, db, dr);   // k_selftest.hip
  else launch_debug_fe(dim3(nblocks(n, 64)), dim3(64), c->stream, op, n, da, db, dr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(r, dr, 32 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_sha512(praos_ctx* c, size_t n, const uint8_t* prefix, const uint64_t* msg_off, const uint32_t* msg_len,
                       const uint8_t* msg_bytes, size_t msg_bytes_len, uint8_t* out) {
  if (!c) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<uint64_t> off(n);
  size_t total = 0;
  for (size_t i = 0; i < n; i++) { off[i] = total; total += (msg_len[i] + 7) & ~(size_t)7; }
  std::vector<uint8_t> arena(total + 16, 0);
  for (size_t i = 0; i < n; i++)
    if (msg_len[i]) std::memcpy(arena.data() + off[i], msg_bytes + msg_off[i], msg_len[i]);
  (void)msg_bytes_len;
  Scratch s(c);
  auto dp = s.up(prefix, 64 * n);
  auto doff = s.up(off.data(), 8 * n);
  auto dlen = s.up(msg_len, 4 * n);
  auto dmsg = s.up(arena.data(), arena.size());
  auto dout = s.zeros<uint8_t>(64 * n);
  if (!s.ok) return PRAOS_E_OOM;
  launch_debug_sha512(dim3(nblocks(n, 64)), dim3(64), c->stream, n, dp, doff, dlen, dmsg, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, 64 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_blake2b(praos_ctx* c, size_t n, const uint8_t* in64, uint8_t* out) {
  if (!c) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto di = s.up(in64, 64 * n);
  auto dout = s.zeros<uint8_t>(32 * n);
  if (!s.ok) return PRAOS_E_OOM;
  launch_debug_blake2b(dim3(nblocks(n, 64)), dim3(64), c->stream, n, di, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, 32 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_sc_reduce(praos_ctx* c, size_t n, const uint8_t* in64, uint8_t* out) {
  if (!c) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto di = s.up(in64, 64 * n);
  auto dout = s.zeros<uint8_t>(32 * n);
  if (!s.ok) return PRAOS_E_OOM;
  launch_debug_sc_reduce(dim3(nblocks(n, 64)), dim3(64), c->stream, n, di, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, 32 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_decode(praos_ctx* c, size_t n, const uint8_t* in32, uint8_t* out, uint8_t* ok) {
  if (!c) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto di = s.up(in32, 32 * n);
  auto dout = s.zeros<uint8_t>(32 * n);
  auto dok = s.zeros<uint8_t>(n);
  if (!s.ok) return PRAOS_E_OOM;
  launch_debug_decode(dim3(nblocks(n, 64)), dim3(64), c->stream, n, di, dout, dok);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, 32 * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(ok, dok, n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_scalarmult_base(praos_ctx* c, size_t n, const uint8_t* sc, uint8_t* out) {
  if (!c) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto di = s.up(sc, 32 * n);
  auto dout = s.zeros<uint8_t>(32 * n);
  if (!s.ok) return PRAOS_E_OOM;
  launch_debug_smul_base(dim3(nblocks(n, NT)), dim3(NT), c->stream, n, c->btab, di, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, 32 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_leader(praos_ctx* c, size_t n, const uint8_t* leader, const uint8_t* x_raw16, uint8_t* is_leader,
                       int32_t* iters) {
  if (!c) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto dl = s.up(leader, 32 * n);
  auto dx = s.up(x_raw16, 16 * n);
  auto dres = s.zeros<uint8_t>(n);
  auto dit = s.zeros<int32_t>(4 * n);
  if (!s.ok) return PRAOS_E_OOM;
  launch_leader(dim3(nblocks(n, NT)), dim3(NT), c->stream, n, dl, (const int32_t*)nullptr, (const uint32_t*)nullptr,
                (const uint32_t*)dx, 0, 8, (const uint16_t*)nullptr, (const uint16_t*)nullptr,
                (const uint16_t*)nullptr, (uint16_t*)nullptr, dres, dit, (const uint16_t*)nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(is_leader, dres, n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(iters, dit, 4 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_leader512(praos_ctx* c, size_t n, const uint8_t* leader64, const uint8_t* x_raw16, uint8_t* is_leader,
                          int32_t* iters) {
  if (!c) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto dl = s.up(leader64, 64 * n);
  auto dx = s.up(x_raw16, 16 * n);
  auto dres = s.zeros<uint8_t>(n);
  auto dit = s.zeros<int32_t>(4 * n);
  if (!s.ok) return PRAOS_E_OOM;
  launch_leader(dim3(nblocks(n, NT)), dim3(NT), c->stream, n, dl, (const int32_t*)nullptr, (const uint32_t*)nullptr,
                (const uint32_t*)dx, 0, 16, (const uint16_t*)nullptr, (const uint16_t*)nullptr,
                (const uint16_t*)nullptr, (uint16_t*)nullptr, dres, dit, (const uint16_t*)nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(is_leader, dres, n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(iters, dit, 4 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_hash_to_curve(praos_ctx* c, size_t n, const uint8_t* pk, const uint8_t* alpha, uint8_t* out) {
  if (!c) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto dpk = s.up(pk, 32 * n);
  auto dal = s.up(alpha, 32 * n);
  auto dout = s.zeros<uint8_t>(32 * n);
  if (!s.ok) return PRAOS_E_OOM;
  launch_debug_h2c(dim3(nblocks(n, 64)), dim3(64), c->stream, n, dpk, dal, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, 32 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_fe_multi(praos_ctx* c, int op, size_t n, const uint8_t* in, uint8_t* out) {
  if (!c || !in || !out || op < 0 || (op & 7) > 4 || op > 12) return PRAOS_E_ARG;
  if (n == 0) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto di = s.up(in, 256 * n);
  auto dout = s.zeros<uint8_t>(128 * n);
  if (!s.ok) return PRAOS_E_OOM;
  launch_selftest_fe_multi(c->stream, op, n, di, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, 128 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_ge(praos_ctx* c, int build, int op, size_t n, const uint8_t* p, const uint8_t* q, uint8_t* out) {
  if (!c || !p || !q || !out || build < 0 || build > 1 || op < 0 || op > 8) return PRAOS_E_ARG;
  if (n == 0) return PRAOS_OK;
  if (op == 7 || op == 8) {                          // the selects index tables with the digit
    for (size_t i = 0; i < n; i++) {
      int32_t d;
      uint32_t t;
      std::memcpy(&d, q + 128 * i, 4);
      std::memcpy(&t, q + 128 * i + 4, 4);
      if (op == 7 ? (d < -8 || d > 7) : (d < -128 || d > 127 || t >= BCOMB_TABLES)) return PRAOS_E_ARG;
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto dp = s.up(p, 128 * n);
  auto dq = s.up(q, 128 * n);
  auto dout = s.zeros<uint8_t>(128 * n);
  if (!s.ok) return PRAOS_E_OOM;
  if (build) launch_selftest4_ge(c->stream, op, n, dp, dq, dout, c->btab);
  else launch_selftest_ge(c->stream, op, n, dp, dq, dout, c->btab);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, 128 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

// every 32-byte little-endian scalar of s[0 .. n) is below 2^bits
static bool scalars_below(const uint8_t* s, size_t n, int bits) {
  for (size_t i = 0; i < n; i++)
    for (int k = bits / 8; k < 32; k++)
      if (k == bits / 8 ? (s[32 * i + k] >> (bits % 8)) != 0 : s[32 * i + k] != 0) return false;
  return true;
}

int praos_debug_msm(praos_ctx* c, int variant, int build, size_t n, const uint8_t* P, const uint8_t* Q,
                    const uint8_t* sp, const uint8_t* sq, const uint8_t* sb, uint8_t* out) {
  if (!c || !out || variant < 0 || variant > 6 || build < 0 || build > 1 || !P || !sp) return PRAOS_E_ARG;
  const bool use_q = variant == 2, use_b = variant != 2 && variant != 5;
  const bool wide = variant == 6, cached = variant == 3 || variant == 4 || wide;
  if (wide && n > 4096) return PRAOS_E_ARG;            // 88 KB of tables per lane
  if ((use_q && (!Q || !sq)) || (use_b && !sb)) return PRAOS_E_ARG;
  if (n == 0) return PRAOS_OK;
  if (n > (1u << 20)) return PRAOS_E_ARG;
  // the recodings' documented ranges (scalarmult.hpp)
  if (!scalars_below(sp, n, (variant == 1 || variant == 4 || wide) ? 128 : 253)) return PRAOS_E_ARG;
  if (use_q && !scalars_below(sq, n, 128)) return PRAOS_E_ARG;
  if (use_b && !scalars_below(sb, n, 253)) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (cached) {
    const int rc = ensure_bcomb16(c);
    if (rc != PRAOS_OK) return rc;
  }
  Scratch s(c);
  auto dP = s.up(P, 32 * n);
  auto dQ = use_q ? s.up(Q, 32 * n) : (uint8_t*)nullptr;
  auto dsp = s.up(sp, 32 * n);
  auto dsq = use_q ? s.up(sq, 32 * n) : (uint8_t*)nullptr;
  auto dsb = use_b ? s.up(sb, 32 * n) : (uint8_t*)nullptr;
  auto dout = s.zeros<uint8_t>(32 * n);
  ge_cached* tabs = nullptr;
  ge_cached* ktab = nullptr;
  if (cached) {
    // the key tables as the product builds them: entry e is key e, both passes of k_keys.hip
    // (pass 1 from k_keys4.hip when build = 1)
    constexpr size_t KT_BYTES = 16 * 8 * CACHED_BYTES;   // KT_STRIDE entries per key (scalarmult.hpp)
    std::vector<uint32_t> rep(n);
    for (size_t i = 0; i < n; i++) rep[i] = (uint32_t)i;
    const uint32_t cnt[4] = {(uint32_t)n, 0, 0, 0};
    auto drep = s.up(rep.data(), 4 * n);
    auto dcnt = s.up(cnt, sizeof cnt);
    auto kinfo = s.zeros<uint32_t>(9 * 4 * n);
    ktab = s.zeros<ge_cached>(KT_BYTES * n);
    KeyWide w;                                           // variant 6: every key in the wide tier, wide index = entry
    if (wide) {
      w.min_uses = 1;
      w.cap = (uint32_t)n;
      w.wide_ent = drep;
      w.wcnt = dcnt;
      w.wtab = s.zeros<ge_cached>(WT_BYTES * n);
      w.wbase = s.zeros<ge_cached>(WT_BYTES / 32 * n);
    }
    if (!s.ok) return PRAOS_E_OOM;
    launch_key_precompute(variant == 3 ? 0 : 1, c->stream, dcnt, (uint32_t)n, drep, dP, ktab, kinfo, 0, nullptr,
                          (uint32_t)n, build, w);
    if (wide) ktab = w.wtab;
  } else {
    tabs = s.zeros<ge_cached>(LT_VRF_B * n);
  }
  if (!s.ok) return PRAOS_E_OOM;
  if (build) launch_selftest4_msm(c->stream, variant, n, dP, dQ, dsp, dsq, dsb, c->btab, c->bcomb16, tabs, ktab, dout);
  else launch_selftest_msm(c->stream, variant, n, dP, dQ, dsp, dsq, dsb, c->btab, c->bcomb16, tabs, ktab, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, 32 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_hash_bytes(praos_ctx* c, int kind, size_t n, const uint8_t* arena, size_t arena_len,
                           const uint64_t* off, const uint32_t* len, const uint8_t* aux, const uint64_t* parts,
                           size_t n_parts, uint8_t* out) {
  if (!c || kind < 0 || kind > 4 || (!arena && arena_len) || n > (1u << 24) || n_parts > (1u << 26))
    return PRAOS_E_ARG;
  if (n == 0) return PRAOS_OK;
  const bool stream = kind >= 3;
  const size_t items = kind == 2 ? 4 * n : n, out_len = kind == 3 ? 64 : 32;
  if (!off || !len || !out || ((kind == 1 || kind == 2) && !aux) || (stream && !parts && n_parts)) return PRAOS_E_ARG;
  auto bad = [&](const std::string& what, size_t i) {
    c->err = "praos_debug_hash_bytes: " + what + " " + std::to_string(i);
    return PRAOS_E_ARG;
  };
  auto inside = [&](uint64_t o, uint64_t l) { return o <= arena_len && l <= arena_len - o; };
  if (stream) {
    for (size_t i = 0; i < n; i++)
      if (off[i] > n_parts || len[i] > n_parts - off[i]) return bad("part list outside the table, item", i);
    for (size_t p = 0; p < n_parts; p++) {
      const uint64_t a = parts[2 * p], b = parts[2 * p + 1];
      if (b >> 63) {
        const uint64_t k = b & ~(1ull << 63);
        if (k < 1 || k > 8) return bad("literal length outside 1..8, part", p);
      } else if (!inside(a, b)) {
        return bad("range outside the arena, part", p);
      }
    }
  } else {
    for (size_t j = 0; j < items; j++)
      if (!inside(off[j], len[j])) return bad("range outside the arena, item", j);
    for (size_t i = 0; i < n && kind == 1; i++)
      if (aux[4 * i] > 2 || off[i] < aux[4 * i]) return bad("literal prefix longer than 2 or than the offset, item", i);
    for (size_t i = 0; i < n && kind == 2; i++)
      if (aux[i] > 4) return bad("more than 4 segments, block", i);
  }
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  // the arena as arena_upload leaves it: the bytes, then zeros to the next multiple of 8 and 16 more
  const size_t padded = arena_room(arena_len);
  std::vector<uint8_t> host(padded, 0);
  if (arena_len) std::memcpy(host.data(), arena, arena_len);
  Scratch s(c);
  auto da = s.up(host.data(), padded);
  auto doff = s.up(off, 8 * items);
  auto dlen = s.up(len, 4 * items);
  auto daux = kind == 1 ? s.up(aux, 4 * n) : kind == 2 ? s.up(aux, n) : (uint8_t*)nullptr;
  auto dparts = stream ? s.up(parts, 16 * n_parts) : (uint64_t*)nullptr;
  auto dout = s.zeros<uint8_t>(out_len * items);
  if (!s.ok) return PRAOS_E_OOM;
  if (kind == 2) launch_seg_hash(dim3(nblocks(4 * n, NT)), dim3(NT), c->stream, n, da, doff, dlen, daux, dout);
  else launch_selftest_hash(c->stream, kind, n, da, doff, dlen, daux, dparts, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, out_len * items, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_int(praos_ctx* c, int op, size_t n, const uint8_t* a, const uint8_t* b, const uint8_t* cc,
                    uint8_t* out) {
  if (!c) return PRAOS_E_ARG;
  auto bad = [&](const std::string& what) {
    c->err = "praos_debug_int: " + what;
    return PRAOS_E_ARG;
  };
  if (op < 0 || op > 8) return bad("unknown op " + std::to_string(op));
  if (n == 0) return PRAOS_OK;
  if (n > (1u << 24)) return bad("more than 2^24 items");
  if (!a || !out || (op == 1 && (!b || !cc)) || (op == 8 && !b)) return bad("null array");
  // the routines' documented ranges (scalarmult.hpp, leader.hpp)
  if (op >= 3 && op <= 5 && !scalars_below(a, n, 253)) return bad("scalar not below 2^253");
  if (op == 6 && !scalars_below(a, n, 128)) return bad("scalar not below 2^128");
  for (size_t i = 0; i < n && op == 8; i++) {
    uint32_t k;
    std::memcpy(&k, b + 32 * i, 4);
    if (k < 2 || k >= 65536) return bad("divisor outside 2..65535, item " + std::to_string(i));
  }
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto da = s.up(a, 32 * n);
  auto db = (op == 1 || op == 8) ? s.up(b, 32 * n) : (uint8_t*)nullptr;
  auto dc = op == 1 ? s.up(cc, 32 * n) : (uint8_t*)nullptr;
  auto dout = s.zeros<uint8_t>(32 * n);
  if (!s.ok) return PRAOS_E_OOM;
  launch_selftest_int(c->stream, op, n, da, db, dc, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, 32 * n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_span_equal(praos_ctx* c, size_t n, const uint8_t* arena, size_t arena_len, const uint64_t* a_off,
                           const uint64_t* b_off, const uint32_t* len, uint8_t* out) {
  if (!c || (!arena && arena_len) || n > (1u << 24)) return PRAOS_E_ARG;
  if (n == 0) return PRAOS_OK;
  if (!a_off || !b_off || !len || !out) return PRAOS_E_ARG;
  for (size_t i = 0; i < n; i++)
    for (const uint64_t o : {a_off[i], b_off[i]})
      if (o > arena_len || len[i] > arena_len - o) {
        c->err = "praos_debug_span_equal: span outside the arena, pair " + std::to_string(i);
        return PRAOS_E_ARG;
      }
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  Scratch s(c);
  auto da = s.up(arena, arena_len);          // the bytes alone: the kernel reads nothing past them
  auto d_a = s.up(a_off, 8 * n);
  auto d_b = s.up(b_off, 8 * n);
  auto dlen = s.up(len, 4 * n);
  auto dout = s.zeros<uint8_t>(n);
  if (!s.ok) return PRAOS_E_OOM;
  launch_span_equal(c->stream, n, da, arena_len, d_a, d_b, dlen, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, dout, n, hipMemcpyDeviceToHost));
  return PRAOS_OK;
}

int praos_debug_row_set(praos_ctx* c, size_t n, const uint8_t* flag, const uint8_t* tag, const uint8_t* key32,
                        uint32_t tag_mask, int dedup, const uint32_t* limit, uint32_t* item_row, uint32_t* n_rows) {
  if (!c || !n_rows || n >= (1u << 24)) return PRAOS_E_ARG;
  *n_rows = 0;
  if (n == 0) return PRAOS_OK;
  if (!flag || !item_row || (dedup && (!tag || !key32))) return PRAOS_E_ARG;
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  RowSet rs;
  uint8_t *d_flag = nullptr, *d_tag = nullptr, *d_key = nullptr;
  uint64_t *ioff = nullptr, *row_off = nullptr;          // the spans the numbering compacts: zeros here
  uint32_t *ilen = nullptr, *row_len = nullptr, *total = nullptr, *d_limit = nullptr;
  size_t spans_at = 0, spans_end = 0;
  DevBuf buf;
  if (carve_alloc(buf, [&](Carve& m) {
        rs.layout(m, n);
        d_flag = m.take<uint8_t>(n);
        d_tag = m.take<uint8_t>(n);
        d_key = m.take<uint8_t>(32 * n);
        total = m.take<uint32_t>(4);
        d_limit = m.take<uint32_t>(4);
        spans_at = m.off;
        ioff = m.take<uint64_t>(8 * n);
        ilen = m.take<uint32_t>(4 * n);
        row_off = m.take<uint64_t>(8 * n);
        row_len = m.take<uint32_t>(4 * n);
        spans_end = m.off;
      }) != hipSuccess) {
    c->err = "device allocation failed";
    return PRAOS_E_OOM;
  }
  HIPCHK(c, hipMemsetAsync((uint8_t*)buf.p + spans_at, 0, spans_end - spans_at, s));
  HIPCHK(c, hipMemsetAsync(total, 0, 4, s));
  HIPCHK(c, hipMemcpyAsync(d_flag, flag, n, hipMemcpyHostToDevice, s));
  if (dedup) {
    HIPCHK(c, hipMemcpyAsync(d_tag, tag, n, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_key, key32, 32 * n, hipMemcpyHostToDevice, s));
    HIPCHK(c, rs.reset(s));
    rs.set(s, d_flag, d_tag, d_key, tag_mask);
  } else {
    if (limit) HIPCHK(c, hipMemcpyAsync(d_limit, limit, 4, hipMemcpyHostToDevice, s));
    rs.ident(s, limit ? d_limit : nullptr, d_flag, 0);
  }
  rs.number(s, total, ioff, ilen, row_off, row_len);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(item_row, rs.item_row, 4 * n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(n_rows, total, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return PRAOS_OK;
}

}  // extern "C"
