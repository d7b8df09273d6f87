// praos_xfer.hip -- host <-> device transfers of libpraos_hip: the pinned staging buffers and their
// copy threads, the staged copies in both directions, and the caller ranges page-locked with
// praos_host_register, which skip the staging.
#include "api_internal.hpp"

using namespace praos_impl;

static bool is_registered(praos_ctx* c, const void* p, size_t len) {
  std::lock_guard<std::mutex> g(c->reg_mu);
  const uintptr_t a = (uintptr_t)p;
  for (const auto& r : c->registered)
    if (a >= r.first && len <= r.second && a - r.first <= r.second - len) return true;
  return false;
}

// The piecewise upload, written once: fill(pin, off, len) puts bytes [off, off + len) of the source
// into a pinned buffer, which the DMA engine then moves while the host fills the other one.
template <typename Fill>
static hipError_t staged_upload(praos_ctx* c, uint8_t* dst, size_t bytes, hipStream_t st, Fill&& fill) {
  for (size_t off = 0, k = 0; off < bytes; off += STAGE_PIECE, k++) {
    const size_t len = std::min(STAGE_PIECE, bytes - off);
    hipError_t e = hipEventSynchronize(c->pin_ev[k & 1]);    // the DMA that last used this buffer
    if (e != hipSuccess) return e;
    fill(c->pin[k & 1], off, len);
    e = hipMemcpyAsync(dst + off, c->pin[k & 1], len, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(c->pin_ev[k & 1], st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

namespace praos_impl {

// Large H2D / D2H copies through two pinned buffers: the host threads fill (drain) one
// piece while the DMA engine moves the other, so pageable caller memory moves at PCIe
// speed instead of through the runtime's own pageable path.  Small copies go direct.
// the arena's zero padding after its last byte (< 64 bytes), copied from pinned zeros on st
hipError_t zero_pad(praos_ctx* c, uint8_t* dst, size_t pad, hipStream_t st) {
  if (!c->zero_h) {
    if (hipHostMalloc((void**)&c->zero_h, 64, hipHostMallocDefault) != hipSuccess) return hipErrorOutOfMemory;
    std::memset(c->zero_h, 0, 64);
  }
  return hipMemcpyAsync(dst, c->zero_h, pad, hipMemcpyHostToDevice, st);
}

bool stage_init(praos_ctx* c) {
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

hipError_t h2d_on(praos_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (bytes < (4u << 20) || is_registered(c, src, bytes) || !stage_init(c))
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);   // registered memory: direct DMA
  return staged_upload(c, (uint8_t*)dst, bytes, st, [&](uint8_t* pin, size_t off, size_t len) {
    c->pool->copy(pin, (const uint8_t*)src + off, len);
  });
}
// D2H on stream st, whose producers the caller has ordered before (an event wait); returns
// when the bytes are in dst
hipError_t d2h_on(praos_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (bytes < (4u << 20) || is_registered(c, dst, bytes) || !stage_init(c)) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
  }
  const size_t np = (bytes + STAGE_PIECE - 1) / STAGE_PIECE;
  hipError_t e = hipSuccess;
  for (size_t k = 0; k <= np && e == hipSuccess; k++) {
    if (k < np) {     // start piece k, then drain piece k - 1 while it moves
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

// the blocking calls' copies: on the ctx stream
hipError_t h2d(praos_ctx* c, void* dst, const void* src, size_t bytes) { return h2d_on(c, dst, src, bytes, c->stream); }
hipError_t d2h(praos_ctx* c, void* dst, const void* src, size_t bytes) { return d2h_on(c, dst, src, bytes, c->stream); }

// H2D of the concatenation of spans through the two pinned staging buffers: the pool's
// threads gather each 16 MB piece (many small spans or a few large ones) while the DMA
// engine moves the previous piece
hipError_t h2d_gather(praos_ctx* c, uint8_t* dst, const praos_span* sp, size_t ns, size_t total,
                      hipStream_t st) {
  if (!stage_init(c)) return hipErrorOutOfMemory;
  std::vector<size_t> pre(ns + 1, 0);
  for (size_t j = 0; j < ns; j++) pre[j + 1] = pre[j] + sp[j].len;
  return staged_upload(c, dst, total, st, [&](uint8_t* pin, size_t off, size_t len) {
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
  });
}

}  // namespace praos_impl

// the staging copy threads of a context onto the given CPUs (the replay's thread placement)
void rp_copy_pin(praos_ctx* c, const std::vector<int>& cpus) {
  if (c && c->device >= 0 && stage_init(c)) c->pool->pin(cpus);
}

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

extern "C" {

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

}  // extern "C"
