// praos_blocks.hip -- validation of stored blocks: block-integrity batches (k_block.hip), CRC-32 of
// spans (k_crc32.hip), Byron integrity (k_byron.hip), the device half of PBFT header validation
// (k_pbft.hip) and ImmutableDB chunk validation, which composes them.
#include "api_internal.hpp"

using namespace praos_impl;

// nothing is launched on a span outside the arena: the kernels do not range-check
static int spans_inside(praos_ctx* c, const char* who, const uint64_t* off, const uint32_t* len, size_t n,
                        uint64_t bytes_len) {
  const size_t i = first_bad_span(off, len, n, bytes_len);
  if (i == n) return PRAOS_OK;
  c->err = std::string(who) + ": span " + std::to_string(i) + " outside the arena";
  return PRAOS_E_ARG;
}

extern "C" {

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
  launch_kes(c->stream, n, KeyItems{}, c->btab, batch_kes_in(b, slots_per_kes_period, bk));
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
  if (praos_host_only_(c)) return PRAOS_E_STATE;
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

int praos_crc32(praos_ctx* c, const praos_header_bytes* s, uint32_t* crc) {
  if (!c || !s || (s->n && (!s->off || !s->len || !crc)) || (!s->bytes && s->bytes_len) || s->n > 0x7fffffffu)
    return PRAOS_E_ARG;
  if (spans_inside(c, "praos_crc32", s->off, s->len, s->n, s->bytes_len) != PRAOS_OK) return PRAOS_E_ARG;
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  if (s->n == 0) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = s->n;
  ScratchBatch scratch(c, n);
  praos_batch* b = scratch.b;
  b->arena_len = s->bytes_len;
  bool ok = dalloc(b, &b->arena, arena_room(s->bytes_len)) == hipSuccess;
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
    if (spans_inside(c, "praos_block_batch_crc32", off.data(), len.data(), n, b->arena_len) != PRAOS_OK)
      return PRAOS_E_ARG;
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
  if (praos_host_only_(c)) return PRAOS_E_STATE;
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
  ScratchBatch scratch(c, n);
  praos_batch* b = scratch.b;
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
    launch_pbft_sig(st, n, KeyItems{list, count}, c->btab, d_keys, d_sig, d_hram, d_bits, b->tab_ocert);
  };
  if (cached) {
    RunShape shape = run_shape(c, n, false, false);
    shape.pool_keys = 0;                               // the batch's own entries, not the pool-key store
    const RunPlan P = plan_run(c->knobs, shape);
    const int r = kc_lists(c, b, P, k, n, d_keys, st, KeyItems{d_vlist, d_vcount}, 0);
    if (r == PRAOS_OK) kc_precompute(c, P, k, d_keys, 0, st, n);
    if (r != PRAOS_OK) return r;
    launch_pbft_sig_ck(st, n, key_hits(k), c->bcomb16, d_keys, d_sig, d_hram, d_bits);
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
  ScratchBatch scratch(c, n);
  return pbft_verify_dev(c, scratch.b, n, arena, arena_len, hoff, hlen, d_is_ebb, p, delegs, n_delegs, out);
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
  if (spans_inside(c, "praos_verify_pbft_headers", in->off, in->len, n, in->bytes_len) != PRAOS_OK) return PRAOS_E_ARG;
  if (!praos_pbft_delegs_ok_(delegs, n_delegs)) {
    c->err = "pbft: duplicate hash in the delegation map";
    return PRAOS_E_ARG;
  }
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  if (n == 0) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // the arena behind 8 zero bytes: the header hash reads the two bytes before a header (its
  // 82 0k prefix replaces them), and a header may start at offset 0 of the caller's arena
  constexpr size_t FRONT = 8;
  std::vector<uint64_t> off(n);
  for (size_t i = 0; i < n; i++) off[i] = in->off[i] + FRONT;
  const size_t alen = FRONT + in->bytes_len;
  ScratchBatch scratch(c, n);
  praos_batch* b = scratch.b;
  uint8_t* d_ebb = nullptr;
  bool ok = dalloc(b, &b->arena, arena_room(alen)) == hipSuccess;
  ok &= dalloc(b, &b->hoff, 8 * n) == hipSuccess;
  ok &= dalloc(b, &b->hlen, 4 * n) == hipSuccess;
  ok &= dalloc(b, &d_ebb, n) == hipSuccess;
  if (!ok) { c->err = "device allocation failed"; return PRAOS_E_OOM; }
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemsetAsync(b->arena, 0, FRONT, st));
  HIPCHK(c, hipMemsetAsync(b->arena + alen, 0, arena_pad(alen), st));
  if (in->bytes_len) HIPCHK(c, h2d(c, b->arena + FRONT, in->bytes, in->bytes_len));
  HIPCHK(c, hipMemcpyAsync(b->hoff, off.data(), 8 * n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(b->hlen, in->len, 4 * n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_ebb, is_ebb, n, hipMemcpyHostToDevice, st));
  return pbft_verify_dev(c, b, n, b->arena, alen, b->hoff, b->hlen, d_ebb, p, delegs, n_delegs, out);
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
  if (praos_host_only_(c)) return PRAOS_E_STATE;
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

}  // extern "C"
