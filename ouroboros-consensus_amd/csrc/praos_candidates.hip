// praos_candidates.hip -- headers as the ChainSync client receives them (call
// stack 3): host C++ on top of the wire kernels (k_wire.hip), the row set of api_internal.hpp and
// the internal from-bytes batch of replay_internal.hpp.
//
//   praos_unwrap_wire_headers   every era: the inner header span and the header hash of each
//                               wire item (k_wire_split).
//   praos_validate_candidates   K candidate fragments of Praos wire headers, each from its own
//                               HeaderState (MiniProtocol/ChainSync/Client.hs:794-812):
//     device   k_wire_split, the row set (its hash set, then the numbering of the distinct headers
//              in order of first appearance, which writes their spans into the row span arrays),
//              k_decode_praos and k_vrf_nonce over those rows only;
//     host     the speculative nonce chain of each fragment from its own state (the replay's
//              chain thread: tick, candidate freeze, epoch nonce per header), which gives every
//              item an epoch nonce out of one table of at most 256; the first nonce seen for a
//              header takes its row, each further (header, nonce) pair an extra row decoded
//              from the same span by a second k_decode_praos launch;
//     device   the crypto run (rp_run) under the per-row nonces;
//     host     rp_fold per fragment in the client's mode, reading rows through the item-to-row
//              map, on at most min(K, 16) threads.
//   praos_validate_candidates_tpraos   the same pipeline for the TPraos eras (wire indices 1 to 4):
//                               batch, decode, nonce chain (TICKN's extra entropy) and fold in
//                               their TPraos modes; one implementation with the call above.
//   praos_validate_candidates_pbft     K fragments of Byron wire headers (wire index 0), each from
//                               its own tip and PBftState: the same front half, then
//                               praos_verify_pbft_headers' kernels over the distinct headers read
//                               from the wire arena, and the PBFT fold in the client's mode.
// All three share the front half (front_begin / front_run): only the era mask differs.
#include "api_internal.hpp"

#include <atomic>
#include <unordered_map>

namespace {

constexpr uint32_t NONE = PRAOS_NO_ROW;
constexpr unsigned MAX_FOLD_THREADS = 16;

// the item-side buffers of both entry points
struct ItemBufs {
  uint64_t *off, *ioff;
  uint32_t *len, *hint, *ilen;
  uint8_t *status, *era, *kind, *hash;
  void layout(Carve& m, size_t n) {
    off = m.take<uint64_t>(8 * n); ioff = m.take<uint64_t>(8 * n);
    len = m.take<uint32_t>(4 * n); hint = m.take<uint32_t>(4 * n); ilen = m.take<uint32_t>(4 * n);
    status = m.take<uint8_t>(n); era = m.take<uint8_t>(n); kind = m.take<uint8_t>(n);
    hash = m.take<uint8_t>(32 * n);
  }
};

// a call takes fewer than 2^30 items
bool cand_items_ok(const praos_header_bytes* s) { return items_ok(s) && s->n < (1ull << 30); }

// runs f(j) for j in [0, k) on at most min(k, 16) threads (never sized by the machine's cores)
void par_for(size_t k, const std::function<void(size_t)>& f) {
  const unsigned nt = (unsigned)std::min<size_t>(k, MAX_FOLD_THREADS);
  if (nt <= 1) {
    for (size_t j = 0; j < k; j++) f(j);
    return;
  }
  std::atomic<size_t> next{0};
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; t++)
    th.emplace_back([&] {
      for (size_t j; (j = next.fetch_add(1)) < k;) f(j);
    });
  for (auto& t : th) t.join();
}

// ---- the front half of every candidates call: the wire items go up once, are unwrapped and hashed
// (k_wire_split), byte-identical headers of the eras in era_mask are found and numbered in order
// of first appearance (the row set), and wire_status, the item-to-row map and the row count come
// back.  The era mask is all that differs between the calls.
bool frag_bounds_ok(const size_t* frag_first, size_t k, bool have_frags, size_t n) {
  return frag_first && (k == 0 || have_frags) && frag_first[0] == 0 && frag_first[k] == n;
}

// a device, an epoch where the call needs one, and no stored-bytes call in flight on the
// context's streams
int front_begin(praos_ctx* c, bool need_epoch) {
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  if (need_epoch && !c->have_epoch) { praos_set_error_(c, "candidates: no epoch installed (praos_set_epoch)"); return PRAOS_E_STATE; }
  return praos_verify_drain(c);
}

struct Front {
  uint8_t* arena = nullptr;                      // the wire arena (ld64u's pad behind it)
  ItemBufs d{};
  uint64_t* d_row_off = nullptr;                 // the rows' spans (room for N)
  uint32_t* d_row_len = nullptr;
  uint8_t* d_row_ebb = nullptr;                  // with row_kind: the rows' Byron kind is 0 (room for N)
  uint32_t R = 0;                                // distinct headers
  std::vector<uint32_t> base_row;                // item -> row (NONE: outside the set)
};

// N > 0.  The buffers are carved from the context's scratch and stay valid until the next
// candidates call; everything is final (the copy stream synchronised) on return.
int front_run(praos_ctx* c, const praos_header_bytes& items, uint32_t n_eras, uint32_t era_mask, bool row_kind,
              uint8_t* wire_status, Front& f) {
  const size_t N = items.n, bytes = items.bytes_len;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->cstream;
  // one device buffer, kept with the context between calls: the wire arena (with ld64u's pad), the
  // item buffers, the row set and the rows' spans and kinds (room for N: the extra (header, nonce)
  // rows of the Praos calls are written behind the R distinct ones, R2 <= N in all)
  ItemBufs& d = f.d;
  RowSet rs;
  uint32_t* total = nullptr;
  if (!carve_kept(c, [&](Carve& m) {
        f.arena = m.take<uint8_t>(arena_room(bytes));
        d.layout(m, N);
        rs.layout(m, N);
        total = m.take<uint32_t>(4);
        f.d_row_off = m.take<uint64_t>(8 * N);
        f.d_row_len = m.take<uint32_t>(4 * N);
        f.d_row_ebb = m.take<uint8_t>(N);
      })) {
    praos_set_error_(c, "candidates: device allocation failed");
    return PRAOS_E_OOM;
  }

  const praos_span whole{items.bytes, bytes};
  f.R = 0;
  f.base_row.assign(N, NONE);
  {
    const int rc = rp_upload_bytes(c, f.arena, &whole, bytes ? 1 : 0);
    if (rc != PRAOS_OK) return rc;
  }
  HIPCHK(c, items_upload(items, d.off, d.len, st));
  HIPCHK(c, rs.reset(st));
  launch_wire_split(st, N, f.arena, bytes, d.off, d.len, n_eras, d.status, d.era, d.kind, d.hint, d.ioff, d.ilen, d.hash);
  rs.set(st, d.status, d.era, d.hash, era_mask);
  rs.number(st, total, d.ioff, d.ilen, f.d_row_off, f.d_row_len);
  if (row_kind) launch_hdr_row_kind(st, N, rs.item_slot, rs.item_rep, rs.rep_row, d.kind, (uint32_t)N, f.d_row_ebb);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(&f.R, total, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(wire_status, d.status, N, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(f.base_row.data(), rs.item_row, 4 * N, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return PRAOS_OK;
}

}  // namespace

extern "C" int praos_unwrap_wire_headers(praos_ctx* c, const praos_header_bytes* items, uint32_t n_eras,
                                         praos_wire_out* out) {
  if (!c || !cand_items_ok(items) || !out) return PRAOS_E_ARG;
  const size_t n = items->n, bytes = items->bytes_len;
  if (n && (!out->status || !out->era || !out->byron_kind || !out->size_hint || !out->off || !out->len)) {
    praos_set_error_(c, "unwrap: status, era, byron_kind, size_hint, off and len are required");
    return PRAOS_E_ARG;
  }
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  if (n == 0) return PRAOS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->cstream;
  uint8_t* arena = nullptr;
  ItemBufs d;
  DevBuf buf;
  const hipError_t device_allocation = carve_alloc(buf, [&](Carve& m) {
    arena = m.take<uint8_t>(arena_room(bytes));     // ld64u's pad (arena.hpp)
    d.layout(m, n);
  });
  HIPCHK(c, device_allocation);
  HIPCHK(c, pad_zero(arena, bytes, st));
  if (bytes) HIPCHK(c, hipMemcpyAsync(arena, items->bytes, bytes, hipMemcpyHostToDevice, st));
  HIPCHK(c, items_upload(*items, d.off, d.len, st));
  launch_wire_split(st, n, arena, bytes, d.off, d.len, n_eras, d.status, d.era, d.kind, d.hint, d.ioff, d.ilen,
                    out->header_hash ? d.hash : nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out->status, d.status, n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out->era, d.era, n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out->byron_kind, d.kind, n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out->size_hint, d.hint, 4 * n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out->off, d.ioff, 8 * n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out->len, d.ilen, 4 * n, hipMemcpyDeviceToHost, st));
  if (out->header_hash) HIPCHK(c, hipMemcpyAsync(out->header_hash, d.hash, 32 * n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return PRAOS_OK;
}

namespace {

// the speculative nonce chain of one fragment (praos_replay.hip's chain thread): the epoch nonce
// tickChainDepState reaches at each item as if every header before it were valid, as runs (first
// item, nonce), and the evolving nonce after each item.  extra_entropy NULL: the Praos tick;
// non-NULL (TPraos calls only, which may also pass NULL): TICKN's tick, the extra entropy combined
// into every new epoch nonce.  Dead after an item without a decoded header: the fold stops there
// whatever comes after.
struct Run {
  size_t first;
  praos_nonce eta;
};
void spec_chain(const praos_chain_state& st, const praos_epoch_info& ei, size_t n, const uint32_t* base_row,
                const praos_decoded& d, const uint8_t* nonce, const praos_nonce* extra_entropy, std::vector<Run>& runs,
                praos_nonce* evol) {
  auto epoch_of = [&](uint64_t s) {
    return s < ei.epoch_base_slot ? ei.epoch_base_no : ei.epoch_base_no + (s - ei.epoch_base_slot) / ei.epoch_length;
  };
  int32_t origin = st.last_slot_origin;
  uint64_t sp_epoch = origin ? 0 : epoch_of(st.last_slot);
  praos_nonce evolving = st.evolving, candidate = st.candidate, epoch_nonce = st.epoch_nonce, lab = st.lab,
              leb = st.last_epoch_block;
  bool dead = false;
  runs.clear();
  for (size_t i = 0; i < n; i++) {
    const uint32_t r = base_row[i];
    if (dead || r == NONE || (d.status[r] & PRAOS_DEC_FAILED)) {
      dead = true;
      if (runs.empty()) runs.push_back({i, epoch_nonce});
      evol[i] = evolving;
      continue;
    }
    const uint64_t slot = d.slot[r];
    const uint64_t e_new = epoch_of(slot);
    if (e_new > (origin ? 0 : sp_epoch)) {
      epoch_nonce = praos_host::nonce_combine(candidate, leb);
      if (extra_entropy) epoch_nonce = praos_host::nonce_combine(epoch_nonce, *extra_entropy);   // TICKN (TPraos)
      leb = lab;
    }
    if (runs.empty() || !praos_host::nonce_eq(runs.back().eta, epoch_nonce)) runs.push_back({i, epoch_nonce});
    origin = 0;
    sp_epoch = e_new;
    lab.neutral = d.prev_is_genesis[r] ? 1 : 0;
    std::memset(lab.hash, 0, 32);
    if (!lab.neutral) std::memcpy(lab.hash, d.prev_hash + 32 * (size_t)r, 32);
    praos_nonce eta;
    std::memcpy(eta.hash, nonce + 32 * (size_t)r, 32);
    eta.neutral = 0;
    evolving = praos_host::nonce_combine(evolving, eta);
    evol[i] = evolving;
    const uint64_t first_next =
        slot < ei.epoch_base_slot ? ei.epoch_base_slot
                                  : ei.epoch_base_slot + (e_new - ei.epoch_base_no + 1) * ei.epoch_length;
    if (slot + ei.stability_window < first_next) candidate = evolving;
  }
}

}  // namespace

namespace {

// the outputs of praos_validate_candidates / praos_validate_candidates_tpraos, by pointer.  Exactly
// one of rows / tp_rows is non-NULL: rows in the Praos call (tpraos false), tp_rows in the TPraos
// call (tpraos true), where failures, leader_out and leader_proof belong too (NULL in the Praos call).
struct CandOut {
  uint8_t* wire_status;
  uint32_t* row;
  uint8_t* verdict;
  uint16_t* failures;            // TPraos
  size_t rows_cap;
  size_t* n_rows;
  uint8_t* eta_idx;
  praos_nonce* etas;
  uint32_t* n_etas;
  uint64_t* stats;               // 5
  const praos_out* rows;         // Praos
  const praos_tpraos_out* tp_rows;   // TPraos
  praos_decoded* dec;
  uint8_t *leader_out, *leader_proof;   // TPraos, may be NULL
};

// Both protocols' candidates call.  in->praos_eras is the mask of the wire indices judged (never
// 0 here); tpraos: the batch, the decode, the nonce chain's tick (extra_entropy, may be NULL) and
// the fold run in their TPraos modes.
int candidates_impl(praos_ctx* c, const praos_candidates_in* in, bool tpraos, const praos_nonce* extra_entropy,
                    praos_fragments* frags, const CandOut* out) {
  const size_t N = in->items.n, K = frags->k, bytes = in->items.bytes_len;
  if (!frag_bounds_ok(frags->frag_first, K, frags->frag != nullptr, N) || in->ei.epoch_length == 0 ||
      (N && (!out->wire_status || !out->row || !out->verdict))) {
    praos_set_error_(c, "candidates: frag_first must run from 0 to the item count; epoch_length > 0; "
                        "wire_status, row and verdict are required");
    return PRAOS_E_ARG;
  }
  for (size_t j = 0; j < K; j++) {
    const praos_chain_state& s = frags->frag[j].state;
    if (frags->frag_first[j] > frags->frag_first[j + 1] || s.m > s.cap || (s.cap && (!s.counter_hash28 || !s.counter))) {
      praos_set_error_(c, "candidates: fragment " + std::to_string(j) + ": bounds out of order or a counter map without room");
      return PRAOS_E_ARG;
    }
  }
  {
    const int rd = front_begin(c, true);
    if (rd != PRAOS_OK) return rd;
  }
  *out->n_rows = 0;
  *out->n_etas = 0;
  std::memset(out->stats, 0, 5 * sizeof(uint64_t));
  out->stats[0] = N;
  for (size_t j = 0; j < K; j++) frags->frag[j].chain_stop = frags->frag[j].processed = 0;
  if (N == 0) return PRAOS_OK;
  const uint32_t era_mask = in->praos_eras;
  // ---- device: unwrap + hash, dedup (the shared front half), then the decode of the distinct headers
  Front f;
  {
    const int rc = front_run(c, in->items, in->n_eras, era_mask, false, out->wire_status, f);
    if (rc != PRAOS_OK) return rc;
  }
  hipStream_t st = c->cstream;
  uint8_t* const arena = f.arena;
  uint64_t* const d_row_off = f.d_row_off;
  uint32_t* const d_row_len = f.d_row_len;
  const uint32_t R = f.R;
  const std::vector<uint32_t>& base_row = f.base_row;
  // a replay batch with room for the distinct headers, whatever rows_cap says: the count the
  // caller needs comes out of the nonce chains over their decoded columns
  praos_batch* b = nullptr;
  struct Keep {                                  // the batch goes back to the context on every path
    praos_ctx* c;
    praos_batch*& b;
    ~Keep() {
      if (b) { rp_batch_quiesce(b); rp_batch_keep(c, 0, b); }
    }
  } keep{c, b};
  b = rp_batch_take(c, 0, std::max<size_t>(R, 1), 8, tpraos);
  if (!b) { praos_set_error_(c, "candidates: device allocation failed"); return PRAOS_E_OOM; }
  std::vector<uint64_t> row_off(R);
  std::vector<uint32_t> row_len(R);
  praos_decoded dec{};
  uint8_t* nonce_h = nullptr;
  {
    int rc = rp_decode_rows(c, b, arena, bytes, d_row_off, d_row_len, 0, R);
    if (rc != PRAOS_OK) return rc;
    if (R) {
      HIPCHK(c, hipMemcpyAsync(row_off.data(), d_row_off, 8 * (size_t)R, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipMemcpyAsync(row_len.data(), d_row_len, 4 * (size_t)R, hipMemcpyDeviceToHost, st));
    }
    rc = rp_download_decoded(c, b, &dec, &nonce_h);            // (synchronises the copy stream)
    if (rc != PRAOS_OK) return rc;
  }
  size_t unwrapped = 0;
  for (size_t i = 0; i < N; i++) unwrapped += base_row[i] != NONE;
  out->stats[1] = unwrapped;
  out->stats[2] = R;

  // ---- host: each fragment's nonce chain, then one table of nonces and the rows
  const size_t* F = frags->frag_first;
  std::vector<std::vector<Run>> runs(K);
  std::vector<praos_nonce> evol(N);
  par_for(K, [&](size_t j) {
    spec_chain(frags->frag[j].state, in->ei, F[j + 1] - F[j], base_row.data() + F[j], dec, nonce_h,
               tpraos ? extra_entropy : nullptr, runs[j], evol.data() + F[j]);
  });
  std::vector<praos_nonce> etas;
  std::vector<uint8_t> row_eta(R, 0);
  std::vector<uint8_t> row_set(R, 0);
  std::vector<uint32_t> extra_base;
  std::unordered_map<uint64_t, uint32_t> extra;               // (base row, nonce) -> extra row
  bool too_many = false;
  for (size_t j = 0; j < K; j++) {
    for (size_t q = 0; q < runs[j].size(); q++) {
      size_t e = 0;
      while (e < etas.size() && !praos_host::nonce_eq(etas[e], runs[j][q].eta)) e++;
      if (e == etas.size()) etas.push_back(runs[j][q].eta);
      if (etas.size() > 256) { too_many = true; continue; }
      const size_t lo = F[j] + runs[j][q].first, hi = q + 1 < runs[j].size() ? F[j] + runs[j][q + 1].first : F[j + 1];
      for (size_t i = lo; i < hi; i++) {
        const uint32_t r = base_row[i];
        uint32_t row = r;
        if (r != NONE) {
          if (!row_set[r]) {
            row_set[r] = 1;
            row_eta[r] = (uint8_t)e;
          } else if (row_eta[r] != e) {
            const uint64_t key = ((uint64_t)r << 8) | e;
            auto it = extra.find(key);
            if (it == extra.end()) {
              it = extra.emplace(key, (uint32_t)(R + extra_base.size())).first;
              extra_base.push_back(r);
              row_eta.push_back((uint8_t)e);
            }
            row = it->second;
          }
        }
        out->row[i] = row;
      }
    }
  }
  *out->n_etas = (uint32_t)etas.size();
  if (too_many) {
    praos_set_error_(c, "candidates: " + std::to_string(etas.size()) + " distinct epoch nonces in one call (at most 256)");
    return PRAOS_E_ARG;
  }
  const size_t R2 = (size_t)R + extra_base.size();
  *out->n_rows = R2;
  out->stats[3] = R2;
  out->stats[4] = extra_base.size();
  if (R2 > out->rows_cap) {
    praos_set_error_(c, "candidates: rows_cap " + std::to_string(out->rows_cap) + " < " + std::to_string(R2) + " rows");
    return PRAOS_E_ARG;
  }
  if (etas.empty()) {                                          // (only empty fragments)
    praos_nonce z{};
    z.neutral = 1;
    etas.push_back(z);
  }
  for (size_t e = 0; e < etas.size() && out->etas; e++) out->etas[e] = etas[e];

  // ---- device: the extra rows' decode, the crypto run under the per-row nonces
  std::vector<uint64_t> xoff(extra_base.size());
  std::vector<uint32_t> xlen(extra_base.size());
  uint16_t* bits_h = nullptr;
  int32_t* pidx_h = nullptr;
  bool have_all = false;                         // dec / nonce_h hold the extra rows too
  {
    for (size_t x = 0; x < extra_base.size(); x++) { xoff[x] = row_off[extra_base[x]]; xlen[x] = row_len[extra_base[x]]; }
    if (!xoff.empty()) {                         // (R2 <= N: the span arrays have room)
      HIPCHK(c, hipMemcpyAsync(d_row_off + R, xoff.data(), 8 * xoff.size(), hipMemcpyHostToDevice, st));
      HIPCHK(c, hipMemcpyAsync(d_row_len + R, xlen.data(), 4 * xlen.size(), hipMemcpyHostToDevice, st));
    }
    int rc;
    if (rp_batch_fits(b, R2, 0)) {
      rc = rp_decode_rows(c, b, arena, bytes, d_row_off, d_row_len, R, R2);
    } else {
      // more extra rows than the batch's headroom: a batch with room for every row, all of them
      // decoded again from the spans already on the device
      rp_batch_quiesce(b);
      rp_batch_destroy(c, b);
      b = rp_batch_take(c, 0, R2, 8, tpraos);
      if (!b) { praos_set_error_(c, "candidates: device allocation failed"); return PRAOS_E_OOM; }
      rc = rp_decode_rows(c, b, arena, bytes, d_row_off, d_row_len, 0, R2);
      if (rc == PRAOS_OK) rc = rp_download_decoded(c, b, &dec, &nonce_h);
      have_all = true;
    }
    if (rc != PRAOS_OK) return rc;
    if (R2) {
      rc = rp_run(c, b, etas.data(), (uint32_t)etas.size(), row_eta.data());
      if (rc != PRAOS_OK) return rc;
    }
    rp_batch_results(b, &bits_h, &pidx_h);
    rc = rp_download_results(c, b, bits_h, pidx_h);
    if (rc != PRAOS_OK) return rc;
  }

  // ---- host: the fold's per-row inputs (the pinned decode download; with extra rows, copies
  // long enough for them: an extra row has its base row's fields), then each fragment's fold
  std::vector<uint64_t> x_slot, x_bno, x_ocn;
  std::vector<uint32_t> x_bsize;
  std::vector<uint8_t> x_prev, x_gen, x_cold, x_hh, x_nonce;
  const uint64_t *f_slot = dec.slot, *f_bno = dec.block_no, *f_ocn = dec.ocert_n;
  const uint32_t* f_bsize = dec.body_size;
  const uint8_t *f_prev = dec.prev_hash, *f_gen = dec.prev_is_genesis, *f_cold = dec.cold_vk, *f_hh = dec.header_hash,
                *f_nonce = nonce_h;
  if (!extra_base.empty()) {
    row_len.resize(R2);
    for (size_t x = 0; x < extra_base.size(); x++) row_len[R + x] = xlen[x];
  }
  if (!extra_base.empty() && !have_all) {
    auto grow = [&](auto& v, const auto* src, size_t rec) {
      v.resize(rec * R2);
      std::memcpy(v.data(), src, sizeof(*src) * rec * R);
      for (size_t x = 0; x < extra_base.size(); x++)
        std::memcpy(v.data() + rec * (R + x), src + rec * extra_base[x], sizeof(*src) * rec);
    };
    grow(x_slot, dec.slot, 1); grow(x_bno, dec.block_no, 1); grow(x_ocn, dec.ocert_n, 1);
    grow(x_bsize, dec.body_size, 1);
    grow(x_prev, dec.prev_hash, 32); grow(x_gen, dec.prev_is_genesis, 1); grow(x_cold, dec.cold_vk, 32);
    grow(x_hh, dec.header_hash, 32); grow(x_nonce, nonce_h, 32);
    f_slot = x_slot.data(); f_bno = x_bno.data(); f_ocn = x_ocn.data(); f_bsize = x_bsize.data();
    f_prev = x_prev.data(); f_gen = x_gen.data(); f_cold = x_cold.data(); f_hh = x_hh.data(); f_nonce = x_nonce.data();
  }
  if (R2 == 0) {                                 // no row at all: the fold still wants arrays to point at
    row_eta.assign(1, 0);
    row_len.assign(1, 0);
  }
  std::mutex err_mu;
  int first_rc = PRAOS_OK;
  size_t first_j = 0;
  std::string first_err;
  par_for(K, [&](size_t j) {
    praos_fragment& fr = frags->frag[j];
    const size_t n = F[j + 1] - F[j];
    const uint32_t* map = out->row + F[j];
    // the forecast horizon: the client waits at the first header the ledger view does not reach
    size_t cut = n;
    for (size_t i = 0; i < n; i++) {
      const uint32_t r = map[i];
      if (r == NONE || (bits_h[r] & PRAOS_BIT_INPUT)) break;   // (the fold stops here at the latest)
      if (f_slot[r] >= in->view_end_slot) { cut = i; break; }
    }
    praos_headers h{};
    h.n = cut;
    h.slot = f_slot;
    h.cold_vk = f_cold;
    h.ocert_n = f_ocn;
    praos_out crypto{bits_h, pidx_h, nullptr, nullptr, const_cast<uint8_t*>(f_nonce)};
    praos_envelope env{};
    env.block_no = f_bno;
    env.header_hash = f_hh;
    env.header_size = row_len.data();
    env.body_size = f_bsize;
    env.tip_is_origin = fr.tip_is_origin;
    env.tip_slot = fr.tip_slot;
    env.tip_block_no = fr.tip_block_no;
    std::memcpy(env.tip_hash, fr.tip_hash, 32);
    env.max_major_pv = in->max_major_pv;
    env.lv_prot_major = in->lv_prot_major;
    env.max_header_size = in->max_header_size;
    env.max_body_size = in->max_body_size;
    size_t stop = 0, done = 0;
    std::string err;
    uint8_t* v = out->verdict + F[j];
    const int rc = rp_fold(c, &h, f_prev, f_gen, &crypto, &env, &in->ei, &fr.state, etas.data(), (uint32_t)etas.size(),
                           row_eta.data(), evol.data() + F[j], tpraos, tpraos ? extra_entropy : nullptr, v,
                           tpraos && out->failures ? out->failures + F[j] : nullptr, &stop, &done, nullptr, map, true,
                           &err);
    if (rc != PRAOS_OK) {
      std::lock_guard<std::mutex> g(err_mu);
      if (first_rc == PRAOS_OK || j < first_j) { first_rc = rc; first_j = j; first_err = err; }
      return;
    }
    // (a fold that ended on a nonce it did not tick to -- only after a failure -- judged up to done)
    fr.chain_stop = stop;
    fr.processed = done;
    for (size_t i = done; i < n; i++) v[i] = PRAOS_V_NOT_REACHED;
    if (tpraos && out->failures)                 // the failure set goes with PRAOS_V_TPRAOS alone
      for (size_t i = 0; i < n; i++)
        if (v[i] != PRAOS_V_TPRAOS) out->failures[F[j] + i] = 0;
    fr.tip_is_origin = env.tip_is_origin;
    fr.tip_slot = env.tip_slot;
    fr.tip_block_no = env.tip_block_no;
    std::memcpy(fr.tip_hash, env.tip_hash, 32);
  });
  if (first_rc != PRAOS_OK) {
    praos_set_error_(c, "candidates: fragment " + std::to_string(first_j) + ": " + first_err);
    return first_rc;
  }

  // ---- the rows' outputs
  if (R2) {
    if (tpraos) {
      if (out->tp_rows->bits) std::memcpy(out->tp_rows->bits, bits_h, 2 * R2);
      if (out->tp_rows->pool_idx) std::memcpy(out->tp_rows->pool_idx, pidx_h, 4 * R2);
      if (out->tp_rows->beta_eta || out->tp_rows->beta_leader || out->tp_rows->nonce) {
        praos_tpraos_out o = *out->tp_rows;
        o.bits = bits_h;                                       // (required there; the same values again)
        o.pool_idx = nullptr;
        const int rc = praos_batch_download_tpraos(c, b, &o);
        if (rc != PRAOS_OK) return rc;
      }
      const int rc = rp_download_leader(c, b, out->leader_out, out->leader_proof);
      if (rc != PRAOS_OK) return rc;
    } else {
      if (out->rows->bits) std::memcpy(out->rows->bits, bits_h, 2 * R2);
      if (out->rows->pool_idx) std::memcpy(out->rows->pool_idx, pidx_h, 4 * R2);
      if (out->rows->beta || out->rows->leader || out->rows->nonce) {
        praos_out o = *out->rows;
        o.bits = bits_h;                                       // (required there; the same values again)
        o.pool_idx = nullptr;
        const int rc = praos_batch_download(c, b, &o);
        if (rc != PRAOS_OK) return rc;
      }
    }
    const int rc = praos_batch_download_decoded(c, b, out->dec);
    if (rc != PRAOS_OK) return rc;
    if (out->eta_idx) std::memcpy(out->eta_idx, row_eta.data(), R2);
  }
  return PRAOS_OK;
}

}  // namespace

extern "C" int praos_validate_candidates(praos_ctx* c, const praos_candidates_in* in, praos_fragments* frags,
                                         praos_candidates_out* out) {
  if (!c || !in || !frags || !out || !cand_items_ok(&in->items)) return PRAOS_E_ARG;
  praos_candidates_in a = *in;
  if (!a.praos_eras) a.praos_eras = (1u << 5) | (1u << 6);
  const CandOut o{out->wire_status, out->row, out->verdict, nullptr, out->rows_cap, &out->n_rows, out->eta_idx, out->etas,
                  &out->n_etas, out->stats, &out->rows, nullptr, &out->dec, nullptr, nullptr};
  return candidates_impl(c, &a, false, nullptr, frags, &o);
}

// TPraos (Shelley .. Alonzo, wire indices 1 to 4): the same pipeline with the batch taken, the rows
// decoded (the 15-field BHBody; k_vrf_nonce gives mkNonceFromOutputVRF of the eta certificate),
// the nonce chain ticked (TICKN's extra entropy) and the fragments folded in their TPraos modes.
// The overlay installed with praos_set_overlay applies as in every TPraos batch.
extern "C" int praos_validate_candidates_tpraos(praos_ctx* c, const praos_tpraos_candidates_in* in,
                                                praos_fragments* frags, praos_tpraos_candidates_out* out) {
  if (!c || !in || !frags || !out || !cand_items_ok(&in->items)) return PRAOS_E_ARG;
  praos_candidates_in a{};
  a.items = in->items;
  a.n_eras = in->n_eras;
  a.praos_eras = in->tpraos_eras ? in->tpraos_eras : ((1u << 1) | (1u << 2) | (1u << 3) | (1u << 4));
  a.view_end_slot = in->view_end_slot;
  a.ei = in->ei;
  a.max_major_pv = in->max_major_pv;
  a.lv_prot_major = in->lv_prot_major;
  a.max_header_size = in->max_header_size;
  a.max_body_size = in->max_body_size;
  const CandOut o{out->wire_status, out->row, out->verdict, out->failures, out->rows_cap, &out->n_rows, out->eta_idx,
                  out->etas, &out->n_etas, out->stats, nullptr, &out->rows, &out->dec, out->leader_out, out->leader_proof};
  return candidates_impl(c, &a, true, in->extra_entropy, frags, &o);
}

// ---- Byron: K candidate fragments of era-0 wire headers, each from its own tip and PBftState.
//     device   the front half with era mask 1 << 0 and the rows' kinds (k_hdr_row_kind), then
//              praos_verify_pbft_headers' kernels over the rows, read from the wire arena;
//     host     the PBFT fold per fragment in the client's mode, through the item-to-row map.
extern "C" int praos_validate_candidates_pbft(praos_ctx* c, const praos_pbft_candidates_in* in,
                                              praos_pbft_fragments* frags, praos_pbft_candidates_out* out) {
  if (!c || !in || !frags || !out || !cand_items_ok(&in->items)) return PRAOS_E_ARG;
  const size_t N = in->items.n, K = frags->k, bytes = in->items.bytes_len;
  const praos_pbft_params& p = in->params;
  if (!frag_bounds_ok(frags->frag_first, K, frags->frag != nullptr, N) || p.epoch_slots == 0 || p.window_size == 0 ||
      (in->n_delegs && !in->delegs) || (N && (!out->wire_status || !out->row || !out->verdict))) {
    praos_set_error_(c, "candidates: frag_first must run from 0 to the item count; epoch_slots and window_size > 0; "
                        "wire_status, row and verdict are required");
    return PRAOS_E_ARG;
  }
  for (size_t j = 0; j < K; j++) {
    const praos_pbft_state& s = frags->frag[j].state;
    if (frags->frag_first[j] > frags->frag_first[j + 1] || s.n > s.cap || s.cap < p.window_size || s.n > p.window_size ||
        !s.slot || !s.genesis_hash) {
      praos_set_error_(c, "candidates: fragment " + std::to_string(j) +
                              ": bounds out of order, or a state without n <= window_size <= cap");
      return PRAOS_E_ARG;
    }
  }
  if (!praos_pbft_delegs_ok_(in->delegs, in->n_delegs)) {
    praos_set_error_(c, "pbft: duplicate hash in the delegation map");
    return PRAOS_E_ARG;
  }
  {
    const int rd = front_begin(c, false);
    if (rd != PRAOS_OK) return rd;
  }
  out->n_rows = 0;
  std::memset(out->stats, 0, sizeof out->stats);
  out->stats[0] = N;
  for (size_t j = 0; j < K; j++) frags->frag[j].chain_stop = frags->frag[j].processed = 0;
  if (N == 0) return PRAOS_OK;

  // ---- device: unwrap + hash, dedup, the rows' kinds
  Front f;
  {
    const int rc = front_run(c, in->items, in->n_eras, 1u << 0, true, out->wire_status, f);
    if (rc != PRAOS_OK) return rc;
  }
  const size_t R = f.R;
  size_t unwrapped = 0;
  for (size_t i = 0; i < N; i++) {
    out->row[i] = f.base_row[i];
    unwrapped += f.base_row[i] != NONE;
  }
  out->stats[1] = unwrapped;
  out->stats[2] = R;
  out->n_rows = R;
  if (R > out->rows_cap) {
    praos_set_error_(c, "candidates: rows_cap " + std::to_string(out->rows_cap) + " < " + std::to_string(R) + " rows");
    return PRAOS_E_ARG;
  }

  // ---- device: decode, delegate look-up and signature of each row.  k_pbft_decode reads the two
  // bytes in front of a header; a Byron inner span starts at least 8 bytes into its wire item
  // (82 00 82 82 0k hint d8 18 + the byte string's head), so the wire arena needs no front pad.
  const size_t Ra = std::max<size_t>(R, 1);
  std::vector<uint8_t> r_bits(Ra), r_prev(32 * Ra), r_gen(Ra), r_hh(32 * Ra), r_dh, r_ebb(Ra);
  std::vector<int32_t> r_gk(Ra);
  std::vector<uint64_t> r_slot(Ra), r_bno(Ra);
  if (out->rows.delegate_hash) r_dh.resize(28 * Ra);
  praos_pbft_out rows{r_bits.data(), r_gk.data(), r_slot.data(), r_bno.data(), r_prev.data(), r_gen.data(), r_hh.data(),
                      out->rows.delegate_hash ? r_dh.data() : nullptr};
  if (R) {
    HIPCHK(c, hipMemcpy(r_ebb.data(), f.d_row_ebb, R, hipMemcpyDeviceToHost));
    const int rc = rp_pbft_verify_rows(c, R, f.arena, bytes, f.d_row_off, f.d_row_len, f.d_row_ebb, &p, in->delegs,
                                       in->n_delegs, &rows);
    if (rc != PRAOS_OK) return rc;
    uint32_t ps[4] = {0, 0, 0, 0};
    (void)praos_pbft_stats(c, ps);
    out->stats[3] = (uint64_t)ps[2] + ps[3];
  }

  // ---- host: each fragment's fold
  const size_t* F = frags->frag_first;
  std::mutex err_mu;
  int first_rc = PRAOS_OK;
  size_t first_j = 0;
  std::string first_err;
  par_for(K, [&](size_t j) {
    praos_pbft_fragment& fr = frags->frag[j];
    const size_t n = F[j + 1] - F[j];
    const uint32_t* map = out->row + F[j];
    // the forecast horizon: the client waits at the first header the ledger view does not reach
    size_t cut = n;
    for (size_t i = 0; i < n; i++) {
      const uint32_t r = map[i];
      if (r == NONE || (r_bits[r] & PRAOS_PBFT_BIT_DECODE)) break;   // (the fold stops here at the latest)
      if (r_slot[r] >= in->view_end_slot) { cut = i; break; }
    }
    size_t stop = 0, done = 0;
    std::string err;
    uint8_t* v = out->verdict + F[j];
    uint64_t* a = out->aux ? out->aux + F[j] : nullptr;
    const int rc = rp_pbft_fold_client(cut, map, R, &rows, r_ebb.data(), &p, in->delegs, in->n_delegs, &fr.tip, &fr.state,
                                       v, a, &stop, &done, &err);
    if (rc != PRAOS_OK) {
      std::lock_guard<std::mutex> g(err_mu);
      if (first_rc == PRAOS_OK || j < first_j) { first_rc = rc; first_j = j; first_err = err; }
      return;
    }
    fr.chain_stop = stop;
    fr.processed = done;
    for (size_t i = done; i < n; i++) {
      v[i] = PRAOS_V_NOT_REACHED;
      if (a) a[i] = 0;
    }
  });
  if (first_rc != PRAOS_OK) {
    praos_set_error_(c, "candidates: fragment " + std::to_string(first_j) + ": " + first_err);
    return first_rc;
  }

  // ---- the rows' outputs
  if (R) {
    auto give = [&](void* dst, const void* src, size_t b) {
      if (dst) std::memcpy(dst, src, b);
    };
    give(out->rows.bits, r_bits.data(), R);
    give(out->rows.gk_idx, r_gk.data(), 4 * R);
    give(out->rows.slot, r_slot.data(), 8 * R);
    give(out->rows.block_no, r_bno.data(), 8 * R);
    give(out->rows.prev_hash, r_prev.data(), 32 * R);
    give(out->rows.prev_is_genesis, r_gen.data(), R);
    give(out->rows.header_hash, r_hh.data(), 32 * R);
    give(out->rows.delegate_hash, r_dh.data(), 28 * R);
    give(out->row_is_ebb, r_ebb.data(), R);
  }
  return PRAOS_OK;
}
