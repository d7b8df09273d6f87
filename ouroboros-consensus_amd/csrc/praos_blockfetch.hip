// praos_blockfetch.hip -- host side of praos_verify_fetched_blocks (k_blockfetch.hip; DESIGN
// section 35): wire blocks of several peers, each distinct one checked once.
//
// One call: the arena, the spans and the expected points up; k_bf_unwrap; the stored-block splits
// and header decoders over the inner spans (k_block_split + k_decode_praos, k_byron_split with
// Byron on); k_bf_key; the row set of api_internal.hpp: with dedup its hash set over (tag, header
// hash, length), the representatives (count) and k_bf_class, which compares every other member of a
// class with its representative and writes the classes that are numbered; without it ident.  The
// numbering gives the rows in order of first appearance.  The host
// waits for the row count (it sizes the row arrays: the first round trip).  Then k_bf_rows, the
// segment hashes and the join over the rows with no KES launch, the Byron body proof of the
// Byron rows, k_bf_bits, k_bf_verdict, the downloads and the fold per range on the host.  With
// cfg->witnesses praos_txwit.hip's txw_run follows over a batch whose blocks are the rows (its
// three round trips).
#include "api_internal.hpp"

namespace {

bool any_row_array(const praos_bf_rows* r) {
  return r && (r->item || r->tag || r->is_ebb || r->slot || r->block_no || r->header_hash || r->prev_hash ||
               r->hdr_off || r->hdr_len || r->blk_off || r->blk_len || r->body_hash || r->bits || r->which);
}

// the fold per range over the verdicts (in place: the items after a range's stop become NOT_REACHED)
void fold_ranges(const praos_bf_ranges* rg, uint8_t* verdict, praos_bf_range_out* po) {
  for (size_t r = 0; r < rg->k; r++) {
    const uint64_t i0 = rg->item_first[r], i1 = rg->item_first[r + 1];
    const uint64_t items = i1 - i0, points = rg->exp_first[r + 1] - rg->exp_first[r];
    uint64_t stop = items;
    for (uint64_t j = 0; j < items; j++)
      if (verdict[i0 + j] != PRAOS_BF_OK) { stop = j; break; }
    for (uint64_t j = stop + 1; j < items; j++) verdict[i0 + j] = PRAOS_BF_NOT_REACHED;
    if (po && po->stop) po->stop[r] = stop;
    if (po && po->accepted) po->accepted[r] = stop;
    if (po && po->status)
      po->status[r] = stop < items ? PRAOS_BF_RANGE_FAILED : items < points ? PRAOS_BF_RANGE_TOO_FEW : PRAOS_BF_RANGE_COMPLETE;
  }
}

int bf_run(praos_ctx* c, const praos_header_bytes* in, const praos_bf_ranges* rg, const praos_bf_cfg* cfg,
           praos_bf_items* po, praos_bf_range_out* pr, praos_bf_rows* rows, praos_txw_blocks* bo, praos_txw_txs* txs,
           praos_txw_wits* wits) {
  const size_t n = in->n, bytes = in->bytes_len, E = (size_t)rg->exp_first[rg->k];
  const bool byron = cfg->byron_epoch_slots != 0;
  hipStream_t s = c->stream;
  const dim3 g(nblocks(n, NT)), blk(NT);
  // the expected point of every item (NONE: past its range's points)
  std::vector<uint32_t> h_exp(n);
  for (size_t r = 0; r < rg->k; r++) {
    const uint64_t i0 = rg->item_first[r], points = rg->exp_first[r + 1] - rg->exp_first[r];
    for (uint64_t j = 0; i0 + j < rg->item_first[r + 1]; j++)
      h_exp[i0 + j] = j < points ? (uint32_t)(rg->exp_first[r] + j) : 0xffffffffu;
  }
  const size_t arena_sz = arena_room(bytes);
  uint8_t* arena = nullptr;
  uint64_t *d_off = nullptr, *ioff = nullptr, *hoff = nullptr, *seg_off = nullptr, *slot = nullptr, *block_no = nullptr,
           *ocert_n = nullptr, *ocert_c0 = nullptr, *body_off = nullptr, *pmaj = nullptr, *pmin = nullptr,
           *b_epoch = nullptr, *row_off = nullptr, *exp_slot = nullptr;
  uint32_t *d_len = nullptr, *ilen = nullptr, *hlen = nullptr, *seg_len = nullptr, *body_len = nullptr, *body_size = nullptr,
           *row_len = nullptr, *slot2 = nullptr, *min2 = nullptr, *total = nullptr, *exp_idx = nullptr;
  RowSet rs;
  uint8_t *status = nullptr, *tag = nullptr, *nseg = nullptr, *split = nullptr, *kind = nullptr, *elig = nullptr,
          *key = nullptr, *cold = nullptr, *vrf_vk = nullptr, *vrf_out = nullptr, *vrf_proof = nullptr, *hot = nullptr,
          *ocert_sig = nullptr, *kes_sig = nullptr, *signed_body = nullptr, *prev = nullptr, *gen = nullptr,
          *claimed = nullptr, *hh = nullptr, *verdict = nullptr, *exp_hash = nullptr;
  uint16_t* dec = nullptr;
  DevBuf buf;
  if (carve_alloc(buf, [&](Carve& m) {
        arena = m.take<uint8_t>(arena_sz);
        d_off = m.take<uint64_t>(8 * n);
        d_len = m.take<uint32_t>(4 * n);
        status = m.take<uint8_t>(n);
        tag = m.take<uint8_t>(n);
        ioff = m.take<uint64_t>(8 * n);
        ilen = m.take<uint32_t>(4 * n);
        hoff = m.take<uint64_t>(8 * n);
        hlen = m.take<uint32_t>(4 * n);
        seg_off = m.take<uint64_t>(8 * 4 * n);
        seg_len = m.take<uint32_t>(4 * 4 * n);
        nseg = m.take<uint8_t>(n);
        split = m.take<uint8_t>(n);
        kind = m.take<uint8_t>(n);
        // k_decode_praos's columns: the header fields the call reads (slot .. dec), then the ones
        // the kernel writes for the crypto passes, which nothing here reads (the kernel is unchanged)
        slot = m.take<uint64_t>(8 * n);
        block_no = m.take<uint64_t>(8 * n);
        prev = m.take<uint8_t>(32 * n);
        gen = m.take<uint8_t>(n);
        claimed = m.take<uint8_t>(32 * n);
        hh = m.take<uint8_t>(32 * n);
        dec = m.take<uint16_t>(2 * n);
        cold = m.take<uint8_t>(32 * n);
        vrf_vk = m.take<uint8_t>(32 * n);
        vrf_out = m.take<uint8_t>(64 * n);
        vrf_proof = m.take<uint8_t>(80 * n);
        hot = m.take<uint8_t>(32 * n);
        ocert_sig = m.take<uint8_t>(64 * n);
        kes_sig = m.take<uint8_t>(448 * n);
        ocert_n = m.take<uint64_t>(8 * n);
        ocert_c0 = m.take<uint64_t>(8 * n);
        body_off = m.take<uint64_t>(8 * n);
        body_len = m.take<uint32_t>(4 * n);
        signed_body = m.take<uint8_t>((size_t)TP_SIGNED_STRIDE * n + 16);
        body_size = m.take<uint32_t>(4 * n);
        pmaj = m.take<uint64_t>(8 * n);
        pmin = m.take<uint64_t>(8 * n);
        b_epoch = m.take<uint64_t>(8 * n);
        // classes and rows
        elig = m.take<uint8_t>(n);
        key = m.take<uint8_t>(32 * n);
        rs.layout(m, n);
        slot2 = m.take<uint32_t>(4 * n);
        min2 = m.take<uint32_t>(4 * n);
        row_off = m.take<uint64_t>(8 * n);
        row_len = m.take<uint32_t>(4 * n);
        total = m.take<uint32_t>(16);                            // [0] rows, [2] any Byron item with a row
        exp_idx = m.take<uint32_t>(4 * n);
        exp_slot = m.take<uint64_t>(8 * E);
        exp_hash = m.take<uint8_t>(32 * E);
        verdict = m.take<uint8_t>(n);
      }) != hipSuccess) {
    c->err = "device allocation failed";
    return PRAOS_E_OOM;
  }
  (void)hipGetLastError();
  HIPCHK(c, pad_zero(arena, bytes, s));
  if (bytes) HIPCHK(c, praos_impl::h2d(c, arena, in->bytes, bytes));
  HIPCHK(c, items_upload(*in, d_off, d_len, s));
  HIPCHK(c, hipMemcpyAsync(exp_idx, h_exp.data(), 4 * n, hipMemcpyHostToDevice, s));
  if (E) {
    HIPCHK(c, hipMemcpyAsync(exp_slot, rg->exp_slot, 8 * E, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(exp_hash, rg->exp_hash, 32 * E, hipMemcpyHostToDevice, s));
  }
  HIPCHK(c, hipMemsetAsync(kind, 0, n, s));
  HIPCHK(c, hipMemsetAsync(total, 0, 16, s));
  // ---- per item: unwrap, split, header fields, header hash
  launch_bf_unwrap(s, n, arena, bytes, d_off, d_len, cfg->n_eras, status, tag, ioff, ilen, hoff, hlen);
  launch_block_split(g, blk, s, n, arena, bytes, hoff, hlen, seg_off, seg_len, nseg, split);
  launch_decode_praos(g, blk, s, n, arena, bytes, hoff, hlen, slot, cold, vrf_vk, vrf_out, vrf_proof, hot, ocert_sig,
                      kes_sig, ocert_n, ocert_c0, body_off, body_len, signed_body, block_no, prev, gen, body_size, claimed,
                      pmaj, pmin, hh, dec, 1, TP_SIGNED_STRIDE);
  if (byron)   // Byron lanes get their columns from k_byron_split; the others keep the decode's
    launch_byron_split(g, blk, s, n, arena, bytes, ioff, ilen, cfg->byron_epoch_slots, hoff, hlen, slot, block_no, prev,
                       gen, hh, split, dec, kind, b_epoch, nullptr);
  HIPCHK(c, hipGetLastError());
  // ---- rows: one per distinct block, in order of first appearance
  launch_bf_key(s, n, status, split, dec, tag, ilen, hh, elig, cfg->dedup ? key : nullptr, total + 2);
  // (the classes that are numbered are slot2 / min2: the hash set's with the deviants k_bf_class
  // found taken out, each a class of its own)
  RowSet cls = rs;
  cls.item_slot = slot2;
  cls.slot_min = min2;
  if (cfg->dedup) {
    HIPCHK(c, rs.reset(s));
    rs.set(s, elig, tag, key, 0xffffffffu);
    rs.count(s);
    launch_bf_class(s, n, arena, rs.item_slot, rs.item_rep, ioff, ilen, slot2, min2);
  } else {
    cls.ident(s, nullptr, elig, 0);
  }
  cls.number(s, total, ioff, ilen, row_off, row_len);
  HIPCHK(c, hipGetLastError());
  uint32_t h_total[3] = {0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(h_total, total, 12, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  const size_t R = std::min<size_t>(h_total[0], n);
  const bool byron_rows = byron && h_total[2] != 0;          // no Byron row: no lane tables, no Byron pass
  if (rows) rows->n_rows = R;
  // ---- per row: the body check
  praos_bf_dev_rows o{};
  uint8_t *r_bits = nullptr, *r_which = nullptr, *r_calc = nullptr, *r_seg_hash = nullptr, *r_zero = nullptr,
          *r_kind = nullptr, *r_bres = nullptr, *r_bwhich = nullptr, *r_gen = nullptr, *r_split = nullptr;
  uint16_t* r_dec = nullptr;
  uint64_t* r_epoch = nullptr;
  uint32_t* r_spans = nullptr;
  DevBuf buf_r;
  if (R) {
    if (carve_alloc(buf_r, [&](Carve& m) {
          o.item = m.take<uint32_t>(4 * R);
          o.tag = m.take<uint8_t>(R);
          o.is_ebb = m.take<uint8_t>(R);
          o.slot = m.take<uint64_t>(8 * R);
          o.block_no = m.take<uint64_t>(8 * R);
          o.hdr_off = m.take<uint64_t>(8 * R);
          o.hdr_len = m.take<uint32_t>(4 * R);
          o.header_hash = m.take<uint8_t>(32 * R);
          o.prev_hash = m.take<uint8_t>(32 * R);
          o.claimed = m.take<uint8_t>(32 * R);
          o.nseg = m.take<uint8_t>(R);
          o.seg_off = m.take<uint64_t>(8 * 4 * R);
          o.seg_len = m.take<uint32_t>(4 * 4 * R);
          r_seg_hash = m.take<uint8_t>(32 * 4 * R);
          r_zero = m.take<uint8_t>(2 * R);                     // no split / decode failure, no KES bits: rows decode
          r_bits = m.take<uint8_t>(R);
          r_which = m.take<uint8_t>(R);
          r_calc = m.take<uint8_t>(32 * R);
          if (byron_rows) {
            r_kind = m.take<uint8_t>(R);
            r_bres = m.take<uint8_t>(R);
            r_bwhich = m.take<uint8_t>(R);
            r_gen = m.take<uint8_t>(R);
            r_split = m.take<uint8_t>(R);
            r_dec = m.take<uint16_t>(2 * R);
            r_epoch = m.take<uint64_t>(8 * R);
            r_spans = m.take<uint32_t>(4 * (size_t)PRAOS_BYRON_SPANS * R);
          }
        }) != hipSuccess) {
      c->err = "device allocation failed";
      return PRAOS_E_OOM;
    }
    (void)hipGetLastError();
    HIPCHK(c, hipMemsetAsync(r_zero, 0, 2 * R, s));
    const praos_bf_dev_items d{tag, kind, slot, block_no, hoff, hlen, hh, prev, claimed, nseg, seg_off, seg_len};
    launch_bf_rows(s, n, R, slot2, rs.rep_row, &d, &o);
    const dim3 gr(nblocks(R, NT));
    launch_seg_hash(dim3(nblocks(4 * R, NT)), blk, s, R, arena, o.seg_off, o.seg_len, o.nseg, r_seg_hash);
    launch_block_join(gr, blk, s, R, o.nseg, r_zero, (const uint16_t*)r_zero, (const uint16_t*)r_zero, r_seg_hash,
                      o.claimed, r_bits, r_calc);
    HIPCHK(c, hipGetLastError());
    if (byron_rows) {
      // the span table of the Byron rows (the row columns are written again with the same values),
      // then blockMatchesHeader; the signature and protocol-magic bits are dropped by k_bf_bits
      const int rt = praos_impl::txw_lane_tables(c, R);
      if (rt != PRAOS_OK) return rt;
      launch_byron_split(gr, blk, s, R, arena, bytes, row_off, row_len, cfg->byron_epoch_slots, o.hdr_off, o.hdr_len,
                         o.slot, o.block_no, o.prev_hash, r_gen, o.header_hash, r_split, r_dec, r_kind, r_epoch, r_spans);
      launch_byron_integrity(gr, blk, s, R, arena, row_off, row_len, r_kind, r_spans, 0, c->btab, c->txw_tabs, r_bres,
                             r_bwhich);
      HIPCHK(c, hipGetLastError());
    }
    launch_bf_bits(s, R, o.tag, r_bres, r_bwhich, r_bits, r_which, r_calc);
  }
  launch_bf_verdict(s, n, R, byron ? 1 : 0, status, tag, rs.item_row, exp_idx, exp_slot, exp_hash, slot, hh, r_bits, r_which,
                    verdict);
  HIPCHK(c, hipGetLastError());
  // ---- the downloads and the fold
  const Down down{s};
  std::vector<uint8_t> h_verdict(n);
  HIPCHK(c, down(h_verdict.data(), verdict, n));
  if (po) {
    HIPCHK(c, down(po->status, status, n));
    HIPCHK(c, down(po->tag, tag, n));
    HIPCHK(c, down(po->row, rs.item_row, 4 * n));
  }
  const bool short_r = any_row_array(rows) && rows->cap < R;
  if (any_row_array(rows) && !short_r && R) {
    HIPCHK(c, down(rows->item, o.item, 4 * R));
    HIPCHK(c, down(rows->tag, o.tag, R));
    HIPCHK(c, down(rows->is_ebb, o.is_ebb, R));
    HIPCHK(c, down(rows->slot, o.slot, 8 * R));
    HIPCHK(c, down(rows->block_no, o.block_no, 8 * R));
    HIPCHK(c, down(rows->header_hash, o.header_hash, 32 * R));
    HIPCHK(c, down(rows->prev_hash, o.prev_hash, 32 * R));
    HIPCHK(c, down(rows->hdr_off, o.hdr_off, 8 * R));
    HIPCHK(c, down(rows->hdr_len, o.hdr_len, 4 * R));
    HIPCHK(c, down(rows->blk_off, row_off, 8 * R));
    HIPCHK(c, down(rows->blk_len, row_len, 4 * R));
    HIPCHK(c, down(rows->body_hash, r_calc, 32 * R));
    HIPCHK(c, down(rows->bits, r_bits, R));
    HIPCHK(c, down(rows->which, r_which, R));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  fold_ranges(rg, h_verdict.data(), pr);
  if (po && po->verdict) std::memcpy(po->verdict, h_verdict.data(), n);
  // ---- the transactions' key witnesses, the rows as blocks
  int rw = PRAOS_OK;
  if (cfg->witnesses) {
    praos_batch bb;
    bb.n = R;
    bb.is_block = true;
    bb.arena = arena;
    bb.arena_len = bytes;
    bb.blk_off = row_off;
    bb.blk_len = row_len;
    const praos_txw_cfg wcfg{byron ? 1u : 0u, cfg->max_lanes};
    // blocks_out holds rows->cap entries (it has no cap of its own): written only when the rows fit
    rw = praos_impl::txw_run(c, &bb, &wcfg, rows && rows->cap >= R ? bo : nullptr, txs, wits);
    if (rw != PRAOS_OK && rw != PRAOS_E_ARG) return rw;
  }
  if (short_r) {
    c->err = "praos_verify_fetched_blocks: rows->cap too small";
    return PRAOS_E_ARG;
  }
  return rw;
}

}  // namespace

extern "C" int praos_verify_fetched_blocks(praos_ctx* c, const praos_header_bytes* items, const praos_bf_ranges* rg,
                                           const praos_bf_cfg* cfg, praos_bf_items* per_item,
                                           praos_bf_range_out* per_range, praos_bf_rows* rows, praos_txw_blocks* blocks_out,
                                           praos_txw_txs* txs, praos_txw_wits* wits) {
  if (!c || !items || !rg || !cfg) return PRAOS_E_ARG;
  if (cfg->n_eras < 1 || cfg->n_eras > 31) {
    c->err = "praos_verify_fetched_blocks: n_eras must be 1..31";
    return PRAOS_E_ARG;
  }
  const size_t n = items->n;
  if (n && !items_ok(items)) return PRAOS_E_ARG;
  if (n > (1ull << 30)) { c->err = "praos_verify_fetched_blocks: too many items in one call"; return PRAOS_E_ARG; }
  if (!rg->item_first || !rg->exp_first || rg->item_first[0] != 0 || rg->item_first[rg->k] != n ||
      rg->exp_first[0] != 0 || rg->exp_first[rg->k] > 0x7fffffffull ||
      (rg->exp_first[rg->k] && (!rg->exp_slot || !rg->exp_hash))) {
    c->err = "praos_verify_fetched_blocks: the ranges do not cover the items";
    return PRAOS_E_ARG;
  }
  for (size_t r = 0; r < rg->k; r++)
    if (rg->item_first[r + 1] < rg->item_first[r] || rg->exp_first[r + 1] < rg->exp_first[r]) {
      c->err = "praos_verify_fetched_blocks: the ranges do not ascend";
      return PRAOS_E_ARG;
    }
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  if (rows) rows->n_rows = 0;
  if (txs) txs->n_rows = 0;
  if (wits) wits->n_wits = 0;
  if (n == 0) {
    fold_ranges(rg, nullptr, per_range);
    if (blocks_out && blocks_out->tx_first) blocks_out->tx_first[0] = 0;
    if (txs && txs->wit_first) txs->wit_first[0] = 0;
    return PRAOS_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const int r = bf_run(c, items, rg, cfg, per_item, per_range, rows, blocks_out, txs, wits);
  (void)hipStreamSynchronize(c->stream);   // the call's buffers are freed on return
  return r;
}
