// praos_txindex.hip -- host side of the transaction index (k_txindex.hip):
// praos_index_block_txs and praos_block_batch_tx_index.
//
// One call: the two splits into buffers of the call's own (a batch's integrity results stay as
// they are), the count pass, the counts down, their prefix sum on the host, the emit / row /
// reduce passes over the provisional rows, the statistics down, the final prefix sum (blocks a
// row found outside the shapes drop out), and -- when a row array was asked for -- the final pass
// with the transaction ids and the rows down.  Two host round trips; the device buffers are
// three allocations carved into their parts.  praos_impl::txi_run with a txi_keep is the same
// call for a pass that follows the index on the device (praos_txwit.hip): the final rows' block,
// witness span and tx_id columns are built, nothing of them is downloaded, and the allocations
// pass to the caller.
#include "api_internal.hpp"

namespace {

void rows_layout(Carve& c, size_t rows, praos_txi_dev_rows& r, const praos_txi_rows* want) {
  auto on = [&](const void* p) { return !want || p; };
  r = praos_txi_dev_rows{};
  if (on(want ? want->block : nullptr)) r.block = c.take<uint32_t>(4 * rows);
  if (on(want ? want->body_off : nullptr)) r.body_off = c.take<uint64_t>(8 * rows);
  if (on(want ? want->body_len : nullptr)) r.body_len = c.take<uint32_t>(4 * rows);
  if (on(want ? want->wit_off : nullptr)) r.wit_off = c.take<uint64_t>(8 * rows);
  if (on(want ? want->wit_len : nullptr)) r.wit_len = c.take<uint32_t>(4 * rows);
  if (on(want ? want->aux_off : nullptr)) r.aux_off = c.take<uint64_t>(8 * rows);
  if (on(want ? want->aux_len : nullptr)) r.aux_len = c.take<uint32_t>(4 * rows);
  if (on(want ? want->size : nullptr)) r.size = c.take<uint32_t>(4 * rows);
  if (on(want ? want->n_out : nullptr)) r.n_out = c.take<uint32_t>(4 * rows);
  if (on(want ? want->ex_steps : nullptr)) r.ex_steps = c.take<uint64_t>(8 * rows);
  if (on(want ? want->is_valid : nullptr)) r.is_valid = c.take<uint8_t>(rows);
  if (on(want ? want->tx_id : nullptr)) r.tx_id = c.take<uint8_t>(32 * rows);
}

bool any_row_array(const praos_txi_rows* r) {
  return r && (r->block || r->body_off || r->body_len || r->wit_off || r->wit_len || r->aux_off || r->aux_len ||
               r->size || r->n_out || r->ex_steps || r->is_valid || r->tx_id);
}

}  // namespace

int praos_impl::txi_run(praos_ctx* c, praos_batch* b, const praos_txi_cfg* cfg, praos_txi_stats* st,
                        praos_txi_rows* rows, txi_keep* keep) {
  const size_t n = b->n;
  if (keep) rows = nullptr;
  const int byron = cfg->byron != 0;
  if (rows) rows->n_rows = 0;
  if (n == 0) {
    if (st && st->tx_first) st->tx_first[0] = 0;
    return PRAOS_OK;
  }
  hipStream_t s = c->stream;
  // ---- the splits and the count pass
  uint64_t *hoff = nullptr, *seg_off = nullptr, *b_hoff = nullptr, *b_slot = nullptr, *b_bno = nullptr, *b_epoch = nullptr;
  uint32_t *hlen = nullptr, *seg_len = nullptr, *b_hlen = nullptr, *b_spans = nullptr;
  uint8_t *nseg = nullptr, *split = nullptr, *b_prev = nullptr, *b_gen = nullptr, *b_hh = nullptr, *b_split = nullptr,
          *b_kind = nullptr;
  uint16_t* b_dec = nullptr;
  uint32_t *cnt = nullptr, *first = nullptr, *tfirst = nullptr, *bad = nullptr, *d_ntx = nullptr;
  uint8_t *status = nullptr, *kind = nullptr;
  uint64_t *d_size = nullptr, *d_nout = nullptr, *d_ex = nullptr;
  DevBuf buf_a;
  if (carve_alloc(buf_a, [&](Carve& m) {
        hoff = m.take<uint64_t>(8 * n);
        hlen = m.take<uint32_t>(4 * n);
        seg_off = m.take<uint64_t>(8 * 4 * n);
        seg_len = m.take<uint32_t>(4 * 4 * n);
        nseg = m.take<uint8_t>(n);
        split = m.take<uint8_t>(n);
        if (byron) {
          b_hoff = m.take<uint64_t>(8 * n);
          b_hlen = m.take<uint32_t>(4 * n);
          b_slot = m.take<uint64_t>(8 * n);
          b_bno = m.take<uint64_t>(8 * n);
          b_prev = m.take<uint8_t>(32 * n);
          b_gen = m.take<uint8_t>(n);
          b_hh = m.take<uint8_t>(32 * n);
          b_split = m.take<uint8_t>(n);
          b_dec = m.take<uint16_t>(2 * n);
          b_kind = m.take<uint8_t>(n);
          b_epoch = m.take<uint64_t>(8 * n);
          b_spans = m.take<uint32_t>(4 * (size_t)PRAOS_BYRON_SPANS * n);
        }
        cnt = m.take<uint32_t>(4 * n);
        first = m.take<uint32_t>(4 * (n + 1));
        tfirst = m.take<uint32_t>(4 * (n + 1));
        bad = m.take<uint32_t>(4 * n);
        status = m.take<uint8_t>(n);
        kind = m.take<uint8_t>(n);
        d_ntx = m.take<uint32_t>(4 * n);
        d_size = m.take<uint64_t>(8 * n);
        d_nout = m.take<uint64_t>(8 * n);
        d_ex = m.take<uint64_t>(8 * n);
      }) != hipSuccess) {
    c->err = "device allocation failed";
    return PRAOS_E_OOM;
  }
  const uint32_t* txp_o = byron ? b_spans + (size_t)PRAOS_BYRON_SPAN_TXP * n : nullptr;
  const uint32_t* txp_l = byron ? b_spans + (size_t)(PRAOS_BYRON_SPAN_TXP + 1) * n : nullptr;
  HIPCHK(c, hipMemcpyAsync(hoff, b->blk_off, 8 * n, hipMemcpyDeviceToDevice, s));
  HIPCHK(c, hipMemcpyAsync(hlen, b->blk_len, 4 * n, hipMemcpyDeviceToDevice, s));
  HIPCHK(c, hipMemsetAsync(bad, 0, 4 * n, s));
  (void)hipGetLastError();
  launch_block_split(dim3(nblocks(n, NT)), dim3(NT), s, n, b->arena, b->arena_len, hoff, hlen, seg_off, seg_len, nseg,
                     split);
  HIPCHK(c, hipGetLastError());
  if (byron) {   // epoch_slots only scales the slot column, which is not read here
    launch_byron_split(dim3(nblocks(n, NT)), dim3(NT), s, n, b->arena, b->arena_len, b->blk_off, b->blk_len, 1, b_hoff,
                       b_hlen, b_slot, b_bno, b_prev, b_gen, b_hh, b_split, b_dec, b_kind, b_epoch, b_spans);
    HIPCHK(c, hipGetLastError());
  }
  launch_txi_count(s, n, b->arena, b->arena_len, b->blk_off, b->blk_len, byron, seg_off, seg_len, nseg, split, b_kind,
                   txp_o, txp_l, cnt, status, kind);
  HIPCHK(c, hipGetLastError());
  std::vector<uint32_t> h_cnt(n), h_first(n + 1);
  HIPCHK(c, hipMemcpyAsync(h_cnt.data(), cnt, 4 * n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  uint64_t prov = 0;
  for (size_t i = 0; i < n; i++) {
    h_first[i] = (uint32_t)prov;
    prov += h_cnt[i];
    if (prov > 0xfffffff0ull) { c->err = "praos_index_block_txs: too many transactions in one call"; return PRAOS_E_ARG; }
  }
  h_first[n] = (uint32_t)prov;
  // ---- the provisional rows
  praos_txi_dev_rows pr{};
  DevBuf buf_b;
  size_t rows_bytes = 0;
  if (prov) {
    if (carve_alloc(buf_b, [&](Carve& m) { rows_layout(m, (size_t)prov, pr, nullptr); rows_bytes = m.off; }) !=
        hipSuccess) {
      c->err = "device allocation failed";
      return PRAOS_E_OOM;
    }
    HIPCHK(c, hipMemsetAsync(buf_b.p, 0, rows_bytes, s));
    HIPCHK(c, hipMemsetAsync(pr.is_valid, 1, (size_t)prov, s));
    HIPCHK(c, hipMemcpyAsync(first, h_first.data(), 4 * (n + 1), hipMemcpyHostToDevice, s));
    launch_txi_emit(s, n, b->arena, b->blk_off, seg_off, seg_len, txp_o, txp_l, kind, status, cnt, first,
                    &pr);
    HIPCHK(c, hipGetLastError());
    launch_txi_rows(s, (size_t)prov, b->arena, kind, &pr, bad);
    HIPCHK(c, hipGetLastError());
  } else {
    HIPCHK(c, hipMemsetAsync(first, 0, 4 * (n + 1), s));
  }
  launch_txi_reduce(s, n, cnt, first, bad, &pr, status, d_ntx, d_size, d_nout, d_ex);
  HIPCHK(c, hipGetLastError());
  std::vector<uint32_t> h_ntx(n), h_tfirst(n + 1);
  HIPCHK(c, hipMemcpyAsync(h_ntx.data(), d_ntx, 4 * n, hipMemcpyDeviceToHost, s));
  if (st) {
    if (st->status) HIPCHK(c, hipMemcpyAsync(st->status, status, n, hipMemcpyDeviceToHost, s));
    if (st->txs_size) HIPCHK(c, hipMemcpyAsync(st->txs_size, d_size, 8 * n, hipMemcpyDeviceToHost, s));
    if (st->n_out) HIPCHK(c, hipMemcpyAsync(st->n_out, d_nout, 8 * n, hipMemcpyDeviceToHost, s));
    if (st->ex_steps) HIPCHK(c, hipMemcpyAsync(st->ex_steps, d_ex, 8 * n, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  uint64_t total = 0;
  for (size_t i = 0; i < n; i++) {
    h_tfirst[i] = (uint32_t)total;
    if (st && st->tx_first) st->tx_first[i] = total;
    if (st && st->n_tx) st->n_tx[i] = h_ntx[i];
    total += h_ntx[i];
  }
  h_tfirst[n] = (uint32_t)total;
  if (st && st->tx_first) st->tx_first[n] = total;
  if (rows) rows->n_rows = (size_t)total;
  // the buffers of a call whose results stay on the device pass to the caller
  auto hand_over = [&](DevBuf& a, DevBuf& b2, DevBuf& c2, const praos_txi_dev_rows& fr) {
    keep->buf[0] = a.p;
    keep->buf[1] = b2.p;
    keep->buf[2] = c2.p;
    a.p = b2.p = c2.p = nullptr;
    keep->kind = kind;
    keep->tfirst = tfirst;
    keep->rows = fr;
    keep->total = (size_t)total;
  };
  if (keep && total == 0) {
    DevBuf none;
    hand_over(buf_a, buf_b, none, praos_txi_dev_rows{});
    return PRAOS_OK;
  }
  if (!keep && (!any_row_array(rows) || total == 0)) return PRAOS_OK;
  if (!keep && rows->cap < total) {
    c->err = "praos_index_block_txs: rows->cap too small";
    return PRAOS_E_ARG;
  }
  // ---- the final rows, the transaction ids, the downloads
  praos_txi_dev_rows fr{};
  DevBuf buf_c;
  praos_txi_rows kept{};   // what the pass after the index reads: any non-null pointer selects the array
  kept.block = (uint32_t*)&kept;
  kept.wit_off = (uint64_t*)&kept;
  kept.wit_len = (uint32_t*)&kept;
  kept.tx_id = (uint8_t*)&kept;
  if (carve_alloc(buf_c, [&](Carve& m) { rows_layout(m, (size_t)total, fr, keep ? &kept : rows); }) != hipSuccess) {
    c->err = "device allocation failed";
    return PRAOS_E_OOM;
  }
  HIPCHK(c, hipMemcpyAsync(tfirst, h_tfirst.data(), 4 * (n + 1), hipMemcpyHostToDevice, s));
  launch_txi_final(s, (size_t)prov, b->arena, status, first, tfirst, &pr, &fr);
  HIPCHK(c, hipGetLastError());
  if (keep) {
    HIPCHK(c, hipStreamSynchronize(s));   // h_tfirst has been read
    hand_over(buf_a, buf_b, buf_c, fr);
    return PRAOS_OK;
  }
  const size_t t = (size_t)total;
  const Down down{s};
  HIPCHK(c, down(rows->block, fr.block, 4 * t));
  HIPCHK(c, down(rows->body_off, fr.body_off, 8 * t));
  HIPCHK(c, down(rows->body_len, fr.body_len, 4 * t));
  HIPCHK(c, down(rows->wit_off, fr.wit_off, 8 * t));
  HIPCHK(c, down(rows->wit_len, fr.wit_len, 4 * t));
  HIPCHK(c, down(rows->aux_off, fr.aux_off, 8 * t));
  HIPCHK(c, down(rows->aux_len, fr.aux_len, 4 * t));
  HIPCHK(c, down(rows->size, fr.size, 4 * t));
  HIPCHK(c, down(rows->n_out, fr.n_out, 4 * t));
  HIPCHK(c, down(rows->ex_steps, fr.ex_steps, 8 * t));
  HIPCHK(c, down(rows->is_valid, fr.is_valid, t));
  HIPCHK(c, down(rows->tx_id, fr.tx_id, 32 * t));
  HIPCHK(c, hipStreamSynchronize(s));
  return PRAOS_OK;
}

extern "C" {

int praos_block_batch_tx_index(praos_ctx* c, praos_batch* b, const praos_txi_cfg* cfg, praos_txi_stats* stats,
                               praos_txi_rows* rows) {
  if (!c || !b || !b->is_block || !cfg) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const int r = praos_impl::txi_run(c, b, cfg, stats, rows, nullptr);
  (void)hipStreamSynchronize(c->stream);   // the call's buffers are freed on return
  return r;
}

int praos_index_block_txs(praos_ctx* c, const praos_header_bytes* blocks, const praos_txi_cfg* cfg,
                          praos_txi_stats* stats, praos_txi_rows* rows) {
  if (!c || !blocks || !cfg) return PRAOS_E_ARG;
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  if (blocks->n == 0) {
    if (rows) rows->n_rows = 0;
    if (stats && stats->tx_first) stats->tx_first[0] = 0;
    return PRAOS_OK;
  }
  praos_batch* b = praos_block_batch_upload(c, blocks);
  if (!b) return PRAOS_E_OOM;
  const int r = praos_block_batch_tx_index(c, b, cfg, stats, rows);
  praos_batch_free(c, b);
  return r;
}

}  // extern "C"
