// praos_gentx.hip -- host side of praos_verify_gen_txs (k_gentx.hip): wire
// transactions of several peers, each distinct one checked once.
//
// One call: the arena and the spans up; k_gtx_split; the first numbering (the row set of
// api_internal.hpp: its hash set with dedup, ident without) gives provisional rows in order of
// first appearance; k_gtx_rows over them; the second numbering (ident over the rows it kept, into
// row arrays of its own) drops the rows it refused; k_gtx_final gathers the
// final rows and maps every item to its row.  Both numberings and the kernels between them read
// the provisional row count on the device, so the host first waits for the final count (it
// sizes the witness step's row arrays); then praos_txwit.hip's txw_rows_run (the witness counts
// down, its second wait) and the downloads.  Three host round trips.
#include "api_internal.hpp"

namespace {

constexpr uint8_t TXK_SHELLEY = 1;   // k_txindex.hip's kind of a Shelley-based block: the rows' one kind

bool any_row_array(const praos_gtx_txs* t) {
  return t && (t->item || t->era || t->body_off || t->body_len || t->wit_off || t->wit_len || t->aux_off ||
               t->aux_len || t->size || t->in_block_size || t->ex_mem || t->ex_steps || t->is_valid || t->tx_id ||
               t->wstatus || t->n_vkey || t->n_boot || t->n_bad || t->wit_first);
}
bool any_wit_array(const praos_txw_wits* w) {
  return w && (w->tx || w->kind || w->key_off || w->sig_off || w->ok || w->key_hash);
}

int gtx_run(praos_ctx* c, const praos_header_bytes* in, const praos_gtx_cfg* cfg, praos_gtx_items* po,
            praos_gtx_txs* txs, praos_txw_wits* wits) {
  const size_t n = in->n, bytes = in->bytes_len;
  hipStream_t s = c->stream;
  const size_t arena_sz = arena_room(bytes);     // ld64u's pad (arena.hpp)
  uint8_t* arena = nullptr;
  uint64_t* d_off = nullptr;
  uint32_t* d_len = nullptr;
  praos_gtx_dev_items d{};
  praos_gtx_dev_rows o{};
  RowSet rs;
  uint32_t *total = nullptr, *row_item = nullptr, *row_final = nullptr, *row_scratch = nullptr, *len_scratch = nullptr;
  uint64_t *off_scratch = nullptr, *ex_mem = nullptr, *ex_steps = nullptr;
  uint8_t *row_ok = nullptr, *p_txid = nullptr, *kind1 = nullptr;
  DevBuf buf;
  if (carve_alloc(buf, [&](Carve& m) {
        arena = m.take<uint8_t>(arena_sz);
        d_off = m.take<uint64_t>(8 * n);
        d_len = m.take<uint32_t>(4 * n);
        d.status = m.take<uint8_t>(n);
        d.era = m.take<uint8_t>(n);
        d.kind = m.take<uint8_t>(n);
        d.is_valid = m.take<uint8_t>(n);
        d.ioff = m.take<uint64_t>(8 * n);
        d.ilen = m.take<uint32_t>(4 * n);
        d.body_off = m.take<uint64_t>(8 * n);
        d.body_len = m.take<uint32_t>(4 * n);
        d.wit_off = m.take<uint64_t>(8 * n);
        d.wit_len = m.take<uint32_t>(4 * n);
        d.aux_off = m.take<uint64_t>(8 * n);
        d.aux_len = m.take<uint32_t>(4 * n);
        d.size = m.take<uint32_t>(4 * n);
        d.hash = m.take<uint8_t>(32 * n);
        o.item = m.take<uint32_t>(4 * n);
        o.era = m.take<uint8_t>(n);
        o.body_off = m.take<uint64_t>(8 * n);
        o.body_len = m.take<uint32_t>(4 * n);
        o.wit_off = m.take<uint64_t>(8 * n);
        o.wit_len = m.take<uint32_t>(4 * n);
        o.aux_off = m.take<uint64_t>(8 * n);
        o.aux_len = m.take<uint32_t>(4 * n);
        o.size = m.take<uint32_t>(4 * n);
        o.in_block_size = m.take<uint32_t>(4 * n);
        o.ex_mem = m.take<uint64_t>(8 * n);
        o.ex_steps = m.take<uint64_t>(8 * n);
        o.is_valid = m.take<uint8_t>(n);
        o.tx_id = m.take<uint8_t>(32 * n);
        o.block = m.take<uint32_t>(4 * n);
        rs.layout(m, n);
        row_item = m.take<uint32_t>(4 * n);
        row_final = m.take<uint32_t>(4 * n);
        row_scratch = m.take<uint32_t>(4 * n);
        off_scratch = m.take<uint64_t>(8 * n);
        len_scratch = m.take<uint32_t>(4 * n);
        total = m.take<uint32_t>(8);                             // [0] provisional rows, [1] final rows
        row_ok = m.take<uint8_t>(n);
        ex_mem = m.take<uint64_t>(8 * n);
        ex_steps = m.take<uint64_t>(8 * n);
        p_txid = m.take<uint8_t>(32 * n);
        kind1 = m.take<uint8_t>(1);
      }) != hipSuccess) {
    c->err = "device allocation failed";
    return PRAOS_E_OOM;
  }
  (void)hipGetLastError();
  HIPCHK(c, pad_zero(arena, bytes, s));
  if (bytes) HIPCHK(c, hipMemcpyAsync(arena, in->bytes, bytes, hipMemcpyHostToDevice, s));
  HIPCHK(c, items_upload(*in, d_off, d_len, s));
  HIPCHK(c, hipMemsetAsync(row_item, 0xff, 4 * n, s));
  HIPCHK(c, hipMemsetAsync(kind1, TXK_SHELLEY, 1, s));
  if (!cfg->dedup) d.hash = nullptr;
  launch_gtx_split(s, n, arena, bytes, d_off, d_len, cfg->n_eras, &d);
  // ---- provisional rows: the distinct items in order of first appearance
  if (cfg->dedup) {
    HIPCHK(c, rs.reset(s));
    rs.set(s, d.status, d.era, d.hash, 0xfffffffeu);           // every era but Byron
  } else {
    rs.ident(s, nullptr, d.status, PRAOS_WIRE_OK);
  }
  rs.number(s, total, d.ioff, d.ilen, off_scratch, len_scratch);
  launch_hdr_rep(s, n, rs.item_slot, rs.item_rep, rs.rep_row, row_item);
  launch_gtx_rows(s, n, total, arena, row_item, &d, row_ok, ex_mem, ex_steps, p_txid);
  // ---- final rows: the provisional rows k_gtx_rows kept, in the same order.  The same arrays but
  // for the rows: k_gtx_final reads the first numbering's item_row beside the second's row_final.
  RowSet fin = rs;
  fin.rep_row = row_final;
  fin.item_row = row_scratch;
  fin.ident(s, total, row_ok, 1);
  fin.number(s, total + 1, d.ioff, d.ilen, off_scratch, len_scratch);
  HIPCHK(c, hipMemsetAsync(o.block, 0, 4 * n, s));
  launch_gtx_final(s, n, total, row_item, row_ok, row_final, ex_mem, ex_steps, p_txid, &d, rs.item_row, &o);
  HIPCHK(c, hipGetLastError());
  uint32_t h_total[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(h_total, total, 8, hipMemcpyDeviceToHost, s));
  const Down down{s};
  if (po) {
    HIPCHK(c, down(po->status, d.status, n));
    HIPCHK(c, down(po->era, d.era, n));
    HIPCHK(c, down(po->row, rs.item_row, 4 * n));
    HIPCHK(c, down(po->byron_kind, d.kind, n));
    HIPCHK(c, down(po->payload_off, d.ioff, 8 * n));
    HIPCHK(c, down(po->payload_len, d.ilen, 4 * n));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  const size_t T = std::min<size_t>(h_total[1], n);
  if (txs) txs->n_rows = T;
  if (T == 0) {
    if (txs && txs->wit_first) txs->wit_first[0] = 0;
    return PRAOS_OK;
  }
  // ---- the witness passes
  praos_impl::txw_rows R;
  const int rr = praos_impl::txw_rows_run(c, "praos_verify_gen_txs", arena, bytes, T, kind1, o.block, o.wit_off,
                                          o.wit_len, o.tx_id, cfg->max_lanes, R);
  if (wits) wits->n_wits = (size_t)R.W;
  if (rr != PRAOS_OK) return rr;
  const uint64_t W = R.W;
  const bool want_t = any_row_array(txs), want_w = any_wit_array(wits);
  const bool short_t = want_t && txs->cap < T, short_w = want_w && wits->cap < W;
  if (short_t || short_w) {
    HIPCHK(c, hipStreamSynchronize(s));
    c->err = short_t ? "praos_verify_gen_txs: txs->cap too small" : "praos_verify_gen_txs: wits->cap too small";
    return PRAOS_E_ARG;
  }
  if (want_t) {
    HIPCHK(c, down(txs->item, o.item, 4 * T));
    HIPCHK(c, down(txs->era, o.era, T));
    HIPCHK(c, down(txs->body_off, o.body_off, 8 * T));
    HIPCHK(c, down(txs->body_len, o.body_len, 4 * T));
    HIPCHK(c, down(txs->wit_off, o.wit_off, 8 * T));
    HIPCHK(c, down(txs->wit_len, o.wit_len, 4 * T));
    HIPCHK(c, down(txs->aux_off, o.aux_off, 8 * T));
    HIPCHK(c, down(txs->aux_len, o.aux_len, 4 * T));
    HIPCHK(c, down(txs->size, o.size, 4 * T));
    HIPCHK(c, down(txs->in_block_size, o.in_block_size, 4 * T));
    HIPCHK(c, down(txs->ex_mem, o.ex_mem, 8 * T));
    HIPCHK(c, down(txs->ex_steps, o.ex_steps, 8 * T));
    HIPCHK(c, down(txs->is_valid, o.is_valid, T));
    HIPCHK(c, down(txs->tx_id, o.tx_id, 32 * T));
    HIPCHK(c, down(txs->wstatus, R.st, T));
    HIPCHK(c, down(txs->n_vkey, R.nv, 4 * T));
    HIPCHK(c, down(txs->n_boot, R.nb, 4 * T));
    HIPCHK(c, down(txs->n_bad, R.txbad, 4 * T));
    if (txs->wit_first)
      for (size_t p = 0; p <= T; p++) txs->wit_first[p] = R.wfirst[p];
  }
  if (want_w) {
    const int rw = praos_impl::txw_rows_down_wits(c, wits, R);
    if (rw != PRAOS_OK) return rw;
  }
  HIPCHK(c, hipStreamSynchronize(s));
  return PRAOS_OK;
}

}  // namespace

extern "C" int praos_verify_gen_txs(praos_ctx* c, const praos_header_bytes* items, const praos_gtx_cfg* cfg,
                                    praos_gtx_items* per_item, praos_gtx_txs* txs, praos_txw_wits* wits) {
  if (!c || !items || !cfg) return PRAOS_E_ARG;
  if (cfg->n_eras < 1 || cfg->n_eras > 32) { c->err = "praos_verify_gen_txs: n_eras must be 1..32"; return PRAOS_E_ARG; }
  if (items->n && !items_ok(items)) return PRAOS_E_ARG;
  if (items->n > 0x7fffffffull) { c->err = "praos_verify_gen_txs: too many items in one call"; return PRAOS_E_ARG; }
  if (praos_host_only_(c)) return PRAOS_E_STATE;
  if (txs) txs->n_rows = 0;
  if (wits) wits->n_wits = 0;
  if (items->n == 0) {
    if (txs && txs->wit_first) txs->wit_first[0] = 0;
    return PRAOS_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const int r = gtx_run(c, items, cfg, per_item, txs, wits);
  (void)hipStreamSynchronize(c->stream);   // the call's buffers are freed on return
  return r;
}
