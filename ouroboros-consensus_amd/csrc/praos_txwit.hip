// praos_txwit.hip -- host side of the key-witness check (k_txwit.hip):
// praos_verify_tx_witnesses and praos_block_batch_tx_witnesses.
//
// One call: the transaction index with its final rows kept on the device (praos_txindex.hip), the
// count pass over the rows, the counts down and their prefix sum on the host (it sizes the witness
// arrays, as the index's does the rows), the emit pass, the verifies in slices of at most
// max_lanes witnesses over one slice's lane tables, the two reductions, the downloads.  Three host
// round trips, two of them the index's.  Every slice runs on the context's stream, one after the
// other over the same tables; a witness's result depends on its own bytes alone, so the outputs do
// not depend on the slice size.
#include "api_internal.hpp"

namespace {

// Witnesses per launch by default.  A lane's tables take LT_ED_B = 1 KiB, so this is 256 MiB of
// tables, kept by the context between calls: it holds the 196,608 lanes the device keeps resident
// at k_txw_verify's three waves per SIMD (256 CUs x 4 SIMDs x 3 x 64) with a third to spare, so a
// slice's tail overlaps less of the next one's start than its own length.
constexpr size_t TXW_LANES = 262144;

bool any_tx_array(const praos_txw_txs* t) {
  return t && (t->block || t->status || t->n_vkey || t->n_boot || t->n_bad || t->tx_id || t->wit_first);
}
bool any_wit_array(const praos_txw_wits* w) {
  return w && (w->tx || w->kind || w->key_off || w->sig_off || w->ok || w->key_hash);
}

int txw_run(praos_ctx* c, praos_batch* b, const praos_txw_cfg* cfg, praos_txw_blocks* bo, praos_txw_txs* txs,
            praos_txw_wits* wits) {
  const size_t n = b->n;
  if (txs) txs->n_rows = 0;
  if (wits) wits->n_wits = 0;
  if (n == 0) {
    if (bo && bo->tx_first) bo->tx_first[0] = 0;
    if (txs && txs->wit_first) txs->wit_first[0] = 0;
    return PRAOS_OK;
  }
  hipStream_t s = c->stream;
  // ---- the index, its final rows left on the device
  txi_keep K;
  praos_txi_cfg icfg{cfg->byron, 0};
  praos_txi_stats ist{};
  ist.status = bo ? bo->status : nullptr;
  ist.n_tx = bo ? bo->n_tx : nullptr;
  ist.tx_first = bo ? bo->tx_first : nullptr;
  const int r = praos_impl::txi_run(c, b, &icfg, &ist, nullptr, &K);
  if (r != PRAOS_OK) return r;
  const size_t T = K.total;
  if (txs) txs->n_rows = T;
  auto zero_blocks = [&] {
    if (bo && bo->n_wit) std::memset(bo->n_wit, 0, 4 * n);
    if (bo && bo->n_bad) std::memset(bo->n_bad, 0, 4 * n);
    if (bo && bo->n_shape) std::memset(bo->n_shape, 0, 4 * n);
  };
  if (T == 0) {
    zero_blocks();
    if (txs && txs->wit_first) txs->wit_first[0] = 0;
    HIPCHK(c, hipStreamSynchronize(s));
    return PRAOS_OK;
  }
  // ---- the count pass
  uint8_t* d_st = nullptr;
  uint32_t *d_nv = nullptr, *d_nb = nullptr, *d_cnt = nullptr, *d_wfirst = nullptr, *d_txbad = nullptr,
           *d_bwit = nullptr, *d_bbad = nullptr, *d_bshape = nullptr;
  uint64_t *d_v0 = nullptr, *d_v2 = nullptr;
  DevBuf buf_t;
  if (carve_alloc(buf_t, [&](Carve& m) {
        d_st = m.take<uint8_t>(T);
        d_nv = m.take<uint32_t>(4 * T);
        d_nb = m.take<uint32_t>(4 * T);
        d_cnt = m.take<uint32_t>(4 * T);
        d_wfirst = m.take<uint32_t>(4 * (T + 1));
        d_txbad = m.take<uint32_t>(4 * T);
        d_v0 = m.take<uint64_t>(8 * T);
        d_v2 = m.take<uint64_t>(8 * T);
        d_bwit = m.take<uint32_t>(4 * n);
        d_bbad = m.take<uint32_t>(4 * n);
        d_bshape = m.take<uint32_t>(4 * n);
      }) != hipSuccess) {
    c->err = "device allocation failed";
    return PRAOS_E_OOM;
  }
  (void)hipGetLastError();
  launch_txw_count(s, T, b->arena, b->arena_len, K.kind, K.rows.block, K.rows.wit_off, K.rows.wit_len, d_st, d_nv, d_nb,
                   d_cnt, d_v0, d_v2);
  HIPCHK(c, hipGetLastError());
  std::vector<uint32_t> h_cnt(T), h_wfirst(T + 1);
  HIPCHK(c, hipMemcpyAsync(h_cnt.data(), d_cnt, 4 * T, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  uint64_t W = 0;
  for (size_t p = 0; p < T; p++) {
    h_wfirst[p] = (uint32_t)W;
    W += h_cnt[p];
    if (W > 0xfffffff0ull) { c->err = "praos_verify_tx_witnesses: too many witnesses in one call"; return PRAOS_E_ARG; }
  }
  h_wfirst[T] = (uint32_t)W;
  if (wits) wits->n_wits = (size_t)W;
  HIPCHK(c, hipMemcpyAsync(d_wfirst, h_wfirst.data(), 4 * (T + 1), hipMemcpyHostToDevice, s));
  // ---- the witness records and the verifies
  uint32_t* d_tx = nullptr;
  uint8_t *d_kind = nullptr, *d_ok = nullptr, *d_kh = nullptr;
  uint64_t *d_koff = nullptr, *d_soff = nullptr;
  DevBuf buf_w;
  if (W) {
    if (carve_alloc(buf_w, [&](Carve& m) {
          d_tx = m.take<uint32_t>(4 * W);
          d_kind = m.take<uint8_t>(W);
          d_koff = m.take<uint64_t>(8 * W);
          d_soff = m.take<uint64_t>(8 * W);
          d_ok = m.take<uint8_t>(W);
          d_kh = m.take<uint8_t>(28 * W);
        }) != hipSuccess) {
      c->err = "device allocation failed";
      return PRAOS_E_OOM;
    }
    const size_t lanes = std::min<size_t>((size_t)W, cfg->max_lanes ? cfg->max_lanes : TXW_LANES);
    if (c->txw_lanes < lanes) {
      HIPCHK(c, hipStreamSynchronize(s));
      (void)hipFree(c->txw_tabs);
      c->txw_tabs = nullptr;
      c->txw_lanes = 0;
      if (hipMalloc(&c->txw_tabs, lanes * LT_ED_B) != hipSuccess) {
        c->txw_tabs = nullptr;
        c->err = "device allocation failed";
        return PRAOS_E_OOM;
      }
      c->txw_lanes = lanes;
    }
    launch_txw_emit(s, T, b->arena, K.rows.wit_off, K.rows.wit_len, d_nv, d_nb, d_v0, d_v2, d_wfirst, W, d_tx, d_kind,
                    d_koff, d_soff);
    HIPCHK(c, hipGetLastError());
    for (size_t w0 = 0; w0 < W; w0 += lanes) {
      launch_txw_verify(s, w0, std::min<size_t>((size_t)W, w0 + lanes), c->btab, b->arena, d_tx, d_kind, d_koff, d_soff,
                        K.rows.tx_id, d_ok, d_kh, c->txw_tabs);
      HIPCHK(c, hipGetLastError());
    }
  }
  launch_txw_tx(s, T, d_wfirst, d_ok, d_txbad);
  HIPCHK(c, hipGetLastError());
  launch_txw_blocks(s, n, K.tfirst, d_st, d_cnt, d_txbad, d_bwit, d_bbad, d_bshape);
  HIPCHK(c, hipGetLastError());
  auto down = [&](void* dst, const void* src, size_t bytes) {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
  };
  if (bo) {
    HIPCHK(c, down(bo->n_wit, d_bwit, 4 * n));
    HIPCHK(c, down(bo->n_bad, d_bbad, 4 * n));
    HIPCHK(c, down(bo->n_shape, d_bshape, 4 * n));
  }
  const bool want_t = any_tx_array(txs), want_w = any_wit_array(wits);
  const bool short_t = want_t && txs->cap < T, short_w = want_w && wits->cap < W;
  if (short_t || short_w) {
    HIPCHK(c, hipStreamSynchronize(s));
    c->err = short_t ? "praos_verify_tx_witnesses: txs->cap too small" : "praos_verify_tx_witnesses: wits->cap too small";
    return PRAOS_E_ARG;
  }
  if (want_t) {
    HIPCHK(c, down(txs->block, K.rows.block, 4 * T));
    HIPCHK(c, down(txs->status, d_st, T));
    HIPCHK(c, down(txs->n_vkey, d_nv, 4 * T));
    HIPCHK(c, down(txs->n_boot, d_nb, 4 * T));
    HIPCHK(c, down(txs->n_bad, d_txbad, 4 * T));
    HIPCHK(c, down(txs->tx_id, K.rows.tx_id, 32 * T));
    if (txs->wit_first)
      for (size_t p = 0; p <= T; p++) txs->wit_first[p] = h_wfirst[p];
  }
  if (want_w && W) {
    HIPCHK(c, down(wits->tx, d_tx, 4 * (size_t)W));
    HIPCHK(c, down(wits->kind, d_kind, (size_t)W));
    HIPCHK(c, down(wits->key_off, d_koff, 8 * (size_t)W));
    HIPCHK(c, down(wits->sig_off, d_soff, 8 * (size_t)W));
    HIPCHK(c, down(wits->ok, d_ok, (size_t)W));
    HIPCHK(c, down(wits->key_hash, d_kh, 28 * (size_t)W));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  return PRAOS_OK;
}

}  // namespace

extern "C" {

int praos_block_batch_tx_witnesses(praos_ctx* c, praos_batch* b, const praos_txw_cfg* cfg, praos_txw_blocks* blocks_out,
                                   praos_txw_txs* txs, praos_txw_wits* wits) {
  if (!c || !b || !b->is_block || !cfg) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const int r = txw_run(c, b, cfg, blocks_out, txs, wits);
  (void)hipStreamSynchronize(c->stream);   // the call's buffers are freed on return
  return r;
}

int praos_verify_tx_witnesses(praos_ctx* c, const praos_header_bytes* blocks, const praos_txw_cfg* cfg,
                              praos_txw_blocks* blocks_out, praos_txw_txs* txs, praos_txw_wits* wits) {
  if (!c || !blocks || !cfg) return PRAOS_E_ARG;
  if (c->device < 0) { c->err = "host-only context: no HIP device"; return PRAOS_E_STATE; }
  if (blocks->n == 0) {
    if (txs) txs->n_rows = 0;
    if (wits) wits->n_wits = 0;
    if (blocks_out && blocks_out->tx_first) blocks_out->tx_first[0] = 0;
    if (txs && txs->wit_first) txs->wit_first[0] = 0;
    return PRAOS_OK;
  }
  praos_batch* b = praos_block_batch_upload(c, blocks);
  if (!b) return PRAOS_E_OOM;
  const int r = praos_block_batch_tx_witnesses(c, b, cfg, blocks_out, txs, wits);
  praos_batch_free(c, b);
  return r;
}

}  // extern "C"
