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
//
// The passes after the index are txw_rows_run, over any device rows (kind table, row block, wit
// span, tx_id): praos_verify_gen_txs (praos_gentx.hip) runs the same step over the rows of wire
// transactions, which have no block -- a one-entry kind table and a row_block of zeros.
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

}  // namespace

namespace praos_impl {

// the context's lane tables hold at least `lanes` lanes (grown, never shrunk; the stream is drained
// before they are replaced)
int txw_lane_tables(praos_ctx* c, size_t lanes) {
  if (c->txw_lanes >= lanes) return PRAOS_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  (void)hipFree(c->txw_tabs);
  c->txw_tabs = nullptr;
  c->txw_lanes = 0;
  if (hipMalloc(&c->txw_tabs, lanes * LT_ED_B) != hipSuccess) {
    c->txw_tabs = nullptr;
    c->err = "device allocation failed";
    return PRAOS_E_OOM;
  }
  c->txw_lanes = lanes;
  return PRAOS_OK;
}

// count, the counts down and their prefix sum up, emit, the verify slices, the per-row reduction:
// everything is enqueued on the context's stream; R owns the buffers and holds wit_first and W
int txw_rows_run(praos_ctx* c, const char* who, const uint8_t* arena, uint64_t arena_len, size_t T,
                 const uint8_t* blk_kind, const uint32_t* row_block, const uint64_t* wit_off, const uint32_t* wit_len,
                 const uint8_t* tx_id, uint32_t max_lanes, txw_rows& R) {
  hipStream_t s = c->stream;
  if (carve_alloc(R.buf_t, [&](Carve& m) {
        R.st = m.take<uint8_t>(T);
        R.nv = m.take<uint32_t>(4 * T);
        R.nb = m.take<uint32_t>(4 * T);
        R.cnt = m.take<uint32_t>(4 * T);
        R.d_wfirst = m.take<uint32_t>(4 * (T + 1));
        R.txbad = m.take<uint32_t>(4 * T);
        R.v0 = m.take<uint64_t>(8 * T);
        R.v2 = m.take<uint64_t>(8 * T);
      }) != hipSuccess) {
    c->err = "device allocation failed";
    return PRAOS_E_OOM;
  }
  (void)hipGetLastError();
  launch_txw_count(s, T, arena, arena_len, blk_kind, row_block, wit_off, wit_len, R.st, R.nv, R.nb, R.cnt, R.v0, R.v2);
  HIPCHK(c, hipGetLastError());
  std::vector<uint32_t> h_cnt(T);
  R.wfirst.assign(T + 1, 0);
  HIPCHK(c, hipMemcpyAsync(h_cnt.data(), R.cnt, 4 * T, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  uint64_t W = 0;
  for (size_t p = 0; p < T; p++) {
    R.wfirst[p] = (uint32_t)W;
    W += h_cnt[p];
    if (W > 0xfffffff0ull) { c->err = std::string(who) + ": too many witnesses in one call"; return PRAOS_E_ARG; }
  }
  R.wfirst[T] = (uint32_t)W;
  R.W = W;
  HIPCHK(c, hipMemcpyAsync(R.d_wfirst, R.wfirst.data(), 4 * (T + 1), hipMemcpyHostToDevice, s));
  if (W) {
    if (carve_alloc(R.buf_w, [&](Carve& m) {
          R.tx = m.take<uint32_t>(4 * W);
          R.kind = m.take<uint8_t>(W);
          R.koff = m.take<uint64_t>(8 * W);
          R.soff = m.take<uint64_t>(8 * W);
          R.ok = m.take<uint8_t>(W);
          R.kh = m.take<uint8_t>(28 * W);
        }) != hipSuccess) {
      c->err = "device allocation failed";
      return PRAOS_E_OOM;
    }
    const size_t lanes = std::min<size_t>((size_t)W, max_lanes ? max_lanes : TXW_LANES);
    const int rt = txw_lane_tables(c, lanes);
    if (rt != PRAOS_OK) return rt;
    launch_txw_emit(s, T, arena, wit_off, wit_len, R.nv, R.nb, R.v0, R.v2, R.d_wfirst, W, R.tx, R.kind, R.koff, R.soff);
    HIPCHK(c, hipGetLastError());
    for (size_t w0 = 0; w0 < W; w0 += lanes) {
      launch_txw_verify(s, w0, std::min<size_t>((size_t)W, w0 + lanes), c->btab, arena, R.tx, R.kind, R.koff, R.soff,
                        tx_id, R.ok, R.kh, c->txw_tabs);
      HIPCHK(c, hipGetLastError());
    }
  }
  launch_txw_tx(s, T, R.d_wfirst, R.ok, R.txbad);
  HIPCHK(c, hipGetLastError());
  return PRAOS_OK;
}

// the witness records into the caller's arrays (enqueued; the caller synchronises)
int txw_rows_down_wits(praos_ctx* c, praos_txw_wits* wits, const txw_rows& R) {
  hipStream_t s = c->stream;
  const size_t W = (size_t)R.W;
  if (!W) return PRAOS_OK;
  const Down down{s};
  HIPCHK(c, down(wits->tx, R.tx, 4 * W));
  HIPCHK(c, down(wits->kind, R.kind, W));
  HIPCHK(c, down(wits->key_off, R.koff, 8 * W));
  HIPCHK(c, down(wits->sig_off, R.soff, 8 * W));
  HIPCHK(c, down(wits->ok, R.ok, W));
  HIPCHK(c, down(wits->key_hash, R.kh, 28 * W));
  return PRAOS_OK;
}

// the whole call over a block batch: b's n, arena and block spans are all it reads of the batch
// (praos_blockfetch.hip passes one whose blocks are the rows of distinct wire blocks)
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
  // ---- the witness passes over the rows
  praos_impl::txw_rows R;
  const int rr = praos_impl::txw_rows_run(c, "praos_verify_tx_witnesses", b->arena, b->arena_len, T, K.kind, K.rows.block,
                                          K.rows.wit_off, K.rows.wit_len, K.rows.tx_id, cfg->max_lanes, R);
  if (wits) wits->n_wits = (size_t)R.W;
  if (rr != PRAOS_OK) return rr;
  const uint64_t W = R.W;
  uint32_t *d_bwit = nullptr, *d_bbad = nullptr, *d_bshape = nullptr;
  DevBuf buf_b;
  if (carve_alloc(buf_b, [&](Carve& m) {
        d_bwit = m.take<uint32_t>(4 * n);
        d_bbad = m.take<uint32_t>(4 * n);
        d_bshape = m.take<uint32_t>(4 * n);
      }) != hipSuccess) {
    c->err = "device allocation failed";
    return PRAOS_E_OOM;
  }
  launch_txw_blocks(s, n, K.tfirst, R.st, R.cnt, R.txbad, d_bwit, d_bbad, d_bshape);
  HIPCHK(c, hipGetLastError());
  const Down down{s};
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
    HIPCHK(c, down(txs->status, R.st, T));
    HIPCHK(c, down(txs->n_vkey, R.nv, 4 * T));
    HIPCHK(c, down(txs->n_boot, R.nb, 4 * T));
    HIPCHK(c, down(txs->n_bad, R.txbad, 4 * T));
    HIPCHK(c, down(txs->tx_id, K.rows.tx_id, 32 * T));
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

}  // namespace praos_impl

extern "C" {

int praos_block_batch_tx_witnesses(praos_ctx* c, praos_batch* b, const praos_txw_cfg* cfg, praos_txw_blocks* blocks_out,
                                   praos_txw_txs* txs, praos_txw_wits* wits) {
  if (!c || !b || !b->is_block || !cfg) return PRAOS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const int r = praos_impl::txw_run(c, b, cfg, blocks_out, txs, wits);
  (void)hipStreamSynchronize(c->stream);   // the call's buffers are freed on return
  return r;
}

int praos_verify_tx_witnesses(praos_ctx* c, const praos_header_bytes* blocks, const praos_txw_cfg* cfg,
                              praos_txw_blocks* blocks_out, praos_txw_txs* txs, praos_txw_wits* wits) {
  if (!c || !blocks || !cfg) return PRAOS_E_ARG;
  if (praos_host_only_(c)) return PRAOS_E_STATE;
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
