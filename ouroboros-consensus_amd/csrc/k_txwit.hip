// k_txwit.hip -- the key witnesses of stored blocks' transactions: every VKey
// witness and bootstrap witness checked as an Ed25519 signature over its transaction's txId, the
// check applyBlockLedgerResult with STS.ValidateAll (Shelley/Ledger/Ledger.hs:335-352) and the
// mempool's applyShelleyTx (Shelley/Ledger/Mempool.hs:215-239) make once per witness on the CPU.
//
// Input: the final rows of the transaction index (k_txindex.hip: block, witness-set span, tx_id)
// and its kind per block.  The witness set is a map; the value under its first key 0 is the VKey
// witnesses [[vkey, sig], ...], under its first key 2 the bootstrap witnesses [[vkey, sig,
// chain_code, attributes], ...], each optionally in tag 258; the rules are praos_hip.h's.
//   k_txw_count   one lane per row: the map walked to keys 0 and 2, every item of the two values
//                 checked against the shapes and counted; the values' offsets are kept for the
//                 emit pass.  A Byron row is SKIPPED, a row outside the shapes SHAPE; both count 0.
//   k_txw_emit    one lane per row with witnesses: (row, kind, key offset, signature offset) at
//                 wit_first[row] + j, the key-0 items first.
//   k_txw_verify  one lane per witness of a slice: R, S and A from the arena, hram = SHA-512(R ||
//                 A || tx_id) (96 bytes, one block), Blake2b-224 of A for a VKey witness, then
//                 ed25519_verify_core with the lane's own tables, as k_pbft_sig and k_ocert run
//                 it.  The two hashes are in the verify kernel, as k_ocert's are: they are a
//                 thousandth of the curve arithmetic and their registers are dead before it, and
//                 a pass of their own would write and read back 160 bytes per witness.
//   k_txw_tx      one lane per row: the row's witnesses that do not verify.
//   k_txw_blocks  one lane per block: n_wit, n_bad, n_shape over the block's rows.
// The walks read item heads with byte loads, one lane per witness set, as k_txi_rows does: they
// are latency-bound and short beside the verifies.
// CPU restatement: tests/tx_witness_model.py.
#include "byron_dev.hpp"
#include "tx_dev.hpp"

namespace {

// Where the witness records of one row go (emit pass; count pass: tx = null)
struct WitOut {
  uint32_t* __restrict__ tx;
  uint8_t* __restrict__ kind;
  uint64_t* __restrict__ key_off;
  uint64_t* __restrict__ sig_off;
};

// The value of key 0 (arity 2) or key 2 (arity 4) at c: [tag 258] array of items [vkey 32, sig 64
// (, chain_code, attributes)].  Returns false outside the shapes; cnt = its items.  With o.tx set
// item j < lim is written at base + j.
__device__ bool walk_wits(Cur& c, uint32_t arity, uint64_t& cnt, const WitOut& o, uint32_t row, uint8_t kd,
                          uint64_t base, uint64_t lim) {
  uint32_t mt, ai;
  uint64_t arg;
  bool indef;
  if (!head(c, mt, ai, arg, indef)) return false;
  if (mt == 6) {
    if (arg != 258) return false;
    if (!head(c, mt, ai, arg, indef)) return false;
  }
  if (mt != 4) return false;
  Lvl l{arg, indef};
  bool ok = true;
  uint64_t k = 0;
  while (ok && more(c, l, ok)) {
    uint64_t key_at = 0, sig_at = 0;
    Lvl e;
    if (!open_k(c, arity, e)) return false;
    if (!(rd_bytes(c, 32, key_at) && rd_bytes(c, 64, sig_at))) return false;
    if (arity == 4 && !(cbor_skip_regs(c) && cbor_skip_regs(c))) return false;
    if (!shut(c, e)) return false;
    if (o.tx && k < lim) {
      o.tx[base + k] = row;
      o.kind[base + k] = kd;
      o.key_off[base + k] = key_at;
      o.sig_off[base + k] = sig_at;
    }
    k++;
  }
  cnt = k;
  return ok;
}

struct TxwCount {
  const uint8_t* __restrict__ arena;
  uint64_t arena_len;
  const uint8_t* __restrict__ blk_kind;
  const uint32_t* __restrict__ row_block;
  const uint64_t* __restrict__ wit_off;
  const uint32_t* __restrict__ wit_len;
  uint8_t* __restrict__ status;
  uint32_t* __restrict__ n_vkey;
  uint32_t* __restrict__ n_boot;
  uint32_t* __restrict__ cnt;
  uint64_t* __restrict__ v0;          // offset of the value under key 0 (0: none), of key 2
  uint64_t* __restrict__ v2;
};

__global__ void __launch_bounds__(NT) k_txw_count(size_t nrows, TxwCount a) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nrows) return;
  uint8_t st = PRAOS_TXW_OK;
  uint64_t nv = 0, nb = 0, at0 = 0, at2 = 0;
  const uint64_t wo = a.wit_off[p];
  const uint32_t wl = a.wit_len[p];
  if (a.blk_kind[a.row_block[p]] == TXK_BYRON) {
    st = PRAOS_TXW_SKIPPED;
  } else if (!(wo <= a.arena_len && wl <= a.arena_len - wo)) {
    st = PRAOS_TXW_SHAPE;   // the index leaves no such row
  } else {
    Cur c{a.arena, wo, wo + wl, true};
    uint32_t mt, ai;
    uint64_t arg;
    bool indef;
    bool ok = head(c, mt, ai, arg, indef);
    if (ok && mt == 5) {
      Lvl m{arg, indef};
      bool seen0 = false, seen2 = false;
      const WitOut none{nullptr, nullptr, nullptr, nullptr};
      while (ok && !(seen0 && seen2) && more(c, m, ok)) {
        const uint64_t ks = c.p;
        uint32_t kmt;
        uint64_t key;
        if (!head(c, kmt, ai, key, indef)) { ok = false; break; }
        if (kmt == 0 && key == 0 && !seen0) {
          seen0 = true;
          at0 = c.p;
          ok = walk_wits(c, 2, nv, none, 0, 0, 0, 0);
        } else if (kmt == 0 && key == 2 && !seen2) {
          seen2 = true;
          at2 = c.p;
          ok = walk_wits(c, 4, nb, none, 0, 0, 0, 0);
        } else {
          skip_pair(c, ks, kmt, ok);
        }
      }
    }
    // a count past u32 cannot come from a block whose length is u32; refused all the same
    if (!ok || nv + nb > 0xffffffffull) st = PRAOS_TXW_SHAPE;
  }
  if (st != PRAOS_TXW_OK) nv = nb = at0 = at2 = 0;
  a.status[p] = st;
  a.n_vkey[p] = (uint32_t)nv;
  a.n_boot[p] = (uint32_t)nb;
  a.cnt[p] = (uint32_t)(nv + nb);
  a.v0[p] = at0;
  a.v2[p] = at2;
}

__global__ void __launch_bounds__(NT) k_txw_emit(size_t nrows, const uint8_t* __restrict__ arena,
                                                 const uint64_t* __restrict__ wit_off,
                                                 const uint32_t* __restrict__ wit_len,
                                                 const uint32_t* __restrict__ n_vkey,
                                                 const uint32_t* __restrict__ n_boot,
                                                 const uint64_t* __restrict__ v0, const uint64_t* __restrict__ v2,
                                                 const uint32_t* __restrict__ wit_first, uint64_t n_wits, WitOut o) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nrows) return;
  const uint32_t nv = n_vkey[p], nb = n_boot[p];
  if (nv + nb == 0) return;
  const uint64_t base = wit_first[p], end = wit_off[p] + wit_len[p];
  if (base > n_wits || (uint64_t)nv + nb > n_wits - base) return;   // the host's prefix sum says otherwise
  uint64_t k;
  if (nv) {
    Cur c{arena, v0[p], end, true};
    (void)walk_wits(c, 2, k, o, (uint32_t)p, 0, base, nv);
  }
  if (nb) {
    Cur c{arena, v2[p], end, true};
    (void)walk_wits(c, 4, k, o, (uint32_t)p, 2, base + nv, nb);
  }
}

struct TxwVerify {
  const uint8_t* __restrict__ arena;
  const uint32_t* __restrict__ tx;
  const uint8_t* __restrict__ kind;
  const uint64_t* __restrict__ key_off;
  const uint64_t* __restrict__ sig_off;
  const uint8_t* __restrict__ tx_id;     // rows x 32
  uint8_t* __restrict__ ok;
  uint8_t* __restrict__ key_hash;        // n_wits x 28
  ge_cached* __restrict__ tabs;          // per-lane tables of one slice (LT_ED entries per lane)
};

// witnesses [w0, w1): lane t of the launch takes witness w0 + t and table region t
__global__ void __launch_bounds__(NT, LB_ED) k_txw_verify(size_t w0, size_t w1, const ge_niels* __restrict__ gbtab,
                                                         TxwVerify a) {
  __shared__ ge_niels sbtab[BTAB_N];
  const ge_niels* btab = stage_btab<1>(gbtab, sbtab);
  const size_t t = (size_t)blockIdx.x * NT + threadIdx.x;
  const size_t w = w0 + t;
  if (w >= w1) return;
  uint32_t pk[8], sg[16], id[8], hram[16];
  ld_bytes32(pk, a.arena, a.key_off[w]);
  const uint64_t so = a.sig_off[w];
  ld_bytes32(sg, a.arena, so);
  ld_bytes32(sg + 8, a.arena, so + 32);
  load_words(id, a.tx_id + 32 * (size_t)a.tx[w], 8);
  {
    uint64_t H[8], W[16];
    sha512_init(H);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      W[i] = be_word(sg[2 * i], sg[2 * i + 1]);
      W[4 + i] = be_word(pk[2 * i], pk[2 * i + 1]);
      W[8 + i] = be_word(id[2 * i], id[2 * i + 1]);
    }
    W[12] = 0x8000000000000000ULL;
    W[13] = 0;
    W[14] = 0;
    W[15] = 96u * 8u;
    sha512_block(H, W);
    sha512_digest_words(hram, H);
  }
  uint32_t kh[8];
  blake2b_32(kh, pk, 28);
  const bool vkey = a.kind[w] == 0;
  uint32_t* q = (uint32_t*)(a.key_hash + 28 * w);
#pragma unroll
  for (int k = 0; k < 7; k++) q[k] = vkey ? kh[k] : 0u;
  a.ok[w] = ed25519_verify_core(pk, sg, sg + 8, hram, btab, lane_tab(a.tabs, t, LT_ED)) ? 1 : 0;
}

__global__ void __launch_bounds__(NT) k_txw_tx(size_t nrows, const uint32_t* __restrict__ wit_first,
                                               const uint8_t* __restrict__ ok, uint32_t* __restrict__ n_bad) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nrows) return;
  uint32_t bad = 0;
  for (uint32_t w = wit_first[p]; w < wit_first[p + 1]; w++) bad += ok[w] ? 0u : 1u;
  n_bad[p] = bad;
}

__global__ void __launch_bounds__(NT) k_txw_blocks(size_t n, const uint32_t* __restrict__ tfirst,
                                                   const uint8_t* __restrict__ status,
                                                   const uint32_t* __restrict__ cnt,
                                                   const uint32_t* __restrict__ tx_bad, uint32_t* __restrict__ n_wit,
                                                   uint32_t* __restrict__ n_bad, uint32_t* __restrict__ n_shape) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t nw = 0, bad = 0, shp = 0;
  for (uint32_t p = tfirst[i]; p < tfirst[i + 1]; p++) {
    nw += cnt[p];
    bad += tx_bad[p];
    shp += status[p] == PRAOS_TXW_SHAPE ? 1u : 0u;
  }
  n_wit[i] = nw;
  n_bad[i] = bad;
  n_shape[i] = shp;
}

}  // namespace

// ---- host launchers (kernels are only launchable from their own module)
void launch_txw_count(hipStream_t stream, size_t nrows, const uint8_t* arena, uint64_t arena_len,
                      const uint8_t* blk_kind, const uint32_t* row_block, const uint64_t* wit_off,
                      const uint32_t* wit_len, uint8_t* status, uint32_t* n_vkey, uint32_t* n_boot, uint32_t* cnt,
                      uint64_t* v0, uint64_t* v2) {
  TxwCount a{arena, arena_len, blk_kind, row_block, wit_off, wit_len, status, n_vkey, n_boot, cnt, v0, v2};
  hipLaunchKernelGGL(k_txw_count, dim3((unsigned)((nrows + NT - 1) / NT)), dim3(NT), 0, stream, nrows, a);
}

void launch_txw_emit(hipStream_t stream, size_t nrows, const uint8_t* arena, const uint64_t* wit_off,
                     const uint32_t* wit_len, const uint32_t* n_vkey, const uint32_t* n_boot, const uint64_t* v0,
                     const uint64_t* v2, const uint32_t* wit_first, uint64_t n_wits, uint32_t* tx, uint8_t* kind,
                     uint64_t* key_off, uint64_t* sig_off) {
  WitOut o{tx, kind, key_off, sig_off};
  hipLaunchKernelGGL(k_txw_emit, dim3((unsigned)((nrows + NT - 1) / NT)), dim3(NT), 0, stream, nrows, arena, wit_off,
                     wit_len, n_vkey, n_boot, v0, v2, wit_first, n_wits, o);
}

void launch_txw_verify(hipStream_t stream, size_t w0, size_t w1, const ge_niels* gbtab, const uint8_t* arena,
                       const uint32_t* tx, const uint8_t* kind, const uint64_t* key_off, const uint64_t* sig_off,
                       const uint8_t* tx_id, uint8_t* ok, uint8_t* key_hash, ge_cached* tabs) {
  TxwVerify a{arena, tx, kind, key_off, sig_off, tx_id, ok, key_hash, tabs};
  hipLaunchKernelGGL(k_txw_verify, dim3((unsigned)((w1 - w0 + NT - 1) / NT)), dim3(NT), 0, stream, w0, w1, gbtab, a);
}

void launch_txw_tx(hipStream_t stream, size_t nrows, const uint32_t* wit_first, const uint8_t* ok, uint32_t* n_bad) {
  hipLaunchKernelGGL(k_txw_tx, dim3((unsigned)((nrows + NT - 1) / NT)), dim3(NT), 0, stream, nrows, wit_first, ok,
                     n_bad);
}

void launch_txw_blocks(hipStream_t stream, size_t n, const uint32_t* tfirst, const uint8_t* status,
                       const uint32_t* cnt, const uint32_t* tx_bad, uint32_t* n_wit, uint32_t* n_bad,
                       uint32_t* n_shape) {
  hipLaunchKernelGGL(k_txw_blocks, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, tfirst, status, cnt,
                     tx_bad, n_wit, n_bad, n_shape);
}
