// k_byron.hip -- Byron blocks and EBBs of an ImmutableDB chunk (the
// storage path's last block format).
//
// Stored form (Byron/Ledger/Serialisation.hs:165-177): 82 00 83 <hdr> <body> <extra> is an EBB,
// 82 01 83 <hdr> <body> <extra> a main block; header hash = Blake2b-256(82 0k || hdr).
//   main header = [pm, prev(bytes32), proof, consensus, extra]
//     proof     = [[nTx, txRoot(32), witHash(32)], sscProof, dlgHash(32), updHash(32)]
//     consensus = [[epoch, slotInEpoch], issuerXPub(64), [difficulty],
//                  [2, [[certEpoch, issuerXPub, delegateXPub, certSig(64)], sig(64)]]]
//   EBB header  = [pm, prev(bytes32), bodyProof(bytes32), [epoch, [difficulty]], extra]
//   main body   = [txPayload, sscPayload, dlgPayload, updPayload], txPayload = a definite or
//                 indefinite list of [tx, witnesses]
//
//   k_byron_split      one lane per stored block (pass A of the chunk parse, and the first
//                      step of the integrity batch): envelope and header by the shapes above,
//                      the columns the Shelley path fills (header span, slot, block_no,
//                      prev_hash / prev_is_genesis, header hash), a kind byte (0 not a Byron
//                      item: the lane's columns are left alone; 1 EBB; 2 main block; 3 a
//                      Byron item that does not decode) and, for main blocks, the span table
//                      k_byron_integrity reads (BS_*, offsets relative to the block).
//   k_byron_integrity  one lane per block: verifyHeaderIntegrity (Byron/Ledger/Integrity.hs:
//                      21-53, PBFT.hs:55-75: pm == configured pm, Ed25519 under the first 32
//                      bytes of delegateXPub over "01" || issuerXPub || 09 || CBOR(pm) || 85 ||
//                      the stored prev, proof, slot-id, difficulty and extra items) and
//                      blockMatchesHeader (Block.hs:161-162: dlgHash, updHash, nTx, witHash,
//                      txRoot; the ssc proof is not compared).  SHA-512 and the witness hash
//                      stream from the arena through a 128-byte register buffer (no staging
//                      copy, no length cap); the transaction leaves and the witness gather
//                      are one walk of txPayload by the block's own lane; the Merkle root is
//                      a binary-counter stack of at most 32 hashes folded from the right
//                      (node = H(01 || l || r), leaf = H(00 || tx), empty = H("")): the tree
//                      that splits at the largest power of two below n.
// This is as far as the library decodes Byron blocks: the reference's transaction, ssc,
// delegation and update decoders are stricter (a body whose items are well-formed CBOR but not
// valid payloads is a ReadFailure there, accepted here).
// CPU restatement: tests/byron_model.py.
#include "byron_dev.hpp"

namespace {

// span table of a main block, column-major ([BS_*][i]), u32 relative to the block's start
enum : uint32_t {
  BS_PM = 0,
  BS_PREV_O, BS_PREV_L, BS_PROOF_O, BS_PROOF_L, BS_SID_O, BS_SID_L, BS_DIFF_O, BS_DIFF_L, BS_EXTRA_O, BS_EXTRA_L,
  BS_ISSUER, BS_DELEG, BS_SIG,                       // raw 64-byte strings
  BS_TXROOT, BS_WITH, BS_DLGH, BS_UPDH,              // raw 32-byte hashes of the proof
  BS_NTX_LO, BS_NTX_HI,
  BS_TXP_O, BS_TXP_L, BS_SSC_O, BS_SSC_L, BS_DLG_O, BS_DLG_L, BS_UPD_O, BS_UPD_L,
  BS_COUNT
};
static_assert(BS_COUNT == PRAOS_BYRON_SPANS, "span table width");
static_assert(BS_TXP_O == PRAOS_BYRON_SPAN_TXP && BS_TXP_L == BS_TXP_O + 1, "the columns k_txindex.hip reads");

__global__ void __launch_bounds__(NT) k_byron_split(size_t n, const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                    const uint64_t* __restrict__ blk_off,
                                                    const uint32_t* __restrict__ blk_len, uint64_t epoch_slots,
                                                    uint64_t* __restrict__ hoff, uint32_t* __restrict__ hlen,
                                                    uint64_t* __restrict__ slot, uint64_t* __restrict__ block_no,
                                                    uint8_t* __restrict__ prev_hash, uint8_t* __restrict__ prev_genesis,
                                                    uint8_t* __restrict__ header_hash, uint8_t* __restrict__ split_status,
                                                    uint16_t* __restrict__ dec_status, uint8_t* __restrict__ kind,
                                                    uint64_t* __restrict__ epoch_out, uint32_t* __restrict__ spans) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t off = blk_off[i];
  const uint32_t len = blk_len[i];
  kind[i] = 0;
  if (!(off <= arena_len && len <= arena_len - off)) return;
  Cur c{arena, off, off + len, true};
  uint32_t mt, ai;
  uint64_t arg, k01;
  bool indef;
  if (!(head(c, mt, ai, arg, indef) && mt == 4 && !indef && arg >= 1)) return;
  if (!(head(c, mt, ai, k01, indef) && mt == 0 && k01 <= 1)) return;
  // a Byron item from here on: what does not fit the shapes is a decode failure
  kind[i] = 3;
  const bool ebb = k01 == 0;
  bool ok = arg == 2 && rd_list(c, 3);
  uint64_t ho = 0, he = 0, bo = 0, be = 0;
  if (ok) {
    ho = c.p;
    ok = cbor_skip_regs(c);
    he = bo = c.p;
    ok = ok && cbor_skip_regs(c);
    be = c.p;
    ok = ok && cbor_skip_regs(c) && c.p == c.end;
  }
  if (!ok) return;
  Cur h{arena, ho, he, true};
  uint64_t pm = 0, prev_at = 0, epoch = 0, sie = 0, diff = 0, t;
  uint32_t sp[BS_COUNT];
#pragma unroll
  for (uint32_t k = 0; k < BS_COUNT; k++) sp[k] = 0;
  auto rel = [&](uint64_t p) { return (uint32_t)(p - off); };
  ok = rd_list(h, 5) && rd_uint(h, 0xffffffffu, pm);
  sp[BS_PREV_O] = rel(h.p);
  ok = ok && rd_bytes(h, 32, prev_at);
  sp[BS_PREV_L] = rel(h.p) - sp[BS_PREV_O];
  if (ebb) {
    ok = ok && rd_bytes(h, 32, t) && rd_list(h, 2) && rd_uint(h, ~0ull, epoch) && rd_list(h, 1) &&
         rd_uint(h, ~0ull, diff) && cbor_skip_regs(h) && h.p == he;
  } else {
    sp[BS_PROOF_O] = rel(h.p);
    ok = ok && rd_list(h, 4) && rd_list(h, 3) && rd_uint(h, ~0ull, t);
    sp[BS_NTX_LO] = (uint32_t)t;
    sp[BS_NTX_HI] = (uint32_t)(t >> 32);
    ok = ok && rd_bytes(h, 32, t);
    sp[BS_TXROOT] = rel(t);
    ok = ok && rd_bytes(h, 32, t);
    sp[BS_WITH] = rel(t);
    ok = ok && cbor_skip_regs(h) && rd_bytes(h, 32, t);
    sp[BS_DLGH] = rel(t);
    ok = ok && rd_bytes(h, 32, t);
    sp[BS_UPDH] = rel(t);
    sp[BS_PROOF_L] = rel(h.p) - sp[BS_PROOF_O];
    ok = ok && rd_list(h, 4);
    sp[BS_SID_O] = rel(h.p);
    ok = ok && rd_list(h, 2) && rd_uint(h, ~0ull, epoch) && rd_uint(h, 0xffffu, sie);
    sp[BS_SID_L] = rel(h.p) - sp[BS_SID_O];
    ok = ok && rd_bytes(h, 64, t);
    sp[BS_ISSUER] = rel(t);
    sp[BS_DIFF_O] = rel(h.p);
    ok = ok && rd_list(h, 1) && rd_uint(h, ~0ull, diff);
    sp[BS_DIFF_L] = rel(h.p) - sp[BS_DIFF_O];
    ok = ok && rd_list(h, 2) && rd_uint(h, ~0ull, t) && t == 2 && rd_list(h, 2) && rd_list(h, 4) &&
         rd_uint(h, ~0ull, t) && rd_bytes(h, 64, t) && rd_bytes(h, 64, t);
    sp[BS_DELEG] = rel(t);
    ok = ok && rd_bytes(h, 64, t) && rd_bytes(h, 64, t);
    sp[BS_SIG] = rel(t);
    sp[BS_EXTRA_O] = rel(h.p);
    ok = ok && cbor_skip_regs(h) && h.p == he;
    sp[BS_EXTRA_L] = rel(h.p) - sp[BS_EXTRA_O];
    // body = [txPayload, ssc, dlg, upd]
    Cur b{arena, bo, be, true};
    ok = ok && rd_list(b, 4);
    sp[BS_TXP_O] = rel(b.p);
    uint64_t cnt = 0;
    ok = ok && head(b, mt, ai, cnt, indef) && mt == 4;
    for (uint64_t j = 0; ok && (indef ? (b.p < be && arena[b.p] != 0xFF) : j < cnt); j++)
      ok = rd_list(b, 2) && cbor_skip_regs(b) && cbor_skip_regs(b);
    if (ok && indef) { ok = b.p < be; b.p++; }
    sp[BS_TXP_L] = rel(b.p) - sp[BS_TXP_O];
    sp[BS_SSC_O] = rel(b.p);
    ok = ok && cbor_skip_regs(b);
    sp[BS_SSC_L] = rel(b.p) - sp[BS_SSC_O];
    sp[BS_DLG_O] = rel(b.p);
    ok = ok && cbor_skip_regs(b);
    sp[BS_DLG_L] = rel(b.p) - sp[BS_DLG_O];
    sp[BS_UPD_O] = rel(b.p);
    ok = ok && cbor_skip_regs(b) && b.p == be;
    sp[BS_UPD_L] = rel(b.p) - sp[BS_UPD_O];
  }
  if (!ok) return;
  sp[BS_PM] = (uint32_t)pm;
  kind[i] = ebb ? 1 : 2;
  hoff[i] = ho;
  hlen[i] = (uint32_t)(he - ho);
  slot[i] = epoch * epoch_slots + sie;
  block_no[i] = diff;
  epoch_out[i] = epoch;
  // an EBB of epoch 0 has GenesisHash (Block.hs:215-221): its 32 bytes are no block's hash
  const bool gen = ebb && epoch == 0;
  uint32_t w[8];
  ld_bytes32(w, arena, prev_at);
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = gen ? 0u : w[k];
  store_words(prev_hash + 32 * i, w, 8);
  prev_genesis[i] = gen ? 1 : 0;
  b2b256_pre(w, arena, ho, he - ho, 2, 0x82u | (ebb ? 0u : 0x100u));
  store_words(header_hash + 32 * i, w, 8);
  split_status[i] = 0;
  dec_status[i] = 0;
  if (spans && !ebb) {
#pragma unroll
    for (uint32_t k = 0; k < BS_COUNT; k++) spans[(size_t)k * n + i] = sp[k];
  }
}

__global__ void __launch_bounds__(NT) k_byron_integrity(size_t n, const uint8_t* __restrict__ arena,
                                                        const uint64_t* __restrict__ blk_off,
                                                        const uint32_t* __restrict__ blk_len,
                                                        const uint8_t* __restrict__ kind,
                                                        const uint32_t* __restrict__ spans, uint32_t cfg_pm,
                                                        const ge_niels* __restrict__ gbtab, ge_cached* __restrict__ tabs,
                                                        uint8_t* __restrict__ result, uint8_t* __restrict__ which) {
  if ((size_t)blockIdx.x * NT >= n) return;
  __shared__ ge_niels sbtab[BTAB_N];
  const ge_niels* btab = stage_btab<1>(gbtab, sbtab);
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const uint32_t kd = kind[i];
  if (kd != 2) {
    result[i] = kd == 1 ? 0 : PRAOS_BLK_DECODE;   // verifyBlockIntegrity of an EBB is True
    which[i] = 0;
    return;
  }
  const uint64_t off = blk_off[i], end = off + blk_len[i];
  auto S = [&](uint32_t k) { return spans[(size_t)k * n + i]; };
  auto A = [&](uint32_t k) { return off + S(k); };
  uint8_t bits = 0, wh = 0;
  const uint32_t pm = S(BS_PM);
  if (pm != cfg_pm) bits |= PRAOS_BLK_PM;

  // ---- the PBFT signature: SHA-512(R || A || message), pieces streamed from the arena
  uint32_t hram[16];
  {
    // 09 || CBOR(pm) || 85 as little-endian bytes of one word
    uint64_t enc;
    uint32_t el;
    if (pm < 24) { enc = pm; el = 1; }
    else if (pm < 0x100u) { enc = 0x18u | ((uint64_t)pm << 8); el = 2; }
    else if (pm < 0x10000u) { enc = 0x19u | ((uint64_t)(pm >> 8) << 8) | ((uint64_t)(pm & 0xffu) << 16); el = 3; }
    else { enc = 0x1au | ((uint64_t)__builtin_bswap32(pm) << 8); el = 5; }
    const uint64_t mid = 0x09u | (enc << 8) | (0x85ull << (8 * (1 + el)));
    Hs<true> s;
    s.init();
#pragma nounroll
    for (uint32_t p = 0; p < 10; p++) {
      uint64_t pos = 0, len = 0, lit = 0;
      switch (p) {
        case 0: pos = A(BS_SIG); len = 32; break;
        case 1: pos = A(BS_DELEG); len = 32; break;
        case 2: lit = 0x3130; len = 2; break;                       // "01"
        case 3: pos = A(BS_ISSUER); len = 64; break;
        case 4: lit = mid; len = 2 + el; break;
        case 5: pos = A(BS_PREV_O); len = S(BS_PREV_L); break;
        case 6: pos = A(BS_PROOF_O); len = S(BS_PROOF_L); break;
        case 7: pos = A(BS_SID_O); len = S(BS_SID_L); break;
        case 8: pos = A(BS_DIFF_O); len = S(BS_DIFF_L); break;
        default: pos = A(BS_EXTRA_O); len = S(BS_EXTRA_L); break;
      }
      const bool is_lit = p == 2 || p == 4;
      while (len) {
        const uint32_t k = len < 8 ? (uint32_t)len : 8u;
        s.put(is_lit ? lit : ld64u(arena, pos), k);
        pos += k;
        len -= k;
      }
    }
    s.sha512_finish(hram);
  }
  uint32_t pk[8], sg[16];
  ld_bytes32(pk, arena, A(BS_DELEG));
  ld_bytes32(sg, arena, A(BS_SIG));
  ld_bytes32(sg + 8, arena, A(BS_SIG) + 32);
  if (!ed25519_verify_core(pk, sg, sg + 8, hram, btab, lane_tab(tabs, i, LT_ED))) bits |= PRAOS_BLK_PBFT_SIG;

  // ---- blockMatchesHeader
  uint32_t got[8], want[8];
  auto differs = [&]() {
    bool d = false;
#pragma unroll
    for (int k = 0; k < 8; k++) d |= got[k] != want[k];
    return d;
  };
#pragma nounroll
  for (uint32_t k = 0; k < 2; k++) {   // dlgPayload, updPayload
    b2b256_pre(got, arena, A(k ? BS_UPD_O : BS_DLG_O), S(k ? BS_UPD_L : BS_DLG_L), 0, 0);
    ld_bytes32(want, arena, A(k ? BS_UPDH : BS_DLGH));
    if (differs()) wh |= k ? PRAOS_BYRON_W_UPD : PRAOS_BYRON_W_DLG;
  }
  // one walk of txPayload: leaf hashes into the Merkle stack, witnesses into the gather hash
  uint32_t stk[32][8];
  uint32_t sp = 0;
  uint64_t cnt = 0, ndef = 0;
  bool ok = true, indef = false;
  Cur c{arena, A(BS_TXP_O), A(BS_TXP_O) + S(BS_TXP_L), true};
  {
    uint32_t mt, ai;
    ok = head(c, mt, ai, ndef, indef) && mt == 4;
  }
  Hs<false> wg;
  wg.init();
  uint32_t st = 0;
#pragma nounroll
  while (ok && st < 2) {
    uint64_t pos = 0, len = 1, lit = 0x9f;
    bool is_lit = true;
    if (st == 0) {
      st = 1;
    } else if (indef ? (c.p < c.end && arena[c.p] != 0xFF) : cnt < ndef) {
      ok = rd_list(c, 2);
      const uint64_t ts = c.p;
      ok = ok && cbor_skip(c);
      const uint64_t ws = c.p;
      ok = ok && cbor_skip(c) && c.p <= end;
      if (!ok) break;
      cnt++;
      b2b256_pre(got, arena, ts, ws - ts, 1, 0);           // leaf = H(00 || tx)
      // binary counter: leaf number cnt closes one subtree per trailing zero bit of cnt
      for (uint64_t q = cnt; (q & 1) == 0 && sp >= 1; q >>= 1) {
        uint32_t in[16];
        sp--;
#pragma unroll
        for (int k = 0; k < 8; k++) { in[k] = stk[sp][k]; in[8 + k] = got[k]; }
        blake2b256_tag64(got, 1, in);                       // node = H(01 || l || r)
      }
      if (sp < 32) {
#pragma unroll
        for (int k = 0; k < 8; k++) stk[sp][k] = got[k];
        sp++;
      } else {
        ok = false;
      }
      pos = ws;
      len = c.p - ws;
      is_lit = false;
    } else {
      lit = 0xff;
      st = 2;
    }
    while (len) {
      const uint32_t k = len < 8 ? (uint32_t)len : 8u;
      wg.put(is_lit ? lit : ld64u(arena, pos), k);
      pos += k;
      len -= k;
    }
  }
  if (!ok) {   // k_byron_split accepted these bytes: not reached on an unchanged arena
    result[i] = PRAOS_BLK_DECODE;
    which[i] = 0;
    return;
  }
  if (cnt != ((uint64_t)S(BS_NTX_LO) | ((uint64_t)S(BS_NTX_HI) << 32))) wh |= PRAOS_BYRON_W_NTX;
  wg.compress(true);
#pragma unroll
  for (int k = 0; k < 4; k++) { got[2 * k] = (uint32_t)wg.h[k]; got[2 * k + 1] = (uint32_t)(wg.h[k] >> 32); }
  ld_bytes32(want, arena, A(BS_WITH));
  if (differs()) wh |= PRAOS_BYRON_W_WIT;
  // fold the stack from the right; the empty tree is H("")
  if (sp == 0) {
    uint64_t z[16], hh[4];
#pragma unroll
    for (int k = 0; k < 16; k++) z[k] = 0;
    blake2b_1block(hh, z, 0, 32);
#pragma unroll
    for (int k = 0; k < 4; k++) { got[2 * k] = (uint32_t)hh[k]; got[2 * k + 1] = (uint32_t)(hh[k] >> 32); }
  } else {
    sp--;
#pragma unroll
    for (int k = 0; k < 8; k++) got[k] = stk[sp][k];
    while (sp) {
      uint32_t in[16];
      sp--;
#pragma unroll
      for (int k = 0; k < 8; k++) { in[k] = stk[sp][k]; in[8 + k] = got[k]; }
      blake2b256_tag64(got, 1, in);
    }
  }
  ld_bytes32(want, arena, A(BS_TXROOT));
  if (differs()) wh |= PRAOS_BYRON_W_ROOT;
  if (wh) bits |= PRAOS_BLK_BODY_HASH;
  result[i] = bits;
  which[i] = wh | (cnt == 1 ? PRAOS_BYRON_W_ONE_TX : 0);
}

}  // namespace

// ---- host launchers
void launch_byron_split(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len,
                        const uint64_t* blk_off, const uint32_t* blk_len, uint64_t epoch_slots, uint64_t* hoff,
                        uint32_t* hlen, uint64_t* slot, uint64_t* block_no, uint8_t* prev_hash, uint8_t* prev_genesis,
                        uint8_t* header_hash, uint8_t* split_status, uint16_t* dec_status, uint8_t* kind,
                        uint64_t* epoch_out, uint32_t* spans) {
  hipLaunchKernelGGL(k_byron_split, grid, block, 0, stream, n, arena, arena_len, blk_off, blk_len, epoch_slots, hoff,
                     hlen, slot, block_no, prev_hash, prev_genesis, header_hash, split_status, dec_status, kind, epoch_out, spans);
}

void launch_byron_integrity(dim3 grid, dim3 block, hipStream_t stream, size_t n, const uint8_t* arena,
                            const uint64_t* blk_off, const uint32_t* blk_len, const uint8_t* kind,
                            const uint32_t* spans, uint32_t cfg_pm, const ge_niels* gbtab, ge_cached* tabs,
                            uint8_t* result, uint8_t* which) {
  hipLaunchKernelGGL(k_byron_integrity, grid, block, 0, stream, n, arena, blk_off, blk_len, kind, spans, cfg_pm, gbtab,
                     tabs, result, which);
}
