// k_pbft.hip -- Byron header validation, the per-header half of validateHeader
// (HeaderValidation.hs:297-344 validateEnvelope's inputs, Protocol/PBFT.hs:320-353
// updateChainDepState's signature and delegate lookup; Byron/Ledger/PBFT.hs:43-69 validateView).
//
// Input: stored Byron headers as the secondary index slices them out of a block, and an is_ebb
// byte per header (the reference takes it from the block's two prefix bytes, the nested context
// of Byron/Ledger/Serialisation.hs).  Header shapes: k_byron.hip's.
//
//   k_pbft_decode  one lane per header: slot (epoch * epoch_slots + slotInEpoch, an EBB's
//                  epoch * epoch_slots), block number (difficulty), prev hash (GenesisHash for an
//                  EBB of epoch 0), header hash Blake2b-256(82 0k || header), PRAOS_PBFT_BIT_DECODE.
//                  For a main header also the verify inputs -- the delegate's Ed25519 key (the
//                  first 32 bytes of delegateXPub), the signature, and hram = SHA-512(R || A ||
//                  "01" || issuerXPub || 09 || CBOR(configured pm) || 85 || the stored prev, proof,
//                  slot-id, difficulty and extra items), streamed from the arena -- and hashVerKey
//                  of the delegate, Blake2b-224(SHA3-256(58 40 || delegateXPub)), binary searched
//                  in the caller's delegation table (sorted by delegate hash; gk_idx -1 and
//                  PRAOS_PBFT_BIT_NOT_DELEGATE when absent).  Main headers that decode are appended
//                  to the verify list; EBBs and undecodable headers skip the verify.
//   k_pbft_sig     uncached verify over a list: ed25519_verify_core with per-lane tables.
//   k_pbft_sig_ck  cached verify over the key cache's hit list (k_keys.hip, kind 0): a 4-window
//                  chain against the delegate key's tables and the radix-2^16 comb.
//   k_pbft_keyhash hashVerKey of n extended public keys.
// The Ed25519 rules are ed25519_verify_core's (S canonical, R and A not of small order, A
// canonical), the same as k_byron_integrity's: the block check and the header check agree.
// CPU restatement: tests/pbft_model.py.
#include "byron_dev.hpp"
#include "sha3.hpp"

namespace {

struct PbftDec {
  const uint8_t* __restrict__ arena;
  uint64_t arena_len;
  const uint64_t* __restrict__ hoff;
  const uint32_t* __restrict__ hlen;
  const uint8_t* __restrict__ is_ebb;
  uint64_t epoch_slots;
  uint32_t pm;
  const uint32_t* __restrict__ dtab;     // n_delegs x 8 words: delegate hash (7), caller index
  uint32_t n_delegs;
  uint64_t* __restrict__ slot;
  uint64_t* __restrict__ block_no;
  uint8_t* __restrict__ prev_hash;
  uint8_t* __restrict__ prev_genesis;
  uint8_t* __restrict__ header_hash;
  uint8_t* __restrict__ bits;
  int32_t* __restrict__ gk_idx;
  uint8_t* __restrict__ dhash;           // n x 28: the delegate's key hash
  uint8_t* __restrict__ keys;            // n x 32
  uint8_t* __restrict__ sig;             // n x 64
  uint8_t* __restrict__ hram;            // n x 64
  uint32_t* __restrict__ vlist;
  uint32_t* __restrict__ vcount;
};

// the inputs of the signature verifies (k_pbft_decode writes them)
struct PbftSig {
  const uint8_t* __restrict__ keys;      // n x 32: the delegate's Ed25519 key
  const uint8_t* __restrict__ sig;       // n x 64: R || S
  const uint8_t* __restrict__ hram;      // n x 64: SHA-512(R || A || message)
  uint8_t* __restrict__ bits;            // |= PRAOS_PBFT_BIT_SIG
  ge_cached* __restrict__ tabs;          // per-lane tables (LT_ED entries per item), uncached only
};

__device__ __forceinline__ void pbft_load(const PbftSig& a, size_t i, uint32_t pk[8], uint32_t sg[16],
                                          uint32_t hram[16]) {
  load_words(pk, a.keys + 32 * i, 8);
  load_words(sg, a.sig + 64 * i, 16);
  load_words(hram, a.hram + 64 * i, 16);
}

// hashVerKey: Blake2b-224(SHA3-256(58 40 || xpub)), 7 little-endian words
__device__ __forceinline__ void byron_key_hash(uint32_t out[7], const uint64_t key[8]) {
  uint64_t d[4];
  sha3_256_xpub(d, key);
  uint32_t in[8], h[8];
#pragma unroll
  for (int k = 0; k < 4; k++) { in[2 * k] = (uint32_t)d[k]; in[2 * k + 1] = (uint32_t)(d[k] >> 32); }
  blake2b_32(h, in, 28);
#pragma unroll
  for (int k = 0; k < 7; k++) out[k] = h[k];
}

// 28 bytes at a 4-byte aligned address
__device__ __forceinline__ void store_hash28(uint8_t* __restrict__ p, const uint32_t w[7]) {
  uint32_t* q = (uint32_t*)p;
#pragma unroll
  for (int k = 0; k < 7; k++) q[k] = w[k];
}

// the order of the delegation table: 7 little-endian words, word 0 first
__device__ __forceinline__ int hash_cmp(const uint32_t a[7], const uint32_t* __restrict__ b) {
  int r = 0;
#pragma unroll
  for (int k = 6; k >= 0; k--) r = a[k] < b[k] ? -1 : (a[k] > b[k] ? 1 : r);
  return r;
}

// one header; returns true when the lane takes the signature verify
__device__ bool pbft_decode_one(const PbftDec& a, size_t i) {
  const uint8_t* __restrict__ arena = a.arena;
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = 0;
  // the columns of a header that does not decode
  a.bits[i] = PRAOS_PBFT_BIT_DECODE;
  a.gk_idx[i] = -1;
  a.slot[i] = 0;
  a.block_no[i] = 0;
  a.prev_genesis[i] = 0;
  store_words(a.prev_hash + 32 * i, w, 8);
  store_words(a.header_hash + 32 * i, w, 8);
  store_hash28(a.dhash + 28 * i, w);
  const uint64_t ho = a.hoff[i];
  const uint32_t hl = a.hlen[i];
  if (!(ho >= 2 && ho <= a.arena_len && hl <= a.arena_len - ho)) return false;
  const uint64_t he = ho + hl;
  const bool ebb = a.is_ebb[i] != 0;
  Cur h{arena, ho, he, true};
  uint64_t pm = 0, prev_at = 0, epoch = 0, sie = 0, diff = 0, t;
  uint64_t prev_o, prev_l, proof_o = 0, proof_l = 0, sid_o = 0, sid_l = 0, diff_o = 0, diff_l = 0, extra_o = 0,
                           extra_l = 0, issuer_at = 0, deleg_at = 0, sig_at = 0;
  bool ok = rd_list(h, 5) && rd_uint(h, 0xffffffffu, pm);
  prev_o = h.p;
  ok = ok && rd_bytes(h, 32, prev_at);
  prev_l = h.p - prev_o;
  if (ebb) {
    ok = ok && rd_bytes(h, 32, t) && rd_list(h, 2) && rd_uint(h, ~0ull, epoch) && rd_list(h, 1) &&
         rd_uint(h, ~0ull, diff) && cbor_skip_regs(h) && h.p == he;
  } else {
    proof_o = h.p;
    ok = ok && rd_list(h, 4) && rd_list(h, 3) && rd_uint(h, ~0ull, t) && rd_bytes(h, 32, t) && rd_bytes(h, 32, t) &&
         cbor_skip_regs(h) && rd_bytes(h, 32, t) && rd_bytes(h, 32, t);
    proof_l = h.p - proof_o;
    ok = ok && rd_list(h, 4);
    sid_o = h.p;
    ok = ok && rd_list(h, 2) && rd_uint(h, ~0ull, epoch) && rd_uint(h, 0xffffu, sie);
    sid_l = h.p - sid_o;
    ok = ok && rd_bytes(h, 64, issuer_at);
    diff_o = h.p;
    ok = ok && rd_list(h, 1) && rd_uint(h, ~0ull, diff);
    diff_l = h.p - diff_o;
    ok = ok && rd_list(h, 2) && rd_uint(h, ~0ull, t) && t == 2 && rd_list(h, 2) && rd_list(h, 4) &&
         rd_uint(h, ~0ull, t) && rd_bytes(h, 64, t) && rd_bytes(h, 64, deleg_at) && rd_bytes(h, 64, t) &&
         rd_bytes(h, 64, sig_at);
    extra_o = h.p;
    ok = ok && cbor_skip_regs(h) && h.p == he;
    extra_l = h.p - extra_o;
  }
  if (!ok) return false;
  a.slot[i] = epoch * a.epoch_slots + sie;
  a.block_no[i] = diff;
  // an EBB of epoch 0 has GenesisHash (Block.hs:215-221): its 32 bytes are no block's hash
  const bool gen = ebb && epoch == 0;
  ld_bytes32(w, arena, prev_at);
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = gen ? 0u : w[k];
  store_words(a.prev_hash + 32 * i, w, 8);
  a.prev_genesis[i] = gen ? 1 : 0;
  b2b256_pre(w, arena, ho, hl, 2, 0x82u | (ebb ? 0u : 0x100u));
  store_words(a.header_hash + 32 * i, w, 8);
  if (ebb) {
    a.bits[i] = 0;
    return false;
  }
  // ---- the delegate: key column, key hash, delegation table
  uint64_t dk[8];
#pragma unroll
  for (int k = 0; k < 8; k++) dk[k] = ld64u(arena, deleg_at + 8 * k);
#pragma unroll
  for (int k = 0; k < 4; k++) { w[2 * k] = (uint32_t)dk[k]; w[2 * k + 1] = (uint32_t)(dk[k] >> 32); }
  store_words(a.keys + 32 * i, w, 8);
  uint32_t kh[7];
  byron_key_hash(kh, dk);
  store_hash28(a.dhash + 28 * i, kh);
  int32_t gk = -1;
  {
    uint32_t lo = 0, hi = a.n_delegs;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      const int c = hash_cmp(kh, a.dtab + 8 * (size_t)mid);
      if (c == 0) { gk = (int32_t)a.dtab[8 * (size_t)mid + 7]; break; }
      if (c < 0) hi = mid; else lo = mid + 1;
    }
  }
  a.gk_idx[i] = gk;
  a.bits[i] = gk < 0 ? PRAOS_PBFT_BIT_NOT_DELEGATE : 0;
  // ---- the signature's inputs: R || S, and hram over the streamed message
  uint32_t sg[16];
  ld_bytes32(sg, arena, sig_at);
  ld_bytes32(sg + 8, arena, sig_at + 32);
  store_words(a.sig + 64 * i, sg, 16);
  uint32_t el;
  const uint64_t mid = sign_tag_mid(a.pm, el);
  Hs<true> s;
  s.init();
#pragma nounroll
  for (uint32_t p = 0; p < 10; p++) {
    uint64_t pos = 0, len = 0, lit = 0;
    switch (p) {
      case 0: pos = sig_at; len = 32; break;
      case 1: pos = deleg_at; len = 32; break;
      case 2: lit = 0x3130; len = 2; break;                       // "01"
      case 3: pos = issuer_at; len = 64; break;
      case 4: lit = mid; len = el; break;
      case 5: pos = prev_o; len = prev_l; break;
      case 6: pos = proof_o; len = proof_l; break;
      case 7: pos = sid_o; len = sid_l; break;
      case 8: pos = diff_o; len = diff_l; break;
      default: pos = extra_o; len = extra_l; break;
    }
    const bool is_lit = p == 2 || p == 4;
    while (len) {
      const uint32_t k = len < 8 ? (uint32_t)len : 8u;
      s.put(is_lit ? lit : ld64u(arena, pos), k);
      pos += k;
      len -= k;
    }
  }
  uint32_t hr[16];
  s.sha512_finish(hr);
  store_words(a.hram + 64 * i, hr, 16);
  return true;
}

__global__ void __launch_bounds__(NT) k_pbft_decode(size_t n, PbftDec a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool verify = i < n && pbft_decode_one(a, i);     // every lane stays for the ballot
  const uint64_t m = __ballot(verify);
  if (m == 0) return;
  const int leader = __ffsll((unsigned long long)m) - 1;
  const uint32_t lane = __lane_id();
  uint32_t base = 0;
  if ((int)lane == leader) base = atomicAdd(a.vcount, (uint32_t)__popcll(m));
  base = __shfl(base, leader);
  if (verify) a.vlist[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)i;
}

__global__ void __launch_bounds__(NT, LB_ED) k_pbft_sig(const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ count,
                                                        const ge_niels* __restrict__ gbtab, PbftSig a) {
  const size_t items = (size_t)*count;
  if ((size_t)blockIdx.x * NT >= items) return;                // whole block idle
  __shared__ ge_niels sbtab[BTAB_N];
  const ge_niels* btab = stage_btab<1>(gbtab, sbtab);
  const size_t t = (size_t)blockIdx.x * NT + threadIdx.x;
  if (t >= items) return;
  const size_t i = list[t];
  uint32_t pk[8], sg[16], hram[16];
  pbft_load(a, i, pk, sg, hram);
  if (!ed25519_verify_core(pk, sg, sg + 8, hram, btab, lane_tab(a.tabs, i, LT_ED))) a.bits[i] |= PRAOS_PBFT_BIT_SIG;
}

__global__ void __launch_bounds__(NT, LB_ED) k_pbft_sig_ck(const uint32_t* __restrict__ list,
                                                           const uint32_t* __restrict__ count,
                                                           const int32_t* __restrict__ item_entry,
                                                           const ge_cached* __restrict__ ktab,
                                                           const uint32_t* __restrict__ kinfo,
                                                           const ge_niels* __restrict__ gbtab, PbftSig a) {
  const size_t items = *count;
  if ((size_t)blockIdx.x * blockDim.x >= items) return;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= items) return;
  const size_t i = list[t];
  const size_t e = (size_t)item_entry[i];
  uint32_t pk[8], sg[16], hram[16];
  pbft_load(a, i, pk, sg, hram);
  if (!ed25519_verify_cached(sg, sg + 8, hram, kinfo[9 * e], ktab + e * KT_STRIDE, gbtab))   // the comb, read in place
    a.bits[i] |= PRAOS_PBFT_BIT_SIG;
}

__global__ void __launch_bounds__(NT) k_pbft_keyhash(size_t n, const uint8_t* __restrict__ keys64,
                                                     uint8_t* __restrict__ out28) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t dk[8];
  const uint64_t* src = (const uint64_t*)(keys64 + 64 * i);
#pragma unroll
  for (int k = 0; k < 8; k++) dk[k] = src[k];
  uint32_t w[7];
  byron_key_hash(w, dk);
  store_hash28(out28 + 28 * i, w);
}

}  // namespace

// ---- host launchers
void launch_pbft_decode(hipStream_t stream, size_t n, const uint8_t* arena, uint64_t arena_len, const uint64_t* hoff,
                        const uint32_t* hlen, const uint8_t* is_ebb, uint64_t epoch_slots, uint32_t pm,
                        const uint32_t* dtab, uint32_t n_delegs, uint64_t* slot, uint64_t* block_no,
                        uint8_t* prev_hash, uint8_t* prev_genesis, uint8_t* header_hash, uint8_t* bits, int32_t* gk_idx,
                        uint8_t* dhash, uint8_t* keys, uint8_t* sig, uint8_t* hram, uint32_t* vlist, uint32_t* vcount) {
  PbftDec a{arena, arena_len, hoff, hlen, is_ebb, epoch_slots, pm, dtab, n_delegs, slot, block_no, prev_hash,
            prev_genesis, header_hash, bits, gk_idx, dhash, keys, sig, hram, vlist, vcount};
  hipLaunchKernelGGL(k_pbft_decode, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, a);
}
void launch_pbft_sig(hipStream_t stream, size_t n, KeyItems items, const ge_niels* gbtab, const uint8_t* keys,
                     const uint8_t* sig, const uint8_t* hram, uint8_t* bits, ge_cached* tabs) {
  PbftSig a{keys, sig, hram, bits, tabs};
  hipLaunchKernelGGL(k_pbft_sig, launch_grid(n), dim3(NT), 0, stream, items.list, items.count, gbtab, a);
}
void launch_pbft_sig_ck(hipStream_t stream, size_t n, const KeyHits& h, const ge_niels* comb, const uint8_t* keys,
                        const uint8_t* sig, const uint8_t* hram, uint8_t* bits) {
  PbftSig a{keys, sig, hram, bits, nullptr};
  hipLaunchKernelGGL(k_pbft_sig_ck, launch_grid(n), dim3(NT), 0, stream, h.list, h.count, h.item_entry, h.ktab,
                     h.kinfo, comb, a);
}
void launch_pbft_keyhash(hipStream_t stream, size_t n, const uint8_t* keys64, uint8_t* out28) {
  hipLaunchKernelGGL(k_pbft_keyhash, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, stream, n, keys64, out28);
}
