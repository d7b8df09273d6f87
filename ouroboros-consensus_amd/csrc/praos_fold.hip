// praos_fold.hip -- the sequential part of Praos / TPraos updateChainDepState on the host (verdict
// order, envelope, OCert counters, nonces) and the PraosState CBOR codec.  Pure host code: no HIP
// call on any of its paths.
#include "api_internal.hpp"

// ---------------------------------------------------------------- sequential part (host)
// First-error-wins order of Praos.updateChainDepState (Praos.hs:441-459):
// validateKESSignature (:567 c0<=kp, :568 kp<c0+maxKESEvo, :580 OCert, :582 KES,
// :584-590 counter), then validateVRFSignature (:537 unknown, :539 vrf key,
// :543 proof, :549 leader).  Counter source (:601-606): the counter map, else
// 0 if the issuer is in the pool distribution, else missing.

// First failing check of one header in the reference order (Praos.hs:449-455 with
// validateKESSignature :558-606 and validateVRFSignature :528-556).  has_counter / m
// = the counter-map lookup of :601-606 (PoolDistr membership counts as m = 0).
static uint8_t header_verdict(uint16_t b, bool have, uint64_t m, uint64_t n) {
  if (b & PRAOS_BIT_INPUT) return PRAOS_V_INPUT;
  if (b & PRAOS_BIT_KES_BEFORE_START) return PRAOS_V_KES_BEFORE_START;
  if (b & PRAOS_BIT_KES_AFTER_END) return PRAOS_V_KES_AFTER_END;
  if (b & PRAOS_BIT_OCERT_SIG) return PRAOS_V_OCERT_SIG;
  if (b & (PRAOS_BIT_KES_MERKLE | PRAOS_BIT_KES_LEAF)) return PRAOS_V_KES_SIG;
  if (!have) return PRAOS_V_COUNTER_MISSING;
  if (!(m <= n)) return PRAOS_V_COUNTER_TOO_SMALL;
  if (!(n <= m + 1)) return PRAOS_V_COUNTER_OVER_INC;
  if (b & PRAOS_BIT_VRF_KEY_UNKNOWN) return PRAOS_V_VRF_KEY_UNKNOWN;
  if (b & PRAOS_BIT_VRF_KEY_WRONG) return PRAOS_V_VRF_KEY_WRONG;
  if (b & (PRAOS_BIT_VRF_PROOF | PRAOS_BIT_VRF_OUTPUT)) return PRAOS_V_VRF_BAD_PROOF;
  if (b & PRAOS_BIT_LEADER) return PRAOS_V_LEADER_TOO_BIG;
  return PRAOS_V_OK;
}

// TPraos predicate failures of one header (PRAOS_TPF_*), as PRTCL collects them
// (small-steps ValidateAll: every `?!` of OVERLAY and OCERT is recorded):
//   OVERLAY (cardano-protocol-tpraos Rules/Overlay.hs): NotActiveSlotOVERLAY; or, in an
//     active overlay slot, WrongGenesisColdKeyOVERLAY (?!) and pbftVrfChecks (an Either:
//     its first failure -- WrongGenesisVRFKey, BadNonce, BadLeaderValue); or, outside the
//     overlay, praosVrfChecks (an Either: VRFKeyUnknown, VRFKeyWrongVRFKey, BadNonce,
//     BadLeaderValue, VRFLeaderValueTooBig -- first failure);
//   OCERT (Rules/OCert.hs): KESBeforeStart, KESAfterEnd, InvalidSignature, InvalidKesSignature,
//     then the counter (currentIssueNo: Nothing -> NoCounterForKeyHash; else CounterTooSmall,
//     CounterOverIncremented).
static uint16_t tpraos_failures(uint16_t b, bool have, uint64_t m, uint64_t n) {
  uint16_t f = 0;
  if (b & PRAOS_BIT_TP_NOT_ACTIVE) {
    f |= PRAOS_TPF_NOT_ACTIVE;
  } else if (b & PRAOS_BIT_TP_OVERLAY) {
    if (b & PRAOS_BIT_TP_GEN_COLD) f |= PRAOS_TPF_GEN_COLD;
    if (b & PRAOS_BIT_TP_GEN_VRF) f |= PRAOS_TPF_GEN_VRF;
    else if (b & PRAOS_BIT_TP_VRF_NONCE) f |= PRAOS_TPF_BAD_NONCE;
    else if (b & PRAOS_BIT_TP_VRF_LEADER) f |= PRAOS_TPF_BAD_LEADER;
  } else {
    if (b & PRAOS_BIT_VRF_KEY_UNKNOWN) f |= PRAOS_TPF_VRF_KEY_UNKNOWN;
    else if (b & PRAOS_BIT_VRF_KEY_WRONG) f |= PRAOS_TPF_VRF_KEY_WRONG;
    else if (b & PRAOS_BIT_TP_VRF_NONCE) f |= PRAOS_TPF_BAD_NONCE;
    else if (b & PRAOS_BIT_TP_VRF_LEADER) f |= PRAOS_TPF_BAD_LEADER;
    else if (b & PRAOS_BIT_LEADER) f |= PRAOS_TPF_LEADER_TOO_BIG;
  }
  if (b & PRAOS_BIT_KES_BEFORE_START) f |= PRAOS_TPF_KES_BEFORE_START;
  if (b & PRAOS_BIT_KES_AFTER_END) f |= PRAOS_TPF_KES_AFTER_END;
  if (b & PRAOS_BIT_OCERT_SIG) f |= PRAOS_TPF_OCERT_SIG;
  if (b & (PRAOS_BIT_KES_MERKLE | PRAOS_BIT_KES_LEAF)) f |= PRAOS_TPF_KES_SIG;
  if (!have) {
    f |= PRAOS_TPF_COUNTER_MISSING;
  } else {
    if (!(m <= n)) f |= PRAOS_TPF_COUNTER_TOO_SMALL;
    if (!(n <= m + 1)) f |= PRAOS_TPF_COUNTER_OVER_INC;
  }
  return f;
}

static std::string issuer_hash(const praos_ctx* c, const praos_headers* h, const praos_out* crypto, size_t i) {
  const int32_t pidx = crypto->pool_idx ? crypto->pool_idx[i] : -1;
  if (pidx >= 0 && (size_t)pidx < c->pools.size()) return std::string((const char*)c->pools[pidx].hash28, 28);
  uint8_t hh[28];
  praos_host::blake2b(hh, 28, h->cold_vk + 32 * i, 32);
  return std::string((const char*)hh, 28);
}

using praos_host::nonce_combine;
using praos_host::nonce_eq;

extern "C" {

int praos_apply_batch(praos_ctx* c, const praos_headers* h, const praos_out* crypto, praos_counters* counters,
                      uint8_t* verdict, size_t* chain_stop) {
  if (!c || !h || !crypto || !crypto->bits || !verdict) return PRAOS_E_ARG;
  if (!c->have_epoch) return PRAOS_E_STATE;
  std::map<std::string, uint64_t> cmap;
  if (counters)
    for (size_t k = 0; k < counters->m; k++)
      cmap[std::string((const char*)counters->hash28 + 28 * k, 28)] = counters->counter[k];
  size_t stop = h->n;
  for (size_t i = 0; i < h->n; i++) {
    const std::string hk = issuer_hash(c, h, crypto, i);
    const uint64_t n = h->ocert_n[i];
    auto it = cmap.find(hk);
    const bool have = it != cmap.end() || c->pool_by_hash.count(hk);
    const uint8_t v = header_verdict(crypto->bits[i], have, it != cmap.end() ? it->second : 0, n);
    verdict[i] = v;
    if (v == PRAOS_V_OK) cmap[hk] = n;               // reupdateChainDepState, Praos.hs:484-485
    else if (stop == h->n) stop = i;
  }
  if (chain_stop) *chain_stop = stop;
  if (counters)
    for (size_t k = 0; k < counters->m; k++)
      counters->counter[k] = cmap[std::string((const char*)counters->hash28 + 28 * k, 28)];
  return PRAOS_OK;
}

}  // extern "C"

// validateEnvelope (HeaderValidation.hs:297-344) with the Praos additionalEnvelopeChecks
// (envelopeChecks, Shelley/Protocol/Praos.hs:66-80), against the tip the chain has
// reached (AnnTip: slot, block number, header hash).  First failure in that order.
struct EnvTip {
  int32_t origin;
  uint64_t slot, block_no;
  uint8_t hash[32];
};
static uint8_t envelope_verdict(const praos_envelope* e, const EnvTip& tip, const praos_headers* h,
                                const uint8_t* prev_hash, const uint8_t* prev_is_genesis, size_t i) {
  const uint64_t expected_block = tip.origin ? 0 : tip.block_no + 1;     // expectedFirstBlockNo / succ
  if (e->block_no[i] != expected_block) return PRAOS_V_ENV_BLOCK_NO;
  const uint64_t min_slot = tip.origin ? 0 : tip.slot + 1;                // minimumPossibleSlotNo / succ
  if (!(h->slot[i] >= min_slot)) return PRAOS_V_ENV_SLOT_NO;
  const bool genesis = prev_is_genesis && prev_is_genesis[i];
  const bool prev_ok = tip.origin ? genesis : (!genesis && std::memcmp(prev_hash + 32 * i, tip.hash, 32) == 0);
  if (!prev_ok) return PRAOS_V_ENV_PREV_HASH;                             // checkPrevHash'
  if (!(e->lv_prot_major <= e->max_major_pv)) return PRAOS_V_ENV_OBSOLETE_NODE;
  if (!((uint64_t)e->header_size[i] <= e->max_header_size)) return PRAOS_V_ENV_HEADER_SIZE;
  if (!((uint64_t)e->body_size[i] <= e->max_body_size)) return PRAOS_V_ENV_BLOCK_SIZE;
  return PRAOS_V_OK;
}

// OCert counters of the fold, indexed densely: slot k < npools is pool k of the epoch's
// distribution (caller order, found through the device's pool_idx), slots >= npools
// hold issuers outside it (keys from the incoming state, or headers whose issuer the
// distribution lacks).  has[k] = the praosStateOCertCounters map has the key.
struct CounterTab {
  std::vector<uint64_t> ctr;
  std::vector<uint8_t> has;
  std::vector<std::string> extra_keys;
  std::map<std::string, uint32_t> extra;
};

static uint32_t counter_slot(const std::map<std::string, int32_t>& by_hash, CounterTab& T, const uint8_t* hash28) {
  const std::string k((const char*)hash28, 28);
  auto p = by_hash.find(k);
  if (p != by_hash.end()) return (uint32_t)p->second;
  auto e = T.extra.find(k);
  if (e != T.extra.end()) return e->second;
  const uint32_t slot = (uint32_t)T.ctr.size();
  T.extra.emplace(k, slot);
  T.extra_keys.push_back(k);
  T.ctr.push_back(0);
  T.has.push_back(0);
  return slot;
}

static int fold_impl(praos_ctx* c, const praos_headers* h, const uint8_t* prev_hash, const uint8_t* prev_is_genesis,
                     const praos_out* crypto, praos_envelope* env, const praos_epoch_info* ei,
                     praos_chain_state* st, uint8_t* verdict, size_t* chain_stop, size_t* processed,
                     const praos_nonce* etas = nullptr, uint32_t netas = 0, const uint8_t* eta_idx = nullptr,
                     bool tpraos = false, const praos_nonce* extra_entropy = nullptr, uint16_t* failures = nullptr,
                     const praos_nonce* evol_after = nullptr, const rp_view* view = nullptr,
                     const uint32_t* map = nullptr, bool client = false, std::string* err_out = nullptr) {
  // map (praos_validate_candidates): item i of the fold reads row map[i] of every per-header input
  // (h, prev_hash, crypto, env's arrays, eta_idx) and writes verdict[i] / failures[i] / reads
  // evol_after[i]; PRAOS_NO_ROW = an item without a header (PRAOS_V_INPUT).  NULL: row i.  client:
  // the ChainSync client's fold -- DoesntFit before validateHeader, and the fold ends at the first
  // failure.  err_out: the error text goes there instead of the context (concurrent folds).
  if (!c) return PRAOS_E_ARG;
  auto fail = [&](const char* m, int rc) {
    if (err_out) *err_out = m;
    else c->err = m;
    return rc;
  };
  if (!h || !crypto || !crypto->bits || !crypto->nonce || !verdict || !ei || !st || !prev_hash)
    return fail("fold: a required pointer is NULL (headers, crypto bits / nonce, verdict, epoch info, state, prev_hash)",
                PRAOS_E_ARG);
  if (ei->epoch_length == 0 || st->m > st->cap || (st->cap && (!st->counter_hash28 || !st->counter)))
    return fail("fold: epoch_length 0 or a counter map without room", PRAOS_E_ARG);
  if (env && h->n && (!env->block_no || !env->header_hash || !env->header_size || !env->body_size))
    return fail("fold: the envelope needs block_no, header_hash, header_size and body_size", PRAOS_E_ARG);
  if (!c->have_epoch) return fail("fold: no epoch installed (praos_set_epoch)", PRAOS_E_STATE);
  if (eta_idx && (!etas || netas == 0)) return fail("fold: eta_idx without etas", PRAOS_E_ARG);
  praos_nonce eta0{};
  eta0.neutral = c->eta0_neutral;
  if (!c->eta0_neutral) std::memcpy(eta0.hash, c->eta0, 32);
  auto epoch_of = [&](uint64_t s, bool* ok) -> uint64_t {
    *ok = s >= ei->epoch_base_slot;
    return ei->epoch_base_no + (*ok ? (s - ei->epoch_base_slot) / ei->epoch_length : 0);
  };
  // Working state W (the fold) and the returned state: the reference stops the
  // chain at the first invalid header, so *st is the state after the last valid
  // header before chain_stop.  Later headers keep being judged (would-be
  // verdicts) against W, which carries on as if the failing header were absent.
  struct Work {
    int32_t origin;
    uint64_t last_slot;
    praos_nonce evolving, candidate, epoch_nonce, lab, leb;
    EnvTip tip;
  };
  // the ledger view's pools: the batch's own (per-epoch replay) or the context's praos_set_epoch
  const uint32_t np = view ? view->npools : (uint32_t)c->pools.size();
  const praos_pool* vpools = view ? view->pools.data() : c->pools.data();
  const std::map<std::string, int32_t>& by_hash = view ? view->by_hash : c->pool_by_hash;
  CounterTab T;
  T.ctr.assign(np, 0);
  T.has.assign(np, 0);
  for (size_t k = 0; k < st->m; k++) {
    const uint32_t slot = counter_slot(by_hash, T, st->counter_hash28 + 28 * k);
    T.ctr[slot] = st->counter[k];
    T.has[slot] = 1;
  }
  Work W;
  if (env) {
    W.tip.origin = env->tip_is_origin;
    W.tip.slot = env->tip_slot;
    W.tip.block_no = env->tip_block_no;
    std::memcpy(W.tip.hash, env->tip_hash, 32);
  }
  W.origin = st->last_slot_origin;
  W.last_slot = st->last_slot;
  W.evolving = st->evolving; W.candidate = st->candidate; W.epoch_nonce = st->epoch_nonce;
  W.lab = st->lab; W.leb = st->last_epoch_block;
  bool frozen = false;
  Work F;                                            // state at the chain stop
  std::vector<uint64_t> Fctr;                        // and its counters (T is W's)
  std::vector<uint8_t> Fhas;
  size_t stop = h->n, i = 0;
  auto freeze = [&] {
    if (frozen) return;
    F = W;
    Fctr = T.ctr;
    Fhas = T.has;
    frozen = true;
    stop = i;
  };
  for (; i < h->n; i++) {
    const size_t r = map ? map[i] : i;
    if (map && (map[i] == PRAOS_NO_ROW || (crypto->bits[r] & PRAOS_BIT_INPUT))) {
      // no header to read (it did not unwrap or decode): the chain ends here
      verdict[i] = PRAOS_V_INPUT;
      if (failures) failures[i] = 0;
      freeze();
      if (client) { i++; break; }
      continue;
    }
    const uint64_t slot = h->slot[r];
    bool ok = true;
    const uint64_t e_new = epoch_of(slot, &ok);
    if (!ok) return fail("slot before the epoch base", PRAOS_E_ARG);
    // tickChainDepState (Praos.hs:407-431) with isNewEpoch (Ledger/Util.hs:27-40)
    const uint64_t e_old = W.origin ? 0 : epoch_of(W.last_slot, &ok);
    praos_nonce tick_epoch = W.epoch_nonce, tick_leb = W.leb;
    if (e_new > e_old) {
      tick_epoch = nonce_combine(W.candidate, W.leb);
      if (tpraos && extra_entropy) tick_epoch = nonce_combine(tick_epoch, *extra_entropy);   // TICKN
      tick_leb = W.lab;
    }
    // the crypto outputs of header i were computed for this nonce: a tick to another one
    // ends the fold (the caller re-verifies from here under the right nonce)
    if (eta_idx && eta_idx[r] >= netas) return fail("eta_idx out of range", PRAOS_E_ARG);
    if (!nonce_eq(tick_epoch, eta_idx ? etas[eta_idx[r]] : eta0)) break;
    // the issuer's counter slot (hashKey of the cold key, Praos.hs:595-606)
    const int32_t pidx = crypto->pool_idx ? crypto->pool_idx[r] : -1;
    uint32_t k;
    if (pidx >= 0 && (uint32_t)pidx < np) {
      k = (uint32_t)pidx;
    } else {
      uint8_t hh[28];
      praos_host::blake2b(hh, 28, h->cold_vk + 32 * r, 32);
      k = counter_slot(by_hash, T, hh);
    }
    const uint64_t n = h->ocert_n[r];
    const bool has = T.has[k];
    uint8_t v;
    if (tpraos) {
      // currentIssueNo: the counter map, else 0 for a pool or a genesis delegate
      const bool known = has || k < np || c->gen_delegate_hashes.count(T.extra_keys[k - np]) > 0;
      const uint16_t f = (crypto->bits[r] & PRAOS_BIT_INPUT) ? 0 : tpraos_failures(crypto->bits[r], known,
                                                                                    has ? T.ctr[k] : 0, n);
      if (failures) failures[i] = f;
      v = (crypto->bits[r] & PRAOS_BIT_INPUT) ? PRAOS_V_INPUT : (f ? PRAOS_V_TPRAOS : PRAOS_V_OK);
    } else {
      v = header_verdict(crypto->bits[r], has || k < np, has ? T.ctr[k] : 0, n);
    }
    // validateHeader (HeaderValidation.hs:419-428): the envelope before the protocol checks
    if (env && v != PRAOS_V_INPUT) {
      const uint8_t ve = envelope_verdict(env, W.tip, h, prev_hash, prev_is_genesis, r);
      if (ve != PRAOS_V_OK) {
        v = ve;
        if (failures) failures[i] = 0;               // validateEnvelope failed: PRTCL does not run
      }
    }
    if (client && env && v != PRAOS_V_INPUT) {
      // Client.hs:794-810: the header must fit onto the candidate's head before validateHeader
      const bool genesis = prev_is_genesis && prev_is_genesis[r];
      const bool fits = W.tip.origin ? genesis : (!genesis && std::memcmp(prev_hash + 32 * r, W.tip.hash, 32) == 0);
      if (!fits) v = PRAOS_V_DOESNT_FIT;
    }
    verdict[i] = v;
    if (v != PRAOS_V_OK) {
      freeze();
      if (client) { i++; break; }
      continue;
    }
    // reupdateChainDepState (Praos.hs:468-502)
    W.epoch_nonce = tick_epoch;
    W.leb = tick_leb;
    W.origin = 0;
    W.last_slot = slot;
    W.lab.neutral = prev_is_genesis && prev_is_genesis[r];
    std::memset(W.lab.hash, 0, 32);
    if (!W.lab.neutral) std::memcpy(W.lab.hash, prev_hash + 32 * r, 32);
    praos_nonce eta{};
    std::memcpy(eta.hash, crypto->nonce + 32 * r, 32);
    eta.neutral = 0;
    // evol_after (the replay's nonce chain, run ahead as if every header were valid) equals
    // this chain up to the first invalid header; from there W skips the failed headers
    W.evolving = (evol_after && !frozen) ? evol_after[i] : nonce_combine(W.evolving, eta);
    const uint64_t first_next = ei->epoch_base_slot + (e_new - ei->epoch_base_no + 1) * ei->epoch_length;
    if (slot + ei->stability_window < first_next) W.candidate = W.evolving;
    T.ctr[k] = n;
    T.has[k] = 1;
    if (env) {                                       // HeaderState tip := getAnnTip hdr
      W.tip.origin = 0;
      W.tip.slot = slot;
      W.tip.block_no = env->block_no[r];
      std::memcpy(W.tip.hash, env->header_hash + 32 * r, 32);
    }
  }
  const Work& R = frozen ? F : W;
  const std::vector<uint64_t>& Rctr = frozen ? Fctr : T.ctr;
  const std::vector<uint8_t>& Rhas = frozen ? Fhas : T.has;
  size_t m = 0;
  for (size_t k = 0; k < Rhas.size(); k++) m += Rhas[k];
  if (m > st->cap) return fail("counter map capacity exceeded", PRAOS_E_ARG);
  size_t j = 0;
  for (size_t k = 0; k < Rhas.size(); k++) {
    if (!Rhas[k]) continue;
    const uint8_t* key = k < np ? vpools[k].hash28 : (const uint8_t*)T.extra_keys[k - np].data();
    std::memcpy(st->counter_hash28 + 28 * j, key, 28);
    st->counter[j++] = Rctr[k];
  }
  st->m = m;
  st->last_slot_origin = R.origin;
  st->last_slot = R.last_slot;
  st->evolving = R.evolving; st->candidate = R.candidate; st->epoch_nonce = R.epoch_nonce;
  st->lab = R.lab; st->last_epoch_block = R.leb;
  if (env) {
    env->tip_is_origin = R.tip.origin;
    env->tip_slot = R.tip.slot;
    env->tip_block_no = R.tip.block_no;
    std::memcpy(env->tip_hash, R.tip.hash, 32);
  }
  if (chain_stop) *chain_stop = std::min(stop, i);
  if (processed) *processed = i;
  return PRAOS_OK;
}

int rp_fold(praos_ctx* c, const praos_headers* h, const uint8_t* prev_hash, const uint8_t* prev_is_genesis,
            const praos_out* crypto, praos_envelope* env, const praos_epoch_info* ei, praos_chain_state* st,
            const praos_nonce* etas, uint32_t k, const uint8_t* eta_idx, const praos_nonce* evolving_after,
            bool tpraos, const praos_nonce* extra_entropy, uint8_t* verdict, uint16_t* failures, size_t* chain_stop,
            size_t* processed, const rp_view* view, const uint32_t* map, bool client, std::string* err_out) {
  if (!etas || !eta_idx || k == 0) return PRAOS_E_ARG;
  return fold_impl(c, h, prev_hash, prev_is_genesis, crypto, env, ei, st, verdict, chain_stop, processed, etas, k,
                   eta_idx, tpraos, extra_entropy, failures, evolving_after, view, map, client, err_out);
}

extern "C" {

int praos_update_chain_dep_state(praos_ctx* c, const praos_headers* h, const uint8_t* prev_hash,
                                 const uint8_t* prev_is_genesis, const praos_out* crypto,
                                 const praos_epoch_info* ei, praos_chain_state* st, uint8_t* verdict,
                                 size_t* chain_stop, size_t* processed) {
  return fold_impl(c, h, prev_hash, prev_is_genesis, crypto, nullptr, ei, st, verdict, chain_stop, processed);
}

int praos_ticked_epoch_nonce(const praos_chain_state* st, const praos_epoch_info* ei, uint64_t slot,
                             praos_nonce* out) {
  if (!st || !ei || !out || ei->epoch_length == 0 || slot < ei->epoch_base_slot) return PRAOS_E_ARG;
  auto epoch_of = [&](uint64_t s) {
    return ei->epoch_base_no + (s < ei->epoch_base_slot ? 0 : (s - ei->epoch_base_slot) / ei->epoch_length);
  };
  const uint64_t e_old = st->last_slot_origin ? 0 : epoch_of(st->last_slot);
  *out = epoch_of(slot) > e_old ? nonce_combine(st->candidate, st->last_epoch_block) : st->epoch_nonce;
  return PRAOS_OK;
}

int praos_tpraos_ticked_epoch_nonce(const praos_chain_state* st, const praos_epoch_info* ei, uint64_t slot,
                                    const praos_nonce* extra_entropy, praos_nonce* out) {
  if (!st || !ei || !out || ei->epoch_length == 0 || slot < ei->epoch_base_slot) return PRAOS_E_ARG;
  auto epoch_of = [&](uint64_t s) {
    return ei->epoch_base_no + (s < ei->epoch_base_slot ? 0 : (s - ei->epoch_base_slot) / ei->epoch_length);
  };
  const uint64_t e_old = st->last_slot_origin ? 0 : epoch_of(st->last_slot);
  if (epoch_of(slot) > e_old) {        // TICKN: eta_c ⭒ eta_h ⭒ extraEntropy
    *out = nonce_combine(st->candidate, st->last_epoch_block);
    if (extra_entropy) *out = nonce_combine(*out, *extra_entropy);
  } else {
    *out = st->epoch_nonce;
  }
  return PRAOS_OK;
}

int praos_validate_headers(praos_ctx* c, const praos_headers* h, const uint8_t* prev_hash,
                           const uint8_t* prev_is_genesis, const praos_out* crypto, praos_envelope* env,
                           const praos_epoch_info* ei, praos_chain_state* st, uint8_t* verdict, size_t* chain_stop,
                           size_t* processed) {
  if (!env) return PRAOS_E_ARG;
  return fold_impl(c, h, prev_hash, prev_is_genesis, crypto, env, ei, st, verdict, chain_stop, processed);
}

int praos_validate_headers_nonces(praos_ctx* c, const praos_headers* h, const uint8_t* prev_hash,
                                  const uint8_t* prev_is_genesis, const praos_out* crypto, praos_envelope* env,
                                  const praos_epoch_info* ei, praos_chain_state* st, const praos_nonce* etas,
                                  uint32_t k, const uint8_t* eta_idx, uint8_t* verdict, size_t* chain_stop,
                                  size_t* processed) {
  if (!eta_idx || !etas || k == 0) return PRAOS_E_ARG;
  return fold_impl(c, h, prev_hash, prev_is_genesis, crypto, env, ei, st, verdict, chain_stop, processed, etas, k,
                   eta_idx);
}

int praos_tpraos_update_chain_dep_state(praos_ctx* c, const praos_tpraos_headers* th, const uint8_t* prev_hash,
                                        const uint8_t* prev_is_genesis, const praos_tpraos_out* crypto,
                                        praos_envelope* env, const praos_epoch_info* ei,
                                        const praos_nonce* extra_entropy, praos_chain_state* st, uint8_t* verdict,
                                        uint16_t* failures, size_t* chain_stop, size_t* processed) {
  if (!th || !crypto) return PRAOS_E_ARG;
  praos_out o{};
  o.bits = crypto->bits;
  o.pool_idx = crypto->pool_idx;
  o.nonce = crypto->nonce;                           // mkNonceFromOutputVRF of the eta certificate
  return fold_impl(c, &th->h, prev_hash, prev_is_genesis, &o, env, ei, st, verdict, chain_stop, processed, nullptr, 0,
                   nullptr, true, extra_entropy, failures);
}

int praos_tpraos_validate_headers_nonces(praos_ctx* c, const praos_tpraos_headers* th, const uint8_t* prev_hash,
                                         const uint8_t* prev_is_genesis, const praos_tpraos_out* crypto,
                                         praos_envelope* env, const praos_epoch_info* ei,
                                         const praos_nonce* extra_entropy, praos_chain_state* st,
                                         const praos_nonce* etas, uint32_t k, const uint8_t* eta_idx,
                                         uint8_t* verdict, uint16_t* failures, size_t* chain_stop,
                                         size_t* processed) {
  if (!th || !crypto || !etas || !eta_idx || k == 0) return PRAOS_E_ARG;
  praos_out o{};
  o.bits = crypto->bits;
  o.pool_idx = crypto->pool_idx;
  o.nonce = crypto->nonce;
  return fold_impl(c, &th->h, prev_hash, prev_is_genesis, &o, env, ei, st, verdict, chain_stop, processed, etas, k,
                   eta_idx, true, extra_entropy, failures);
}

}  // extern "C"

// ---------------------------------------------------------------- PraosState CBOR
// Serialise (PraosState c) (Praos.hs:274-310): encodeVersion 0 [lastSlot, counters,
// evolving, candidate, epoch, lab, lastEpochBlock]; WithOrigin: Origin = [0], At s =
// [1, s]; Nonce: NeutralNonce = [0], Nonce h = [1, bytes(32)]; counters = CBOR map
// KeyHash (bytes 28) -> Word64 in ascending key order (Data.Map).  Shortest-form heads.
namespace {
struct CborW {
  uint8_t* out;
  size_t cap, n;
  void byte(uint32_t b) { if (n < cap) out[n] = (uint8_t)b; n++; }
  void head(uint32_t mt, uint64_t v) {
    if (v < 24) { byte((mt << 5) | (uint32_t)v); return; }
    const int nb = v < 256 ? 1 : v < 65536 ? 2 : v < (1ull << 32) ? 4 : 8;
    byte((mt << 5) | (nb == 1 ? 24u : nb == 2 ? 25u : nb == 4 ? 26u : 27u));
    for (int k = nb - 1; k >= 0; k--) byte((uint32_t)(v >> (8 * k)));
  }
  void bytes(const uint8_t* p, size_t len) { head(2, len); for (size_t k = 0; k < len; k++) byte(p[k]); }
  void nonce(const praos_nonce& x) {
    if (x.neutral) { head(4, 1); head(0, 0); }
    else { head(4, 2); head(0, 1); bytes(x.hash, 32); }
  }
};
struct CborR {
  const uint8_t* p;
  size_t len, pos;
  bool ok = true;
  bool head(uint32_t want_mt, uint64_t* v) {
    if (!ok || pos >= len) return ok = false;
    const uint32_t ib = p[pos++], mt = ib >> 5, ai = ib & 31;
    if (mt != want_mt) return ok = false;
    if (ai < 24) { *v = ai; return true; }
    if (ai > 27) return ok = false;
    const int nb = 1 << (ai - 24);
    if (pos + nb > len) return ok = false;
    uint64_t x = 0;
    for (int k = 0; k < nb; k++) x = (x << 8) | p[pos++];
    *v = x;
    return true;
  }
  bool expect(uint32_t mt, uint64_t want) { uint64_t v; return head(mt, &v) && (v == want || (ok = false)); }
  bool bytes(uint8_t* dst, size_t n) {
    uint64_t l;
    if (!head(2, &l) || l != n || pos + n > len) return ok = false;
    std::memcpy(dst, p + pos, n);
    pos += n;
    return true;
  }
  bool nonce(praos_nonce& x) {
    uint64_t l, tag;
    if (!head(4, &l) || !head(0, &tag)) return false;
    std::memset(&x, 0, sizeof x);
    if (l == 1 && tag == 0) { x.neutral = 1; return true; }
    if (l == 2 && tag == 1) { x.neutral = 0; return bytes(x.hash, 32); }
    return ok = false;
  }
};
}  // namespace

extern "C" {

int praos_state_encode(const praos_chain_state* st, uint8_t* out, size_t cap, size_t* len) {
  if (!st || !len || (cap && !out) || (st->m && (!st->counter_hash28 || !st->counter))) return PRAOS_E_ARG;
  std::vector<size_t> order(st->m);
  for (size_t k = 0; k < st->m; k++) order[k] = k;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return std::memcmp(st->counter_hash28 + 28 * a, st->counter_hash28 + 28 * b, 28) < 0;
  });
  for (size_t k = 1; k < order.size(); k++)
    if (!std::memcmp(st->counter_hash28 + 28 * order[k - 1], st->counter_hash28 + 28 * order[k], 28))
      return PRAOS_E_ARG;                                   // duplicate key: not a Map
  CborW w{out, cap, 0};
  w.head(4, 2); w.head(0, 0);                               // encodeVersion 0
  w.head(4, 7);
  if (st->last_slot_origin) { w.head(4, 1); w.head(0, 0); }
  else { w.head(4, 2); w.head(0, 1); w.head(0, st->last_slot); }
  w.head(5, st->m);
  for (size_t k : order) { w.bytes(st->counter_hash28 + 28 * k, 28); w.head(0, st->counter[k]); }
  w.nonce(st->evolving); w.nonce(st->candidate); w.nonce(st->epoch_nonce); w.nonce(st->lab);
  w.nonce(st->last_epoch_block);
  *len = w.n;
  return w.n <= cap ? PRAOS_OK : PRAOS_E_ARG;
}

int praos_state_decode(const uint8_t* in, size_t len, praos_chain_state* st) {
  if (!in || !st || (st->cap && (!st->counter_hash28 || !st->counter))) return PRAOS_E_ARG;
  CborR r{in, len, 0};
  uint64_t v, tag, m;
  r.expect(4, 2); r.expect(0, 0); r.expect(4, 7);
  if (!r.ok) return PRAOS_E_ARG;
  if (!r.head(4, &v) || !r.head(0, &tag)) return PRAOS_E_ARG;
  if (v == 1 && tag == 0) { st->last_slot_origin = 1; st->last_slot = 0; }
  else if (v == 2 && tag == 1 && r.head(0, &st->last_slot)) st->last_slot_origin = 0;
  else return PRAOS_E_ARG;
  if (!r.head(5, &m) || m > st->cap) return PRAOS_E_ARG;
  for (size_t k = 0; k < m; k++) {
    if (!r.bytes(st->counter_hash28 + 28 * k, 28) || !r.head(0, &st->counter[k])) return PRAOS_E_ARG;
    if (k && std::memcmp(st->counter_hash28 + 28 * (k - 1), st->counter_hash28 + 28 * k, 28) >= 0)
      return PRAOS_E_ARG;                                   // Data.Map decoding wants ascending keys
  }
  st->m = m;
  if (!r.nonce(st->evolving) || !r.nonce(st->candidate) || !r.nonce(st->epoch_nonce) || !r.nonce(st->lab) ||
      !r.nonce(st->last_epoch_block))
    return PRAOS_E_ARG;
  return r.pos == len ? PRAOS_OK : PRAOS_E_ARG;
}

}  // extern "C"
