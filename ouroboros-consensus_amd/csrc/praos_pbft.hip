// praos_pbft.hip -- the host half of Byron header validation: hashVerKey on the host, the
// sequential fold (validateEnvelope with the Byron instance, then PBFT updateChainDepState) and
// the PBftState codec.  No device code; works on a host-only context.
//   Protocol/PBFT.hs:320-353            updateChainDepState
//   Protocol/PBFT/State.hs:206-228      append        :277-305  the state codec
//   Byron/Ledger/HeaderValidation.hs:39-75   the Byron envelope instance
//   HeaderValidation.hs:297-344         validateEnvelope
// CPU restatement: tests/pbft_model.py.
#include "praos_hip.h"
#include "host_util.hpp"
#include "replay_internal.hpp"
#include "sha3.hpp"

#include <algorithm>
#include <array>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

using Hash28 = std::array<uint8_t, 28>;

// hashVerKey on the host: Blake2b-224(SHA3-256(58 40 || xpub64))
void praos_pbft_key_hash_host_(const uint8_t* keys64, size_t n, uint8_t* out28) {
  for (size_t i = 0; i < n; i++) {
    uint8_t msg[66] = {0x58, 0x40}, d[32];
    std::memcpy(msg + 2, keys64 + 64 * i, 64);
    (void)sha3_256_small(d, msg, 66);
    praos_host::blake2b(out28 + 28 * i, 28, d, 32);
  }
}

// the Bimap: no duplicate in either column
bool praos_pbft_delegs_ok_(const uint8_t* delegs, uint32_t n) {
  for (int col = 0; col < 2; col++) {
    std::vector<Hash28> v(n);
    for (uint32_t k = 0; k < n; k++) std::memcpy(v[k].data(), delegs + 56 * (size_t)k + 28 * col, 28);
    std::sort(v.begin(), v.end());
    if (std::adjacent_find(v.begin(), v.end()) != v.end()) return false;
  }
  return true;
}

namespace {

struct Window {
  std::deque<std::pair<uint64_t, uint32_t>> sig;   // (slot, key id), oldest first
  std::vector<Hash28> keys;                        // key id -> genesis key hash
  std::vector<uint64_t> counts;
  uint32_t intern(const uint8_t* h) {
    Hash28 k;
    std::memcpy(k.data(), h, 28);
    for (uint32_t i = 0; i < keys.size(); i++)
      if (keys[i] == k) return i;
    keys.push_back(k);
    counts.push_back(0);
    return (uint32_t)keys.size() - 1;
  }
};

struct Tip {
  bool origin, is_ebb;
  uint64_t slot, block_no;
  uint8_t hash[32];
};

}  // namespace

// The fold of praos_pbft_update_chain_dep_state (map == nullptr, client == false: header i is row
// i, would-be verdicts after the first failure) and the ChainSync client's (item i reads row
// map[i] of h and is_ebb, PRAOS_V_DOESNT_FIT ahead of the envelope, the fold ends at the first
// failure).  Arguments are checked by the callers.
static int pbft_fold(size_t n, const uint32_t* map, size_t n_rows, const praos_pbft_out* h, const uint8_t* is_ebb,
                     const praos_pbft_params* p, const uint8_t* delegs, uint32_t n_delegs, praos_pbft_tip* tip,
                     praos_pbft_state* st, uint8_t* verdict, uint64_t* aux, size_t* chain_stop, size_t* processed,
                     bool client, std::string* err) {
  Window w;
  for (uint64_t k = 0; k < st->n; k++) {
    const uint32_t id = w.intern(st->genesis_hash + 28 * k);
    w.sig.emplace_back(st->slot[k], id);
    w.counts[id]++;
  }
  std::vector<uint32_t> deleg_id(n_delegs);
  for (uint32_t k = 0; k < n_delegs; k++) deleg_id[k] = w.intern(delegs + 56 * (size_t)k);
  Tip t{tip->origin != 0, tip->is_ebb != 0, tip->slot, tip->block_no, {0}};
  std::memcpy(t.hash, tip->hash, 32);
  // the state and tip at the first failing header
  bool stopped = false;
  Window w_stop;
  Tip t_stop{};
  *chain_stop = n;
  size_t done = n;
  for (size_t i = 0; i < n; i++) {
    const size_t r = map ? map[i] : i;
    uint8_t v = PRAOS_V_OK;
    uint64_t a = 0;
    bool ebb = false;
    uint64_t slot = 0, bno = 0;
    do {
      if (map && (map[i] == PRAOS_NO_ROW || r >= n_rows)) { v = PRAOS_V_INPUT; break; }
      ebb = is_ebb[r] != 0;
      slot = h->slot[r];
      bno = h->block_no[r];
      if (h->bits[r] & PRAOS_PBFT_BIT_DECODE) { v = PRAOS_V_INPUT; break; }
      const bool gen = h->prev_is_genesis[r] != 0;
      const bool prev_ok = t.origin ? gen : (!gen && std::memcmp(t.hash, h->prev_hash + 32 * r, 32) == 0);
      if (client && !prev_ok) { v = PRAOS_V_DOESNT_FIT; break; }
      // ---- validateEnvelope
      const uint64_t exp_bno = t.origin ? 0 : ((!t.is_ebb && ebb) ? t.block_no : t.block_no + 1);
      if (bno != exp_bno) { v = PRAOS_V_ENV_BLOCK_NO; a = exp_bno; break; }
      const uint64_t min_slot = t.origin ? 0 : ((t.is_ebb && !ebb) ? t.slot : t.slot + 1);
      if (!(slot >= min_slot)) { v = PRAOS_V_ENV_SLOT_NO; a = min_slot; break; }
      if (!prev_ok) { v = PRAOS_V_ENV_PREV_HASH; break; }
      if (ebb && slot % p->epoch_slots != 0) { v = PRAOS_V_ENV_EBB_IN_SLOT; a = slot; break; }
      if (ebb) break;                                    // PBftValidateBoundary: the state is left alone
      // ---- PBFT updateChainDepState
      if (h->bits[r] & PRAOS_PBFT_BIT_SIG) { v = PRAOS_V_PBFT_INVALID_SIG; break; }
      if (!w.sig.empty() && slot < w.sig.back().first) { v = PRAOS_V_PBFT_INVALID_SLOT; break; }
      if (h->gk_idx[r] < 0) { v = PRAOS_V_PBFT_NOT_DELEGATE; break; }
      if (h->gk_idx[r] >= (int64_t)n_delegs) {
        if (err) *err = "pbft: gk_idx of row " + std::to_string(r) + " outside the delegation map";
        return PRAOS_E_ARG;
      }
      const uint32_t id = deleg_id[(size_t)h->gk_idx[r]];
      const uint64_t after = w.counts[id] + 1 -
                             ((w.sig.size() == p->window_size && w.sig.front().second == id) ? 1 : 0);
      if (after > p->threshold) { v = PRAOS_V_PBFT_EXCEEDED; a = after; break; }
      const bool trim = w.sig.size() == p->window_size;   // the size before the append
      w.sig.emplace_back(slot, id);
      w.counts[id]++;
      if (trim) {
        w.counts[w.sig.front().second]--;
        w.sig.pop_front();
      }
    } while (false);
    verdict[i] = v;
    if (aux) aux[i] = a;
    if (v != PRAOS_V_OK) {
      if (!stopped) {
        stopped = true;
        *chain_stop = i;
        w_stop = w;            // nothing of header i has been applied
        t_stop = t;
      }
      if (client) { done = i + 1; break; }   // the client disconnects here
      continue;                // the working copy skips the invalid header
    }
    t.origin = false;
    t.is_ebb = ebb;
    t.slot = slot;
    t.block_no = bno;
    std::memcpy(t.hash, h->header_hash + 32 * r, 32);
  }
  if (processed) *processed = done;
  const Window& wr = stopped ? w_stop : w;
  const Tip& tr = stopped ? t_stop : t;
  st->n = wr.sig.size();
  for (size_t k = 0; k < wr.sig.size(); k++) {
    st->slot[k] = wr.sig[k].first;
    std::memcpy(st->genesis_hash + 28 * k, wr.keys[wr.sig[k].second].data(), 28);
  }
  tip->origin = tr.origin ? 1 : 0;
  tip->is_ebb = tr.is_ebb ? 1 : 0;
  tip->slot = tr.slot;
  tip->block_no = tr.block_no;
  std::memcpy(tip->hash, tr.hash, 32);
  return PRAOS_OK;
}

int rp_pbft_fold_client(size_t n, const uint32_t* map, size_t n_rows, const praos_pbft_out* h,
                        const uint8_t* row_is_ebb, const praos_pbft_params* p, const uint8_t* delegs,
                        uint32_t n_delegs, praos_pbft_tip* tip, praos_pbft_state* st, uint8_t* verdict, uint64_t* aux,
                        size_t* chain_stop, size_t* processed, std::string* err_out) {
  return pbft_fold(n, map, n_rows, h, row_is_ebb, p, delegs, n_delegs, tip, st, verdict, aux, chain_stop, processed,
                   true, err_out);
}

extern "C" {

int praos_pbft_update_chain_dep_state(praos_ctx* c, size_t n, const praos_pbft_out* h, const uint8_t* is_ebb,
                                      const praos_pbft_params* p, const uint8_t* delegs, uint32_t n_delegs,
                                      praos_pbft_tip* tip, praos_pbft_state* st, uint8_t* verdict, uint64_t* aux,
                                      size_t* chain_stop) {
  if (!c || !p || !tip || !st || !chain_stop || (n_delegs && !delegs) || p->epoch_slots == 0 || p->window_size == 0)
    return PRAOS_E_ARG;
  if (n && (!h || !is_ebb || !verdict || !h->bits || !h->gk_idx || !h->slot || !h->block_no || !h->prev_hash ||
            !h->prev_is_genesis || !h->header_hash))
    return PRAOS_E_ARG;
  if (st->n > st->cap || st->cap < p->window_size || st->n > p->window_size || (st->cap && (!st->slot || !st->genesis_hash))) {
    praos_set_error_(c, "pbft: state needs n <= window_size <= cap");
    return PRAOS_E_ARG;
  }
  if (!praos_pbft_delegs_ok_(delegs, n_delegs)) {
    praos_set_error_(c, "pbft: duplicate hash in the delegation map");
    return PRAOS_E_ARG;
  }
  for (size_t i = 0; i < n; i++)
    if (h->gk_idx[i] < -1 || h->gk_idx[i] >= (int64_t)n_delegs) {
      praos_set_error_(c, "pbft: gk_idx of header " + std::to_string(i) + " outside the delegation map");
      return PRAOS_E_ARG;
    }
  return pbft_fold(n, nullptr, n, h, is_ebb, p, delegs, n_delegs, tip, st, verdict, aux, chain_stop, nullptr, false,
                   nullptr);
}

static size_t put_head(std::vector<uint8_t>& o, uint8_t mt, uint64_t v) {
  const uint8_t m = (uint8_t)(mt << 5);
  if (v < 24) { o.push_back(m | (uint8_t)v); return 1; }
  int nb = v < 0x100 ? 1 : (v < 0x10000 ? 2 : (v < 0x100000000ull ? 4 : 8));
  o.push_back(m | (uint8_t)(nb == 1 ? 24 : nb == 2 ? 25 : nb == 4 ? 26 : 27));
  for (int k = nb - 1; k >= 0; k--) o.push_back((uint8_t)(v >> (8 * k)));
  return 1 + nb;
}

int praos_pbft_state_encode(const praos_pbft_state* st, uint8_t* out, size_t cap, size_t* len) {
  if (!st || !len || st->n > st->cap || (st->n && (!st->slot || !st->genesis_hash))) return PRAOS_E_ARG;
  // invert: key -> slots, newest first
  std::vector<std::pair<Hash28, uint64_t>> v(st->n);
  for (uint64_t k = 0; k < st->n; k++) {
    std::memcpy(v[k].first.data(), st->genesis_hash + 28 * k, 28);
    v[k].second = k;                                      // position in the window
  }
  std::stable_sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  size_t keys = 0;
  for (size_t k = 0; k < v.size(); k++) keys += k == 0 || v[k].first != v[k - 1].first;
  std::vector<uint8_t> o;
  o.push_back(0x82);
  o.push_back(0x01);
  put_head(o, 5, keys);
  for (size_t k = 0; k < v.size();) {
    size_t e = k;
    while (e < v.size() && v[e].first == v[k].first) e++;
    put_head(o, 2, 28);
    o.insert(o.end(), v[k].first.begin(), v[k].first.end());
    o.push_back(0x9f);
    for (size_t j = e; j-- > k;) put_head(o, 0, st->slot[v[j].second]);
    o.push_back(0xff);
    k = e;
  }
  *len = o.size();
  if (o.size() > cap || (o.size() && !out)) return PRAOS_E_ARG;
  std::memcpy(out, o.data(), o.size());
  return PRAOS_OK;
}

namespace {
struct Rd {
  const uint8_t* p;
  size_t n, at = 0;
  bool head(uint8_t& mt, uint8_t& ai, uint64_t& v) {
    if (at >= n) return false;
    const uint8_t b = p[at++];
    mt = b >> 5;
    ai = b & 31;
    if (ai < 24) { v = ai; return true; }
    if (ai > 27) { v = 0; return ai == 31; }
    const size_t nb = (size_t)1 << (ai - 24);
    if (nb > n - at) return false;
    v = 0;
    for (size_t k = 0; k < nb; k++) v = (v << 8) | p[at++];
    return true;
  }
};
}  // namespace

int praos_pbft_state_decode(const uint8_t* in, size_t len, praos_pbft_state* st) {
  if (!in || !st) return PRAOS_E_ARG;
  Rd r{in, len};
  uint8_t mt, ai;
  uint64_t v, nkeys;
  if (!(r.head(mt, ai, v) && mt == 4 && ai != 31 && v == 2)) return PRAOS_E_ARG;
  if (!(r.head(mt, ai, v) && mt == 0 && v == 1)) return PRAOS_E_ARG;          // version 1
  if (!(r.head(mt, ai, nkeys) && mt == 5 && ai != 31 && nkeys <= len)) return PRAOS_E_ARG;
  struct Entry { Hash28 key; std::vector<uint64_t> slots; };
  std::vector<Entry> es;
  for (uint64_t k = 0; k < nkeys; k++) {
    Entry e;
    if (!(r.head(mt, ai, v) && mt == 2 && ai != 31 && v == 28 && 28 <= len - r.at)) return PRAOS_E_ARG;
    std::memcpy(e.key.data(), in + r.at, 28);
    r.at += 28;
    uint64_t cnt;
    if (!(r.head(mt, ai, cnt) && mt == 4)) return PRAOS_E_ARG;
    const bool indef = ai == 31;
    for (uint64_t j = 0; indef ? (r.at < len && in[r.at] != 0xff) : j < cnt; j++) {
      if (!(r.head(mt, ai, v) && mt == 0 && ai != 31)) return PRAOS_E_ARG;
      e.slots.push_back(v);
    }
    if (indef) {
      if (r.at >= len) return PRAOS_E_ARG;
      r.at++;
    }
    es.push_back(std::move(e));
  }
  if (r.at != len) return PRAOS_E_ARG;
  std::stable_sort(es.begin(), es.end(), [](const Entry& a, const Entry& b) { return a.key < b.key; });
  for (size_t k = 1; k < es.size(); k++)
    if (es[k].key == es[k - 1].key) return PRAOS_E_ARG;
  std::vector<std::pair<uint64_t, const Hash28*>> sg;
  for (const Entry& e : es)
    for (uint64_t s : e.slots) sg.emplace_back(s, &e.key);
  std::stable_sort(sg.begin(), sg.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  st->n = sg.size();
  if (sg.size() > st->cap || (sg.size() && (!st->slot || !st->genesis_hash))) return PRAOS_E_ARG;
  for (size_t k = 0; k < sg.size(); k++) {
    st->slot[k] = sg[k].first;
    std::memcpy(st->genesis_hash + 28 * k, sg[k].second->data(), 28);
  }
  return PRAOS_OK;
}

}  // extern "C"
