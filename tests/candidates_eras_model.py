"""Checkers of praos_validate_candidates_pbft (tests/test_gpu_candidates_pbft.py) and
praos_validate_candidates_tpraos (tests/test_gpu_candidates_tpraos.py), in the style of
tests/candidates_model.py.

Byron: unwrap in Python (praos_hip.wire), dedup with a dict, the rows from pbft_corpus.model_rows (the
sequential restatement of k_pbft.hip in tests/pbft_model.py: no GPU), and each fragment folded the
way the ChainSync client does (MiniProtocol/ChainSync/Client.hs:794-812): the DoesntFit check
against the fragment's tip, then validateHeader -- pbft_model.fold, one header at a time -- up to
the first failure or the forecast horizon.

TPraos: candidates_model.Model with the TPraos rules of oracle/tpraos.py and oracle/chainstate.py
(TICKN's extra entropy at every tick, PRTCL's failure set) over bits that
verify_tpraos_header_bytes gives under every nonce the fold ticks to.
"""
import numpy as np

import candidates_model as cm
import chainstate as cs
import pbft_corpus as pc
import pbft_model as pm
import tpraos as tp
from praos_hip import abi, wire

V_DOESNT_FIT, V_NOT_REACHED = 25, 255


class Hdr:
    """header bytes standing in for a block in pbft_corpus.model_rows"""

    def __init__(self, header, kind):
        self.header, self.kind = bytes(header), kind


def wrap_blocks(blocks, hint=lambda i, b: len(b.header) + 7 * i):
    """the wire items of byron_corpus blocks (kind 0 = EBB, 1 = main header)"""
    return [wire.wrap(0, b.header, b.kind, hint(i, b)) for i, b in enumerate(blocks)]


def pack(items):
    """(arena u8[], off u64[], len u32[]) of wire items, a few bytes between them"""
    arena, off, ln = bytearray(), [], []
    for i, it in enumerate(items):
        arena += bytes([0xA5] * (i % 3))
        off.append(len(arena))
        ln.append(len(it))
        arena += it
    return (np.frombuffer(bytes(arena), np.uint8).copy(), np.array(off, np.uint64), np.array(ln, np.uint32))


class PbftModel:
    """One delegation map and one set of PBFT parameters."""

    def __init__(self, window_size, threshold, epoch_slots, protocol_magic, delegs, n_eras=wire.N_ERAS):
        self.window, self.threshold, self.es, self.magic = window_size, threshold, epoch_slots, protocol_magic
        self.delegs, self.n_eras = delegs, n_eras
        self.rows = {}         # (kind, header bytes) -> pbft_model.verify_header's dict

    def key(self, item):
        st, era, kind, _, off, ln = wire.unwrap(item, n_eras=self.n_eras)
        if st != wire.WIRE_OK or era != 0:
            return None
        return (kind, bytes(item[off:off + ln]))

    def row(self, key):
        if key not in self.rows:
            kind, hdr = key
            self.rows[key] = pc.model_rows([Hdr(hdr, kind)], self.delegs, self.es, self.magic)[0]
        return self.rows[key]

    def fold(self, items, tip, state, view_end_slot=1 << 64):
        """One fragment from (tip, state).  Returns dict(verdict, aux, chain_stop, processed, tip,
        state, keys): tip and state those at chain_stop."""
        keys = [self.key(it) for it in items]
        n = len(items)
        verdict, aux = [V_NOT_REACHED] * n, [0] * n
        win = [(int(s), bytes(g)) for s, g in state]
        stop, processed = None, n
        for i in range(n):
            h = self.row(keys[i]) if keys[i] is not None else None
            if h is None or h["bits"] & pm.BIT_DECODE:
                verdict[i], stop, processed = pm.V_INPUT, i, i + 1
                break
            if h["slot"] >= view_end_slot:
                processed = i
                break
            ebb = keys[i][0] == 0
            fits = bool(h["prev_is_genesis"]) if tip is None else (not h["prev_is_genesis"] and
                                                                   bytes(h["prev_hash"]) == tip[2])
            if not fits:
                verdict[i], stop, processed = V_DOESNT_FIT, i, i + 1      # checked before validateHeader
                break
            v, a, s1, tip1, win1 = pm.fold([h], [int(ebb)], self.window, self.threshold, self.es, self.delegs, tip, win)
            verdict[i], aux[i] = v[0], a[0]
            assert v[0] != pm.V_ENV_PREV_HASH
            if v[0] != pm.V_OK:
                stop, processed = i, i + 1
                break
            tip, win = tip1, win1
        return {"verdict": verdict, "aux": aux, "chain_stop": processed if stop is None else stop,
                "processed": processed, "tip": tip, "state": win, "keys": keys}

    def check(self, items, frag_first, frags_in, got, frags_out, view_end_slot=1 << 64):
        """Every fragment of a praos_validate_candidates_pbft result (got, frags_out: what
        wire.validate_candidates_pbft returned / updated) against the model's fold from frags_in; the
        rows against the model's, in order of first appearance.  Returns the distinct keys."""
        all_keys = []
        for j, f in enumerate(frags_in):
            lo, hi = frag_first[j], frag_first[j + 1]
            want = self.fold(items[lo:hi], f["tip"], f["state"], view_end_slot)
            all_keys += want["keys"]
            g = frags_out[j]
            assert list(got["verdict"][lo:hi]) == want["verdict"], (j, list(got["verdict"][lo:hi]), want["verdict"])
            assert [int(a) for a in got["aux"][lo:hi]] == want["aux"], j
            assert (g["chain_stop"], g["processed"]) == (want["chain_stop"], want["processed"]), j
            assert g["tip"] == want["tip"], (j, g["tip"], want["tip"])
            assert g["state"] == want["state"], j
        distinct = list(dict.fromkeys(k for k in all_keys if k is not None))
        index = {k: r for r, k in enumerate(distinct)}
        for i, it in enumerate(items):
            assert got["wire_status"][i] == wire.unwrap(it, n_eras=self.n_eras)[0], i
            want_row = wire.NO_ROW if all_keys[i] is None else index[all_keys[i]]
            assert int(got["row"][i]) == want_row, i                  # rows in order of first appearance
        st = got["stats"]
        assert st["items"] == len(items) and st["unwrapped"] == sum(k is not None for k in all_keys)
        assert st["distinct_headers"] == got["n_rows"] == len(distinct)
        rows = [self.row(k) for k in distinct]
        verifies = sum(1 for r in rows if not r["bits"] & pm.BIT_DECODE and r["delegate_hash"] != bytes(28))
        assert st["sig_verifies"] == verifies
        if rows:
            want = pc.rows_to_columns(rows)
            for c, w in want.items():
                if c in got["rows"]:
                    assert (np.asarray(got["rows"][c]).reshape(len(rows), -1) == w.reshape(len(rows), -1)).all(), c
            assert list(got["row_is_ebb"]) == [int(k[0] == 0) for k in distinct]
        return distinct


V_TPRAOS = 19


class TPraosModel(cm.Model):
    """One ledger view (pools, params, the overlay's genesis delegates), one epoch layout, the
    envelope limits, TICKN's extra entropy."""

    def __init__(self, ctx, pools, params, epoch_info, limits, extra_entropy=None, gen_hashes=(), n_eras=wire.N_ERAS,
                 tpraos_eras=wire.TPRAOS_ERAS):
        super().__init__(ctx, pools, params, epoch_info, limits, n_eras, tpraos_eras)
        self.extra = extra_entropy
        self.known |= set(gen_hashes)              # currentIssueNo's Just 0: pools and genesis delegates
        self.cols = {}                             # header bytes -> the decoded columns of its row

    def _run(self, hdrs, eta):
        arena = np.frombuffer(b"".join(hdrs), np.uint8)
        ln = np.array([len(h) for h in hdrs], np.uint32)
        off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.uint64)]).astype(np.uint64)
        self.ctx.set_epoch(eta, self.pools, self.params)
        return self.ctx.verify_tpraos_header_bytes(arena, off, ln, decoded=True)

    def _decode(self, hdrs):
        todo = [h for h in dict.fromkeys(hdrs) if h not in self.dec]
        if not todo:
            return
        _, D = self._run(todo, bytes(32))          # the decode does not read the nonce
        for i, h in enumerate(todo):
            self.cols[h] = {k: np.array(v[i]) for k, v in D.items()}
            if D["status"][i] & abi.DEC_FAILED:
                self.dec[h] = None
            else:
                self.dec[h] = {"slot": int(D["slot"][i]), "block_no": int(D["block_no"][i]),
                               "prev": None if D["prev_is_genesis"][i] else bytes(D["prev_hash"][i]),
                               "hk": cm.b2b(D["cold_vk"][i], 28), "ocert_n": int(D["ocert_n"][i]),
                               "body_size": int(D["body_size"][i]), "hash": bytes(D["header_hash"][i]),
                               "size": len(h)}

    def _verify(self, hdrs, eta):
        todo = [h for h in dict.fromkeys(hdrs) if (h, eta) not in self.crypto]
        if not todo:
            return
        o, _ = self._run(todo, eta)
        for i, h in enumerate(todo):
            self.crypto[(h, eta)] = (int(o["bits"][i]), bytes(o["nonce"][i]))

    def fold(self, items, state, tip, view_end_slot=1 << 64):
        keys = [self.key(it) for it in items]
        self._decode([k[1] for k in keys if k is not None])
        w, n = cm.copy_state(state), len(items)
        verdict, failures = [V_NOT_REACHED] * n, [0] * n
        stop, processed, etas = None, n, []
        for i in range(n):
            d = self.dec[keys[i][1]] if keys[i] is not None else None
            if d is None:
                verdict[i], stop, processed = cs.V_INPUT, i, i + 1
                etas.append(None)
                break
            s = d["slot"]
            if s >= view_end_slot:
                processed = i
                break
            e_new = self.epoch(s)
            e_old = 0 if w["last_slot"] is None else self.epoch(w["last_slot"])
            t_epoch, t_leb = w["epoch_nonce"], w["leb"]
            if e_new > e_old:                                        # TICKN
                t_epoch, t_leb = cs.combine(cs.combine(w["candidate"], w["leb"]), self.extra), w["lab"]
            if (keys[i][1], t_epoch) not in self.crypto:
                run = [keys[j][1] for j in range(i, n) if keys[j] is not None and self.dec.get(keys[j][1]) and
                       self.epoch(self.dec[keys[j][1]]["slot"]) == e_new]
                self._verify(run, t_epoch)
            bits, nonce = self.crypto[(keys[i][1], t_epoch)]
            etas.append(t_epoch)
            if bits & tp.BIT_INPUT:
                v, f = cs.V_INPUT, 0
            else:
                m = w["counters"].get(d["hk"], 0 if d["hk"] in self.known else None)
                f = tp.failures(bits, m, d["ocert_n"])
                v = V_TPRAOS if f else cs.V_OK
                env = dict(self.limits, block_no=[d["block_no"]], header_size=[d["size"]], body_size=[d["body_size"]])
                ve = cs.envelope_verdict(env, tip, 0, s, d["prev"])
                v = ve if ve != cs.V_OK else v
                fits = (d["prev"] is None) if tip is None else (d["prev"] is not None and d["prev"] == tip[2])
                if not fits:
                    v = V_DOESNT_FIT                                 # checked before validateHeader
            verdict[i], failures[i] = v, (f if v == V_TPRAOS else 0)
            if v != cs.V_OK:
                stop, processed = i, i + 1
                break
            w["epoch_nonce"], w["leb"] = t_epoch, t_leb
            w["last_slot"] = s
            w["lab"] = d["prev"]
            w["evolving"] = cs.combine(w["evolving"], nonce)
            if s + self.window < self.base_slot + (e_new - self.base_no + 1) * self.length:
                w["candidate"] = w["evolving"]
            w["counters"][d["hk"]] = d["ocert_n"]
            tip = (s, d["block_no"], d["hash"])
        hashes = [self.dec[k[1]]["hash"] if k is not None and self.dec.get(k[1]) else None for k in keys[:processed]]
        return {"verdict": verdict, "failures": failures, "chain_stop": processed if stop is None else stop,
                "processed": processed, "state": w, "tip": tip, "etas": etas, "hashes": hashes, "keys": keys}

    def check(self, items, frag_first, frags_in, got, frags_out, view_end_slot=1 << 64):
        """candidates_model.Model.check (verdicts, stops, states, tips, rows, first-appearance order),
        then the failure sets and the rows' decoded columns and outputs under their nonces."""
        distinct = super().check(items, frag_first, frags_in, got, frags_out, view_end_slot)
        for j, f in enumerate(frags_in):
            lo, hi = frag_first[j], frag_first[j + 1]
            want = self.fold(items[lo:hi], f["state"], f["tip"], view_end_slot)
            assert [int(x) for x in got["failures"][lo:hi]] == want["failures"], j
        all_keys = [self.key(it) for it in items]
        seen = set()
        for i, k in enumerate(all_keys):
            r = int(got["row"][i])
            if k is None or r in seen:
                continue
            seen.add(r)
            for c in ("status", "slot", "block_no", "prev_hash", "header_hash", "cold_vk", "vrf_vk", "ocert_n", "kes_sig",
                      "signed_body", "leader_out", "leader_proof"):
                assert np.array_equal(got["dec"][c][r], self.cols[k[1]][c]), (i, c)
            eta = got["etas"][got["eta_idx"][r]]
            if (k[1], eta) in self.crypto and self.dec[k[1]] is not None:
                assert (int(got["rows"]["bits"][r]), bytes(got["rows"]["nonce"][r])) == self.crypto[(k[1], eta)], i
        return distinct
