"""Checker of praos_validate_candidates (tests/test_gpu_candidates.py).

Unwrap in Python (praos_hip.wire), dedup with a dict, and fold each fragment the way the ChainSync
client does (MiniProtocol/ChainSync/Client.hs:794-812) with the oracle's rules (oracle/chainstate.py:
verdict, envelope_verdict, the nonce semigroup) over crypto bits that ctx.verify_header_bytes gives
under each epoch nonce the fold ticks to -- the entry point the candidates call does not go through.
"""
import hashlib

import numpy as np

import chainstate as cs
from praos_hip import abi, wire

V_DOESNT_FIT, V_NOT_REACHED = 25, 255


def b2b(m, n=32):
    return hashlib.blake2b(bytes(m), digest_size=n).digest()


def copy_state(st):
    return {k: (dict(v) if isinstance(v, dict) else v) for k, v in st.items()}


class Model:
    """One ledger view (pools, params), one epoch layout, the envelope limits."""

    def __init__(self, ctx, pools, params, epoch_info, limits, n_eras=wire.N_ERAS, praos_eras=wire.PRAOS_ERAS):
        self.ctx, self.pools, self.params = ctx, pools, params
        self.base_slot, self.base_no, self.length, self.window = epoch_info
        self.limits = dict(zip(("max_major_pv", "lv_prot_major", "max_header_size", "max_body_size"), limits))
        self.n_eras, self.praos_eras = n_eras, praos_eras
        self.known = {h for h, _, _ in pools}
        self.dec = {}          # header bytes -> decoded fields (None: does not decode)
        self.crypto = {}       # (header bytes, eta) -> (bits, nonce value)

    def key(self, item):
        st, era, _, _, off, ln = wire.unwrap(item, n_eras=self.n_eras)
        if st != wire.WIRE_OK or not (self.praos_eras >> era) & 1:
            return None
        return (era, bytes(item[off:off + ln]))

    def _decode(self, hdrs):
        todo = [h for h in dict.fromkeys(hdrs) if h not in self.dec]
        if not todo:
            return
        arena = np.frombuffer(b"".join(todo), np.uint8)
        ln = np.array([len(h) for h in todo], np.uint32)
        off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.uint64)]).astype(np.uint64)
        D = self.ctx.decode_headers(arena, off, ln)
        for i, h in enumerate(todo):
            if D["status"][i] & abi.DEC_FAILED:
                self.dec[h] = None
            else:
                self.dec[h] = {"slot": int(D["slot"][i]), "block_no": int(D["block_no"][i]),
                               "prev": None if D["prev_is_genesis"][i] else bytes(D["prev_hash"][i]),
                               "hk": b2b(D["cold_vk"][i], 28), "ocert_n": int(D["ocert_n"][i]),
                               "body_size": int(D["body_size"][i]), "hash": bytes(D["header_hash"][i]),
                               "size": len(h)}

    def _verify(self, hdrs, eta):
        todo = [h for h in dict.fromkeys(hdrs) if (h, eta) not in self.crypto]
        if not todo:
            return
        arena = np.frombuffer(b"".join(todo), np.uint8)
        ln = np.array([len(h) for h in todo], np.uint32)
        off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.uint64)]).astype(np.uint64)
        self.ctx.set_epoch(eta, self.pools, self.params)
        o = self.ctx.verify_header_bytes(arena, off, ln)
        for i, h in enumerate(todo):
            self.crypto[(h, eta)] = (int(o["bits"][i]), bytes(o["nonce"][i]))

    def epoch(self, s):
        return self.base_no + (s - self.base_slot) // self.length

    def fold(self, items, state, tip, view_end_slot=1 << 64):
        """One fragment.  Returns dict(verdict, chain_stop, processed, state, tip, etas (the nonce each
        judged item ran under), hashes (the header hash of each judged item's header))."""
        keys = [self.key(it) for it in items]
        self._decode([k[1] for k in keys if k is not None])
        w, n = copy_state(state), len(items)
        verdict = [V_NOT_REACHED] * n
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
            if e_new > e_old:
                t_epoch, t_leb = cs.combine(w["candidate"], w["leb"]), w["lab"]
            if (keys[i][1], t_epoch) not in self.crypto:
                # the rest of this fragment's epoch under the nonce it has just ticked to
                run = [keys[j][1] for j in range(i, n) if keys[j] is not None and self.dec.get(keys[j][1]) and
                       self.epoch(self.dec[keys[j][1]]["slot"]) == e_new]
                self._verify(run, t_epoch)
            bits, nonce = self.crypto[(keys[i][1], t_epoch)]
            etas.append(t_epoch)
            m = w["counters"].get(d["hk"], 0 if d["hk"] in self.known else None)
            v = cs.verdict(bits, m, d["ocert_n"])
            if v != cs.V_INPUT:
                env = dict(self.limits, block_no=[d["block_no"]], header_size=[d["size"]], body_size=[d["body_size"]])
                ve = cs.envelope_verdict(env, tip, 0, s, d["prev"])
                v = ve if ve != cs.V_OK else v
                fits = (d["prev"] is None) if tip is None else (d["prev"] is not None and d["prev"] == tip[2])
                if not fits:
                    v = V_DOESNT_FIT                      # checked before validateHeader
            verdict[i] = v
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
        return {"verdict": verdict, "chain_stop": processed if stop is None else stop, "processed": processed,
                "state": w, "tip": tip, "etas": etas, "hashes": hashes, "keys": keys}

    def check(self, items, frag_first, frags_in, got, frags_out, view_end_slot=1 << 64):
        """Every fragment of a praos_validate_candidates result (got, frags_out: what
        wire.validate_candidates returned / updated) against the model's fold from frags_in."""
        all_keys = []
        for j, f in enumerate(frags_in):
            lo, hi = frag_first[j], frag_first[j + 1]
            want = self.fold(items[lo:hi], f["state"], f["tip"], view_end_slot)
            all_keys += want["keys"]
            g = frags_out[j]
            assert list(got["verdict"][lo:hi]) == want["verdict"], (j, list(got["verdict"][lo:hi]), want["verdict"])
            assert (g["chain_stop"], g["processed"]) == (want["chain_stop"], want["processed"]), j
            assert g["state"] == want["state"], j
            assert g["tip"] == want["tip"], j
            # every judged item reads a row that holds its header under the nonce it ticked to
            for i in range(want["processed"]):
                r = int(got["row"][lo + i])
                if want["hashes"][i] is None:
                    assert want["keys"][i] is None and r == wire.NO_ROW or bool(got["dec"]["status"][r] & abi.DEC_FAILED)
                    continue
                assert bytes(got["dec"]["header_hash"][r]) == want["hashes"][i], (j, i)
                assert got["etas"][got["eta_idx"][r]] == want["etas"][i], (j, i)
        for i, it in enumerate(items):
            assert got["wire_status"][i] == wire.unwrap(it, n_eras=self.n_eras)[0], i
            assert (got["row"][i] == wire.NO_ROW) == (all_keys[i] is None), i
        # rows: the distinct headers in order of first appearance, then the extra (header, nonce) pairs
        distinct = list(dict.fromkeys(k for k in all_keys if k is not None))
        st = got["stats"]
        assert st["items"] == len(items) and st["unwrapped"] == sum(k is not None for k in all_keys)
        assert st["distinct_headers"] == len(distinct) and st["rows"] == got["n_rows"] == len(distinct) + st["extra_rows"]
        for r, (era, h) in enumerate(distinct):
            assert bytes(got["dec"]["header_hash"][r]) == b2b(h), r
        first = {}
        for i, k in enumerate(all_keys):
            if k is not None:
                r = int(got["row"][i])
                base = distinct.index(k) if len(distinct) < 64 else None
                pair = (bytes(got["dec"]["header_hash"][r]), int(got["eta_idx"][r]))
                assert pair[0] == b2b(k[1]), i
                if base is not None and r >= len(distinct):
                    assert int(got["eta_idx"][r]) != int(got["eta_idx"][base]), i
                first.setdefault(r, i)
        # a row's first item comes before the first item of every later row (first-appearance order)
        order = [first[r] for r in sorted(first)]
        base_order = [i for r, i in sorted(first.items()) if r < len(distinct)]
        assert base_order == sorted(base_order)
        extra_order = [i for r, i in sorted(first.items()) if r >= len(distinct)]
        assert extra_order == sorted(extra_order) and len(order) == len(first)
        return distinct
