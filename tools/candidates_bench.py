#!/usr/bin/env python3
"""praos_validate_candidates against the per-peer way to do the same job.

K peers x n headers of the C5 chain (one epoch, linked), as wire items.  Two sub-cases: identical
fragments, and fragments that share all but their last 5 % (each peer's tail carries its own bytes:
one flipped bit in every KES signature, so the tail is distinct per peer and its first header stops
that peer's fragment).  Two variants, each on a freshly opened context, alternating; 2 warm-up and
7 timed calls each; median and min-max; outputs checked on every run:

  new     one praos_validate_candidates call;
  parent  what a caller had before it: unwrap on the host (the 7-byte wrapper checked and cut,
          vectorised), praos_verify_header_bytes over all K*n inner spans, K host folds
          (praos_validate_headers) from each peer's state.

Prints one JSON line per (K, n, sub-case): both variants' median, min and max over the timed calls
of both rounds, the parent's min-max spread, the new call's stats and the bar the shape falls
under (K >= 8: new median below parent median by more than that spread; K = 1: new median above
it by no more than that spread).  Where the new call's time goes (GPU passes against the host
fold) is read from a kernel trace of one case run on its own, --trace-case.  The parent's output
buffers are allocated outside the timed calls and hold only what its folds read.

  python tools/candidates_bench.py [--k 1,8,32] [--n 2048,54000] [--out FILE]
  python tools/candidates_bench.py --trace-case 8,54000,identical     (one new-call run, for rocprofv3)

--proto tpraos | pbft (default praos: everything above, output unchanged) measures
praos_validate_candidates_tpraos / praos_validate_candidates_pbft the same way:
  tpraos  the "tp" chain (Shelley .. Alonzo BHeaders, wire index 4); the parent is the host unwrap,
          praos_verify_tpraos_header_bytes over all K*n inner spans (bits, pool_idx, nonce and the
          nine decoded columns) and K folds with praos_tpraos_update_chain_dep_state;
  pbft    a forged chain of main headers in one Byron epoch, 7 delegates in turn (k = 2160,
          threshold 475), wire index 0 (default --n 2048,21600); the parent is the host unwrap,
          praos_verify_pbft_headers over all K*n inner spans and K folds with
          praos_pbft_update_chain_dep_state; tail5 flips one bit of every tail header's signature.
          --cache FILE keeps the forged chain between runs (forging signs every header on the host).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ouroboros-consensus_amd"))

import praos_hip  # noqa: E402
from praos_hip import abi, chains  # noqa: E402
from praos_hip.chunk import pack_chunk  # noqa: E402

LIMITS = (9, 8, 1100, 90_112)
WARM, TIMED = 2, 7
NEEDED = ("status", "block_no", "slot", "prev_hash", "prev_is_genesis", "cold_vk", "body_size", "ocert_n", "header_hash")


def genesis(eta0):
    return {"last_slot": None, "counters": {}, "evolving": eta0, "candidate": eta0, "epoch_nonce": eta0,
            "lab": None, "leb": None}


def make_items(ctx, cfg, n):
    """The first n headers of the C5 chain, linked, as wire items of era 5: (arena, off, len) of one peer."""
    H, pools, _, p = chains.make_chain(ctx, cfg, chains.load_schedule("c5"), n, link=True)
    a, off, ln = pack_chunk(H)
    assert int(ln.min()) >= 256 and int(ln.max()) < 65536
    wl = ln.astype(np.int64) + 7
    woff = np.cumsum(wl) - wl
    out = np.zeros(int(wl.sum()), np.uint8)
    pre = np.array([0x82, 0x05, 0xD8, 0x18, 0x59], np.uint8)
    for k in range(5):
        out[woff + k] = pre[k]
    out[woff + 5] = (ln >> 8).astype(np.uint8)
    out[woff + 6] = (ln & 0xFF).astype(np.uint8)
    for L in np.unique(ln):
        rows = np.nonzero(ln == L)[0]
        src = off[rows].astype(np.int64)[:, None] + np.arange(int(L))[None, :]
        out[(woff[rows] + 7)[:, None] + np.arange(int(L))[None, :]] = a[src]
    return out, woff.astype(np.uint64), wl.astype(np.uint32), pools, p, H


def build_case(one, K, sub):
    """K peers' items in one arena.  identical: K copies.  tail5: the last 5 % of each peer's copy has
    bit 0x40 of byte (len - 100 - peer) of every item flipped (inside the KES signature)."""
    arena1, off1, len1 = one
    n = len(off1)
    arena = np.tile(arena1, K)
    off = np.concatenate([off1 + np.uint64(j * len(arena1)) for j in range(K)])
    ln = np.tile(len1, K)
    stop = n
    if sub == "tail5":
        stop = n - max(1, n // 20)
        for j in range(K):
            at = off[j * n + stop:(j + 1) * n].astype(np.int64) + ln[j * n + stop:(j + 1) * n].astype(np.int64) - 100 - j
            arena[at] ^= 0x40
    return arena, off, ln, stop


def host_unwrap(arena, off, ln):
    """The wrapper [5, #6.24(bytes)] with a 2-byte length head, checked and cut on the host."""
    o = off.astype(np.int64)
    ok = ((arena[o] == 0x82) & (arena[o + 1] == 0x05) & (arena[o + 2] == 0xD8) & (arena[o + 3] == 0x18) &
          (arena[o + 4] == 0x59) & ((arena[o + 5].astype(np.uint32) << 8 | arena[o + 6]) + 7 == ln))
    assert ok.all()
    return off + np.uint64(7), (ln - 7).astype(np.uint32)


class New:
    def __init__(self, pools, p, eta0, ei):
        self.ctx = praos_hip.Context(0)
        self.ctx.set_epoch(eta0, pools, p)
        self.eta0, self.ei = eta0, ei

    def prepare(self, K, n):
        pass

    def run(self, arena, off, ln, K, n, rows_cap):
        fr = [{"state": genesis(self.eta0), "tip": None} for _ in range(K)]
        got = self.ctx.validate_candidates(arena, off, ln, [j * n for j in range(K + 1)], fr, self.ei, LIMITS,
                                           rows_cap=rows_cap, rows_out=False)
        return got["verdict"], [(f["chain_stop"], f["tip"], f["state"]) for f in fr], got["stats"]


class Parent:
    def __init__(self, pools, p, eta0, ei):
        self.ctx = praos_hip.Context(0)
        self.ctx.set_epoch(eta0, pools, p)
        self.eta0, self.ei = eta0, ei

    def prepare(self, K, n):
        """The output buffers, allocated once outside the timed calls: only what the fold reads (bits,
        pool_idx, nonce and nine decoded columns; beta and leader are not asked for)."""
        N = K * n
        self.o = {"bits": np.zeros(N, np.uint16), "pool_idx": np.zeros(N, np.int32), "nonce": np.zeros((N, 32), np.uint8)}
        self.os_ = abi.Out(abi.ptr(self.o["bits"], abi.u16p), abi.ptr(self.o["pool_idx"], abi.i32p), None, None,
                           abi.ptr(self.o["nonce"]))
        self.D = {name: np.zeros((N,) + shp, dt) for name, dt, shp in abi.DECODED_FIELDS if name in NEEDED}
        self.d = abi.Decoded()
        for name, dt, _ in abi.DECODED_FIELDS:
            if name in NEEDED:
                setattr(self.d, name, abi.ptr(self.D[name], abi._CT[dt]))

    def run(self, arena, off, ln, K, n, rows_cap):
        c = self.ctx
        ioff, iln = host_unwrap(arena, off, ln)
        N = K * n
        hb = c.header_bytes_struct(arena, ioff, iln)
        o, os_, D, d = self.o, self.os_, self.D, self.d
        c.check(c.L.praos_verify_header_bytes(c.h, ctypes.byref(hb), ctypes.byref(os_), ctypes.byref(d)))
        verdict = np.zeros(N, np.uint8)
        ends = []
        z = np.zeros
        for j in range(K):
            s = slice(j * n, (j + 1) * n)
            H = {"slot": D["slot"][s], "cold_vk": D["cold_vk"][s], "ocert_n": D["ocert_n"][s],
                 "vrf_vk": z((1, 32), np.uint8), "vrf_out": z((1, 64), np.uint8), "vrf_proof": z((1, 80), np.uint8),
                 "hot_vk": z((1, 32), np.uint8), "ocert_c0": z(1, np.uint64), "ocert_sig": z((1, 64), np.uint8),
                 "kes_sig": z((1, 448), np.uint8), "body_off": z(1, np.uint64), "body_len": z(1, np.uint32),
                 "body_bytes": z(8, np.uint8)}
            oj = {"bits": o["bits"][s], "pool_idx": o["pool_idx"][s], "nonce": o["nonce"][s],
                  "beta": z((1, 64), np.uint8), "leader": z((1, 32), np.uint8)}
            st = genesis(self.eta0)
            env = dict(zip(("max_major_pv", "lv_prot_major", "max_header_size", "max_body_size"), LIMITS), tip=None,
                       block_no=D["block_no"][s], header_hash=D["header_hash"][s], header_size=iln[s],
                       body_size=D["body_size"][s])
            v, stop, _ = c.update_chain_dep_state(H, oj, D["prev_hash"][s], st, self.ei,
                                                  prev_is_genesis=D["prev_is_genesis"][s], envelope=env)
            verdict[s] = v
            ends.append((stop, env["tip"], st))
        return verdict, ends, None


# ---------------------------------------------------------------- TPraos
def make_items_tpraos(ctx, cfg, n):
    """The first n headers of the tp chain, linked, as wire items of era 4 (Alonzo)."""
    H, pools, _, p = chains.make_chain(ctx, cfg, chains.load_schedule("tp"), n, link=True)
    a, off, ln = pack_chunk(H, era_tag=5)
    assert int(ln.min()) >= 256 and int(ln.max()) < 65536
    wl = ln.astype(np.int64) + 7
    woff = np.cumsum(wl) - wl
    out = np.zeros(int(wl.sum()), np.uint8)
    pre = np.array([0x82, 0x04, 0xD8, 0x18, 0x59], np.uint8)
    for k in range(5):
        out[woff + k] = pre[k]
    out[woff + 5] = (ln >> 8).astype(np.uint8)
    out[woff + 6] = (ln & 0xFF).astype(np.uint8)
    for L in np.unique(ln):
        rows = np.nonzero(ln == L)[0]
        src = off[rows].astype(np.int64)[:, None] + np.arange(int(L))[None, :]
        out[(woff[rows] + 7)[:, None] + np.arange(int(L))[None, :]] = a[src]
    return out, woff.astype(np.uint64), wl.astype(np.uint32), pools, p, H


def host_unwrap_era(arena, off, ln, era):
    o = off.astype(np.int64)
    ok = ((arena[o] == 0x82) & (arena[o + 1] == era) & (arena[o + 2] == 0xD8) & (arena[o + 3] == 0x18) &
          (arena[o + 4] == 0x59) & ((arena[o + 5].astype(np.uint32) << 8 | arena[o + 6]) + 7 == ln))
    assert ok.all()
    return off + np.uint64(7), (ln - 7).astype(np.uint32)


TP_LIMITS = (9, 8, 1400, 90_112)


class NewTP(New):
    def run(self, arena, off, ln, K, n, rows_cap):
        fr = [{"state": genesis(self.eta0), "tip": None} for _ in range(K)]
        got = self.ctx.validate_candidates_tpraos(arena, off, ln, [j * n for j in range(K + 1)], fr, self.ei, TP_LIMITS,
                                                  rows_cap=rows_cap, rows_out=False)
        return got["verdict"], [(f["chain_stop"], f["tip"], f["state"]) for f in fr], got["stats"]


class ParentTP(Parent):
    def prepare(self, K, n):
        """only what the folds read: bits, pool_idx, nonce and nine decoded columns"""
        N = K * n
        self.o = {"bits": np.zeros(N, np.uint16), "pool_idx": np.zeros(N, np.int32), "nonce": np.zeros((N, 32), np.uint8)}
        self.os_ = abi.TPOut(abi.ptr(self.o["bits"], abi.u16p), abi.ptr(self.o["pool_idx"], abi.i32p), None, None,
                             abi.ptr(self.o["nonce"]))
        self.D = {name: np.zeros((N,) + shp, dt) for name, dt, shp in abi.DECODED_FIELDS if name in NEEDED}
        self.d = abi.Decoded()
        for name, dt, _ in abi.DECODED_FIELDS:
            if name in NEEDED:
                setattr(self.d, name, abi.ptr(self.D[name], abi._CT[dt]))

    def run(self, arena, off, ln, K, n, rows_cap):
        c = self.ctx
        ioff, iln = host_unwrap_era(arena, off, ln, 4)
        N = K * n
        hb = c.header_bytes_struct(arena, ioff, iln)
        o, D = self.o, self.D
        c.check(c.L.praos_verify_tpraos_header_bytes(c.h, ctypes.byref(hb), ctypes.byref(self.os_), ctypes.byref(self.d),
                                                     None, None))
        verdict = np.zeros(N, np.uint8)
        fails = np.zeros(N, np.uint16)
        ends = []
        z = np.zeros
        ei = abi.EpochInfo(*self.ei)
        for j in range(K):
            s = slice(j * n, (j + 1) * n)
            H = {"slot": D["slot"][s], "cold_vk": D["cold_vk"][s], "ocert_n": D["ocert_n"][s],
                 "vrf_vk": z((1, 32), np.uint8), "vrf_out": z((1, 64), np.uint8), "vrf_proof": z((1, 80), np.uint8),
                 "hot_vk": z((1, 32), np.uint8), "ocert_c0": z(1, np.uint64), "ocert_sig": z((1, 64), np.uint8),
                 "kes_sig": z((1, 448), np.uint8), "body_off": z(1, np.uint64), "body_len": z(1, np.uint32),
                 "body_bytes": z(8, np.uint8)}
            th = abi.TPHeaders()
            th.h = c.headers_struct(H)
            lo, lp = z((1, 64), np.uint8), z((1, 80), np.uint8)
            th.leader_out, th.leader_proof = abi.ptr(lo), abi.ptr(lp)
            to = abi.TPOut(abi.ptr(o["bits"][s], abi.u16p), abi.ptr(o["pool_idx"][s], abi.i32p), None, None,
                           abi.ptr(o["nonce"][s]))
            state = genesis(self.eta0)
            st, hk, cv = abi._state_struct(state, n + 8)
            E = abi.Envelope()
            hs = np.ascontiguousarray(iln[s])
            E.block_no, E.header_hash = abi.ptr(D["block_no"][s], abi.u64p), abi.ptr(D["header_hash"][s])
            E.header_size, E.body_size = abi.ptr(hs, abi.u32p), abi.ptr(D["body_size"][s], abi.u32p)
            E.tip_is_origin = 1
            E.max_major_pv, E.lv_prot_major, E.max_header_size, E.max_body_size = TP_LIMITS
            stop, done = ctypes.c_size_t(0), ctypes.c_size_t(0)
            c.check(c.L.praos_tpraos_update_chain_dep_state(
                c.h, ctypes.byref(th), abi.ptr(D["prev_hash"][s]), abi.ptr(D["prev_is_genesis"][s]), ctypes.byref(to),
                ctypes.byref(E), ctypes.byref(ei), None, ctypes.byref(st), abi.ptr(verdict[s]), abi.ptr(fails[s], abi.u16p),
                ctypes.byref(stop), ctypes.byref(done)))
            tip = None if E.tip_is_origin else (int(E.tip_slot), int(E.tip_block_no), bytes(E.tip_hash))
            ends.append((int(stop.value), tip, abi._state_from_struct(st, hk, cv)))
        return verdict, ends, None


# ---------------------------------------------------------------- Byron
PB_ES, PB_K, PB_THR = 21600, 2160, 475
PB_PRE = 13         # 82 00 82 82 01 19 hh ll d8 18 59 hh ll


def forge_pbft(n, cache=None):
    """n linked main headers of Byron epoch 0, slot i, difficulty i + 1, 7 delegates in turn, on top of
    an EBB tip: (headers, signature offsets, delegs, protocol magic, tip)."""
    for d in ("tests", "oracle"):
        sys.path.insert(0, os.path.join(ROOT, d))
    import random

    import byron_corpus as bc
    import pbft_corpus as pc
    r = random.Random(0x9bf7)
    D = [bc.Delegate(r) for _ in range(7)]
    delegs = pc.delegation(r, D)
    prev0 = bytes(r.getrandbits(8) for _ in range(32))
    tip = (0, 0, prev0, 1)
    if cache and os.path.exists(cache):
        z = np.load(cache)
        if len(z["len"]) >= n:
            ln = z["len"][:n]
            off = np.cumsum(ln) - ln
            hdrs = [bytes(z["arena"][int(o):int(o) + int(m)]) for o, m in zip(off, ln)]
            return hdrs, z["sig"][:n], delegs, bc.PM, tip
    hdrs, sig, prev = [], [], prev0
    for i in range(n):
        b = bc.Main(r, D[i % 7], prev, 0, i, i + 1)
        hdrs.append(b.header)
        sig.append(b.header.index(b.sig))
        prev = b.header_hash
    if cache:
        np.savez(cache, arena=np.frombuffer(b"".join(hdrs), np.uint8), len=np.array([len(h) for h in hdrs], np.int64),
                 sig=np.array(sig, np.int64))
    return hdrs, np.array(sig, np.int64), delegs, bc.PM, tip


def make_items_pbft(hdrs):
    parts, off, pos = [], [], 0
    for h in hdrs:
        m = len(h)
        assert 256 <= m < 65536
        it = bytes([0x82, 0x00, 0x82, 0x82, 0x01, 0x19, m >> 8, m & 255, 0xD8, 0x18, 0x59, m >> 8, m & 255]) + h
        off.append(pos)
        pos += len(it)
        parts.append(it)
    ln = np.array([len(p) for p in parts], np.uint32)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(off, np.uint64), ln


def build_case_pbft(one, sig, K, sub):
    arena1, off1, len1 = one
    n = len(off1)
    arena = np.tile(arena1, K)
    off = np.concatenate([off1 + np.uint64(j * len(arena1)) for j in range(K)])
    ln = np.tile(len1, K)
    stop = n
    if sub == "tail5":
        stop = n - max(1, n // 20)
        for j in range(K):
            at = off[j * n + stop:(j + 1) * n].astype(np.int64) + PB_PRE + sig[stop:n] + 8 + j
            arena[at] ^= 0x40
    return arena, off, ln, stop


class NewPbft:
    def __init__(self, delegs, pm, tip):
        self.ctx = praos_hip.Context(0)
        self.delegs, self.tip = delegs, tip
        self.params = abi.Context.pbft_params(PB_K, PB_THR, PB_ES, pm)

    def prepare(self, K, n):
        pass

    def run(self, arena, off, ln, K, n, rows_cap):
        fr = [{"tip": self.tip, "state": []} for _ in range(K)]
        got = self.ctx.validate_candidates_pbft(arena, off, ln, [j * n for j in range(K + 1)], fr, self.params,
                                                self.delegs, rows_cap=rows_cap, rows_out=False)
        return got["verdict"], [(f["chain_stop"], f["tip"], f["state"]) for f in fr], got["stats"]


class ParentPbft(NewPbft):
    def prepare(self, K, n):
        N = K * n
        self.H = {name: np.zeros((N,) + shp, dt) for name, dt, shp in abi.PBFT_OUT_FIELDS if name != "delegate_hash"}
        self.ebb = np.zeros(N, np.uint8)

    def run(self, arena, off, ln, K, n, rows_cap):
        c = self.ctx
        o = off.astype(np.int64)
        m = ln.astype(np.int64) - PB_PRE
        ok = ((arena[o] == 0x82) & (arena[o + 1] == 0) & (arena[o + 2] == 0x82) & (arena[o + 3] == 0x82) &
              (arena[o + 4] == 1) & (arena[o + 5] == 0x19) & (arena[o + 8] == 0xD8) & (arena[o + 9] == 0x18) &
              (arena[o + 10] == 0x59) & ((arena[o + 11].astype(np.int64) << 8 | arena[o + 12]) == m))
        assert ok.all()
        ioff, iln = off + np.uint64(PB_PRE), m.astype(np.uint32)
        N = K * n
        hb = c.header_bytes_struct(arena, ioff, iln)
        d = c._pbft_delegs(self.delegs)
        H = self.H
        c.check(c.L.praos_verify_pbft_headers(c.h, ctypes.byref(hb), abi.ptr(self.ebb), ctypes.byref(self.params),
                                              abi.ptr(d), len(d), ctypes.byref(c._pbft_out(H))))
        verdict = np.zeros(N, np.uint8)
        ends = []
        for j in range(K):
            s = slice(j * n, (j + 1) * n)
            Hj = {k: v[s] for k, v in H.items()}
            v, _, stop, tip, st = c.pbft_update_chain_dep_state(Hj, self.ebb[s], self.params, self.delegs, self.tip, [])
            verdict[s] = v
            ends.append((stop, tip, st))
        return verdict, ends, None


def timed(make, case, K, n, rows_cap, want_stop):
    """2 warm-ups + 7 timed calls on a fresh context; returns the times (ms) and the last outputs."""
    v = make()
    try:
        v.prepare(K, n)
        ts = []
        for r in range(WARM + TIMED):
            t0 = time.perf_counter()
            verdict, ends, stats = v.run(case[0], case[1], case[2], K, n, rows_cap)
            dt = (time.perf_counter() - t0) * 1e3
            assert all(e[0] == want_stop for e in ends), [e[0] for e in ends]
            for j in range(K):
                assert not verdict[j * n:j * n + want_stop].any()
            if r >= WARM:
                ts.append(dt)
        return ts, ends, stats
    finally:
        v.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="1,8,32")
    ap.add_argument("--n", default="2048,54000")
    ap.add_argument("--sub", default="identical,tail5")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-case", default=None, help="K,n,sub: run the new call three times and exit")
    ap.add_argument("--proto", default="praos", choices=("praos", "tpraos", "pbft"))
    ap.add_argument("--cache", default=None, help="pbft: a file that keeps the forged chain between runs")
    ap.add_argument("--forge-only", action="store_true", help="pbft: forge the chain into --cache and exit (no GPU)")
    args = ap.parse_args()
    if args.proto == "pbft" and args.n == "2048,54000":
        args.n = "2048,21600"
    ns = sorted({int(x) for x in args.n.split(",")}) if not args.trace_case else [int(args.trace_case.split(",")[1])]
    case_of = build_case
    if args.proto == "pbft":
        hdrs, sig, delegs, pm, tip = forge_pbft(max(ns), args.cache)
        if args.forge_only:
            return
        arena1, off1, len1 = make_items_pbft(hdrs)
        case_of = lambda one, K, sub: build_case_pbft(one, sig, K, sub)  # noqa: E731
        variants = (("new", lambda: NewPbft(delegs, pm, tip)), ("parent", lambda: ParentPbft(delegs, pm, tip)))
    else:
        cfg = chains.CONFIGS["c5" if args.proto == "praos" else "tp"]
        ei = (0, 0, cfg["epoch_length"], 3 * 2160 * 20)
        gen = praos_hip.Context(0)
        arena1, off1, len1, pools, p, _ = (make_items if args.proto == "praos" else make_items_tpraos)(gen, cfg, max(ns))
        gen.close()
        if args.proto == "praos":
            variants = (("new", lambda: New(pools, p, cfg["eta0"], ei)), ("parent", lambda: Parent(pools, p, cfg["eta0"], ei)))
        else:
            variants = (("new", lambda: NewTP(pools, p, cfg["eta0"], ei)),
                        ("parent", lambda: ParentTP(pools, p, cfg["eta0"], ei)))
    lines = []
    if args.trace_case:
        K, n, sub = args.trace_case.split(",")
        K, n = int(K), int(n)
        case = case_of((arena1[:int(off1[n - 1] + len1[n - 1])], off1[:n], len1[:n]), K, sub)
        ts, _, stats = timed(variants[0][1], case, K, n, n + n // 10 + K * (n // 20 + 1), case[3])
        print(json.dumps({"trace_case": args.trace_case, "ms": ts, "stats": stats}))
        return
    for n in ns:
        one = (arena1[:int(off1[n - 1] + len1[n - 1])], off1[:n], len1[:n])
        for K in [int(x) for x in args.k.split(",")]:
            for sub in args.sub.split(","):
                if K == 1 and sub != "identical":
                    continue
                case = case_of(one, K, sub)
                rows_cap = n + (K * (n // 20 + 1) if sub == "tail5" else 0)
                res = {}
                # variants alternate: new, parent, new, parent -- the second pair is the reported one
                for rnd in range(2):
                    for name, mk in variants:
                        ts, ends, stats = timed(mk, case, K, n, rows_cap, case[3])
                        res.setdefault(name, []).append((ts, ends, stats))
                for j in range(K):          # both variants end every peer in the same state and tip
                    assert res["new"][-1][1][j] == res["parent"][-1][1][j], j
                row = {"K": K, "n": n, "sub": sub, "stats": res["new"][-1][2]}
                if args.proto != "praos":
                    row = dict({"proto": args.proto}, **row)
                for name in ("new", "parent"):
                    ts = [t for r in res[name] for t in r[0]]
                    row[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                                 "rounds_median_ms": [statistics.median(r[0]) for r in res[name]]}
                spread = row["parent"]["max_ms"] - row["parent"]["min_ms"]
                row["parent_spread_ms"] = spread
                if K == 1:
                    row["bar2_met"] = row["new"]["median_ms"] <= row["parent"]["median_ms"] + spread
                else:
                    row["bar1_met"] = row["new"]["median_ms"] < row["parent"]["median_ms"] - spread
                line = json.dumps(row)
                print(line, flush=True)
                lines.append(line)
                if args.out:
                    with open(args.out, "w") as f:
                        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
