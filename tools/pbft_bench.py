#!/usr/bin/env python3
"""Byron header validation throughput on one GPU.

    python tools/pbft_bench.py [--sizes 21600,216000] [--distinct 2048] [--passes 3] [--reps 3]
                               [--warmup 2] [--sweep 1024,4096,...] [--fold 216000]

(a) praos_verify_pbft_headers end to end (upload, decode, key cache, verifies, download) over N
    forged main headers signed by 7 delegates in turn, with the delegate-key cache forced on, forced
    off and at its default cut-over; beside it praos_verify_byron_integrity over the same headers
    wrapped as blocks with empty bodies -- the entry this library had for the PBFT signature before
    header validation existed (one lane per block, every verify uncached, plus a trivial body
    check; its code is unchanged, so the figure is the parent's on the same device and run).
    --distinct signed headers are forged and tiled to N: the verify needs no prev-hash linking,
    and every lane still does its own full decode, hash and verify.  The arenas are tiled for
    real, so each call uploads the bytes it would in use.
(b) The cut-over: cached against uncached medians at the --sweep batch sizes; the cut-over is the
    smallest size from which the cached form stays ahead.
(c) praos_pbft_update_chain_dep_state alone (the host fold) over a valid synthetic chain of
    --fold headers (k = 2160, threshold 475, 7 delegates in turn, an EBB every 21,600 slots),
    in microseconds per header.
The variants are timed in one process in --passes passes, each variant on a freshly opened context
(one open at a time, the order rotated per pass): median of passes x --reps timed runs, --warmup
runs before each group, with min and max (the box's spread).  Every variant's outputs are checked
once per context, and praos_pbft_stats that it ran the kernels its name says.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ouroboros-consensus_amd"))
for d in ("tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, d))
import praos_hip  # noqa: E402
from praos_hip import abi  # noqa: E402

ES, K, THR = 21600, 2160, 475


def forge(m):
    """m distinct signed main blocks with empty bodies, 7 delegates in turn -> (blocks, delegs)"""
    import byron_corpus as bc
    import pbft_corpus as pc
    r = random.Random(0x9bf7)
    D = [bc.Delegate(r) for _ in range(7)]
    prev = bytes(r.getrandbits(8) for _ in range(32))
    blocks = []
    for i in range(m):
        b = bc.Main(r, D[i % 7], prev, i // ES, i % ES, i + 1)
        blocks.append(b)
        prev = b.header_hash
    return blocks, pc.delegation(r, D), bc.PM


def tiled(parts, n):
    """n spans over the parts repeated: (arena, off, len)"""
    m = len(parts)
    one = np.frombuffer(b"".join(parts), np.uint8)
    ln1 = np.array([len(p) for p in parts], np.uint64)
    off1 = np.concatenate([[0], np.cumsum(ln1)[:-1]]).astype(np.uint64)
    reps = (n + m - 1) // m
    arena = np.tile(one, reps)
    off = (np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(len(one)), m) + np.tile(off1, reps))[:n]
    ln = np.tile(ln1, reps)[:n].astype(np.uint32)
    return np.ascontiguousarray(arena[:int(off[-1]) + int(ln[-1])]), np.ascontiguousarray(off), ln


def summary(v):
    return {"median_ms": round(1e3 * statistics.median(v), 3), "min_ms": round(1e3 * min(v), 3),
            "max_ms": round(1e3 * max(v), 3), "samples": len(v)}


def rounds(variants, reps, warmup, raw=False):
    """variants: {name: fn}; alternating rounds -> {name: median / min / max in ms} (raw: the times)"""
    t = {k: [] for k in variants}
    for r in range(warmup + reps):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= warmup:
                t[k].append(dt)
    return t if raw else {k: summary(v) for k, v in t.items()}


def context(ck_min):
    """a context with the cut-over (PRAOS_PBFT_CK_MIN, read at open) forced; None: the default"""
    want = {"PRAOS_PBFT_CK_MIN": ck_min}
    old = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is not None:
            os.environ[k] = str(v)
    try:
        return praos_hip.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def fold_chain(n, delegs):
    """columns of a valid chain of n headers from Origin: an EBB at every epoch start, main
    headers in consecutive slots signed by the delegates in turn"""
    rng = np.random.default_rng(5)
    ebb = np.zeros(n, np.uint8)
    slot = np.zeros(n, np.uint64)
    bno = np.zeros(n, np.uint64)
    gk = np.zeros(n, np.int32)
    s, b, j = 0, 0, 0
    for i in range(n):
        if s % ES == 0 and (i == 0 or not ebb[i - 1]):
            ebb[i], slot[i], bno[i], gk[i] = 1, s, b if i else 0, -1
            continue
        b += 1
        slot[i], bno[i], gk[i] = s, b, j % len(delegs)
        s += 1
        j += 1
    hh = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    prev = np.zeros((n, 32), np.uint8)
    prev[1:] = hh[:-1]
    gen = np.zeros(n, np.uint8)
    gen[0] = 1
    H = {"bits": np.zeros(n, np.uint8), "gk_idx": gk, "slot": slot, "block_no": bno, "prev_hash": prev,
         "prev_is_genesis": gen, "header_hash": hh}
    return H, ebb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="21600,216000")
    ap.add_argument("--distinct", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3, help="timed runs per pass")
    ap.add_argument("--passes", type=int, default=3, help="passes over the variants, a fresh context each")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweep", default="1024,4096,16384,32768,65536,98304,131072,163840")
    ap.add_argument("--fold", type=int, default=216000)
    args = ap.parse_args()
    import torch
    blocks, delegs, pmagic = forge(args.distinct)
    P = abi.Context.pbft_params(K, THR, ES, pmagic)
    # One context is open at a time, opened fresh for every (pass, variant): which of several open
    # contexts a variant runs on moved its time by 10-20 % (the same code path on two contexts), more
    # than the differences measured here.  A context keeps the device buffers of its last call for
    # the next one, so the warm-ups also settle its allocations.
    FORCE = {"cached": 1, "uncached": 1 << 40, "default": None, "byron_integrity": None}
    out = {"device": torch.cuda.get_device_name(0), "distinct": args.distinct, "delegates": 7, "passes": args.passes,
           "note": "distinct signed headers tiled to N; the verify needs no prev-hash linking", "verify": {},
           "cutover_sweep": {}}

    def measure(names, n):
        ha, ho, hl = tiled([b.header for b in blocks], n)
        ba, bo, bl = tiled([b.bytes for b in blocks], n) if "byron_integrity" in names else (None, None, None)
        ebb = np.zeros(n, np.uint8)
        t = {k: [] for k in names}
        for ps in range(args.passes):
            order = names[ps % len(names):] + names[:ps % len(names)]
            for name in order:
                c = context(FORCE[name])
                try:
                    if name == "byron_integrity":
                        fn = lambda: c.verify_byron_integrity(ba, bo, bl, ES, pmagic)
                        res, _ = fn()
                        assert not res.any(), "forged blocks must verify"
                    else:
                        fn = lambda: c.verify_pbft_headers(ha, ho, hl, ebb, P, delegs)
                        H = fn()        # every variant's answer, and the kernels it says it ran
                        assert not H["bits"].any() and (H["gk_idx"] >= 0).all(), f"forged headers must verify ({name})"
                        st = c.pbft_stats()
                        assert st["cached_verifies"] + st["uncached_verifies"] == n, (name, st)
                        if name != "default":
                            assert st["cache"] == (name == "cached"), (name, st)
                            assert st["cached_verifies"] == (n if name == "cached" else 0), (name, st)
                    t[name] += rounds({name: fn}, args.reps, args.warmup, raw=True)[name]
                finally:
                    c.close()
        return {k: summary(v) for k, v in t.items()}, len(ha), (len(ba) if ba is not None else 0)

    for n in [int(x) for x in args.sizes.split(",") if x]:
        r, hb, bb = measure(["cached", "uncached", "default", "byron_integrity"], n)
        for k in r:
            r[k]["headers_per_s"] = round(n / (r[k]["median_ms"] * 1e-3))
        r["header_bytes"], r["block_bytes"] = hb, bb
        r["meets_bar"] = r["default"]["median_ms"] <= r["byron_integrity"]["median_ms"]
        out["verify"][str(n)] = r
    cross = None
    for n in [int(x) for x in args.sweep.split(",") if x]:
        r, _, _ = measure(["cached", "uncached"], n)
        out["cutover_sweep"][str(n)] = r
        if r["cached"]["median_ms"] < r["uncached"]["median_ms"]:
            cross = n if cross is None else cross
        else:
            cross = None
    out["cutover"] = cross
    # (c) the host fold alone
    n = args.fold
    H, ebb = fold_chain(n, delegs)
    c = abi.Context(abi.HOST_ONLY)          # the fold needs no device
    o = abi.Context._pbft_out(H)
    d = abi.Context._pbft_delegs(delegs)
    verdict, aux = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    ss, sh = np.zeros(K, np.uint64), np.zeros((K, 28), np.uint8)
    stop = ctypes.c_size_t(0)

    def fold():
        tip = abi.PbftTip()
        tip.origin = 1
        st = abi.PbftStateC(K, 0, abi.ptr(ss, abi.u64p), abi.ptr(sh))
        c.check(c.L.praos_pbft_update_chain_dep_state(c.h, n, ctypes.byref(o), abi.ptr(ebb), ctypes.byref(P), abi.ptr(d),
                                                      len(d), ctypes.byref(tip), ctypes.byref(st), abi.ptr(verdict),
                                                      abi.ptr(aux, abi.u64p), ctypes.byref(stop)))
        assert stop.value == n and st.n == K, (stop.value, int(verdict[stop.value]) if stop.value < n else 0)
    r = rounds({"fold": fold}, args.reps, args.warmup)["fold"]
    r["headers"] = n
    r["us_per_header"] = round(1e3 * r["median_ms"] / n, 4)
    out["fold"] = r
    c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
