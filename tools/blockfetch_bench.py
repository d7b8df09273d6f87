#!/usr/bin/env python3
"""Fetched-block verification throughput on one GPU.

    python tools/blockfetch_bench.py [--blocks 4096] [--txs 40] [--signers 4096] [--peers 4] [--reps 7] [--warmup 2]

The chunk of tools/txwit_bench.py -- --blocks Babbage blocks of --txs transactions, bodies of 340
bytes, 2 genuine VKey witnesses each, under synthesized headers that name their bodies -- with
every block wrapped as a wire block and asked for at its own point.
(a)  one peer: the whole call (praos_verify_fetched_blocks, every array downloaded) and the same
     with witnesses = 0; beside them the stored-block calls over the same blocks as stored bytes,
     praos_verify_tx_witnesses and praos_verify_block_integrity (upload, run with KES, download);
(b)  --peers peers sending the same blocks, each its own copy of the bytes: dedup on and off, with
     and without witnesses; the per-item results of dedup on are those of dedup off mapped
     through row ("dedup_identical"); "dedup_gate": on is faster than off;
(c)  the bytes the compare kernel reads ((peers - 1) x the wire bytes, each against its
     representative) and the bytes k_seg_hash hashes, for a kernel trace of this run to divide by;
(d)  the host, one core: hashlib.blake2b over every segment plus the join for a sample of the
     bodies, OpenSSL's EVP_DigestVerify (and the oracle) over a sample of the witnesses, scaled to
     the whole and over 16 cores; "meets_bar": (a) is faster.
Every figure: median of --reps timed runs after --warmup, with min and max, upload included, the
output arrays reused.  Prints one JSON line."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ouroboros-consensus_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle  # noqa: E402
import praos_hip  # noqa: E402
from praos_hip import blockfetch  # noqa: E402
from txindex_bench import timed  # noqa: E402
from txwit_bench import CORES, HOST_SAMPLE, SPKP, make_chunk, openssl_verifier, signed_blocks  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--txs", type=int, default=40)
    ap.add_argument("--signers", type=int, default=4096)
    ap.add_argument("--peers", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    t0 = time.perf_counter()
    segs = signed_blocks(args.blocks, args.txs, args.signers)
    ctx = praos_hip.Context(0)
    data, boff, bln, _ = make_chunk(ctx, segs)
    n = len(segs)
    wire = [blockfetch.wrap_block(data[int(o):int(o) + int(l)].tobytes()) for o, l in zip(boff, bln)]
    ln = np.array([len(w) for w in wire], np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(wire), np.uint8)
    nt, nw = n * args.txs, 2 * n * args.txs
    out = {"device": torch.cuda.get_device_name(0), "blocks": n, "txs": nt, "witnesses": nw, "wire_bytes": len(arena),
           "block_bytes": len(data), "build_s": round(time.perf_counter() - t0, 1)}
    # the points: what the blocks' own headers say (a first call, asked for nothing that exists)
    one = np.array([0, n], np.uint64)
    _, _, R, *_ = ctx.verify_fetched_blocks(arena, off, ln, one, one, np.zeros(n, np.uint64), np.zeros((n, 32), np.uint8),
                                            witnesses=False)
    slot, hh = R["slot"].copy(), R["header_hash"].copy()

    def run(ar, o, l, first, k, **kw):
        return ctx.verify_fetched_blocks(ar, o, l, first, first, np.tile(slot, k), np.tile(hh, (k, 1)), **kw)
    # ---- (a) one peer, beside the stored-block calls
    I, G, R, B, T, W, counts = run(arena, off, ln, one, 1)
    assert counts == (n, nt, nw) and (I["verdict"] == 0).all() and (I["row"] == np.arange(n)).all() and G["status"][0] == 0
    assert (R["bits"] == 0).all() and (W["ok"] == 1).all() and (B["n_bad"] == 0).all()
    bB, bT, bW, bcounts = ctx.verify_tx_witnesses(data, boff, bln)
    assert bcounts == (nt, nw) and T["tx_id"].tobytes() == bT["tx_id"].tobytes() and W["key_hash"].tobytes() == bW["key_hash"].tobytes()
    res, bh = ctx.verify_block_integrity(data, boff, bln, SPKP)
    assert (res == 0).all() and bh.tobytes() == R["body_hash"].tobytes()
    buf = ctx.fetched_block_buffers(n, 1, n, nt, nw)
    out["one_peer_all"] = a = timed(lambda: run(arena, off, ln, one, 1, out=buf), args.reps, args.warmup)
    out["one_peer_no_witnesses"] = a0 = timed(lambda: run(arena, off, ln, one, 1, witnesses=False, out=buf), args.reps,
                                              args.warmup)
    assert (buf[5]["ok"] == 1).all() and buf[2]["header_hash"].tobytes() == hh.tobytes()
    bbuf = ctx.tx_witness_buffers(n, nt, nw)
    out["stored_tx_witnesses"] = sw = timed(lambda: ctx.verify_tx_witnesses(data, boff, bln, out=bbuf), args.reps, args.warmup)
    out["stored_block_integrity"] = si = timed(lambda: ctx.verify_block_integrity(data, boff, bln, SPKP), args.reps,
                                               args.warmup)
    out["wire_over_stored_sum"] = round(a["median_ms"] / (sw["median_ms"] + si["median_ms"]), 3)
    out["witness_passes_ms_by_subtraction"] = round(a["median_ms"] - a0["median_ms"], 3)
    # ---- (b) the same blocks from each of the peers, every peer its own copy of the bytes
    K = args.peers
    karena = np.tile(arena, K)
    koff = np.concatenate([off + np.uint64(k * len(arena)) for k in range(K)])
    kln = np.tile(ln, K)
    first = np.arange(K + 1, dtype=np.uint64) * np.uint64(n)
    on_ = run(karena, koff, kln, first, K)
    off_ = run(karena, koff, kln, first, K, dedup=False)
    assert on_[6] == (n, nt, nw) and off_[6] == (K * n, K * nt, K * nw)
    assert (on_[0]["row"] == np.tile(np.arange(n, dtype=np.uint32), K)).all() and (off_[0]["row"] == np.arange(K * n)).all()
    same = (on_[0]["verdict"] == off_[0]["verdict"]).all() and (on_[0]["status"] == off_[0]["status"]).all()
    for name in ("tag", "slot", "block_no", "header_hash", "body_hash", "bits", "which", "blk_len"):
        same = same and (on_[2][name][on_[0]["row"]] == off_[2][name]).all()
    for name in ("n_tx", "n_wit", "n_bad", "n_shape"):
        same = same and (on_[3][name][on_[0]["row"]] == off_[3][name]).all()
    out["peers"], out["dedup_identical"] = K, bool(same)
    del on_, off_
    kbuf = ctx.fetched_block_buffers(K * n, K, K * n, K * nt, K * nw)
    out["peers_dedup_on"] = on = timed(lambda: run(karena, koff, kln, first, K, out=kbuf), args.reps, args.warmup)
    out["peers_dedup_on_no_witnesses"] = on0 = timed(lambda: run(karena, koff, kln, first, K, witnesses=False, out=kbuf),
                                                     args.reps, args.warmup)
    out["peers_dedup_off"] = of = timed(lambda: run(karena, koff, kln, first, K, dedup=False, out=kbuf), args.reps,
                                        args.warmup)
    out["peers_dedup_off_no_witnesses"] = of0 = timed(
        lambda: run(karena, koff, kln, first, K, dedup=False, witnesses=False, out=kbuf), args.reps, args.warmup)
    out["dedup_on_over_off"] = round(on["median_ms"] / of["median_ms"], 3)
    out["dedup_on_over_off_no_witnesses"] = round(on0["median_ms"] / of0["median_ms"], 3)
    out["dedup_gate"] = on["median_ms"] < of["median_ms"]
    # ---- (c) what the two kernels read, for a kernel trace to divide by
    out["compare_bytes"] = 2 * (K - 1) * int(bln.sum())             # each duplicate and its representative
    out["seg_hash_bytes"] = int(sum(len(x) for s in segs for x in s))
    ctx.close()
    # ---- (d) the host, one core
    m = min(256, n)
    t1 = time.perf_counter()
    for s in segs[:m]:
        hashlib.blake2b(b"".join(hashlib.blake2b(x, digest_size=32).digest() for x in s), digest_size=32).digest()
    body_ms = 1e3 * (time.perf_counter() - t1) / m * n
    mw = min(HOST_SAMPLE, nw)
    sample = [(bytes(arena[int(W["key_off"][w]):int(W["key_off"][w]) + 32]), bytes(T["tx_id"][int(W["tx"][w])]),
               bytes(arena[int(W["sig_off"][w]):int(W["sig_off"][w]) + 64])) for w in range(0, nw, nw // mw)][:mw]
    host = {"body_hash_ms_one_core": round(body_ms, 1)}
    for name, fn in (("oracle", oracle.ed25519_verify), ("openssl", openssl_verifier())):
        if fn is None:
            continue
        assert all(fn(*s) for s in sample[:64])
        t1 = time.perf_counter()
        for s in sample:
            fn(*s)
        per = (time.perf_counter() - t1) / len(sample)
        host[name] = {"verifies_per_s_one_core": round(1 / per), "all_ms_one_core": round(body_ms + 1e3 * per * nw, 1),
                      f"all_ms_{CORES}_cores": round((body_ms + 1e3 * per * nw) / CORES, 1)}
    out["host"] = host
    best = min(h[f"all_ms_{CORES}_cores"] for h in host.values() if isinstance(h, dict))
    out["host16_over_gpu"] = round(best / a["median_ms"], 2)
    out["meets_bar"] = a["median_ms"] < best
    print(json.dumps(out))


if __name__ == "__main__":
    main()
