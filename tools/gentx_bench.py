#!/usr/bin/env python3
"""Wire-transaction verification throughput on one GPU.

    python tools/gentx_bench.py [--blocks 4096] [--txs 40] [--signers 4096] [--peers 4] [--reps 7] [--warmup 2]

The workload of tools/txwit_bench.py taken out of its blocks: --blocks x --txs Babbage
transactions, bodies of 340 bytes, 2 genuine VKey witnesses each (the same cached transactions),
each wrapped as a wire GenTx of era index 5.
(a)  the distinct items in one call (praos_verify_gen_txs, every array downloaded), and the same
     transactions as --blocks stored blocks through praos_verify_tx_witnesses (upload included in
     both), with the per-item arrays only for scale;
(b)  every transaction offered by --peers peers (peer after peer): dedup on and dedup off;
     "dedup_gate": on is less than half of off;
(c)  the distinct witnesses on the host, one core: OpenSSL's EVP_DigestVerify (and the oracle)
     over a sample, scaled to the whole and over 16 cores; "meets_bar": (a) is faster.
Every figure: median of --reps timed runs after --warmup, with min and max.  Prints one JSON line."""
import argparse
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
from praos_hip import txsubmission  # noqa: E402
import tx_index_model as tm  # noqa: E402
from txindex_bench import timed  # noqa: E402
from txwit_bench import CORES, HOST_SAMPLE, make_chunk, openssl_verifier, signed_blocks  # noqa: E402

ERA = 5     # Babbage's wire index


def items_of(seg):
    """the (body, witness set) pairs of one block's segments [s1, s2, ...]"""
    bodies = [seg[0][s:e] for s, e in tm._items(seg[0], 0, len(seg[0]), 4)]
    wits = [seg[1][s:e] for s, e in tm._items(seg[1], 0, len(seg[1]), 4)]
    return zip(bodies, wits)


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
    wire = [txsubmission.wrap_gen_tx(ERA, b"\x84" + body + wits + b"\xf5\xf6") for s in segs for body, wits in items_of(s)]
    n = len(wire)
    ln = np.array([len(t) for t in wire], np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(wire), np.uint8)
    ctx = praos_hip.Context(0)
    data, boff, bln, _ = make_chunk(ctx, segs)
    nw = 2 * n
    out = {"device": torch.cuda.get_device_name(0), "txs": n, "witnesses": nw, "wire_bytes": len(arena),
           "block_bytes": len(data), "build_s": round(time.perf_counter() - t0, 1)}
    # ---- (a) distinct items, beside the same transactions as stored blocks
    I, T, W, counts = ctx.verify_gen_txs(arena, off, ln)
    assert counts == (n, nw) and (I["status"] == 0).all() and (I["row"] == np.arange(n)).all()
    assert (W["ok"] == 1).all() and (T["wstatus"] == 0).all() and (T["n_bad"] == 0).all()
    B, bT, bW, bcounts = ctx.verify_tx_witnesses(data, boff, bln)
    assert bcounts == counts and T["tx_id"].tobytes() == bT["tx_id"].tobytes() and (bW["ok"] == 1).all()
    assert W["key_hash"].tobytes() == bW["key_hash"].tobytes()
    # the caller's output arrays, reused call after call (fresh ones would be page-faulted in by every download)
    buf, buf0 = ctx.gen_tx_buffers(n, n, nw), ctx.gen_tx_buffers(n, 0, 0, rows=False)
    bbuf, bbuf0 = ctx.tx_witness_buffers(len(segs), n, nw), ctx.tx_witness_buffers(len(segs), 0, 0, rows=False)
    out["distinct_all_arrays"] = a = timed(lambda: ctx.verify_gen_txs(arena, off, ln, out=buf), args.reps, args.warmup)
    out["distinct_items_only"] = timed(lambda: ctx.verify_gen_txs(arena, off, ln, rows=False, out=buf0), args.reps,
                                       args.warmup)
    assert (buf[2]["ok"] == 1).all() and buf[1]["tx_id"].tobytes() == T["tx_id"].tobytes()
    out["blocks_all_arrays"] = blk = timed(lambda: ctx.verify_tx_witnesses(data, boff, bln, out=bbuf), args.reps,
                                           args.warmup)
    out["blocks_counts_only"] = timed(lambda: ctx.verify_tx_witnesses(data, boff, bln, rows=False, out=bbuf0), args.reps,
                                      args.warmup)
    out["gentx_over_blocks"] = round(a["median_ms"] / blk["median_ms"], 3)
    # ---- (b) every transaction offered by each of the peers
    K = args.peers
    koff, kln = np.tile(off, K), np.tile(ln, K)
    I4, T4, _, c4 = ctx.verify_gen_txs(arena, koff, kln)
    assert c4 == counts and (I4["row"] == np.tile(np.arange(n, dtype=np.uint32), K)).all()
    assert T4["tx_id"].tobytes() == T["tx_id"].tobytes()
    out["peers"] = K
    kbuf, kbuf0 = ctx.gen_tx_buffers(K * n, n, nw), ctx.gen_tx_buffers(K * n, 0, 0, rows=False)
    out["peers_dedup_on"] = on = timed(lambda: ctx.verify_gen_txs(arena, koff, kln, out=kbuf), args.reps, args.warmup)
    out["peers_dedup_on_items_only"] = on0 = timed(lambda: ctx.verify_gen_txs(arena, koff, kln, rows=False, out=kbuf0),
                                                   args.reps, args.warmup)
    assert (kbuf[2]["ok"] == 1).all() and (kbuf[0]["row"] == I4["row"]).all()
    del kbuf
    kbuf = ctx.gen_tx_buffers(K * n, K * n, K * nw)
    out["peers_dedup_off"] = offt = timed(lambda: ctx.verify_gen_txs(arena, koff, kln, dedup=False, out=kbuf), args.reps,
                                          args.warmup)
    out["peers_dedup_off_items_only"] = off0 = timed(
        lambda: ctx.verify_gen_txs(arena, koff, kln, dedup=False, rows=False, out=kbuf0), args.reps, args.warmup)
    assert (kbuf[2]["ok"] == 1).all() and (kbuf[0]["row"] == np.arange(K * n)).all()
    out["dedup_on_over_off_items_only"] = round(on0["median_ms"] / off0["median_ms"], 3)
    out["dedup_on_over_off"] = round(on["median_ms"] / offt["median_ms"], 3)
    out["dedup_gate"] = on["median_ms"] < 0.5 * offt["median_ms"]
    ctx.close()
    # ---- (c) the host, one core, over a sample of the distinct witnesses
    m = min(HOST_SAMPLE, nw)
    sample = [(bytes(arena[int(W["key_off"][w]):int(W["key_off"][w]) + 32]), bytes(T["tx_id"][int(W["tx"][w])]),
               bytes(arena[int(W["sig_off"][w]):int(W["sig_off"][w]) + 64])) for w in range(0, nw, nw // m)][:m]
    host = {}
    for name, fn in (("oracle", oracle.ed25519_verify), ("openssl", openssl_verifier())):
        if fn is None:
            continue
        assert all(fn(*s) for s in sample[:64])
        t1 = time.perf_counter()
        for s in sample:
            fn(*s)
        per = (time.perf_counter() - t1) / len(sample)
        host[name] = {"verifies_per_s_one_core": round(1 / per), "all_ms_one_core": round(1e3 * per * nw, 1),
                      f"all_ms_{CORES}_cores": round(1e3 * per * nw / CORES, 1)}
    out["host"] = host
    best = min(h[f"all_ms_{CORES}_cores"] for h in host.values())
    out["host16_over_gpu"] = round(best / a["median_ms"], 2)
    out["meets_bar"] = a["median_ms"] < best
    print(json.dumps(out))


if __name__ == "__main__":
    main()
