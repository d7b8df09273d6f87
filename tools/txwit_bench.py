#!/usr/bin/env python3
"""Key-witness verification throughput on one GPU.

    python tools/txwit_bench.py [--blocks 4096] [--txs 40] [--signers 4096] [--reps 7] [--warmup 2]

The chunk shape of tools/txindex_bench.py: --blocks linked Babbage blocks with genuine headers
(Context.synthesize), --txs transactions each, bodies of 340 bytes with 2 outputs.  Every
transaction carries 2 VKey witnesses genuinely signed over its txId by 2 of --signers keys (signed
once with the oracle; the transactions are cached under /tmp).
(a)  the resident whole call (praos_block_batch_tx_witnesses over an uploaded batch) with every
     array downloaded; (a') the per-block counts only;
(b)  the same batch's index call (every row array) and integrity run, for scale;
(c)  the same witnesses verified on the host, one core: the oracle's ed25519_verify and OpenSSL's
     EVP_DigestVerify over a sample, scaled to the chunk, and that figure over 16 cores;
(d)  the verify stage: (a') less the index's statistics-only call (what is left is the count,
     emit, verify and reduce passes and one round trip), as witnesses/s, beside
     praos_verify_ocert over as many OCerts (uncached k_ocert, its upload included).
Every figure: median of --reps timed runs after --warmup, with min and max.  Prints one JSON
line; "meets_bar": (a) is faster than the faster host figure of (c) over 16 cores."""
import argparse
import ctypes
import ctypes.util
import hashlib
import json
import os
import pickle
import random
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
from praos_hip import abi, chunk  # noqa: E402
import tx_corpus as tc  # noqa: E402
from txindex_bench import timed  # noqa: E402

SPKP = 129600
HOST_SAMPLE = 16384
CORES = 16


def signed_blocks(n, txs, signers):
    """-> per block its segments [s1, s2, s3, s4]; cached under /tmp"""
    path = f"/tmp/txwit_bench_{n}_{txs}_{signers}.pickle"
    if os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    r = random.Random(0x7A2)
    seeds = [tc.rb(r, 32) for _ in range(signers)]
    pks = [oracle.ed25519_pk(s) for s in seeds]
    out = []
    for _ in range(n):
        bodies, wits = [], []
        for _ in range(txs):
            body = tc.body(r, n_out=2, body_len=340)
            tid = hashlib.blake2b(body, digest_size=32).digest()
            items = []
            for k in r.sample(range(signers), 2):
                items.append(b"\x82\x58\x20" + pks[k] + b"\x58\x40" + oracle.ed25519_sign(seeds[k], tid))
            bodies.append(body)
            wits.append(b"\xa1\x00\x82" + b"".join(items))
        out.append([tc.seq(4, bodies, False), tc.seq(4, wits, False), tc.hd(5, 0), tc.hd(4, 0)])
    with open(path, "wb") as f:
        pickle.dump(out, f)
    return out


def make_chunk(ctx, segs):
    n = len(segs)
    bh = np.frombuffer(b"".join(chunk.hash_tx_seq(s) for s in segs), np.uint8).reshape(n, 32)
    p = abi.params(slots_per_kes_period=SPKP, max_kes_evo=62)
    eta0 = hashlib.blake2b(b"bench-txwit", digest_size=32).digest()
    H, _, _ = ctx.synthesize(n, 100, p, eta0, b"\xc4" * 32, slot_stride=20, body_len=0, body_hash=bh, link=True)
    body = H["body_bytes"]
    parts, off, ln, pos = [], np.zeros(n, np.uint64), np.zeros(n, np.uint32), 0
    for i in range(n):
        bo, bl = int(H["body_off"][i]), int(H["body_len"][i])
        blk = b"".join([chunk.BLOCK_PREFIX, chunk.HEADER_PREFIX, body[bo:bo + bl].tobytes(), chunk.SIG_HEAD,
                        H["kes_sig"][i].tobytes(), *segs[i]])
        parts.append(blk)
        off[i], ln[i] = pos, len(blk)
        pos += len(blk)
    return np.frombuffer(b"".join(parts), np.uint8), off, ln, H


def openssl_verifier():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    C = ctypes.CDLL(name)
    C.EVP_PKEY_new_raw_public_key.restype = ctypes.c_void_p
    C.EVP_PKEY_new_raw_public_key.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    C.EVP_MD_CTX_new.restype = ctypes.c_void_p
    C.EVP_DigestVerifyInit.argtypes = [ctypes.c_void_p] * 5
    C.EVP_DigestVerify.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    C.EVP_MD_CTX_free.argtypes = [ctypes.c_void_p]
    C.EVP_PKEY_free.argtypes = [ctypes.c_void_p]

    def verify(pk, msg, sig):
        key = C.EVP_PKEY_new_raw_public_key(1087, None, pk, 32)          # EVP_PKEY_ED25519
        md = C.EVP_MD_CTX_new()
        C.EVP_DigestVerifyInit(md, None, None, None, key)
        ok = C.EVP_DigestVerify(md, sig, 64, msg, 32) == 1
        C.EVP_MD_CTX_free(md)
        C.EVP_PKEY_free(key)
        return ok
    return verify


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--txs", type=int, default=40)
    ap.add_argument("--signers", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    t0 = time.perf_counter()
    segs = signed_blocks(args.blocks, args.txs, args.signers)
    ctx = praos_hip.Context(0)
    n = args.blocks
    data, off, ln, H = make_chunk(ctx, segs)
    nt, nw = n * args.txs, 2 * n * args.txs
    out = {"device": torch.cuda.get_device_name(0), "blocks": n, "txs": nt, "witnesses": nw, "bytes": len(data),
           "build_s": round(time.perf_counter() - t0, 1)}
    b = ctx.upload_blocks(data, off, ln)
    try:
        B, T, W, counts = ctx.tx_witnesses_blocks(b, n)
        assert counts == (nt, nw) and (B["status"] == 0).all() and (B["n_wit"] == 2 * args.txs).all()
        assert (B["n_bad"] == 0).all() and (W["ok"] == 1).all() and (T["status"] == 0).all()
        kview = np.lib.stride_tricks.sliding_window_view(data, 32)[W["key_off"].astype(np.int64)]
        assert bytes(W["key_hash"][7]) == hashlib.blake2b(kview[7].tobytes(), digest_size=28).digest()
        out["distinct_keys"] = int(len(np.unique(kview, axis=0)))
        buf = ctx.tx_witness_buffers(n, nt, nw)            # the caller's output arrays, reused call after call
        buf0 = ctx.tx_witness_buffers(n, 0, 0, rows=False)
        out["witnesses_all_arrays"] = a = timed(lambda: ctx.tx_witnesses_blocks(b, n, out=buf), args.reps, args.warmup)
        out["witnesses_counts_only"] = a0 = timed(lambda: ctx.tx_witnesses_blocks(b, n, rows=False, out=buf0),
                                                  args.reps, args.warmup)
        assert (buf[2]["ok"] == 1).all() and (buf0[0]["n_wit"] == B["n_wit"]).all()
        out["slices_65536"] = timed(lambda: ctx.tx_witnesses_blocks(b, n, rows=False, out=buf0, max_lanes=65536),
                                    args.reps, 1)
        ibuf = ctx.tx_index_buffers(n, nt)
        ibuf0 = ctx.tx_index_buffers(n, 0, rows=False)
        out["index_rows"] = timed(lambda: ctx.tx_index_blocks(b, n, cap=nt, out=ibuf), args.reps, args.warmup)
        out["index_stats_only"] = i0 = timed(lambda: ctx.tx_index_blocks(b, n, rows=False, cap=0, out=ibuf0),
                                             args.reps, args.warmup)

        def integrity():
            ctx.run_blocks(b, SPKP)
            return ctx.download_blocks(b, n)
        res, _ = integrity()
        assert (res == 0).all(), "the synthetic blocks are intact"
        out["integrity"] = timed(integrity, args.reps, args.warmup)
    finally:
        ctx.free(b)
    # (d) the verify stage beside the uncached OCert verifies of as many certificates
    stage_ms = a0["median_ms"] - i0["median_ms"]
    out["verify_stage_ms"] = round(stage_ms, 3)
    out["verify_stage_wits_per_s"] = round(nw / stage_ms * 1e3)
    # the statistics-only index hashes no transaction id, which the witness call does: the index with
    # every row array (and their download, which the witness call does not make) bounds it from below
    out["verify_stage_ms_low"] = round(a0["median_ms"] - out["index_rows"]["median_ms"], 3)
    reps = -(-nw // n)
    oc = [np.ascontiguousarray(np.tile(H[k], (reps,) + (1,) * (H[k].ndim - 1))[:nw])
          for k in ("cold_vk", "hot_vk", "ocert_n", "ocert_c0", "ocert_sig")]
    ok = ctx.verify_ocert(*oc)
    assert (ok == 1).all()
    out["ocert_uncached_call"] = o = timed(lambda: ctx.verify_ocert(*oc), args.reps, args.warmup)
    out["ocert_uncached_sigs_per_s"] = round(nw / o["median_ms"] * 1e3)
    ctx.close()
    # (c) the host, one core, over a sample of the same witnesses
    m = min(HOST_SAMPLE, nw)
    sample = [(bytes(data[int(W["key_off"][w]):int(W["key_off"][w]) + 32]), bytes(T["tx_id"][int(W["tx"][w])]),
               bytes(data[int(W["sig_off"][w]):int(W["sig_off"][w]) + 64])) for w in range(0, nw, nw // m)][:m]
    host = {}
    for name, fn in (("oracle", oracle.ed25519_verify), ("openssl", openssl_verifier())):
        if fn is None:
            continue
        assert all(fn(*s) for s in sample[:64])
        t1 = time.perf_counter()
        for s in sample:
            fn(*s)
        per = (time.perf_counter() - t1) / len(sample)
        host[name] = {"verifies_per_s_one_core": round(1 / per), "chunk_ms_one_core": round(1e3 * per * nw, 1),
                      f"chunk_ms_{CORES}_cores": round(1e3 * per * nw / CORES, 1)}
    out["host"] = host
    best = min(h[f"chunk_ms_{CORES}_cores"] for h in host.values())
    out["host16_over_gpu"] = round(best / a["median_ms"], 2)
    out["meets_bar"] = a["median_ms"] < best
    print(json.dumps(out))


if __name__ == "__main__":
    main()
