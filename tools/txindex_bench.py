#!/usr/bin/env python3
"""Transaction-index throughput on one GPU.

    python tools/txindex_bench.py [--blocks 4096] [--txs 40] [--body 340] [--wit 100] [--reps 7] [--warmup 2]

A synthetic mainnet-shaped chunk: --blocks linked Babbage blocks with genuine headers
(Context.synthesize), --txs transactions each, bodies of --body bytes with 2 outputs, witness
sets of --wit bytes, one transaction in eight with auxiliary data (64 distinct blocks' worth of
transactions, repeated under different headers).
(a) the resident index (praos_block_batch_tx_index over an uploaded batch, downloads included):
    with every row array (transaction ids hashed) and statistics only;
(b) the same batch's resident integrity run (praos_block_batch_run + download) and CRC pass
    (praos_block_batch_crc32): what the index adds per chunk;
(c) one host core walking the same items -- every segment's top level, each body's map up to key
    1, each witness set's map -- with chunk_scan.hpp's item skip over the same bytes, compiled
    here with g++ -O2: the least a CPU implementation must do (it hashes nothing).
Every figure: median of --reps timed runs after --warmup, with min and max.  Prints one JSON
line; "meets_bar": (a) with every row array is faster than (c)."""
import argparse
import ctypes
import hashlib
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ouroboros-consensus_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import praos_hip  # noqa: E402
from praos_hip import abi, chunk  # noqa: E402
import tx_corpus as tc  # noqa: E402

SPKP = 129600

HOST_WALK = r"""
#include "chunk_scan.hpp"
using namespace chunk_scan;
static bool open_lvl(Cur& c, uint32_t want, uint64_t& left, bool& indef) {
  uint32_t mt, ai;
  return head(c, mt, ai, left, indef) && mt == want;
}
static bool more(Cur& c, uint64_t& left, bool indef) {
  if (indef) { if (c.p < c.end && c.a[c.p] == 0xFF) { c.p++; return false; } return c.p < c.end; }
  if (!left) return false;
  left--;
  return true;
}
static bool skip(Cur& c) {
  const int64_t e = chunk_item_end(c.a, c.p, c.end);
  if (e < 0) return false;
  c.p = (uint64_t)e;
  return true;
}
// the value under the first unsigned key `want` of the map at [s, e): its item count when an array
static bool key_count(const uint8_t* a, uint64_t s, uint64_t e, uint64_t want, uint64_t& cnt) {
  Cur c{a, s, e};
  uint64_t left; bool indef;
  if (!open_lvl(c, 5, left, indef)) return true;
  while (more(c, left, indef)) {
    const uint64_t ks = c.p;
    uint32_t mt, ai; uint64_t arg; bool ki;
    if (!head(c, mt, ai, arg, ki)) return false;
    if (mt == 0 && arg == want) {
      uint64_t n; bool ni;
      if (!open_lvl(c, 4, n, ni)) return true;
      if (!ni) { cnt = n; return true; }
      while (more(c, n, ni)) { if (!skip(c)) return false; cnt++; }
      return true;
    }
    if (mt > 1) { c.p = ks; if (!skip(c)) return false; }
    if (!skip(c)) return false;
  }
  return true;
}
extern "C" int txi_host_walk(const uint8_t* a, const uint64_t* off, const uint32_t* len, size_t n, uint32_t* n_tx,
                             uint64_t* n_out, uint64_t* txs_size) {
  for (size_t i = 0; i < n; i++) {
    Cur c{a, off[i], off[i] + len[i]};
    uint32_t mt, ai; uint64_t arg, left; bool indef;
    if (!head(c, mt, ai, arg, indef) || mt != 4 || arg != 2) return -1;      // [tag, [header, s1..s4]]
    if (!head(c, mt, ai, arg, indef) || mt != 0) return -1;
    if (!head(c, mt, ai, arg, indef) || mt != 4 || arg != 5) return -1;
    if (!skip(c)) return -1;                                                 // the header
    uint64_t ntx = 0, nout = 0, size = 0;
    if (!open_lvl(c, 4, left, indef)) return -1;                             // s1: bodies
    while (more(c, left, indef)) {
      const uint64_t s = c.p;
      if (!skip(c)) return -1;
      uint64_t k = 0;
      if (!key_count(a, s, c.p, 1, k)) return -1;
      nout += k;
      size += 2 + (c.p - s);
      ntx++;
    }
    if (!open_lvl(c, 4, left, indef)) return -1;                             // s2: witness sets
    while (more(c, left, indef)) {
      const uint64_t s = c.p;
      if (!skip(c)) return -1;
      uint64_t k = 0;
      if (!key_count(a, s, c.p, 5, k)) return -1;
      size += c.p - s;
    }
    if (!open_lvl(c, 5, left, indef)) return -1;                             // s3: index -> aux
    while (more(c, left, indef)) {
      bool ki;
      if (!head(c, mt, ai, arg, ki) || mt != 0) return -1;
      const uint64_t s = c.p;
      if (!skip(c)) return -1;
      size += c.p - s - 1;
    }
    if (!skip(c) || c.p != c.end) return -1;                                 // s4
    n_tx[i] = (uint32_t)ntx; n_out[i] = nout; txs_size[i] = size;
  }
  return 0;
}
"""


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return {"median_ms": round(1e3 * statistics.median(t), 3), "min_ms": round(1e3 * min(t), 3),
            "max_ms": round(1e3 * max(t), 3)}


def make_chunk(ctx, n, txs, body_len, wit_len):
    r = random.Random(0x7A1)
    kinds = []
    for _ in range(64):
        bodies = [tc.body(r, n_out=2, body_len=body_len) for _ in range(txs)]
        wits = [tc.witness(r, size=wit_len) for _ in range(txs)]
        aux = [(k, tc.bstr(r, 60)) for k in range(0, txs, 8)]
        kinds.append([tc.seq(4, bodies, False), tc.seq(4, wits, False),
                      tc.seq(5, [(tc.hd(0, k), v) for k, v in aux], False), tc.hd(4, 0)])
    bh = np.frombuffer(b"".join(chunk.hash_tx_seq(kinds[i % 64]) for i in range(n)), np.uint8).reshape(n, 32)
    p = abi.params(slots_per_kes_period=SPKP, max_kes_evo=62)
    eta0 = hashlib.blake2b(b"bench-txindex", digest_size=32).digest()
    H, _, _ = ctx.synthesize(n, 100, p, eta0, b"\xc4" * 32, slot_stride=20, body_len=0, body_hash=bh, link=True)
    body = H["body_bytes"]
    parts, off, ln, pos = [], np.zeros(n, np.uint64), np.zeros(n, np.uint32), 0
    for i in range(n):
        bo, bl = int(H["body_off"][i]), int(H["body_len"][i])
        blk = b"".join([chunk.BLOCK_PREFIX, chunk.HEADER_PREFIX, body[bo:bo + bl].tobytes(), chunk.SIG_HEAD,
                        H["kes_sig"][i].tobytes(), *kinds[i % 64]])
        parts.append(blk)
        off[i], ln[i] = pos, len(blk)
        pos += len(blk)
    return np.frombuffer(b"".join(parts), np.uint8), off, ln


def host_walker(tmp):
    src = os.path.join(tmp, "txi_host_walk.cpp")
    with open(src, "w") as f:
        f.write(HOST_WALK)
    so = os.path.join(tmp, "txi_host_walk.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I",
                    os.path.join(ROOT, "ouroboros-consensus_amd", "csrc"), src, "-o", so], check=True)
    fn = ctypes.CDLL(so).txi_host_walk
    fn.restype = ctypes.c_int
    fn.argtypes = [abi.u8p, abi.u64p, abi.u32p, ctypes.c_size_t, abi.u32p, abi.u64p, abi.u64p]
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--txs", type=int, default=40)
    ap.add_argument("--body", type=int, default=340)
    ap.add_argument("--wit", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    ctx = praos_hip.Context(0)
    n = args.blocks
    data, off, ln = make_chunk(ctx, n, args.txs, args.body, args.wit)
    out = {"device": torch.cuda.get_device_name(0), "blocks": n, "txs": n * args.txs, "bytes": len(data)}
    b = ctx.upload_blocks(data, off, ln)
    try:
        st, rw = ctx.tx_index_blocks(b, n)
        assert (st["status"] == 0).all() and (st["n_tx"] == args.txs).all() and len(rw["block"]) == n * args.txs
        assert (st["n_out"] == 2 * args.txs).all()
        k = int(rw["body_off"][17]), int(rw["body_len"][17])
        assert bytes(rw["tx_id"][17]) == hashlib.blake2b(data[k[0]:k[0] + k[1]].tobytes(), digest_size=32).digest()
        cap = n * args.txs
        buf = ctx.tx_index_buffers(n, cap)            # the caller's output arrays, reused call after call
        buf0 = ctx.tx_index_buffers(n, 0, rows=False)
        a = {"rows": timed(lambda: ctx.tx_index_blocks(b, n, cap=cap, out=buf), args.reps, args.warmup),
             "stats_only": timed(lambda: ctx.tx_index_blocks(b, n, rows=False, cap=0, out=buf0), args.reps,
                                 args.warmup)}
        assert all((buf[1][k][:cap] == rw[k]).all() for k in rw) and (buf0[0]["n_out"] == st["n_out"]).all()
        out["index"] = a

        def integrity():
            ctx.run_blocks(b, SPKP)
            return ctx.download_blocks(b, n)
        res, _ = integrity()
        assert (res == 0).all(), "the synthetic blocks are intact"
        out["integrity"] = timed(integrity, args.reps, args.warmup)
        out["crc"] = timed(lambda: ctx.crc32_blocks(b, n), args.reps, args.warmup)
    finally:
        ctx.free(b)
    with tempfile.TemporaryDirectory() as tmp:
        walk = host_walker(tmp)
        h_ntx, h_out, h_size = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)

        def host():
            rc = walk(abi.ptr(data), abi.ptr(off, abi.u64p), abi.ptr(ln, abi.u32p), n, abi.ptr(h_ntx, abi.u32p),
                      abi.ptr(h_out, abi.u64p), abi.ptr(h_size, abi.u64p))
            assert rc == 0
        out["host_one_core_walk"] = timed(host, args.reps, 1)
        assert (h_ntx == st["n_tx"]).all() and (h_out == st["n_out"]).all() and (h_size == st["txs_size"]).all()
    out["host_over_index"] = round(out["host_one_core_walk"]["median_ms"] / a["rows"]["median_ms"], 2)
    out["meets_bar"] = a["rows"]["median_ms"] < out["host_one_core_walk"]["median_ms"]
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
