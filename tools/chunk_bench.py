#!/usr/bin/env python3
"""CRC-32 and chunk-validation throughput on one GPU ("Chunk validation on the GPU").

    python tools/chunk_bench.py [--mb 256] [--blocks 4096] [--payload 16384] [--reps 7] [--warmup 2]

(a) Resident CRC-32 (praos_block_batch_crc32: the two kernels of k_crc32.hip plus the download of
    4 bytes per span) over --mb megabytes cut into spans of 1 KB, 16 KB and 90 KB; beside it
    zlib.crc32 over the same bytes on one core of this box (what computeCRC costs the reference
    per core) and a device-to-device copy of the same bytes (the bandwidth ceiling: it reads and
    writes every byte, the CRC only reads).
(b) praos_validate_chunk end to end, upload included, on a healthy chunk (--blocks intact blocks
    of --payload bytes with the right checksums and offsets in the index), beside the host
    computing that chunk's CRCs with zlib: all that validating a healthy chunk costs without it.
Every figure: median of --reps timed runs after --warmup, with min and max (the box's spread).
Prints one JSON line.

    python tools/chunk_bench.py --byron [--blocks 2048] [--payload 16384] [--reps 5]

(c) Byron instead of (a) and (b): a healthy forged Byron chunk (tests/byron_corpus.py: an EBB, then
    --blocks main blocks of 8 transactions each, right index) end to end through
    praos_validate_chunk_cfg, beside the Shelley chunk of the same byte size from the same run;
    and the same Byron chunk without an index, where every block takes the PBFT signature and
    the body proof (k_byron_integrity, one lane per block), in blocks per second.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ouroboros-consensus_amd"))
import praos_hip  # noqa: E402
from praos_hip import abi, chunk  # noqa: E402

SPKP = 129600


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


def gbps(nbytes, r):
    return round(nbytes / (r["median_ms"] * 1e-3) / 1e9, 2)


def shelley_chunk(ctx, rng, n, pl):
    """(bytes, offsets, lengths, CRCs) of n intact linked Babbage blocks of pl payload bytes."""
    pay = rng.integers(0, 256, size=(n, pl), dtype=np.uint8)
    payloads = [pay[i].tobytes() for i in range(n)]
    bh = np.frombuffer(b"".join(chunk.hash_tx_seq((chunk.tx_segment(p),) + chunk.SEG_FIXED) for p in payloads),
                       np.uint8).reshape(n, 32)
    p = abi.params(slots_per_kes_period=SPKP, max_kes_evo=62)
    eta0 = hashlib.blake2b(b"bench-chunk", digest_size=32).digest()
    H, _, _ = ctx.synthesize(n, 100, p, eta0, b"\xc4" * 32, slot_stride=20, body_len=0, body_hash=bh, link=True)
    data, off, ln = chunk.pack_blocks(H, payloads)
    data = np.ascontiguousarray(data)
    braw = data.tobytes()
    crc = np.array([zlib.crc32(braw[int(o):int(o) + int(k)]) for o, k in zip(off, ln)], np.uint32)
    return data, off, ln, crc


def byron_chunk(rng, n, per_block):
    """An EBB and n linked main blocks of about per_block bytes (8 transactions each), forged by
    tests/byron_corpus.py; -> (bytes, offsets, CRCs, (epoch_slots, protocol_magic))."""
    for d in ("tests", "oracle"):
        sys.path.insert(0, os.path.join(ROOT, d))
    import random
    import byron_corpus as bc
    r = random.Random(7)
    dlg = bc.Delegate(r)
    es = n + 1
    ebb = bc.EBB(r, bytes(32), 0, 0)
    blobs, prev = [ebb.bytes], ebb.header_hash
    H = bc.H
    probe = bc.Main(r, dlg, prev, 0, 0, 1, (1,) * 8)
    txlen = max(1, (per_block - len(probe.bytes)) // 8)
    raw = rng.integers(0, 256, size=(n, 8, txlen), dtype=np.uint8)
    for i in range(n):
        b = bc.Main(r, dlg, prev, 0, i, i + 1)
        b.txs = [(H(2, txlen) + raw[i, k].tobytes(), H(4, 1) + H(2, 64) + raw[i, k, :64].tobytes().ljust(64, b"\0"))
                 for k in range(8)]
        blobs.append(b.sign().bytes)
        prev = b.header_hash
    off = np.cumsum([0] + [len(b) for b in blobs[:-1]]).astype(np.uint64)
    crc = np.array([zlib.crc32(b) for b in blobs], np.uint32)
    return np.frombuffer(b"".join(blobs), np.uint8), off, crc, (es, bc.PM)


def byron_main(args):
    import torch
    rng = np.random.default_rng(0xB7)
    ctx = praos_hip.Context(0)
    n = args.blocks
    sdata, soff, _, scrc = shelley_chunk(ctx, rng, n + 1, args.payload)
    bdata, boff, bcrc, byron = byron_chunk(rng, n, len(sdata) // (n + 1))
    out = {"device": torch.cuda.get_device_name(0), "blocks": n + 1, "byron_bytes": len(bdata),
           "shelley_bytes": len(sdata)}
    res = ctx.validate_chunk(bdata, bcrc, boff, SPKP, byron=byron)
    assert (res["outcome"], res["blocks"], res["checked"]) == (abi.CHUNK_OK, n + 1, 0), res["outcome"]
    res = ctx.validate_chunk(sdata, scrc, soff, SPKP, byron=byron)
    assert (res["outcome"], res["blocks"], res["checked"]) == (abi.CHUNK_OK, n + 1, 0), res["outcome"]
    rb = timed(lambda: ctx.validate_chunk(bdata, bcrc, boff, SPKP, cap=n + 1, byron=byron), args.reps, args.warmup)
    rs = timed(lambda: ctx.validate_chunk(sdata, scrc, soff, SPKP, cap=n + 1, byron=byron), args.reps, args.warmup)
    rs0 = timed(lambda: ctx.validate_chunk(sdata, scrc, soff, SPKP, cap=n + 1), args.reps, args.warmup)
    out["healthy"] = {"byron": dict(rb, GBps=gbps(len(bdata), rb)), "shelley": dict(rs, GBps=gbps(len(sdata), rs)),
                      "shelley_byron_off": dict(rs0, GBps=gbps(len(sdata), rs0))}
    res = ctx.validate_chunk(bdata, None, None, SPKP, byron=byron)
    assert (res["outcome"], res["blocks"], res["checked"]) == (abi.CHUNK_OK, n + 1, n + 1), res["outcome"]
    ru = timed(lambda: ctx.validate_chunk(bdata, None, None, SPKP, cap=n + 1, byron=byron), args.reps, args.warmup)
    # the index's offsets with stale checksums: every block checked, no host walk
    ru2 = timed(lambda: ctx.validate_chunk(bdata, bcrc ^ np.uint32(1), boff, SPKP, cap=n + 1, byron=byron), args.reps,
                args.warmup)
    out["all_untrusted"] = {"no_index": dict(ru, blocks_per_s=round((n + 1) / (ru["median_ms"] * 1e-3))),
                            "stale_index": dict(ru2, blocks_per_s=round((n + 1) / (ru2["median_ms"] * 1e-3)))}
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--byron", action="store_true")
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=None)
    ap.add_argument("--payload", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    args.blocks = args.blocks or (2048 if args.byron else 4096)
    args.reps = args.reps or (5 if args.byron else 7)
    if args.byron:
        return byron_main(args)
    import torch
    rng = np.random.default_rng(0xC4C)
    total = args.mb << 20
    arena = rng.integers(0, 256, size=total, dtype=np.uint8)
    raw = arena.tobytes()
    ctx = praos_hip.Context(0)
    out = {"bytes": total, "device": torch.cuda.get_device_name(0), "crc": {}}
    src = torch.from_numpy(arena).cuda()
    dst = torch.empty_like(src)

    def d2d():
        dst.copy_(src)
        torch.cuda.synchronize()
    r = timed(d2d, args.reps, args.warmup)
    out["d2d_copy"] = dict(r, GBps=gbps(total, r))
    del src, dst
    for span in (1 << 10, 16 << 10, 90_000):
        n = total // span
        off = (np.arange(n, dtype=np.uint64) * np.uint64(span))
        ln = np.full(n, span, np.uint32)
        b = ctx.upload_blocks(arena, off, ln)
        try:
            got = ctx.crc32_blocks(b, n)
            r = timed(lambda: ctx.crc32_blocks(b, n), args.reps, args.warmup)
        finally:
            ctx.free(b)
        want = None

        def host():
            nonlocal want
            want = [zlib.crc32(raw[o:o + span]) for o in range(0, n * span, span)]
        rh = timed(host, min(args.reps, 3), 1)
        assert (got == np.array(want, np.uint32)).all(), f"CRC mismatch at span {span}"
        out["crc"][str(span)] = {"spans": n, "gpu": dict(r, GBps=gbps(n * span, r)),
                                 "zlib_one_core": dict(rh, GBps=gbps(n * span, rh))}
    # (b) a healthy chunk: intact blocks, right index
    n, pl = args.blocks, args.payload
    data, off, ln, crc = shelley_chunk(ctx, rng, n, pl)
    braw = data.tobytes()
    res = ctx.validate_chunk(data, crc, off, SPKP)
    assert (res["outcome"], res["blocks"], res["checked"]) == (abi.CHUNK_OK, n, 0), \
        (res["outcome"], res["blocks"], res["checked"], res["truncate_at"])
    r = timed(lambda: ctx.validate_chunk(data, crc, off, SPKP, cap=n), args.reps, args.warmup)
    spans = [(int(o), int(o) + int(k)) for o, k in zip(off, ln)]
    rh = timed(lambda: [zlib.crc32(braw[a:e]) for a, e in spans], args.reps, 1)
    rn = timed(lambda: ctx.validate_chunk(data, None, None, SPKP, cap=n), min(args.reps, 3), 1)
    out["validate_chunk"] = {"blocks": n, "bytes": len(braw), "gpu_end_to_end": dict(r, GBps=gbps(len(braw), r)),
                             "host_zlib_crc_pass": dict(rh, GBps=gbps(len(braw), rh)),
                             "gpu_no_index": dict(rn, GBps=gbps(len(braw), rn)),
                             "meets_bar": r["median_ms"] <= rh["median_ms"]}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
