#!/usr/bin/env python3
"""bench.py -- Praos header-crypto validation throughput on MI355X.

Metric (BASELINE.json): Praos headers validated/sec (VRF + KES + OCert + leader).
Default workload (no flags) = configs[4], a mainnet-shaped epoch replay: the first
432,000 blocks of a leader-valid Praos (Babbage) chain -- 3000 pools with stake
sigma_i ~ 1/(i+10) (exact rationals), f = 1/20, one epoch nonce, slotsPerKESPeriod
129600, maxKESEvo 62 -- forged first-leader-wins exactly as db-synthesizer does
(Forging.hs:139-148; schedule shipped in praos_hip/data/c5_schedule.npz, see
praos_hip/chains.py), with canonical HeaderBody CBOR bodies as KES messages and 1 %
of the headers corrupted by the consensus-testlib +1-byte model.  The headers are
signed on the GPU (real Ed25519 / Sum6KES / ECVRF-draft03) and resident in HBM
before the timed region.  One step = one full validation pass (all kernels) over
the GPU's shard.  Multi-GPU: one process per GPU, no collective on the data path
(only the timing max-reduce); weak scaling by default -- each rank validates a full
432k-block shard (the one shipped schedule, so ranks > 0 replay the same blocks);
--scaling strong splits the 432k blocks into contiguous slot ranges, one per rank.

--config c2|c3|c4 measure the single-primitive configs (1M OCert verifies with
distinct keys, 1M VRF verifies + leader checks, 1M Sum6KES verifies), c1 the
10k-block / 100-pool chain of configs[0] (GPU and CPU side by side).

A plain run sets up, warms up, times --steps passes and prints the result line
(metric, value, unit, ms_per_step, ...); --dump-outputs DIR also writes what the last
timed pass computed.  Everything below is measured only with --full: the serial
per-kernel pass and the roofline, the key-cache and dedup figures, the rate with the
dedup off, the strong-scaling proxy, the end-to-end paths, the self-check and the CPU
baseline.

CPU baseline (--full, rank 0, N = 1): the CPU twin libpraos_cpu.so (C++ restatement of the
reference semantics with the same C ABI; the Haskell reference cannot run here)
timed over a bounded sample of the same headers on the host cores this job may use,
plus its single-core rate and an OpenSSL Ed25519 verify rate as an independent
third-party point; the twin's bits are compared with the GPU's on the whole sample
and the oracle (oracle/) checks both on a sub-sample.
"""
import argparse
import json
import multiprocessing as mp
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "ouroboros-consensus_amd"))

# Algorithmic work per unit (int32 lane-ops), counted by construction from the
# kernel schedules (tools/workmodel.py; DESIGN.md sec. 4 "Work model").
sys.path.insert(0, os.path.join(ROOT, "tools"))
from workmodel import (W_OCERT, W_KES, W_VRF, W_LEADER, W_OCERT_CK, W_VRF_CK,  # noqa: E402
                       W_KES_CK, W_KEY_COLD, W_KEY_VRF, W_KEY_KES, W_VRF_V, W_VRF_TP, W_LEADER_TP)
# gfx950 VALU peak (MI355X_MICROARCH.md: a wave64 VALU instruction issues over 2
# cycles, i.e. 32 lane-ops/clk/SIMD = 128 lane-ops/clk/CU) x 256 CUs x 2.4 GHz
PEAK_INT32 = 256 * 128 * 2.4e9
MASK = {"ocert": 1, "kes": 2, "vrf": 4}
# committed rocprofv3 summaries (tools/profile.sh <tag>): <tag>_traffic.json names its workload;
# the first tag whose workload is the bench's supplies traffic and PMC for the roofline kernel
PROFILE_TAGS = ("r06c7", "r06c6", "r06c5", "r05c5", "r05c4", "r05c3", "r05c2", "r05tp", "r04c5", "r04c4b", "r04c3", "r04c2", "r04tp", "r04c4", "r03e")


def profile_tag(workload):
    for tag in PROFILE_TAGS:
        try:
            if json.load(open(os.path.join(ROOT, "profiles", f"{tag}_traffic.json"))).get("workload") == workload:
                return tag
        except (OSError, ValueError):
            continue
    return None


def load_pmc(kernel, workload):
    """VALU issue of `kernel` from the committed rocprofv3 PMC summary of the same workload
    (tools/profile.sh + tools/prof_summary.py): wave-level VALU instructions per launch and
    VALUBusy = SQ_ACTIVE_INST_VALU x 4 (quad-cycles) / (1024 SIMDs x GRBM_GUI_ACTIVE / 8 XCDs),
    the fraction of SIMD cycles the vector ALU was issuing while the kernel ran."""
    tag = profile_tag(workload)
    pmc_file = os.path.join(ROOT, "profiles", f"{tag}_pmc.json")
    try:
        d = json.load(open(pmc_file)).get(kernel)
        valu = d["SQ_ACTIVE_INST_VALU"]["per_dispatch"]
        gui = d["GRBM_GUI_ACTIVE"]["per_dispatch"] / 8
        insts = d["SQ_INSTS_VALU"]["per_dispatch"]
    except (OSError, ValueError, KeyError, TypeError):
        return None
    return {"valu_busy": round(valu * 4 / (256 * 4) / gui, 4), "valu_wave_insts_per_launch": insts,
            "simd_cycles_per_valu_inst": round(gui * 256 * 4 / insts, 2),
            "source": os.path.relpath(pmc_file, ROOT),
            "basis": "VALUBusy = SQ_ACTIVE_INST_VALU x 4 / (1024 SIMDs x GRBM_GUI_ACTIVE / 8 XCDs) (rocprof's "
                     "derived metric); simd_cycles_per_valu_inst = kernel cycles x 1024 SIMDs / SQ_INSTS_VALU, "
                     "against 2 for the guide's nominal issue rate and ~4 measured for one wave's stream; "
                     "GRBM_GUI_ACTIVE spans the dispatch, so values of ~1.0 (within a few %) mean the SIMDs "
                     "issued VALU instructions every cycle the kernel ran"}


CONFIGS = {
    "c1": dict(items=10_000, kernels=7, metric="Praos headers validated/sec (CPU config C1)",
               workload="configs[0]: the first 10,000 blocks of a first-leader-wins Praos (Babbage) chain, "
                        "100 pools, tools-test genesis (GPU and CPU side by side)"),
    "c2": dict(items=1_000_000, pools=None, kernels=1, nkes=64, metric="OCert Ed25519 verifications/sec",
               workload="configs[1]: 1M OCert Ed25519 verifications, distinct cold keys, 1% corrupted"),
    "c3": dict(items=1_000_000, pools=3000, kernels=4, nkes=0, metric="ECVRF-draft03 verifies + leader checks/sec",
               workload="configs[2]: 1M ECVRF-ED25519-SHA512-Elligator2 verifies + leader checks, single eta0, "
                        "3000 pools, the (slot, pool) pairs of the first 1M blocks of a first-leader-wins "
                        "schedule (every clean item a leader), 1% corrupted"),
    "c4": dict(items=1_000_000, pools=3000, kernels=2, nkes=0, metric="Sum6KES verifications/sec",
               workload="configs[3]: 1M Sum6KES verifies (depth-6 Blake2b-256 Merkle path + Ed25519 leaf), "
                        "397-byte messages, 1% corrupted"),
    "tp": dict(items=432_000, pools=3000, kernels=7, metric="TPraos headers validated/sec (2 VRF+KES+OCert+leader)",
               workload="TPraos (Shelley..Alonzo) headers from stored bytes: the first 432k blocks of a "
                        "first-leader-wins TPraos chain (3000 pools, f = 1/20, leader certificate vs 2^512), "
                        "BHeaders decoded on the device, single eta0, 1% corrupted"),
    "c5": dict(items=432_000, kernels=7, metric="Praos headers validated/sec (VRF+KES+OCert+leader)",
               workload="configs[4]: mainnet-shaped epoch replay, the first 432k blocks of a first-leader-wins "
                        "Praos chain per GPU, 3000-pool stake distribution, single eta0, 1% corrupted"),
}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def host_cores():
    """CPUs this job may use (affinity), the machine's count, and the CPU model."""
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 1
    model = platform.processor() or ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return usable, os.cpu_count() or 1, model


def smt_topology():
    """(physical cores, [(cpu, its SMT sibling)]) of the CPUs in this job's mask, from sysfs."""
    try:
        mask = sorted(os.sched_getaffinity(0))
        cores, pairs = set(), []
        for c in range(os.cpu_count() or 0):
            base = f"/sys/devices/system/cpu/cpu{c}/topology"
            cores.add((open(f"{base}/physical_package_id").read().strip(), open(f"{base}/core_id").read().strip()))
        for c in mask:
            sib = open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list").read().strip()
            parts = [int(x) for x in sib.replace("-", ",").split(",") if x]
            other = [x for x in parts if x != c and x in mask]
            if other:
                pairs.append((c, other[0]))
        return len(cores), pairs
    except (OSError, ValueError):
        return None, []


def smt_pair_rate(kind, S, eta0, pool_list, p, spkp, cpus):
    """Items/s of two one-thread CPU twins run at once, each thread pinned to one of `cpus` (its
    twin opened after the pin, so the twin's threads inherit it)."""
    import threading
    from praos_hip import cpu as C
    res, barrier = [None, None], threading.Barrier(2)

    def run(j):
        os.sched_setaffinity(0, {cpus[j]})
        tw = C.CpuContext(1)
        tw.set_epoch(eta0, pool_list, p)
        _twin_run(tw, kind, _sample(S, np.arange(16)), eta0, pool_list, p, spkp)
        barrier.wait()
        t = time.perf_counter()
        _twin_run(tw, kind, S, eta0, pool_list, p, spkp)
        res[j] = time.perf_counter() - t
        tw.close()
    mask = os.sched_getaffinity(0)
    try:
        th = [threading.Thread(target=run, args=(j,)) for j in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        os.sched_setaffinity(0, mask)
    return 2 * len(S["slot"]) / max(res)


def _hdr_dict(H, i):
    off, ln = int(H["body_off"][i]), int(H["body_len"][i])
    return {"slot": int(H["slot"][i]), "cold_vk": bytes(H["cold_vk"][i]), "vrf_vk": bytes(H["vrf_vk"][i]),
            "vrf_out": bytes(H["vrf_out"][i]), "vrf_proof": bytes(H["vrf_proof"][i]),
            "hot_vk": bytes(H["hot_vk"][i]), "n": int(H["ocert_n"][i]), "c0": int(H["ocert_c0"][i]),
            "ocert_sig": bytes(H["ocert_sig"][i]), "kes_sig": bytes(H["kes_sig"][i]),
            "body": bytes(H["body_bytes"][off:off + ln]),
            **({"leader_out": bytes(H["leader_out"][i]), "leader_proof": bytes(H["leader_proof"][i])}
               if "leader_out" in H else {})}


def _oracle_worker(payload):
    """Checks one chunk with the oracle; returns (result bits, busy seconds)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    kind, eta0, c_raw, spkp, maxevo, pools, items = payload
    out = []
    if kind in ("header", "tpraos"):
        ep = oracle.make_epoch(eta0, spkp, maxevo, c_raw, pools)
        t0 = time.perf_counter()
        f = oracle.praos_header if kind == "header" else oracle.tpraos_header
        out = [f(ep, h)["bits"] for h in items]
    elif kind == "ocert":
        t0 = time.perf_counter()
        for h in items:
            m = h["hot_vk"] + h["n"].to_bytes(8, "big") + h["c0"].to_bytes(8, "big")
            out.append(0 if oracle.ed25519_verify(h["cold_vk"], m, h["ocert_sig"]) else 0x0004)
    elif kind == "kes":
        t0 = time.perf_counter()
        for h in items:
            t = h["slot"] // spkp - h["c0"]
            r = oracle.kes_verify(h["hot_vk"], max(t, 0), h["body"], h["kes_sig"])
            out.append({0: 0, 1: 0x0008, 2: 0x0010}[r])
    else:
        raise ValueError(kind)
    return out, time.perf_counter() - t0


def openssl_ed25519_rate(seconds=2.0):
    """Ed25519 verifies/s on one core with OpenSSL's libcrypto (third-party point), or None."""
    import ctypes
    import ctypes.util
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        C = ctypes.CDLL(name)
        C.EVP_PKEY_new_raw_public_key.restype = ctypes.c_void_p
        C.EVP_PKEY_new_raw_public_key.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        C.EVP_MD_CTX_new.restype = ctypes.c_void_p
        C.EVP_DigestVerifyInit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p]
        C.EVP_DigestVerify.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                       ctypes.c_size_t]
        C.EVP_MD_CTX_free.argtypes = [ctypes.c_void_p]
        C.EVP_PKEY_free.argtypes = [ctypes.c_void_p]
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle
        seed, msg = b"\x07" * 32, b"\x01" * 48
        pk, sig = oracle.ed25519_pk(seed), oracle.ed25519_sign(seed, msg)
        key = C.EVP_PKEY_new_raw_public_key(1087, None, pk, 32)          # EVP_PKEY_ED25519
        n, t0 = 0, time.perf_counter()
        ok = True
        while time.perf_counter() - t0 < seconds:
            for _ in range(100):
                md = C.EVP_MD_CTX_new()
                C.EVP_DigestVerifyInit(md, None, None, None, key)
                ok &= C.EVP_DigestVerify(md, sig, 64, msg, 48) == 1
                C.EVP_MD_CTX_free(md)
            n += 100
        C.EVP_PKEY_free(key)
        return round(n / (time.perf_counter() - t0), 1) if ok else None
    except (OSError, AttributeError):
        return None


def _sample(H, idx):
    """Sub-batch of the SoA header dict H at indices idx (bodies repacked)."""
    S = {k: np.ascontiguousarray(H[k][idx]) for k in H if k not in ("body_bytes", "body_off", "body_len")}
    lens = H["body_len"][idx].astype(np.uint64)
    offs = H["body_off"][idx]
    S["body_len"] = np.ascontiguousarray(H["body_len"][idx])
    S["body_off"] = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    S["body_bytes"] = np.concatenate([H["body_bytes"][int(o):int(o) + int(ln)] for o, ln in zip(offs, lens)] +
                                     [np.zeros(8, np.uint8)])
    return S


def _twin_run(ctx, kind, S, eta0, pool_list, p, spkp):
    """One CPU-twin pass over the sample S; returns the per-item result bits."""
    import hashlib
    n = len(S["slot"])
    if kind == "header":
        return ctx.verify_headers(S)["bits"]
    if kind == "tpraos":
        return ctx.verify_tpraos_headers(S)["bits"]
    if kind == "ocert":
        ok = ctx.verify_ocert(S["cold_vk"], S["hot_vk"], S["ocert_n"], S["ocert_c0"], S["ocert_sig"])
        return np.where(ok == 1, 0, 0x0004).astype(np.uint16)
    if kind == "kes":
        t = np.maximum(S["slot"].astype(np.int64) // spkp - S["ocert_c0"].astype(np.int64), 0).astype(np.uint32)
        msgs = [bytes(S["body_bytes"][int(o):int(o) + int(ln)]) for o, ln in zip(S["body_off"], S["body_len"])]
        r = ctx.verify_kes(S["hot_vk"], t, S["kes_sig"], msgs)
        return np.array([{0: 0, 1: 0x0008, 2: 0x0010}[int(x)] for x in r], np.uint16)
    # vrf + leader (configs[2]): alpha = mkInputVRF, leader value of the certified output
    alpha = np.frombuffer(b"".join(hashlib.blake2b(int(s).to_bytes(8, "big") + eta0, digest_size=32).digest()
                                   for s in S["slot"]), np.uint8).reshape(n, 32).copy()
    ok, beta = ctx.verify_vrf(S["vrf_vk"], S["vrf_proof"], alpha)
    lv = np.frombuffer(b"".join(hashlib.blake2b(b"L" + bytes(o), digest_size=32).digest() for o in S["vrf_out"]),
                       np.uint8).reshape(n, 32).copy()
    by_hash = {h: s for h, _, s in pool_list}
    hk = [hashlib.blake2b(bytes(c), digest_size=28).digest() for c in S["cold_vk"]]
    known = np.array([h in by_hash for h in hk])
    sig = np.frombuffer(b"".join(int(by_hash.get(h, 0)).to_bytes(16, "little") for h in hk),
                        np.uint8).reshape(n, 16).copy()
    lead = ctx.check_leader(lv, sig, p) | ~known          # VRFKeyUnknown precedes the leader test
    bits = np.where(ok == 1, 0, 0x0400) | np.where((beta == S["vrf_out"]).all(axis=1), 0, 0x0800)
    return (bits | np.where(lead == 1, 0, 0x1000)).astype(np.uint16)


def cpu_baseline(kind, H, gpu_bits, eta0, c_raw, p, spkp, maxevo, pool_list, seconds, threads, per_item, mask,
                 whole=False, body_corrupted=None):
    """The CPU twin (libpraos_cpu.so, same ABI, `threads` worker threads) timed over a
    bounded sample of the benchmark input, its single-core rate, and the oracle as
    the checker of both implementations on a sub-sample."""
    from praos_hip import cpu as C
    n_total = len(H["slot"])
    n_sample = n_total if whole else int(min(n_total, max(threads * 64, seconds * threads / per_item)))
    idx = np.linspace(0, n_total - 1, n_sample).astype(np.int64)
    S = _sample(H, idx)
    twin = C.CpuContext(threads)
    twin.set_epoch(eta0, pool_list, p)
    _twin_run(twin, kind, _sample(H, idx[:64]), eta0, pool_list, p, spkp)       # warm
    t0 = time.perf_counter()
    bits = _twin_run(twin, kind, S, eta0, pool_list, p, spkp)
    busy = time.perf_counter() - t0
    same = (gpu_bits[idx] & mask) == (bits & mask)
    if body_corrupted is not None:
        # stored-bytes GPU path: a corrupted body byte is decoded (it may land in any field),
        # the twin sees the generator's fields with that body -- compared on accept / reject
        bc = body_corrupted[idx]
        same = np.where(bc, (gpu_bits[idx] != 0) == (bits != 0), same)
    agree = int(same.sum())
    # one core: the first part of the same sample on one thread
    n1 = max(16, min(n_sample, int(3.0 / per_item)))
    twin.set_option(C.OPT_THREADS, 1)
    t1 = time.perf_counter()
    _twin_run(twin, kind, _sample(H, idx[:n1]), eta0, pool_list, p, spkp)
    t1 = time.perf_counter() - t1
    twin.close()
    # SMT: two one-thread twins on the two hardware threads of one core against two on two cores
    # (the all-cores estimate counts physical cores x the rate of a core running both threads)
    smt = None
    phys, pairs = smt_topology()
    if kind == "header" and phys and len(pairs) >= 2:
        a, b = pairs[-1]
        c2 = next((x for x, _ in pairs if x not in (a, b)), None)
        if c2 is not None:
            S2 = _sample(H, idx[: max(16, int(1.5 / per_item))])
            pair = smt_pair_rate(kind, S2, eta0, pool_list, p, spkp, (a, b))
            two = smt_pair_rate(kind, S2, eta0, pool_list, p, spkp, (a, c2))
            smt = {"physical_cores": phys, "pair_cpus": [a, b], "two_core_cpus": [a, c2],
                   "two_threads_one_core": round(pair, 1), "two_threads_two_cores": round(two, 1),
                   "smt_gain": round(pair / (two / 2), 3),
                   "all_cores_smt_estimate": round(phys * (n1 / t1) * pair / (two / 2), 1),
                   "note": "two one-thread twins at once, pinned to the sibling hardware threads of one core "
                           "vs to two cores; estimate = physical cores x single-thread rate x smt_gain"}
    # the oracle (checker) on a sub-sample, in a process pool
    sub = idx[:: max(1, n_sample // 2000)]
    items = [_hdr_dict(H, i) for i in sub]
    workers = max(1, min(threads, 16))
    chunks = [items[k::workers] for k in range(workers)]
    with mp.get_context("spawn").Pool(workers) as pool:
        res = pool.map(_oracle_worker, [(kind if kind != "vrf" else "header", eta0, c_raw, spkp, maxevo, pool_list, c)
                                        for c in chunks])
    obits = [None] * len(sub)
    for k, (b, _) in enumerate(res):
        for j, v in enumerate(b):
            obits[k + j * workers] = v
    omask = mask if kind != "vrf" else 0x1F00
    oracle_agree = sum(1 for j, i in enumerate(sub) if (int(gpu_bits[i]) & omask) == (obits[j] & omask) or
                       (body_corrupted is not None and body_corrupted[i] and
                        (int(gpu_bits[i]) != 0) == (obits[j] != 0)))
    usable, nproc, model = host_cores()
    single = len(range(n1)) / t1
    return {"value": round(n_sample / busy, 1), "unit": "headers/s" if kind in ("header", "tpraos") else "items/s",
            "cores": threads, "kind": "port",
            "sample": f"{n_sample} items evenly spaced over the benchmark input; CPU twin libpraos_cpu.so "
                      f"(C++, radix-2^51, sliding-window Straus, same ABI) on {threads} threads, {busy:.2f}s",
            "single_core": round(single, 1),
            "all_cores_linear_estimate": round(single * nproc, 1),
            **({"smt": smt} if smt else {}),
            "host": {"cpu_model": model, "nproc": nproc, "usable_cores": usable,
                     "threads_used": threads, "note": "threads capped at the box's CPU share (16 per GPU)"},
            "parity_sample": {"n": n_sample, "bit_exact_twin_vs_gpu": agree,
                              "oracle_checked": len(sub), "bit_exact_oracle_vs_gpu": oracle_agree}}


def load_traffic(kernel, workload):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC summary of the same
    workload (FETCH_SIZE x2 gfx950 read correction + WRITE_SIZE, separate --pmc passes,
    tools/prof_summary.py)."""
    tag = profile_tag(workload)
    if tag is None:
        return None, None
    f = os.path.join(ROOT, "profiles", f"{tag}_traffic.json")
    k = json.load(open(f)).get("kernels", {}).get(kernel)
    return (k, os.path.relpath(f, ROOT)) if k else (None, None)


def make_input(ctx, args, cfg, rank, world=1):
    """Returns (H, pool_list, corrupted, params, eta0, c_raw, spkp, maxevo) of the config
    (praos_hip/configs.py, shared with the full-size -m gpu tests).  Strong scaling: rank r
    signs blocks [r*n/world, (r+1)*n/world) of the chain."""
    from praos_hip import configs
    return configs.build(ctx, args.config, n=args.items or cfg["items"], corrupt_per_10000=args.corrupt_per_10000,
                         rank=rank, world=world, scaling=args.scaling)


def headline(args, cfg, n, world, dt, npools):
    """The result line of a plain run (a --full run adds its sections to it): `dt` seconds for
    args.steps timed steps over `n` items on each of `world` GPUs."""
    total = n * world if args.scaling == "weak" else (args.items or cfg["items"])
    return {
        "metric": cfg["metric"],
        "value": round(total * args.steps / dt, 1), "unit": "headers/s" if cfg["kernels"] == 7 else "items/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt * 1e3 / args.steps, 3), "higher_is_better": True, "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": "u32 (GF(2^255-19) radix-2^32 limbs; Fixed E34 bignum)",
        "data": "synthetic: GPU-signed chain" + (" from the shipped first-leader-wins schedule"
                                                  if args.config in ("c1", "c5") else ""),
        "config": {"workload": cfg["workload"], "items_per_gpu": n, "items_total": total, "pools": npools or None,
                   "active_slot_coeff": "1/20",
                   "signed_body": "canonical HeaderBody CBOR" if args.config in ("c1", "c5") else "397 random bytes",
                   "parallelism": f"shard-by-slot-range x{world}"},
    }


DUMP_BYTES = 60_000_000          # budget of one --dump-outputs directory (float32 values)


def dump_outputs(path, out):
    """Writes the output arrays of one validation pass (bits, pool_idx, beta / leader or the two
    TPraos betas, nonce) as <path>/<name>.npy in float32 (every value is an integer below 2^24,
    so exact).  The per-header scalars are written whole; of the per-header byte rows a fixed,
    seeded sample of headers (sorted indices, the same for every run of one size) is kept so
    that the directory stays below DUMP_BYTES."""
    os.makedirs(path, exist_ok=True)
    n = len(out["bits"])
    wide = [k for k, v in out.items() if v.ndim == 2]
    row_bytes = 4 * sum(out[k].shape[1] for k in wide)
    m = int(max(1, min(n, (DUMP_BYTES - 4 * n * (len(out) - len(wide))) // row_bytes)))
    rows = np.sort(np.random.default_rng(0).choice(n, m, replace=False)) if m < n else np.arange(n)
    for k, v in out.items():
        np.save(os.path.join(path, f"{k}.npy"), (v[rows] if v.ndim == 2 else v).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="c5", choices=sorted(CONFIGS))
    ap.add_argument("--items", type=int, default=None, help="items per GPU (default: the config's)")
    ap.add_argument("--corrupt-per-10000", type=int, default=100)
    ap.add_argument("--scaling", default="weak", choices=("weak", "strong"),
                    help="weak: every GPU validates a full shard (default); strong: the config's "
                         "blocks split over the GPUs (c1/c5)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--cpu-workers", type=int, default=16, help="CPU-twin threads (the box's share: 16)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-proxy", action="store_true", help="skip the one-GPU strong-scaling proxy (c1/c5)")
    ap.add_argument("--concurrent", type=int, default=1, help="run OCert/KES/VRF kernels on 3 streams")
    ap.add_argument("--keycache", type=int, default=2,
                    help="min uses of a public key for the per-batch key cache (0 = off)")
    ap.add_argument("--pipeline", type=int, default=0,
                    help="chunks of the stored-bytes e2e pipeline (PRAOS_OPT_PIPELINE; 0 = auto)")
    ap.add_argument("--dedup", type=int, default=1,
                    help="verify each distinct OCert tuple once per batch (PRAOS_OPT_DEDUP; 0 = off)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline: serial per-kernel pass and "
                         "roofline, dedup-off rate, strong-scaling proxy, end-to-end paths, self-check, CPU "
                         "baseline (--no-cpu / --no-e2e / --no-proxy drop parts of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step (what praos_batch_download returns) as "
                         "DIR/<name>.npy in float32")
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    if args.scaling == "strong" and args.config not in ("c1", "c5"):
        ap.error("--scaling strong applies to the chain configs (c1, c5)")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    # PRAOS_BENCH_REHEARSAL=1: every rank on device 0 over gloo (a multi-rank rehearsal of
    # this code path on a one-GPU box; the real multi-GPU run uses RCCL, one GPU per rank)
    rehearsal = os.environ.get("PRAOS_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local = 0
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local)
        dist.init_process_group("gloo" if rehearsal else "nccl")
    import torch

    import praos_hip
    from praos_hip import abi

    from praos_hip import configs
    ctx = praos_hip.Context(local)
    # the dedup belongs to the header pipeline (c1/c5: a chain repeats each pool's OCert);
    # the single-primitive configs measure every signature on its own
    args.dedup = configs.options(ctx, args.config, concurrent=args.concurrent, keycache=args.keycache,
                                 dedup=args.dedup, pipeline=args.pipeline)
    t0 = time.perf_counter()
    H, pool_list, corrupted, p, eta0, c_raw, spkp, maxevo = make_input(ctx, args, cfg, rank, world)
    n = len(H["slot"])
    ctx.set_epoch(eta0, pool_list, p)
    if args.config == "tp":
        from praos_hip.chunk import pack_chunk
        tp_arena, tp_off, tp_len = pack_chunk(H, era_tag=5)
        b = ctx.upload_tpraos_bytes(tp_arena, tp_off, tp_len)
    else:
        b = ctx.upload(H)
    log(f"[rank {rank}] {args.config}: synthesised + uploaded {n} items in {time.perf_counter() - t0:.1f}s")

    log(f"[rank {rank}] warm-up")
    for _ in range(args.warmup):
        ctx.run(b)
        ctx.sync()
    log(f"[rank {rank}] timed steps")
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    kms = np.zeros(8)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ctx.run(b)
        ctx.sync()                                     # per-step HIP-event kernel times
        kms += [ctx.kernel_ms(k) for k in range(8)]
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    if dist:
        t = torch.tensor([dt], device="cpu" if rehearsal else "cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ctx.download_tpraos(b, n) if args.config == "tp" else ctx.download(b, n))
    if not args.full:
        # the plain run ends here: the headline figures alone
        ctx.free(b)
        if rank == 0:
            print(json.dumps(headline(args, cfg, n, world, dt, len(pool_list))), flush=True)
        ctx.close()
        if dist:
            dist.destroy_process_group()
        return
    log(f"[rank {rank}] serial pass")
    # per-kernel durations for the roofline: serial launches (HIP events on the
    # launch stream), untimed, after the timed region
    ctx.set_option(abi.OPT_CONCURRENT, 0)
    kser = np.zeros(8)
    for _ in range(3):
        ctx.run(b)
        ctx.sync()
        kser += [ctx.kernel_ms(k) for k in range(8)]
    kser /= 3
    ctx.set_option(abi.OPT_CONCURRENT, args.concurrent)
    kst = ctx.batch_stats(b)
    dds = ctx.dedup_stats(b)
    # the same steps with the OCert dedup off (every header's OCert signature verified
    # on its own), reported beside the headline for transparency
    nodedup = None
    if args.dedup and cfg["kernels"] & 1:
        ctx.set_option(abi.OPT_DEDUP, 0)
        ctx.run(b)
        ctx.sync()
        torch.cuda.synchronize()
        t0n = time.perf_counter()
        for _ in range(args.steps):
            ctx.run(b)
            ctx.sync()
        torch.cuda.synchronize()
        nodedup = n * args.steps / (time.perf_counter() - t0n)
        ctx.set_option(abi.OPT_DEDUP, args.dedup)
        ctx.run(b)
        ctx.sync()
    out = ctx.download_tpraos(b, n) if args.config == "tp" else ctx.download(b, n)
    ctx.free(b)
    # one-GPU proxy of strong scaling: the rate of a 1/k shard of this batch (rank 0's
    # contiguous slot range at N = k), timed like the headline after one warm-up pass
    proxy = None
    if rank == 0 and not args.no_proxy and args.config in ("c1", "c5") and world == 1:
        proxy = {}
        ksteps = max(args.steps, 30)                   # a 1/8 shard step is ~2 ms: 30 steps for a steady-state rate
        for k in (2, 4, 8):
            m = n // k
            log(f"[rank {rank}] strong proxy 1/{k}")
            bk = ctx.upload(_sample(H, np.arange(m)))
            for _ in range(2):                         # warm-up (buffers for this size, key caches)
                ctx.run(bk)
                ctx.sync()
            tk = time.perf_counter()
            for _ in range(ksteps):
                ctx.run(bk)
                ctx.sync()
            tk = time.perf_counter() - tk
            ctx.free(bk)
            rk = m * ksteps / tk
            proxy[f"n{k}"] = {"items": m, "value": round(rk, 1), "ms_per_step": round(tk * 1e3 / ksteps, 3),
                              "steps": ksteps, "per_gpu_vs_full": round(rk / (n * args.steps / dt), 3)}
    # end to end through the blocking entry point: host SoA in, H2D, all kernels,
    # D2H of bits/beta/leader/nonce (never the headline value)
    e2e = None
    if not args.no_e2e and rank == 0 and args.config != "tp":
        log(f"[rank {rank}] e2e")
        e2e = {}
        if args.config in ("c1", "c5"):
            # stored header bytes (what an ImmutableDB chunk holds, ~860 B per header) ->
            # praos_verify_header_bytes: chunked H2D on a copy stream overlapping the
            # kernels, D2H of each chunk's results while later chunks compute
            from praos_hip.chunk import pack_chunk
            arena, off_, ln_ = pack_chunk(H)
            ob = ctx.alloc_out(n)                                      # caller-owned outputs, reused

            def best_of_3():
                ctx.verify_header_bytes(arena, off_, ln_, out=ob)      # warm (chunk batches allocated)
                ts = []
                for _ in range(3):
                    t_ = time.perf_counter()
                    ctx.verify_header_bytes(arena, off_, ln_, out=ob)
                    ts.append(time.perf_counter() - t_)
                return min(ts)
            te_pageable = best_of_3()
            # the same with the host arena and the output arrays page-locked once
            # (praos_host_register, as a replay reader locks its chunk buffers): direct DMA
            obs = (ob, ctx.alloc_out(n), ctx.alloc_out(n))             # the outputs of three calls in flight
            bufs = [arena] + [v for o_ in obs for v in o_.values() if v.nbytes >= (4 << 20)]
            for a in bufs:
                ctx.host_register(a)
            te = best_of_3()
            cmp = np.asarray(corrupted) != 5                           # (see below)
            plain_exact = bool(all((ob[k][cmp] == out[k][cmp]).all() for k in ob))
            # streaming: batch after batch through praos_verify_header_bytes_submit (three calls in
            # flight: each call's upload, decode and stage V under the previous call's key chains,
            # as the resident steps overlap), every call's outputs written before the clock stops
            for o_ in obs:
                for v in o_.values():
                    v.fill(0)
            for o_ in obs:                                             # warm (the pipe batches)
                ctx.submit_header_bytes(arena, off_, ln_, out=o_)
            ctx.drain()
            stream_calls = 8
            ts_ = []
            for _ in range(2):
                t_ = time.perf_counter()
                for j in range(stream_calls):
                    ctx.submit_header_bytes(arena, off_, ln_, out=obs[j % 3])
                ctx.drain()
                ts_.append((time.perf_counter() - t_) / stream_calls)
            ts = min(ts_)
            stream_exact = bool(all((o_[k][cmp] == out[k][cmp]).all() for o_ in obs for k in ob))
            # a node validating batch after batch of one epoch keeps its pool keys' tables
            # (PRAOS_OPT_POOL_KEYS: cold / VRF key entries kept across calls, filled by the
            # warm-up call of best_of_3); reported beside the value, never as it
            from praos_hip import abi as _abi
            ctx.set_option(_abi.OPT_POOL_KEYS, 2)
            te_pk = best_of_3()
            pk_exact = bool(all((ob[k][cmp] == out[k][cmp]).all() for k in ob))
            ctx.set_option(_abi.OPT_POOL_KEYS, -1)
            for a in bufs:
                ctx.host_unregister(a)
            # a corrupted body byte (corruption kind 5) makes the stored CBOR itself
            # malformed or different, so the byte path rejects that header at decode
            # (PRAOS_BIT_DECODE) where the SoA path rejects it at the KES check: those
            # headers are compared on accept/reject only, every other header bit for bit
            e2e = {"value": round(n / ts, 1), "unit": "headers/s", "ms": round(ts * 1e3, 2),
                   "bit_exact_vs_resident": stream_exact and plain_exact,
                   "vs_resident": round((n / ts) / (n * args.steps / dt), 3),
                   "mode": f"streaming: {stream_calls} calls back to back through praos_verify_header_bytes_submit "
                           "(three in flight: each call's upload, decode and stage V under the previous calls' key "
                           "chains, as the resident steps overlap), then praos_verify_drain; ms = the wall per call, "
                           "every call's outputs in host memory when the clock stops (best of 2 runs)",
                   "single_call": {"value": round(n / te, 1), "ms": round(te * 1e3, 2),
                                   "bit_exact_vs_resident": plain_exact,
                                   "note": "one blocking praos_verify_header_bytes call at a time (best of 3): "
                                           "upload, all kernels and the downloads of that call alone"},
                   "accept_equal_all": bool(((ob["bits"] == 0) == (out["bits"] == 0)).all()),
                   "body_corrupted_excluded": int((~cmp).sum()),
                   "input_bytes": int(len(arena)), "h2d_GBps_equiv": round(len(arena) / te / 1e9, 1),
                   "pool_keys_warm": {"value": round(n / te_pk, 1), "ms": round(te_pk * 1e3, 2),
                                      "bit_exact_vs_resident": pk_exact,
                                      "note": "the same registered calls with the pool-key store on "
                                              "(PRAOS_OPT_POOL_KEYS): the cold / VRF key tables built by the "
                                              "first call are reused by the next (a node validating successive "
                                              "batches of one epoch)"},
                   "pageable": {"value": round(n / te_pageable, 1), "ms": round(te_pageable * 1e3, 2),
                                "note": "the same calls with the arena and outputs in pageable memory: "
                                        "uploads staged through the library's pinned buffers by 16 host threads"},
                   "path": "praos_verify_header_bytes[_submit]: stored header bytes (host arena page-locked once "
                           "with praos_host_register) -> H2D in 8 chunks on a copy stream, each landed chunk decoded "
                           "and its VRF stage V run while later chunks upload -> the rest of the batch once -> "
                           "outputs D2H; streaming: the next calls' uploads, decodes and stage V under this call's "
                           "key chains"}
        # the host-SoA entry point (every decoded field from the host, 1,236 B per header)
        oe = ctx.verify_headers(H)
        te = time.perf_counter()
        ctx.verify_headers(H, out=oe)
        te = time.perf_counter() - te
        t0 = time.perf_counter()
        b2 = ctx.upload(H)
        t1 = time.perf_counter()
        ctx.run(b2)
        ctx.sync()
        t2 = time.perf_counter()
        ctx.download(b2, n, out=oe)
        t3 = time.perf_counter()
        ctx.free(b2)
        in_bytes = sum(v.nbytes for v in H.values())
        e2e_soa = {"value": round(n / te, 1), "unit": "headers/s" if cfg["kernels"] == 7 else "items/s",
                   "ms": round(te * 1e3, 2), "bit_exact_vs_resident": bool((oe["bits"] == out["bits"]).all()),
                   "stages_ms": {"upload": round((t1 - t0) * 1e3, 2), "run": round((t2 - t1) * 1e3, 2),
                                 "download": round((t3 - t2) * 1e3, 2)},
                   "input_bytes": in_bytes, "h2d_GBps": round(in_bytes / (t1 - t0) / 1e9, 1),
                   "path": "praos_verify_headers: host SoA (pageable) -> repack + H2D through pinned staging "
                           "buffers -> kernels -> D2H into caller-owned output arrays; serial stages"}
        if e2e:
            e2e["soa_path"] = e2e_soa
        else:
            e2e = e2e_soa

    # self-check on the whole shard: clean items must pass every check that ran
    clean = corrupted == 0
    crypto_bits = out["bits"] & ~np.uint16(0x1000) if args.config not in ("c1", "c5") else out["bits"]
    clean_ok = int((crypto_bits[clean] == 0).sum())
    corrupt_caught = int((crypto_bits[~clean] != 0).sum())
    # corruptions that land in a field the config does not check cannot be caught
    relevant = configs.CHECKED_KINDS[cfg["kernels"]]
    rel = np.isin(corrupted, relevant)
    corrupt_caught_rel = int((crypto_bits[rel] != 0).sum())

    if rank != 0:
        return
    steps = args.steps
    line = headline(args, cfg, n, world, dt, len(pool_list))
    value = line["config"]["items_total"] * steps / dt
    kms /= steps
    per_kernel = {"ocert": kser[0], "kes": kser[1], "vrf": kser[2], "leader": kser[3]}   # stream spans
    ran = [k for k in ("ocert", "kes", "vrf") if cfg["kernels"] & MASK[k]]
    # algorithmic work of one run (tools/workmodel.py): headers on cached keys
    # run the short chains, plus the per-key precomputation
    work = {"ocert": kst["cold_hits"] * W_OCERT_CK + kst["cold_misses"] * W_OCERT + kst["cold_keys"] * W_KEY_COLD,
            "kes": kst["kes_hits"] * W_KES_CK + kst["kes_misses"] * W_KES + kst["kes_keys"] * W_KEY_KES,
            "vrf": kst["vrf_hits"] * W_VRF_CK + kst["vrf_misses"] * W_VRF + kst["vrf_keys"] * W_KEY_VRF}
    if args.keycache == 0:
        work["ocert"], work["vrf"], work["kes"] = n * W_OCERT, n * W_VRF, n * W_KES
        if dds["ocert_unique"]:
            work["ocert"] = dds["ocert_unique"] * W_OCERT
    dominant = max(ran, key=lambda k: per_kernel[k])
    wk = work[dominant] / n
    dom_ms = per_kernel[dominant]
    dom_work = work[dominant]
    w_pipe = (sum(work[k] for k in ran) + (n * W_LEADER if "vrf" in ran else 0)) / n
    pipe_achieved = n * w_pipe / (kms[4] * 1e-3)
    # the dominant kernel as it runs: the key-cache variant when the cache is on
    dom_kernel = f"k_{dominant}_ck" if (args.keycache and kst.get(f"{'cold' if dominant == 'ocert' else dominant}_hits")) \
        else f"k_{dominant}"
    if dominant == "vrf" and kser[6] > 0:
        # the VRF runs in stages (k_vrf_stage.hip): stage V (H, Gamma, V = [s]H - [c]Gamma) over
        # every header is the largest single kernel of the step; price it alone, on the
        # HIP events around its own launch (serial run, no other kernel on the GPU)
        dom_kernel, dom_ms, dom_work, wk = "k_vrf_v", float(kser[6]), n * W_VRF_V, W_VRF_V
    stream_frac = None
    if dominant == "kes" and kser[7] > 0 and kst["kes_hits"]:
        # the cached Sum6KES kernel alone (HIP events around its launch, serial pass), as stage V
        # is priced for configs[4]; the KES stream (key lists, precompute, tables, misses) beside it
        stream_frac = round(dom_work / (dom_ms * 1e-3) / PEAK_INT32, 4)
        dom_kernel, dom_ms, dom_work = "k_kes_ck", float(kser[7]), kst["kes_hits"] * W_KES_CK
        wk = W_KES_CK
    if args.config == "tp":
        # the TPraos batch runs decode, the OCert / KES passes of the Praos step (dedup, key
        # caches) and both VRF certificates through the staged kernels against the VRF key
        # cache (k_vrf_v per certificate, U cached or per lane, k_vrf_join_tp; each priced as
        # a Praos VRF verify), or with PRAOS_TP_STAGED=0 the one-kernel k_vrf_tp (two uncached
        # certificates per lane, W_VRF_TP); priced as one pipeline over the step
        w_vrf = (2 * (kst["vrf_hits"] * W_VRF_CK + kst["vrf_misses"] * W_VRF) + kst["vrf_keys"] * W_KEY_VRF
                 if kst["vrf_keys"] else n * W_VRF_TP)
        w_pipe = (work["ocert"] + work["kes"] + w_vrf) / n + W_LEADER_TP
        pipe_achieved = n * w_pipe / (kms[4] * 1e-3)
        dom_kernel, dom_ms, dom_work, wk = ("tpraos pipeline (OCert | KES | VRF V/U/join x 2 certificates, k_leader)"
                                            if kst["vrf_keys"] else
                                            "tpraos pipeline (OCert | KES | k_vrf_tp, k_leader)"), float(kms[4]), \
            n * w_pipe, w_pipe
    dom_achieved = dom_work / (dom_ms * 1e-3)
    tk, traffic_src = load_traffic(dom_kernel, cfg["workload"])
    traffic = tk.get("bytes_per_launch") if tk else None
    # the same kernel's average duration in the committed rocprofv3 kernel trace (isolated launches)
    rp_ms = tk.get("rocprof_isolated_avg_ms") if tk else None
    pmc = load_pmc(dom_kernel, cfg["workload"])
    # The headline fraction is the rocprof-backed one: the committed rocprofv3 kernel trace of this
    # workload (tools/profile.sh; the kernel's average over its isolated launches) is the measurement
    # the PMC traffic and VALUBusy come from, so achieved / frac / traffic describe the same runs.
    # The HIP-event time of the kernel alone in this run's serial pass is reported beside it
    # (achieved_events / frac_events): events bracket one launch on its stream and include neither
    # the profiler's per-dispatch serialisation nor its clock behaviour, and read 1-15 % faster.
    ev_achieved = dom_achieved
    if rp_ms:
        dom_achieved = dom_work / (rp_ms * 1e-3)
    line.update({
        "roofline": {"bound": "valu-int32", "kernel": dom_kernel,
                     "achieved": round(dom_achieved / 1e12, 3), "peak": round(PEAK_INT32 / 1e12, 2),
                     "unit": "T int32-ops/s", "frac": round(dom_achieved / PEAK_INT32, 4),
                     "frac_source": "rocprof isolated average (profiles)" if rp_ms else "HIP events (this run)",
                     "achieved_events": round(ev_achieved / 1e12, 3), "frac_events": round(ev_achieved / PEAK_INT32, 4),
                     "traffic": traffic,
                     "traffic_unit": "HBM bytes per launch (rocprofv3 PMC)", "traffic_source": traffic_src,
                     "algorithmic_bytes_per_launch": n * (120 + 336) if dom_kernel == "k_vrf_v" else None,
                     "algorithmic_bytes_basis": "per header: vrf_vk 32 + proof 80 + slot 8 read, the 336-byte "
                                                "stage record (V, H, 8 Gamma, enc Gamma, flag) written"
                                                if dom_kernel == "k_vrf_v" else None,
                     "rocprof_isolated_avg_ms": rp_ms,
                     "frac_rocprof": round(dom_work / (rp_ms * 1e-3) / PEAK_INT32, 4) if rp_ms else None,
                     "work_per_unit": round(wk), "kernel_ms": round(dom_ms, 3),
                     "kernel_ms_concurrent": (round(float(kms[6]), 3) if dom_kernel == "k_vrf_v" else
                                              (round(float(kms[7]), 3) if dom_kernel == "k_kes_ck" else None)),
                     "kes_stream_frac": stream_frac,
                     "pipeline_achieved": round(pipe_achieved / 1e12, 3),
                     "pipeline_frac": round(pipe_achieved / PEAK_INT32, 4), "pipeline_work_per_unit": round(w_pipe),
                     "kernel_ms_serial": {k: round(v, 3) for k, v in per_kernel.items()},
                     "pipeline_ms": round(kms[4], 3), "concurrent_streams": bool(args.concurrent),
                     "peak_basis": "128 int32 lane-ops/clk/CU x 256 CU x 2.4 GHz (VALU issue, MI355X_MICROARCH.md)",
                     "valu_issue_pmc": pmc},
        "keycache": dict(kst, min_uses=args.keycache),
        "ocert_dedup": {"on": bool(args.dedup), "distinct_ocerts_verified": dds["ocert_unique"], "headers": n,
                        "value_without_dedup": round(nodedup, 1) if nodedup else None,
                        "note": "each distinct (cold vk, hot vk, n, c0, sigma) tuple of a batch is verified once "
                                "and its verdict copied to every header carrying the same bytes (PRAOS_OPT_DEDUP)"},
        "self_check": {"clean": int(clean.sum()), "clean_ok": clean_ok, "corrupted": int((~clean).sum()),
                       "corrupted_rejected": corrupt_caught, "corrupted_in_checked_fields": int(rel.sum()),
                       "corrupted_in_checked_fields_rejected": corrupt_caught_rel,
                       "leader_pass": int(((out["bits"] & 0x1000) == 0).sum()) if cfg["kernels"] & 4 else None},
    })
    if e2e:
        line["e2e"] = e2e
    if proxy:
        line["strong_proxy"] = dict(proxy, note="one GPU validating only the first 1/k of the batch (rank 0's "
                                                "shard of a strong-scaling run at N = k); per_gpu_vs_full = its "
                                                "rate / this line's value")
    if world == 1 and not args.no_cpu:
        usable, _, _ = host_cores()
        threads = max(1, min(args.cpu_workers, usable))
        kind, per_item, mask = {7: ("header", 2.5e-4, 0x1F1F), 1: ("ocert", 5e-5, 0x0004),
                                2: ("kes", 6e-5, 0x0018), 4: ("vrf", 1.5e-4, 0x1C00)}[cfg["kernels"]]
        if args.config == "tp":          # TPraos.updateChainDepState's crypto: two VRF certificates
            kind, per_item, mask = "tpraos", 4e-4, 0x1F1F
        line["cpu_baseline"] = cpu_baseline(kind, H, out["bits"], eta0, c_raw, p, spkp, maxevo, pool_list,
                                            args.cpu_seconds, threads, per_item, mask, whole=args.config == "c1",
                                            body_corrupted=(corrupted == 5) if args.config == "tp" else None)
        line["cpu_baseline"]["openssl_ed25519_verify_per_s_1core"] = openssl_ed25519_rate()
        line["gpu_vs_cpu"] = round(value / line["cpu_baseline"]["value"], 1)
        # north_star's ratio is against the reference's ALL-host-core CPU rate: the twin's single-core
        # rate x the host's cores (a linear, i.e. optimistic-for-the-CPU, estimate), at N = 1 and for
        # configs[4] as stated -- one epoch split over 8 GPUs -- from the one-GPU proxy of the 1/8 shard
        allc = line["cpu_baseline"].get("all_cores_linear_estimate")
        if allc:
            line["gpu_vs_cpu_all_cores"] = round(value / allc, 1)
            if proxy and "n8" in proxy:
                line["projected_8gpu_strong"] = {
                    "value": round(8 * proxy["n8"]["value"], 1),
                    "vs_cpu_all_cores": round(8 * proxy["n8"]["value"] / allc, 1),
                    "note": "8 x strong_proxy.n8.value (each GPU validating its contiguous 1/8 of the epoch, no "
                            "exchange) / cpu_baseline.all_cores_linear_estimate"}
                smt = line["cpu_baseline"].get("smt")
                if smt:
                    # the same against the measured SMT estimate (physical cores x one core's rate with both
                    # hardware threads busy): the linear estimate counts each hardware thread as a core
                    line["projected_8gpu_strong"]["vs_cpu_all_cores_smt"] = round(
                        8 * proxy["n8"]["value"] / smt["all_cores_smt_estimate"], 1)
            smt = line["cpu_baseline"].get("smt")
            if smt:
                line["gpu_vs_cpu_all_cores_smt"] = round(value / smt["all_cores_smt_estimate"], 1)
    print(json.dumps(line), flush=True)
    ctx.close()
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
