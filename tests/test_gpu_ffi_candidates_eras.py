"""The TPraos and Byron candidates calls from C (integration/c/ffi_harness.c --candidates-tpraos and
--candidates-pbft, the sequences of Batch.hs validateCandidateFragmentsTPraos /
validateCandidateFragmentsPBft): over an ImmutableDB wrapped in the node-to-node encoding by the
harness itself, the output equals the Python wrappers' on the same inputs -- verdicts, failure sets /
aux, rows, stops, tips and the state CBOR of every fragment, one of them stopped by a broken link,
with a forecast horizon."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import byron_corpus as bc
import pbft_corpus as pc
import pbft_model as pm
from helpers import rng
from test_gpu_ffi import HARNESS, _epoch_file
from test_gpu_pbft import _write_dir
from test_gpu_replay import ENV, EPOCH_LEN, TP_EXTRA, _genesis_state, tchain  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _run(args):
    assert os.path.exists(HARNESS), "build it: make -C integration/c (done by __graft_entry__.build())"
    r = subprocess.run([HARNESS] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_tpraos_phase_equals_the_python_call(ctx, tchain, tmp_path):  # noqa: F811
    from praos_hip import abi, wire
    chain = tchain
    n = len(chain["off"])
    hdrs = [bytes(chain["arena"][int(o):int(o) + int(m)]) for o, m in zip(chain["off"], chain["len"])]
    limits = (ENV["max_major_pv"], 6, ENV["max_header_size"], ENV["max_body_size"])
    ctx.set_epoch(chain["nonces"][0], chain["pools"], chain["params"])

    def call(frags, view_end):
        """frags: [(first, count, state, tip)] over the chain's headers, wrapped as era 4."""
        items = [wire.wrap(4, hdrs[h]) for a, c, _, _ in frags for h in range(a, a + c)]
        arena = np.frombuffer(b"".join(items), np.uint8)
        ln = np.array([len(it) for it in items], np.uint32)
        off = (np.cumsum(ln, dtype=np.uint64) - ln).astype(np.uint64)
        first = np.cumsum([0] + [c for _, c, _, _ in frags]).tolist()
        fr = [{"state": {k: (dict(v) if isinstance(v, dict) else v) for k, v in st.items()}, "tip": tip}
              for _, _, st, tip in frags]
        got = ctx.validate_candidates_tpraos(arena, off, ln, first, fr, chain["epoch_info"], limits,
                                             view_end_slot=view_end, extra_entropy=TP_EXTRA)
        return got, fr, first
    g = _genesis_state(chain["cfg"]["eta0"])
    _, fr0, _ = call([(0, 300, g, None)], (1 << 64) - 1)
    st300, tip300 = fr0[0]["state"], fr0[0]["tip"]
    assert fr0[0]["chain_stop"] == 300
    horizon = 2 * EPOCH_LEN + 100
    # from genesis; from mid-chain; a broken link; a counter ahead of the certificate's; empty
    ahead = {k: (dict(v) if isinstance(v, dict) else v) for k, v in st300.items()}
    D = ctx.verify_tpraos_header_bytes(chain["arena"], chain["off"][300:301], chain["len"][300:301], decoded=True)[1]
    ahead["counters"][hashlib.blake2b(bytes(D["cold_vk"][0]), digest_size=28).digest()] = int(D["ocert_n"][0]) + 3
    frags = [(0, n, g, None), (300, n - 300, st300, tip300), (301, 50, st300, tip300), (300, 20, ahead, tip300),
             (0, 0, g, None)]
    got, fr, first = call(frags, horizon)
    spec = tmp_path / "frags.txt"
    lines = [f"view_end {horizon}"]
    for a, c, st, tip in frags:
        t = "origin" if tip is None else f"{tip[0]}:{tip[1]}:{tip[2].hex()}"
        lines.append(f"frag {a} {c} {abi.state_encode(st).hex()} {t}")
    spec.write_text("\n".join(lines) + "\n")
    ef = str(tmp_path / "epoch.txt")
    _epoch_file(ef, chain, tpraos_extra=TP_EXTRA)
    out = _run(["--candidates-tpraos", chain["path"], ef, spec])
    assert out["phase"] == "candidates_tpraos" and out["spans_ok"] == 1 and out["items"] == len(got["verdict"])
    assert out["n_rows"] == got["n_rows"] and out["n_etas"] == len(got["etas"])
    assert out["stats"] == [got["stats"][k] for k in wire.STATS]
    cut = int(np.nonzero(chain["slots"] >= horizon)[0][0])
    for j, (f, o) in enumerate(zip(fr, out["fragments"])):
        assert o["verdicts"] == [int(v) for v in got["verdict"][first[j]:first[j + 1]]], j
        assert o["failures"] == [int(v) for v in got["failures"][first[j]:first[j + 1]]], j
        assert o["rows"] == [int(v) for v in got["row"][first[j]:first[j + 1]]], j
        assert (o["chain_stop"], o["processed"]) == (f["chain_stop"], f["processed"]), j
        tip = None if o["tip_origin"] else (o["tip_slot"], o["tip_block_no"], bytes.fromhex(o["tip_hash"]))
        assert tip == f["tip"], j
        assert o["state_cbor"] == abi.state_encode(f["state"]).hex(), j
    assert (fr[0]["chain_stop"], fr[0]["processed"]) == (cut, cut) == (fr[1]["chain_stop"] + 300, fr[1]["processed"] + 300)
    assert (fr[2]["chain_stop"], fr[2]["processed"]) == (0, 1) and got["verdict"][first[2]] == wire.V_DOESNT_FIT
    assert got["verdict"][first[3]] == 19 and got["failures"][first[3]] == abi.TPF_COUNTER_TOO_SMALL
    assert fr[4]["processed"] == 0 and got["stats"]["distinct_headers"] == n


def test_pbft_phase_equals_the_python_call(ctx, oracle, tmp_path):
    from praos_hip import abi, wire
    r = rng(0x0ffc)
    D = [bc.Delegate(r) for _ in range(7)]
    blocks = pc.make_chain(r, 40, lambda k: D[k % 7], epochs=3)
    delegs = pc.delegation(r, D)
    W, T, ES, PMAG = 14, 2, pc.EPOCH_SLOTS, pc.PM
    rows = pc.model_rows(blocks, delegs)
    ebb = [int(b.kind == 0) for b in blocks]
    n = len(blocks)
    assert pm.fold(rows, ebb, W, T, ES, delegs)[2] == n
    db = tmp_path / "byron"
    db.mkdir()
    _write_dir(db, blocks, per_chunk=41)

    def at(m):
        _, _, _, tip, st = pm.fold(rows[:m], ebb[:m], W, T, ES, delegs)
        return tip, st
    horizon = rows[100]["slot"]
    frags = [(0, n) + at(0), (42, 60) + at(42), (50, 30) + at(49), (0, 0) + at(0), (60, 20) + (at(60)[0], at(61)[1])]
    # the harness wraps header h as [0, [[kind, its size], #6.24(bytes)]]
    items = [wire.wrap(0, blocks[h].header, blocks[h].kind, len(blocks[h].header)) for a, c, _, _ in frags
             for h in range(a, a + c)]
    arena = np.frombuffer(b"".join(items), np.uint8)
    ln = np.array([len(it) for it in items], np.uint32)
    off = (np.cumsum(ln, dtype=np.uint64) - ln).astype(np.uint64)
    first = np.cumsum([0] + [c for _, c, _, _ in frags]).tolist()
    fr = [{"tip": tip, "state": list(st)} for _, _, tip, st in frags]
    got = ctx.validate_candidates_pbft(arena, off, ln, first, fr, abi.Context.pbft_params(W, T, ES, PMAG), delegs,
                                       view_end_slot=horizon)
    spec = tmp_path / "frags.txt"
    lines = [f"view_end {horizon}"]
    for a, c, tip, st in frags:
        t = "origin" if tip is None else f"{tip[0]}:{tip[1]}:{tip[2].hex()}:{tip[3]}"
        lines.append(f"frag {a} {c} {pm.state_encode(st).hex()} {t}")
    spec.write_text("\n".join(lines) + "\n")
    df = tmp_path / "delegs.txt"
    df.write_text("".join(f"{bytes(g).hex()} {bytes(d).hex()}\n" for g, d in delegs))
    out = _run(["--candidates-pbft", db, W, T, ES, PMAG, df, spec])
    assert out["phase"] == "candidates_pbft" and out["items"] == len(items) and out["n_rows"] == got["n_rows"]
    assert out["stats"] == [got["stats"][k] for k in wire.PBFT_STATS]
    for j, (f, o) in enumerate(zip(fr, out["fragments"])):
        assert o["verdicts"] == [int(v) for v in got["verdict"][first[j]:first[j + 1]]], j
        assert o["aux"] == [int(v) for v in got["aux"][first[j]:first[j + 1]]], j
        assert o["rows"] == [int(v) for v in got["row"][first[j]:first[j + 1]]], j
        assert (o["chain_stop"], o["processed"]) == (f["chain_stop"], f["processed"]), j
        tip = None if o["tip_origin"] else (o["tip_slot"], o["tip_block_no"], bytes.fromhex(o["tip_hash"]), o["tip_is_ebb"])
        assert tip == f["tip"], j
        assert o["state"] == pm.state_encode(f["state"]).hex(), j
    # what the fragments are: valid up to the horizon; valid to its end; a broken link; empty; a
    # window that has the next signer twice already
    assert (fr[0]["chain_stop"], fr[0]["processed"]) == (100, 100) and fr[1]["chain_stop"] == 58
    assert (fr[2]["chain_stop"], fr[2]["processed"]) == (0, 1) and got["verdict"][first[2]] == wire.V_DOESNT_FIT
    assert fr[3]["processed"] == 0
    assert got["verdict"][first[4]] == pm.V_EXCEEDED and got["aux"][first[4]] == 3
