"""The candidates call from C (integration/c/ffi_harness.c --candidates, the sequence of Batch.hs
validateCandidateFragments): over the replay tests' ImmutableDB, wrapped in the node-to-node
encoding by the harness itself, its output equals the Python call's -- verdicts, rows, stops, tips
and the PraosState CBOR of every fragment, one of them stopped by a broken link, with a forecast
horizon."""
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_ffi import HARNESS, _epoch_file
from test_gpu_replay import ENV, EPOCH_LEN, _genesis_state, chain  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def test_harness_phase_equals_the_python_call(ctx, chain, tmp_path):  # noqa: F811
    from praos_hip import abi, wire
    n = len(chain["off"])
    hdrs = [bytes(chain["arena"][int(o):int(o) + int(m)]) for o, m in zip(chain["off"], chain["len"])]
    limits = (ENV["max_major_pv"], ENV["lv_prot_major"], ENV["max_header_size"], ENV["max_body_size"])
    # the state and tip 300 headers in: one clean fragment's own result
    ctx.set_epoch(chain["nonces"][0], chain["pools"], chain["params"])

    def call(frags, view_end):
        """frags: [(first, count, state, tip)] over the chain's headers, wrapped as era 5."""
        items = [wire.wrap(5, hdrs[h]) for a, c, _, _ in frags for h in range(a, a + c)]
        arena = np.frombuffer(b"".join(items), np.uint8)
        ln = np.array([len(it) for it in items], np.uint32)
        off = (np.cumsum(ln, dtype=np.uint64) - ln).astype(np.uint64)
        first = np.cumsum([0] + [c for _, c, _, _ in frags]).tolist()
        fr = [{"state": {k: (dict(v) if isinstance(v, dict) else v) for k, v in st.items()}, "tip": tip}
              for _, _, st, tip in frags]
        got = ctx.validate_candidates(arena, off, ln, first, fr, chain["epoch_info"], limits, view_end_slot=view_end)
        return got, fr, first
    g = _genesis_state(chain["cfg"]["eta0"])
    _, fr0, _ = call([(0, 300, g, None)], (1 << 64) - 1)
    st300, tip300 = fr0[0]["state"], fr0[0]["tip"]
    assert fr0[0]["chain_stop"] == 300
    horizon = 3 * EPOCH_LEN + 100
    frags = [(0, n, g, None), (300, n - 300, st300, tip300), (301, 50, st300, tip300), (0, 0, g, None)]
    got, fr, first = call(frags, horizon)
    spec = tmp_path / "frags.txt"
    lines = [f"view_end {horizon}"]
    for a, c, st, tip in frags:
        t = "origin" if tip is None else f"{tip[0]}:{tip[1]}:{tip[2].hex()}"
        lines.append(f"frag {a} {c} {abi.state_encode(st).hex()} {t}")
    spec.write_text("\n".join(lines) + "\n")
    ef = str(tmp_path / "epoch.txt")
    _epoch_file(ef, chain)
    assert os.path.exists(HARNESS), "build it: make -C integration/c (done by __graft_entry__.build())"
    r = subprocess.run([HARNESS, "--candidates", chain["path"], ef, str(spec)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["phase"] == "candidates" and out["spans_ok"] == 1 and out["items"] == len(got["verdict"])
    assert out["n_rows"] == got["n_rows"] and out["n_etas"] == len(got["etas"])
    assert out["stats"] == [got["stats"][k] for k in wire.STATS]
    cut = int(np.nonzero(chain["slots"] >= horizon)[0][0])
    for j, (f, o) in enumerate(zip(fr, out["fragments"])):
        assert o["verdicts"] == [int(v) for v in got["verdict"][first[j]:first[j + 1]]], j
        assert o["rows"] == [int(v) for v in got["row"][first[j]:first[j + 1]]], j
        assert (o["chain_stop"], o["processed"]) == (f["chain_stop"], f["processed"]), j
        tip = None if o["tip_origin"] else (o["tip_slot"], o["tip_block_no"], bytes.fromhex(o["tip_hash"]))
        assert tip == f["tip"], j
        assert o["state_cbor"] == abi.state_encode(f["state"]).hex(), j
    # what the fragments are: valid up to the horizon; the same from mid-chain; a broken link; empty
    assert (fr[0]["chain_stop"], fr[0]["processed"]) == (cut, cut) == (fr[1]["chain_stop"] + 300, fr[1]["processed"] + 300)
    assert (fr[2]["chain_stop"], fr[2]["processed"]) == (0, 1) and got["verdict"][first[2]] == wire.V_DOESNT_FIT
    assert fr[3]["processed"] == 0 and got["stats"]["distinct_headers"] == n
