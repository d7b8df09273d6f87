"""GPU: forged certificates whose group equation holds (forged_cases.py, validated on the CPU by
test_forged_cases.py), so that ge_has_small_order, ge_is_canonical and sc_is_canonical are the
only barrier: through praos_verify_ocert and praos_verify_vrf, and planted three times each in a
synthesised chain so that they take the cached-key path, with the key cache on and off."""
from fractions import Fraction

import numpy as np
import pytest

import forged_cases as fc
from helpers import arr, b2b, rng

pytestmark = pytest.mark.gpu

BITS_FROM_ORACLE = 0x0001 | 0x0002 | 0x0004 | 0x0008 | 0x0010 | 0x0100 | 0x0200 | 0x0400 | 0x0800 | 0x1000


def test_forged_ocerts(ctx, oracle):
    cases = fc.ed25519_cases()
    ok = ctx.verify_ocert(arr([c["cold_vk"] for c in cases], 32), arr([c["hot_vk"] for c in cases], 32),
                          np.array([c["n"] for c in cases], np.uint64), np.array([c["c0"] for c in cases], np.uint64),
                          arr([c["sig"] for c in cases], 64))
    got = {(c["family"], c["name"]): bool(x) for c, x in zip(cases, ok)}
    want = {(c["family"], c["name"]): not c["forged"] for c in cases}
    assert got == want
    assert want == {(c["family"], c["name"]): oracle.ed25519_verify(c["cold_vk"], fc.ocert_msg(c["hot_vk"], c["n"], c["c0"]),
                                                                     c["sig"]) for c in cases}


def test_forged_vrf_proofs(ctx, oracle):
    cases = fc.vrf_cases(oracle)
    ok, beta = ctx.verify_vrf(arr([c["vrf_vk"] for c in cases], 32), arr([c["proof"] for c in cases], 80),
                              arr([c["alpha"] for c in cases], 32))
    assert {c["name"]: bool(x) for c, x in zip(cases, ok)} == {c["name"]: not c["forged"] for c in cases}
    for c, b in zip(cases, beta):
        assert (oracle.vrf_verify(c["vrf_vk"], c["proof"], c["alpha"]) is not None) == (not c["forged"])
        assert bytes(b) == oracle.vrf_proof_to_hash(c["proof"])              # the identity's beta, whatever the key


def _run_batch(ctx, H, keycache):
    from praos_hip import abi
    ctx.set_option(abi.OPT_KEYCACHE, keycache)
    ctx.set_option(abi.OPT_DEDUP, 0)
    try:
        b = ctx.upload(H)
        ctx.run(b)
        ctx.sync()
        st = ctx.batch_stats(b)
        o = ctx.download(b, len(H["slot"]))
        ctx.free(b)
    finally:
        ctx.set_option(abi.OPT_KEYCACHE, 2)
        ctx.set_option(abi.OPT_DEDUP, 1)
    return o, st


def test_forged_in_chain_cached_and_uncached(ctx, oracle):
    from praos_hip import abi, fixed
    c_raw = fixed.active_slot_log(Fraction(1, 20))
    p = abi.params(slots_per_kes_period=129600, max_kes_evo=62, c_raw=c_raw)
    eta0 = b2b(b"forged")
    n = 400
    H, pools, _ = ctx.synthesize(n, 5, p, eta0, b"\x66" * 32, first_slot=1000, slot_stride=20, body_len=397,
                                 corrupt_per_10000=0)
    pool_list = [(h, v, fixed.from_rational(Fraction(1, 5))) for h, v in pools]
    ctx.set_epoch(eta0, pool_list, p)
    u8 = lambda b: np.frombuffer(b, np.uint8)
    forged_oc, control_oc, forged_vrf, touched = [], [], [], set()
    eds = fc.ed25519_cases()
    for j, c in enumerate(eds):                                               # each key three times: cached
        for k in range(3):
            i = 10 + 3 * j + k
            H["cold_vk"][i], H["hot_vk"][i], H["ocert_sig"][i] = u8(c["cold_vk"]), u8(c["hot_vk"]), u8(c["sig"])
            H["ocert_n"][i], H["ocert_c0"][i] = c["n"], c["c0"]
            (forged_oc if c["forged"] else control_oc).append(i)
            touched.add(i)
    assert max(touched) < 200
    r = rng(0xc4a1)
    for j, y_enc in enumerate(fc.torsion_encodings()):
        for k in range(3):
            i = 200 + 3 * j + k
            alpha = oracle.mk_input_vrf(int(H["slot"][i]), eta0)
            H["vrf_vk"][i], H["vrf_proof"][i] = u8(y_enc), u8(fc.vrf_forge(oracle, y_enc, alpha, r))
            forged_vrf.append(i)
            touched.add(i)
    o1, st1 = _run_batch(ctx, H, 2)
    o0, st0 = _run_batch(ctx, H, 0)
    n_cold = len({c["cold_vk"] for c in eds})
    assert n_cold == 18 and st1["cold_keys"] >= n_cold and st1["vrf_keys"] >= 14
    assert st0["cold_keys"] == 0 and st0["vrf_keys"] == 0 and st0["cold_hits"] == 0 and st0["vrf_hits"] == 0
    # every planted key recurs, so only a pool's single header can miss: the planted ones are on the cached path
    assert st1["cold_misses"] <= 5 and st1["vrf_misses"] <= 5
    assert st1["cold_hits"] + st1["cold_misses"] == n and st1["vrf_hits"] > 300
    for key in ("bits", "beta", "leader", "nonce", "pool_idx"):
        assert np.array_equal(o1[key], o0[key]), key
    ep = oracle.make_epoch(eta0, 129600, 62, c_raw, pool_list)
    for i in range(n):
        off, ln = int(H["body_off"][i]), int(H["body_len"][i])
        h = {"slot": int(H["slot"][i]), "cold_vk": bytes(H["cold_vk"][i]), "vrf_vk": bytes(H["vrf_vk"][i]),
             "vrf_out": bytes(H["vrf_out"][i]), "vrf_proof": bytes(H["vrf_proof"][i]),
             "hot_vk": bytes(H["hot_vk"][i]), "n": int(H["ocert_n"][i]), "c0": int(H["ocert_c0"][i]),
             "ocert_sig": bytes(H["ocert_sig"][i]), "kes_sig": bytes(H["kes_sig"][i]),
             "body": bytes(H["body_bytes"][off:off + ln])}
        ref = oracle.praos_header(ep, h)
        assert int(o1["bits"][i]) & BITS_FROM_ORACLE == ref["bits"], (i, hex(o1["bits"][i]), hex(ref["bits"]))
        assert bytes(o1["beta"][i]) == ref["beta"]
    bits = [int(b) for b in o1["bits"]]
    assert all(bits[i] & abi.BIT_OCERT_SIG for i in forged_oc)
    assert not any(bits[i] & abi.BIT_OCERT_SIG for i in control_oc) and len(control_oc) == 9
    assert all(bits[i] & abi.BIT_VRF_PROOF for i in forged_vrf)
    clean = [i for i in range(n) if i not in touched]                         # the chain's own headers: controls
    assert len(clean) > 200 and not any(bits[i] & (abi.BIT_OCERT_SIG | abi.BIT_VRF_PROOF) for i in clean)
