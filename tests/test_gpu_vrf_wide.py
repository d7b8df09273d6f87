"""The wide tier of the VRF key cache (k_keys.hip, scalarmult.hpp straus_pos): a VRF key used often
enough in a batch gets a table for every 6-bit digit position of the challenge c < 2^128, and the
U = [s]B - [c]Y chains of its headers run 22 additions without a doubling.  The group element is
the chunk tier's, so every encoding and verdict is identical.

  - the chain alone (praos_debug_msm variant 6, wide tables from the key cache's own precompute)
    on crafted challenges -- every digit value at every position, the recoding's carry into digit
    21 -- and random ones, against the integer model and the chunk-tier chain (variant 4);
  - Praos header batches with the tier on (threshold 2) and off, in the three-kernel and the fused
    U + join form, with the cap at one wide key (both tiers in one batch), and with a repeated VRF
    key that does not decode: outputs equal byte for byte and equal to the oracle;
  - a staged TPraos batch, tier on and off;
  - the pool-key store has no wide tier (not built): a resident batch run with the tier on and
    then with the store on gives the same outputs, and the store runs report no wide key.

A VRF key that does not decode is covered through the header batch only (three headers under it,
bit 0x0400 asserted): praos_debug_msm returns encodings, not flags.  Such a key's tables are built
from the point the failed decode left and straus_pos does read them, as the chunk tier's chain
reads its tables; the result is discarded by the key flag.
"""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import ec_model as em
from helpers import arr, b2b, rng

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
L = em.L
FIELDS = ("bits", "pool_idx", "beta", "leader", "nonce")
BITS_FROM_ORACLE = 0x0001 | 0x0002 | 0x0004 | 0x0008 | 0x0010 | 0x0100 | 0x0200 | 0x0400 | 0x0800 | 0x1000


def _golden_vrf_key():
    kats = json.load(open(os.path.join(HERE, "golden", "reference_kats.json")))["kats"]
    k = [k for k in kats if k["kind"] == "praos"][0]
    return bytes.fromhex(k["vrf_vk"])


def crafted_challenges():
    """c < 2^128 by its 6-bit fields (the chain's digit k is field k of c + sum 32 64^k, minus 32)."""
    def fields(v, n=22):
        return sum(v << (6 * k) for k in range(n)) & (2 ** 128 - 1)
    cs = [0, 1, 2 ** 128 - 1]
    # every field 0x20 (w's field 0: digit -32, then carries), 0x1f (digit 31), 0x00 (digit 0: the
    # zero select), 0x3f (digit 31 + a carry chain through every position)
    cs += [fields(0x20), fields(0x1F), fields(0x00), fields(0x3F)]
    # one non-zero digit at each of the 22 positions (position 21: bits 126, 127)
    for k in range(22):
        for d in (1, 0x1F, 0x20, 0x3F):
            c = d << (6 * k)
            if 0 < c < 2 ** 128:
                cs.append(c)
    cs += [2 ** 127, 2 ** 126, 3 << 126, 2 ** 128 - 2 ** 126, (2 ** 128 - 1) ^ fields(0x20)]
    return cs


def _sc(xs):
    return arr([x.to_bytes(32, "little") for x in xs], 32)


def test_wide_chain_crafted_and_random(ctx):
    r = rng(91)
    Y = em.decode(_golden_vrf_key())
    assert Y is not None
    Y2 = em.to_affine(em.mul(0x1234567, em.B_AFF))
    crafted = crafted_challenges()
    assert len(crafted) > 80 and all(0 <= c < 2 ** 128 for c in crafted)
    lanes = [(Y, c, r.getrandbits(253) % L) for c in crafted]
    lanes += [(Y, c, 0) for c in crafted[:8]]
    lanes += [(Y if j % 2 else Y2, r.getrandbits(128), r.getrandbits(253) % L) for j in range(64)]
    P = arr([em.encode_affine(a) for a, _, _ in lanes], 32)
    sp, sb = _sc([c for _, c, _ in lanes]), _sc([s for _, _, s in lanes])
    wide = ctx.debug_msm(6, 0, P, sp, sb=sb)
    chunk = ctx.debug_msm(4, 0, P, sp, sb=sb)
    wide4 = ctx.debug_msm(6, 1, P, sp, sb=sb)        # the tables' first pass from the ILP-4 module
    compared = 0
    for (a, c, s), w, k, w4 in zip(lanes, wide, chunk, wide4):
        want = em.encode(em.add(em.mul(s, em.B_AFF), em.neg(em.mul(c, a))))
        assert bytes(w) == want, ("wide", hex(c), hex(s))
        assert bytes(k) == want, ("chunk", hex(c), hex(s))
        assert bytes(w4) == want, ("wide, ilp4 precompute", hex(c), hex(s))
        compared += 1
    assert compared == len(lanes) >= 64 + 80


def test_wide_chain_rejects_out_of_range(ctx):
    from praos_hip import abi
    P = arr([em.encode_affine(em.B_AFF)], 32)
    for kw in (dict(sp=_sc([2 ** 128]), sb=_sc([5])), dict(sp=_sc([5]), sb=_sc([2 ** 253]))):
        with pytest.raises(abi.PraosError):
            ctx.debug_msm(6, 0, P, **kw)


# ---------------------------------------------------------------- header batches
def _chain(c, n, npools, corrupt_per_10000, seed):
    from praos_hip import abi, fixed
    c_raw = fixed.active_slot_log(Fraction(1, 20))
    p = abi.params(slots_per_kes_period=129600, max_kes_evo=62, c_raw=c_raw)
    eta0 = b2b(b"wide-tier")
    H, pools, corrupted = c.synthesize(n, npools, p, eta0, seed, first_slot=1000, slot_stride=20, body_len=397,
                                       corrupt_per_10000=corrupt_per_10000)
    sig = [fixed.from_rational(Fraction(1, npools))] * npools
    pool_list = [(h, v, s) for (h, v), s in zip(pools, sig)]
    return H, pool_list, corrupted, p, c_raw, eta0


def _run(c, H, wide, cap=0):
    c.set_vrf_wide(wide, cap)
    try:
        b = c.upload(H)
        try:
            c.run(b)
            c.sync()
            out = c.download(b, len(H["slot"]))
            st = c.batch_stats(b)
        finally:
            c.free(b)
    finally:
        c.set_vrf_wide()
    return out, st


@pytest.fixture(scope="module")
def batch512(ctx, oracle):
    """512 Praos headers of 4 pools, 1 % corrupted, three of them under one VRF key that is not on
    the curve (a cached key whose flag rejects it); the oracle's results, computed once."""
    H, pool_list, corrupted, p, c_raw, eta0 = _chain(ctx, 512, 4, 100, b"\x61" * 32)
    bad = next(y.to_bytes(32, "little") for y in range(2, 200) if not oracle.decode_ok(y.to_bytes(32, "little")))
    for i in (77, 200, 201):
        H["vrf_vk"][i] = np.frombuffer(bad, np.uint8)
    ep = oracle.make_epoch(eta0, 129600, 62, c_raw, pool_list)
    ref = []
    for i in range(512):
        off, ln = int(H["body_off"][i]), int(H["body_len"][i])
        h = {"slot": int(H["slot"][i]), "cold_vk": bytes(H["cold_vk"][i]), "vrf_vk": bytes(H["vrf_vk"][i]),
             "vrf_out": bytes(H["vrf_out"][i]), "vrf_proof": bytes(H["vrf_proof"][i]),
             "hot_vk": bytes(H["hot_vk"][i]), "n": int(H["ocert_n"][i]), "c0": int(H["ocert_c0"][i]),
             "ocert_sig": bytes(H["ocert_sig"][i]), "kes_sig": bytes(H["kes_sig"][i]),
             "body": bytes(H["body_bytes"][off:off + ln])}
        ref.append(oracle.praos_header(ep, h))
    return H, pool_list, corrupted, p, eta0, ref


def _check_oracle(out, ref, pool_list):
    hash_of = {h: i for i, (h, _, _) in enumerate(pool_list)}
    for i, r in enumerate(ref):
        assert int(out["bits"][i]) & BITS_FROM_ORACLE == r["bits"], (i, hex(out["bits"][i]), hex(r["bits"]))
        assert bytes(out["beta"][i]) == r["beta"], i
        assert bytes(out["leader"][i]) == r["leader"], i
        assert bytes(out["nonce"][i]) == r["nonce"], i
        assert int(out["pool_idx"][i]) == hash_of.get(r["issuer_hash"], -1), i


def _tier_cases(c, batch):
    H, pool_list, corrupted, p, eta0, ref = batch
    c.set_epoch(eta0, pool_list, p)
    off, st_off = _run(c, H, 0)
    on, st_on = _run(c, H, 2)
    one, st_one = _run(c, H, 2, cap=1)
    assert st_off["vrf_wide_keys"] == 0 and st_off["vrf_wide_hits"] == 0
    # the 4 pools' keys and the repeated bad key are wide; their headers leave the chunk tier's list
    assert st_on["vrf_wide_keys"] >= 5 and st_on["vrf_wide_hits"] >= 480, st_on
    assert st_on["vrf_hits"] == st_off["vrf_hits"] and st_on["vrf_misses"] == st_off["vrf_misses"]
    # cap 1: one wide key, the other keys' hits stay in the chunk tier
    assert st_one["vrf_wide_keys"] == 1 and 0 < st_one["vrf_wide_hits"] < st_one["vrf_hits"], st_one
    assert st_one["vrf_hits"] == st_off["vrf_hits"]
    for o in (on, one):
        for f in FIELDS:
            np.testing.assert_array_equal(o[f], off[f], err_msg=f)
    _check_oracle(on, ref, pool_list)
    _check_oracle(off, ref, pool_list)
    assert all(int(on["bits"][i]) & 0x0400 for i in (77, 200, 201))     # the bad key's proofs rejected
    assert any(corrupted) and all(int(on["bits"][i]) != 0 for i in range(512) if corrupted[i])


def test_headers_three_kernel_form(ctx, batch512):
    """512 headers run the three-kernel VRF (k_vrf_u / k_vrf_u_w, k_vrf_join)."""
    _tier_cases(ctx, batch512)


def test_headers_fused_form(batch512):
    """PRAOS_VRF3=0: U + join in one kernel (k_vrf_fin / k_vrf_fin_w), the large batches' form."""
    import praos_hip
    os.environ["PRAOS_VRF3"] = "0"
    try:
        c2 = praos_hip.Context(0)
    finally:
        del os.environ["PRAOS_VRF3"]
    try:
        _tier_cases(c2, batch512)
    finally:
        c2.close()


def test_tpraos_staged(ctx):
    """A staged TPraos batch (U of both certificates against the VRF key cache), tier on and off."""
    from praos_hip import abi, fixed
    from praos_hip.chunk import pack_chunk
    c_raw = fixed.active_slot_log(Fraction(1, 2))
    p = abi.params(c_raw=c_raw)
    eta0 = b2b(b"wide-tier-tpraos")
    n = 256
    H, pools, corrupted = ctx.synthesize(n, 6, p, eta0, b"\x62" * 32, first_slot=9000, slot_stride=5, body_len=0,
                                         corrupt_per_10000=400, tpraos=True)
    pool_list = [(h, v, fixed.from_rational(Fraction(1, 6))) for (h, v) in pools]
    ctx.set_epoch(eta0, pool_list, p)
    arena, off, ln = pack_chunk(H, era_tag=5)
    outs, stats = [], []
    try:
        for wide in (0, 2):
            ctx.set_vrf_wide(wide)
            b = ctx.upload_tpraos_bytes(arena, off, ln)
            try:
                ctx.run(b)
                ctx.sync()
                outs.append(ctx.download_tpraos(b, n))
                stats.append(ctx.batch_stats(b))
            finally:
                ctx.free(b)
    finally:
        ctx.set_vrf_wide()
    assert stats[0]["vrf_wide_hits"] == 0 and stats[1]["vrf_wide_keys"] >= 6 and stats[1]["vrf_wide_hits"] >= 240
    assert stats[0]["vrf_hits"] == stats[1]["vrf_hits"]
    assert set(outs[0]) == set(outs[1])
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)
    clean = corrupted == 0
    assert int((outs[1]["bits"][clean] & ~np.uint16(0x1000)).astype(bool).sum()) == 0
    assert np.count_nonzero(~clean) and int((outs[1]["bits"][~clean] == 0).sum()) == 0


def test_one_batch_tier_on_then_pool_key_store(ctx, batch512):
    """The tier is not built for the pool-key store: a run that uses the store has no wide tier.
    One resident batch run three times -- tier on, then twice with the store on (its entry ids
    continue the store's, past this batch's own entry arrays) -- gives the same outputs each time,
    and the store runs report no wide key."""
    from praos_hip import abi
    H, pool_list, corrupted, p, eta0, ref = batch512
    ctx.set_epoch(eta0, pool_list, p)
    n = len(H["slot"])
    outs, stats = [], []
    ctx.set_vrf_wide(2, 0)
    b = ctx.upload(H)
    try:
        for mode in (0, 2, 1):
            ctx.set_option(abi.OPT_POOL_KEYS, mode)
            ctx.run(b)
            ctx.sync()
            outs.append(ctx.download(b, n))
            stats.append(ctx.batch_stats(b))
    finally:
        ctx.free(b)
        ctx.set_option(abi.OPT_POOL_KEYS, -1)
        ctx.set_vrf_wide()
    assert stats[0]["vrf_wide_keys"] >= 5 and stats[0]["vrf_wide_hits"] >= 480
    for st in stats[1:]:
        assert st["vrf_wide_keys"] == 0 and st["vrf_wide_hits"] == 0 and st["vrf_misses"] == 0, st
        assert st["vrf_hits"] == n
    for o in outs[1:]:
        for f in FIELDS:
            np.testing.assert_array_equal(o[f], outs[0][f], err_msg=f)
