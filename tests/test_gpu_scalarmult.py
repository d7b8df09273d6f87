"""GPU: the scalar-multiplication chains as the product code instantiates them (praos_debug_msm:
the three Straus chains, the two cached-key comb chains over tables the key cache's own precompute
builds, ge_scalarmult_var) and ge_scalarmult_base, in the default and the ILP-4 build, on structured
scalars and on small-order, mixed-order, identity and cancelling bases -- against the integer model
(ec_model.py), which multiplies by the integer scalar.  Encodings compared byte for byte."""
import functools

import numpy as np
import pytest

import ec_model as em
from group_cases import neg_aff, points
from helpers import arr, rng

pytestmark = pytest.mark.gpu

L = em.L
# variant -> (bits of sp, bits of the second scalar, which second term: "B", "Q" or None)
VARIANTS = {0: (253, 253, "B"), 1: (128, 253, "B"), 2: (253, 128, "Q"), 3: (253, 253, "B"), 4: (128, 253, "B"),
            5: (253, 0, None)}


def _rep(byte_pattern, n=32):
    return int.from_bytes(bytes(byte_pattern) * (n // len(byte_pattern)), "little")


def structured_scalars():
    s = [0, 1, 2, 8, L - 2, L - 1, 2 ** 252, 2 ** 253 - 1]
    s += [_rep([0x77]), _rep([0x88]), _rep([0x7F]), _rep([0x80]), _rep([0x81])]
    s += [_rep([0xFF, 0x7F]), _rep([0x00, 0x80]), _rep([0x01, 0x80])]        # 16-bit digits 7FFF, 8000, 8001
    s += [2 ** 128 - 1, 2 ** 127, 2 ** 128 - 2 ** 64]
    s += [d * 16 ** j for j in range(64) for d in (1, 7, 8, 9, 15)]
    s += byte_position_scalars()
    s += [d * 65536 ** j for j in range(16) for d in (1, 0x7FFF, 0x8000, 0x8001, 0xFFFF)]
    return s


def byte_position_scalars():
    return [d * 256 ** j for j in range(32) for d in (1, 0x7F, 0x80, 0x81, 0xFF)]


def _clip(s, bits):
    return s & (2 ** bits - 1)


def _bases(ctx):
    """The group-law test's points as encodings the device decodes (all of them: they are on the curve)."""
    pts = [(n, a) for n, a in points()]
    enc = [em.encode_affine(a) for _, a in pts]
    _, ok = ctx.debug_decode(arr(enc, 32))
    kept = [(n, a, e) for (n, a), e, k in zip(pts, enc, ok) if k]
    names = [n for n, _, _ in kept]
    assert kept and "order8" in names and "B+order8" in names and "identity" in names
    return kept


@functools.lru_cache(maxsize=None)
def _cases(ctx, variant):
    """Lanes (P, Q, sp, s2) of one variant and the encodings the model expects, computed once and
    used for both builds."""
    bp, b2, second = VARIANTS[variant]
    bases = _bases(ctx)
    by_name = {n: a for n, a, _ in bases}
    hand = [by_name[n] for n in ("B", "-B", "identity", "order8", "B+order8", "random0", "random3")]
    S = structured_scalars()
    r = rng(50 + variant)
    lanes = []
    # structured scalars in both terms, two passes over a handful of bases
    for ps in range(2):
        for i, s in enumerate(S):
            P = hand[(i + 3 * ps) % len(hand)]
            Q = hand[(2 * i + ps + 1) % len(hand)]
            lanes.append((P, Q, _clip(s, bp), _clip(S[(i * 37 + 11 + ps) % len(S)], b2) if b2 else 0))
    # random scalars over all bases
    for j in range(200):
        P = bases[j % len(bases)][1]
        Q = bases[(5 * j + 2) % len(bases)][1]
        lanes.append((P, Q, r.getrandbits(bp), r.getrandbits(b2) if b2 else 0))
    # cancelling terms: the result is the identity
    bx = em.B_AFF
    if second == "B":            # [sb]B - [sp]P with P = +-B
        for j in range(40):
            sp = r.getrandbits(bp) if j >= 8 else _clip(S[j], bp)
            lanes.append((bx, bx, sp, sp % L))
            lanes.append((neg_aff(bx), bx, sp, (L - sp) % L))
    elif second == "Q":          # [sp]P - [sq]Q with Q = +-P (P of order L for the negated form)
        for j in range(40):
            P = bases[(j * 3) % len(bases)][1]
            sq = r.getrandbits(b2)
            lanes.append((P, P, sq, sq))
            B2 = em.to_affine(em.mul(j + 2, bx))
            lanes.append((B2, neg_aff(B2), L - sq, sq))
    want = []
    for P, Q, sp, s2 in lanes:
        a = em.mul(sp, P)
        if second == "B":
            res = em.add(em.mul(s2, bx), em.neg(a))
        elif second == "Q":
            res = em.add(a, em.neg(em.mul(s2, Q)))
        else:
            res = a
        want.append(em.encode(res))
    ncancel = 80 if second else 0
    ident = em.encode(em.IDENT)
    assert all(w == ident for w in want[len(want) - ncancel:])
    return lanes, want


def _sc(xs):
    return arr([x.to_bytes(32, "little") for x in xs], 32)


def _launch(ctx, variant, build, lanes):
    second = VARIANTS[variant][2]
    P = arr([em.encode_affine(l[0]) for l in lanes], 32)
    Q = arr([em.encode_affine(l[1]) for l in lanes], 32)
    sp, s2 = _sc([l[2] for l in lanes]), _sc([l[3] for l in lanes])
    if second == "B":
        return ctx.debug_msm(variant, build, P, sp, sb=s2)
    if second == "Q":
        return ctx.debug_msm(variant, build, P, sp, Q=Q, sq=s2)
    return ctx.debug_msm(variant, build, P, sp)


@pytest.mark.parametrize("build", [0, 1], ids=["default", "ilp4"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_msm_variant(ctx, variant, build):
    lanes, want = _cases(ctx, variant)
    assert 1000 <= len(lanes) <= 2000
    out = _launch(ctx, variant, build, lanes)
    compared = 0
    for l, o, w in zip(lanes, out, want):
        assert bytes(o) == w, (variant, build, em.encode_affine(l[0]).hex(), em.encode_affine(l[1]).hex(),
                               hex(l[2]), hex(l[3]))
        compared += 1
    assert compared == len(lanes) == len(want)


@pytest.mark.parametrize("build", [0, 1], ids=["default", "ilp4"])
def test_comb16_entries(ctx, build):
    """Single entries of the radix-2^16 comb (524,288 points built once per context): variant 3 with
    sp = 0 and sb = d 65536^j, every j (the top digit clipped to the recoding's 2^253)."""
    r = rng(60)
    ds = [1, 2, 0x7FFF, 0x8000, 0x8001, 0xFFFF] + [r.getrandbits(16) | 1 for _ in range(64)]
    sbs = [_clip(d * 65536 ** j, 253) for j in range(16) for d in ds]
    lanes = [(em.B_AFF, em.B_AFF, 0, s) for s in sbs]
    out = _launch(ctx, 3, build, lanes)
    compared = 0
    for s, o in zip(sbs, out):
        assert bytes(o) == em.encode(em.mul(s, em.B_AFF)), hex(s)
        compared += 1
    assert compared == 16 * 70


def test_scalarmult_base_single_table_reads(ctx):
    """ge_scalarmult_base on d 256^j: one entry of one table of the radix-256 comb each."""
    ss = byte_position_scalars()
    out = ctx.debug_scalarmult_base(_sc(ss))
    compared = 0
    for s, o in zip(ss, out):
        assert bytes(o) == em.encode(em.mul(s, em.B_AFF)), hex(s)
        compared += 1
    assert compared == len(ss) == 160


def test_msm_rejects_scalars_out_of_range(ctx):
    from praos_hip import abi
    P = arr([em.encode_affine(em.B_AFF)], 32)
    ok, big, mid = _sc([5]), _sc([2 ** 253]), _sc([2 ** 128])
    bad = [(0, dict(sp=big, sb=ok)), (0, dict(sp=ok, sb=big)), (1, dict(sp=mid, sb=ok)), (2, dict(sp=ok, Q=P, sq=mid)),
           (2, dict(sp=big, Q=P, sq=ok)), (3, dict(sp=ok, sb=big)), (4, dict(sp=mid, sb=ok)), (5, dict(sp=big))]
    for variant, kw in bad:
        with pytest.raises(abi.PraosError):
            ctx.debug_msm(variant, 0, P, **kw)
