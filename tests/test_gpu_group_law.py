"""GPU: every group formula of ge25519.hpp / scalarmult.hpp as points, in the default build and in
the ILP-4 build (praos_debug_ge), against the integer model (ec_model.py): small-order,
mixed-order, identity and cancelling inputs, coordinates at representatives in [p, 2^256).
Compared projectively with the model, and byte for byte between the two builds."""
import functools

import numpy as np
import pytest

import ec_model as em
from group_cases import aff_add, neg_aff, p1p1_variants, p3_variants, pack, points, unpack
from helpers import rng

pytestmark = pytest.mark.gpu

OPS = {"p2_dbl": 0, "add": 1, "madd": 2, "p1p1_to_p2": 3, "p1p1_to_p3": 4, "p3_to_cached": 5, "p3_dbl_to_p3": 6,
       "select_cached": 7, "select_niels": 8}


def _lift(c, i):
    """representatives of a table entry: canonical on even cases, the largest below 2^256 on odd ones"""
    return tuple(em.lift_max(v) for v in c) if i & 1 else tuple(v % em.P for v in c)


def _digit_row(d, t=0):
    return (int.from_bytes(d.to_bytes(4, "little", signed=True) + t.to_bytes(4, "little"), "little"), 0, 0, 0)


@functools.lru_cache(maxsize=None)
def _cases(op):
    """(p rows, q rows, check(out row) per case, description per case) -- built once per op"""
    pts = points()
    r = rng(40 + OPS[op])
    P, Q, chk, desc = [], [], [], []
    zero = (0, 0, 0, 0)
    if op in ("p2_dbl", "p3_to_cached", "p3_dbl_to_p3"):
        for name, a in pts:
            want = aff_add(a, a) if op != "p3_to_cached" else a
            f = {"p2_dbl": em.p1p1_is, "p3_to_cached": em.cached_is, "p3_dbl_to_p3": em.p3_is}[op]
            for k, c in enumerate(p3_variants(a, r)):
                P.append(c); Q.append(zero); chk.append((f, want)); desc.append((name, k))
    elif op in ("p1p1_to_p2", "p1p1_to_p3"):
        f = em.p2_is if op == "p1p1_to_p2" else em.p3_is
        for name, a in pts:
            for k, c in enumerate(p1p1_variants(a, r)):
                P.append(c); Q.append(zero); chk.append((f, a)); desc.append((name, k))
    elif op in ("add", "madd"):
        n = len(pts)
        for i, (name, a) in enumerate(pts):
            # P + P (2B through the addition among them), P + (-P), P + an unrelated point
            for qn, b in (("same", a), ("negated", neg_aff(a)), pts[(7 * i + 3) % n]):
                want = aff_add(a, b)
                zq = [1, em.P - 1, 2 ** 256 - 1, r.getrandbits(256) | 1]
                for k, c in enumerate(p3_variants(a, r)):
                    if op == "add":
                        q = _lift(em.to_cached(em.p3_with_z(b, zq[k % 4])), k // 4)
                    else:
                        q = _lift(em.to_niels(b), k) + (0,)
                    P.append(c); Q.append(q); chk.append((em.p1p1_is, want)); desc.append((name, qn, k))
    elif op == "select_cached":
        for i, (name, a) in enumerate(pts):
            var = p3_variants(a, r)
            mult = [em.to_affine(em.mul(k, a)) for k in range(9)]
            for d in range(-8, 8):
                want = mult[d] if d >= 0 else neg_aff(mult[-d])
                P.append(var[(i + d + 8) % len(var)]); Q.append(_digit_row(d))
                chk.append((em.cached_is, want)); desc.append((name, d))
    elif op == "select_niels":
        base = em.B
        for t in range(32):
            acc, mult = em.IDENT, [(0, 1)]
            for _ in range(128):
                acc = em.add(acc, base)
                mult.append(em.to_affine(acc))
            for d in range(-128, 128):
                want = mult[d] if d >= 0 else neg_aff(mult[-d])
                P.append(zero); Q.append(_digit_row(d, t)); chk.append((em.niels_is, want)); desc.append((t, d))
            base = em.scalarmult(256, base)
    return pack(P), pack(Q), chk, desc


@functools.lru_cache(maxsize=None)
def _run(ctx, op, build):
    p, q, _, _ = _cases(op)
    return ctx.debug_ge(build, OPS[op], p, q)


@pytest.mark.parametrize("build", [0, 1], ids=["default", "ilp4"])
@pytest.mark.parametrize("op", list(OPS))
def test_group_formula(ctx, op, build):
    p, q, chk, desc = _cases(op)
    out = unpack(_run(ctx, op, build))
    compared = 0
    for c, (f, want), d in zip(out, chk, desc):
        assert all(v < 2 ** 256 for v in c) and f(c, want), (op, build, d)
        compared += 1
    assert compared == len(chk) == len(p) > 0


@pytest.mark.parametrize("op", list(OPS))
def test_builds_agree_bytewise(ctx, op):
    """The two-way and the ILP-4 formulas run the same field operations on the same values: their
    raw outputs (not only the points) are equal."""
    a, b = _run(ctx, op, 0), _run(ctx, op, 1)
    assert a.shape == b.shape and len(a) == len(_cases(op)[2])
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert len(bad) == 0, (op, [_cases(op)[3][i] for i in bad[:5]])


def test_select_digit_out_of_range_is_an_argument_error(ctx):
    from praos_hip import abi
    p, q = pack([em.p3_with_z(em.B_AFF, 1)]), None
    for op, d, t in ((7, 8, 0), (7, -9, 0), (8, 128, 0), (8, -129, 0), (8, 1, 32)):
        q = pack([_digit_row(d, t)])
        with pytest.raises(abi.PraosError):
            ctx.debug_ge(0, op, p, q)
