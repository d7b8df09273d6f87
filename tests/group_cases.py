"""Points and coordinate representatives shared by test_gpu_group_law.py and
test_gpu_scalarmult.py (built from ec_model.py alone)."""
import functools

import numpy as np

import ec_model as em
from helpers import rng

FORCED_RAWS = [em.P, em.P + 1, 2 * em.P - 1, 2 ** 256 - 1, 2 ** 256 - 38, 2 ** 255]


@functools.lru_cache(maxsize=None)
def points():
    """(name, affine point): B, -B, the identity, points of order 2, 4 and 8, B + the order-8 point,
    then 64 random points (every fourth one with a small-order component added)."""
    o2, o4, o8 = em.small_order_points()
    bx, by = em.B_AFF
    pts = [("B", em.B_AFF), ("-B", ((-bx) % em.P, by)), ("identity", (0, 1)), ("order2", o2), ("order4", o4),
           ("order8", o8), ("B+order8", em.to_affine(em.add(em.B, em.affine_to_ext(o8))))]
    r = rng(31)
    for i in range(64):
        q = em.mul(r.getrandbits(252), em.B_AFF)
        if i % 4 == 3:
            q = em.add(q, em.scalarmult(1 + (i // 4) % 7, em.affine_to_ext(o8)))
        pts.append((f"random{i}", em.to_affine(q)))
    assert all(em.on_curve(*a) for _, a in pts)
    return tuple(pts)


def neg_aff(a):
    return ((-a[0]) % em.P, a[1])


def aff_add(a, b):
    return em.to_affine(em.add(em.affine_to_ext(a), em.affine_to_ext(b)))


def _z_values(r):
    return [1, em.P - 1, 2 ** 256 - 1, r.getrandbits(256) | 1]


def p3_variants(a, r):
    """Extended coordinates of the affine point: Z in {1, p - 1, 2^256 - 1, random}, then each of
    X, Y, Z, T in turn forced to each raw representative of FORCED_RAWS (28 variants)."""
    v = [em.p3_with_z(a, z) for z in _z_values(r)]
    v += [em.p3_force(a, c, raw) for c in range(4) for raw in FORCED_RAWS]
    return v


def p1p1_variants(a, r):
    zs, ts = _z_values(r), _z_values(r)
    v = [em.p1p1_with(a, zs[k], ts[(k + 1) % 4]) for k in range(4)]
    v += [em.p1p1_force(a, c, raw) for c in range(4) for raw in FORCED_RAWS]
    return v


def pack(rows):
    """rows of four integers below 2^256 -> (n, 128) uint8"""
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for row in rows for x in row), np.uint8).reshape(
        -1, 128).copy()


def unpack(a):
    return [tuple(int.from_bytes(bytes(row[32 * k:32 * k + 32]), "little") for k in range(4)) for row in a]
