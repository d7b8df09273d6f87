"""CPU: the integer reference model (ec_model.py) is right where the standard and the C oracle
can tell, and the operand lists of the field-product tests reach the device's rare carry paths
(a condition on the inputs, evaluated with the limb-level model of the products)."""
import pytest

import ec_model as em
from field_cases import MULTI_OPS, multi_lanes, ring_pairs
from helpers import rbytes, rng


def test_base_point_is_rfc8032():
    x = 15112221349535400772501151409588531511454012693041857206046113283949847762202
    y = 46316835694926478169428394003475163141307993866256225615783033603165251855960
    assert em.B_AFF == (x, y) and em.on_curve(x, y)
    assert em.encode(em.B) == bytes([0x58] + [0x66] * 31)
    assert em.decode(bytes([0x58] + [0x66] * 31)) == em.B_AFF
    assert em.equal(em.scalarmult(em.L, em.B), em.IDENT)
    assert not em.equal(em.scalarmult(em.L - 1, em.B), em.IDENT)


def test_small_order_points():
    o2, o4, o8 = em.small_order_points()
    assert [em.order(q) for q in (o2, o4, o8)] == [2, 4, 8]
    assert all(em.on_curve(*q) for q in (o2, o4, o8))
    mixed = em.to_affine(em.add(em.B, em.affine_to_ext(o8)))
    assert em.on_curve(*mixed)
    # the integer scalar matters: [L](B + T8) = [L mod 8]T8, not the identity
    assert em.equal(em.mul(em.L, mixed), em.scalarmult(em.L % 8, em.affine_to_ext(o8)))
    assert not em.equal(em.mul(em.L, mixed), em.IDENT)


def test_model_agrees_with_oracle(oracle):
    r = rng(21)
    for _ in range(8):
        s = r.getrandbits(255)
        sb = s.to_bytes(32, "little")
        assert em.encode(em.mul(s, em.B_AFF)) == oracle.scalarmult_base(sb)
        assert em.encode(em.scalarmult(s, em.B)) == oracle.scalarmult_base(sb)
    for _ in range(8):
        pk = oracle.ed25519_pk(rbytes(r, 32))
        a = em.decode(pk)
        assert a is not None and em.on_curve(*a) and em.encode_affine(a) == pk
        ok, enc = oracle.reencode(pk)
        assert ok and enc == pk


def test_windowed_mul_is_double_and_add():
    r = rng(22)
    _, _, o8 = em.small_order_points()
    base = em.to_affine(em.add(em.mul(r.getrandbits(250), em.B_AFF), em.affine_to_ext(o8)))
    for k in [0, 1, 2, 15, 16, em.L, 2 ** 253 - 1, 2 ** 256 - 1] + [r.getrandbits(256) for _ in range(6)]:
        assert em.equal(em.mul(k, base), em.scalarmult(k, em.affine_to_ext(base)))


def test_forced_representatives():
    r = rng(23)
    o2, o4, o8 = em.small_order_points()
    pts = [em.B_AFF, (0, 1), o2, o4, o8, em.to_affine(em.mul(r.getrandbits(250), em.B_AFF))]
    raws = [em.P, em.P + 1, 2 * em.P - 1, 2 ** 256 - 1, 2 ** 256 - 38, 2 ** 255]
    for a in pts:
        for coord in range(4):
            for raw in raws:
                c = em.p3_force(a, coord, raw)
                assert all(0 <= v < 2 ** 256 for v in c) and em.p3_is(c, a)
                x, y = a
                if raw % em.P and (x, y, 1, x * y % em.P)[coord]:
                    assert c[coord] == raw
                else:
                    assert c[coord] >= em.P or coord == 2
                c = em.p1p1_force(a, coord, raw)
                assert all(0 <= v < 2 ** 256 for v in c) and em.p1p1_is(c, a)


def test_limb_model_matches_integers():
    for x, y in ring_pairs(3, 50):
        em.product_trace(x, y)          # asserts t == x y and the reduced value == x y mod p
        em.product_trace(x)


def _max_counts(square):
    """Carry counts no operand can exceed: every column sum grows with every limb, so all-ones
    operands maximise each column (a column of n products carries at most n - 1 times)."""
    m = 2 ** 256 - 1
    return em.product_trace(m, None if square else m)[3]


@pytest.mark.parametrize("name", list(MULTI_OPS))
def test_product_inputs_reach_rare_paths(name):
    """In every product slot of every interleaved op the operand list holds (a) a second fold of
    fe_reduce512 that carries out of limb 0, (b) a fold with k >= 38, and (c) for each column
    k = 1 .. 13 a carry count of at least 2 -- or, in the columns too short for that (columns 1
    and 13 of a product hold two terms and can carry once; the cross products of a squaring reach
    two carries only in columns 5 .. 9), the most the column can carry at all."""
    _, M, square = MULTI_OPS[name]
    lanes = multi_lanes(name)
    top = _max_counts(square)
    if not square:
        assert [min(2, c) for c in top[1:14]] == [1] + [2] * 11 + [1]
    else:
        assert [min(2, c) for c in top[1:14]] == [0, 0, 1, 1, 2, 2, 2, 2, 2, 1, 1, 0, 0]
    for m in range(M):
        carried = k38 = False
        best = [0] * 15
        for lane in lanes:
            a, b = lane[m]
            _, k, c, counts = em.product_trace(a, None if square else b)
            carried |= c
            k38 |= k >= 38
            best = [max(u, v) for u, v in zip(best, counts)]
        assert carried, (name, m)
        assert k38, (name, m)
        for col in range(1, 14):
            assert best[col] >= min(2, top[col]), (name, m, col)


def test_single_product_inputs_reach_rare_paths():
    """The same for the list test_fe_ring_ops and the aliased single products run (fe_mul, fe_sq):
    the cross product of the edge values holds (2^256 - 1)^2."""
    for square in (False, True):
        tr = [em.product_trace(x, None if square else y) for x, y in ring_pairs(1, 400)]
        assert any(t[2] for t in tr)
        top = _max_counts(square)
        for col in range(1, 14):
            assert max(t[3][col] for t in tr) >= min(2, top[col])
