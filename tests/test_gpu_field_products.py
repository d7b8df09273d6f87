"""GPU: the interleaved field products (fe_mul2, fe_sq2, fe_mul3, fe_mul4, fe_sq4: the routines
the group formulas really run on), plain and with outputs aliasing inputs, and fe_neg / fe_chi /
fe_iszero / fe_isnegative on weakly reduced inputs, against Python integers.  Bit-exact mod p.
test_ec_model.py checks on the CPU that these operand lists reach the rare carry paths."""
import numpy as np
import pytest

from ec_model import M256, P
from field_cases import ALIASED, MULTI_OPS, multi_lanes, ring_pairs, weak_values

pytestmark = pytest.mark.gpu


def _b(x):
    return x.to_bytes(32, "little")


def _int(row):
    return int.from_bytes(bytes(row), "little")


def _to(xs):
    return np.frombuffer(b"".join(_b(x) for x in xs), np.uint8).reshape(-1, 32).copy()


@pytest.mark.parametrize("aliased", [False, True], ids=["plain", "aliased"])
@pytest.mark.parametrize("name", list(MULTI_OPS))
def test_fe_multi(ctx, name, aliased):
    code, M, square = MULTI_OPS[name]
    lanes = multi_lanes(name)
    assert 0 < len(lanes) <= 4096
    buf = bytearray()
    for lane in lanes:
        for m in range(4):
            a, b = lane[m] if m < M else (0, 0)
            buf += _b(a) + _b(b)
    ins = np.frombuffer(bytes(buf), np.uint8).reshape(len(lanes), 8, 32).copy()
    out = ctx.debug_fe_multi(code | (ALIASED if aliased else 0), ins)
    compared = 0
    for lane, o in zip(lanes, out):
        for m in range(4):
            z = _int(o[m])
            if m >= M:
                assert z == 0
                continue
            a, b = lane[m]
            want = (a * a if square else a * b) % P
            assert z < M256 and z % P == want, (name, aliased, m, [(hex(x), hex(y)) for x, y in lane])
            compared += 1
    assert compared == len(lanes) * M


def test_fe_neg_chi_predicates(ctx):
    xs = weak_values()
    ng = ctx.debug_fe(9, _to(xs))
    chi = ctx.debug_fe(10, _to(xs))
    pr = ctx.debug_fe(11, _to(xs))
    compared = 0
    for x, a, b, c in zip(xs, ng, chi, pr):
        assert _int(a) % P == (-x) % P, hex(x)
        assert _int(b) % P == pow(x % P, (P - 1) // 2, P), hex(x)
        assert _int(c) == (1 if x % P == 0 else 0) | (((x % P) & 1) << 1), hex(x)
        compared += 1
    assert compared == len(xs)
    assert sum(1 for x in xs if x % P == 0) >= 3 and any(x >= 2 * P for x in xs)


@pytest.mark.parametrize("code", [12, 13, 14], ids=["mul_r_is_a", "mul_r_is_b", "sq_r_is_a"])
def test_fe_single_product_aliased(ctx, code):
    pairs = ring_pairs(1, 400)
    xs, ys = [x for x, _ in pairs], [y for _, y in pairs]
    out = ctx.debug_fe(code, _to(xs), _to(ys))
    compared = 0
    for x, y, o in zip(xs, ys, out):
        z = _int(o)
        assert z < M256 and z % P == (x * x if code == 14 else x * y) % P, (code, hex(x), hex(y))
        compared += 1
    assert compared == len(pairs)
