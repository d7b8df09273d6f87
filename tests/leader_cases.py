"""Case list of the leader check over the whole range of x the host accepts (0 .. 16 R, R =
10^34): the negative acc' - e branch, err * x up to 250 bits, divisors up to the last iteration,
and decisions that are not monotone in the leader value.  The model is leader_python of
tests/golden/make_leader_boundary.py, with sigma = 1 and c = -x so that it runs on x itself.
Pure Python and deterministic; test_leader_cases.py checks the claims, test_gpu_leader_range.py
runs the list on the device."""
import functools
import importlib.util
import math
import os
import random

_spec = importlib.util.spec_from_file_location(
    "make_leader_boundary", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_leader_boundary.py"))
_mlb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mlb)
leader_python = _mlb.leader_python

R = 10 ** 34
X_MAX = 16 * R
XS = (0, 1, 2, R // 10 ** 9, R // 20, R // 2, R, 3 * R // 2, 2 * R, 3 * R, 5 * R, 10 * R, 16 * R - 1, 16 * R)
STEPS = 45


def pair_for(x, exact):
    """(sigma_fp, c_raw) with -((sigma_fp * c_raw) // R) == x (the reference's x = -(sigma * c) in Fixed
    E34, i.e. ceil(sigma_fp |c_raw| / R)); exact: R divides the product, else the ceiling rounds up."""
    if x == 0:                                    # x = 0 both ways: c = 0, or no stake under a negative c
        return (R, 0) if exact else (0, -(R // 20))
    s = R if exact else R - 3
    m = (x * R) // s
    assert -((s * -m) // R) == x and ((s * m) % R == 0) == exact, x
    return s, -m


def model(l, bits, x):
    """(is_leader, iterations) of checkLeaderNatValue at x = -(sigma c) given directly"""
    return leader_python(l, bits, R, -x)


@functools.lru_cache(None)
def recurrence(x):
    """The Taylor recurrence for STEPS iterations, decisions ignored: per iteration n the tuple
    (err * x, acc' + e, acc' - e) of the values iteration n forms."""
    out = []
    err, acc = x, R
    for n in range(STEPS):
        errp = ((err * x) // R) // (n + 2)
        accp = acc + err
        e = 3 * errp
        out.append((err * x, accp + e, accp - e))
        err, acc = errp, accp
    return out


def boundaries(x, bits):
    """The leader values at which a comparison of some iteration flips: floor(N / D) >= T, with
    N = 2^bits R and D = 2^bits - l, holds exactly for l >= l_T = 2^bits - floor(N / T)."""
    top = 1 << bits
    out = set()
    for _, hi, lo in recurrence(x):
        for t in (hi, lo):
            if t > 0:
                lt = top - (top * R) // t
                if lt >= 0:
                    out |= {lt - 1, lt, lt + 1}
    return out


def first_upper(x):
    """acc' + e of iteration 0"""
    return R + x + 3 * (((x * x) // R) // 2)


@functools.lru_cache(None)
def equality_points():
    """[(x, T)]: values of x whose first upper threshold T = acc' + e divides 2^bits R, so that
    some leader value gives floor(N / D) = N / D = T exactly and only `>=` against `>` decides
    (the boundaries above give N >= T D with equality only by accident: x = 0 at l = 0).
    T = R 2^k / 5^j; x solves R + x + 3 floor(floor(x^2 / R) / 2) = T where a solution exists."""
    out = []
    for j in range(8):
        for k in range(24):
            if (R << k) % 5 ** j:
                continue
            t = (R << k) // 5 ** j
            if not R < t <= first_upper(X_MAX):
                continue
            x0 = (math.isqrt(R * R + 6 * R * (t - R)) - R) // 3               # root of 1.5 x^2 / R + x + R = t
            out += [(x, t) for x in range(max(1, x0 - 8), x0 + 9) if x <= X_MAX and first_upper(x) == t][:1]
    return sorted(out)


def equalities(bits):
    """[(x, l)] with 2^bits R = T (2^bits - l) for x's first upper threshold T"""
    top = 1 << bits
    out = []
    for x, t in equality_points():
        d = (top * R) // t
        assert d * t == top * R and 0 < top - d < top
        out.append((x, top - d))
    return out


def edges(bits):
    top = 1 << bits
    out = {0, 1, top - 1, top - 2}
    for k in range(32, bits, 32):
        out |= {1 << k, top - (1 << k)}
        out |= {(top - 1) ^ ((1 << k) - 1), 3 << k if 3 << k < top else 1 << k}   # low words all zero
    return out


@functools.lru_cache(None)
def cases(bits):
    """[(x, l)] for the bound 2^bits, shuffled so that one wave of 64 lanes mixes every iteration
    count; the count is 1 mod 64 (the last block holds one lane)."""
    top = 1 << bits
    out = []
    for x in XS:
        ls = edges(bits) | boundaries(x, bits)
        out += [(x, l) for l in sorted(ls) if 0 <= l < top]
    out += [(x, l + d) for x, l in equalities(bits) for d in (-1, 0, 1)]
    r = random.Random(0x1eade2 + bits)
    while len(out) % 64 != 1:
        out.append((r.choice(XS), r.getrandbits(bits)))
    r.shuffle(out)
    return out


@functools.lru_cache(None)
def expected(bits):
    """[(is_leader, iterations)] of cases(bits), from the model"""
    return [model(l, bits, x) for x, l in cases(bits)]
