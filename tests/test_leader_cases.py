"""CPU: the leader cases over the whole accepted range of x (leader_cases.py) reach what they
claim, on the Python model alone; the C oracle (256 and 512 bits) and the CPU twin (256 bits: its
ABI has no 512-bit entry of its own) decide every case as the model does; the host's range limit
of x (csrc/host_util.hpp leader_x_raw) accepts 16 R and rejects 16 R + 1, in libpraos_hip's
praos_set_epoch on a context without a device and in the twin.  Prints the case counts, the
histogram of iteration counts and the largest err * x (pytest -s; DESIGN.md quotes them)."""
from collections import Counter

import numpy as np
import pytest

import leader_cases as lc
from helpers import arr

R = lc.R


def test_pairs():
    for x in (1, 16 * R - 1, 16 * R, 16 * R + 1):
        for exact in (True, False):
            s, c = lc.pair_for(x, exact)
            assert 0 < s < 2 ** 128 and -2 ** 127 <= c < 0
    assert lc.pair_for(0, True) == (R, 0)


@pytest.mark.parametrize("bits", [256, 512])
def test_coverage_on_the_model(bits):
    cases, want = lc.cases(bits), lc.expected(bits)
    top = 1 << bits
    assert len(cases) % 64 == 1 and len(cases) < 20000
    assert all(0 <= l < top and 0 <= x <= lc.X_MAX for x, l in cases)
    assert {x for x, _ in cases} == set(lc.XS) | {x for x, _ in lc.equality_points()} and lc.XS[-1] == lc.X_MAX == 16 * R
    by_x = {x: [(l, w) for (xx, l), w in zip(cases, want) if xx == x] for x in lc.XS}
    max_it, max_ex, neg = 0, 0, set()
    for x, rows in by_x.items():
        rec = lc.recurrence(x)
        its = max(it for _, (_, it) in rows)
        assert its <= lc.STEPS
        max_it = max(max_it, its)
        max_ex = max([max_ex] + [rec[n][0] for n in range(its)])
        if any(rec[n][2] < 0 for n in range(min(it for _, (_, it) in rows))):
            neg.add(x)                                                        # every case of x forms a negative acc' - e
        if x > 0:
            assert {lead for _, (lead, _) in rows} == {True, False}, x
        else:
            assert {w for _, w in rows} == {(False, 1)}                       # x = 0: nobody leads
        assert {0, 1, top - 1, top - 2, 1 << (bits - 32), top - (1 << 32)} <= {l for l, _ in rows}
    assert neg >= {x for x in lc.XS if x >= 2 * R}
    assert max_it >= 38 and max(it for x, rows in by_x.items() if x == 2 * R for _, (_, it) in rows) >= 38
    assert 2 ** 249 <= max_ex < 2 ** 256
    # x = 5 R: l = 0 decides after 5 iterations, the top of the range after 1 (not monotone in l)
    assert lc.model(0, bits, 5 * R) == (True, 5) and lc.model(top - 1, bits, 5 * R) == (False, 1)
    rec = lc.recurrence(5 * R)
    assert rec[0][1] == 6 * R + 75 * R // 2 and rec[0][2] == 6 * R - 75 * R // 2 < 0
    # the exact comparison boundaries: both sides of some l_T decide differently or at another iteration
    flips = sum(1 for x in lc.XS for lt in lc.boundaries(x, bits)
                if 0 < lt < top - 1 and lc.model(lt - 1, bits, x) != lc.model(lt, bits, x))
    assert flips >= 100
    # exact equality floor(N / D) = N / D = acc' + e at iteration 0: ABOVE by `>=` alone, and the
    # neighbour below runs on (once to another verdict)
    eq = lc.equalities(bits)
    assert len(eq) >= 8 and all((x, l + d) in cases for x, l in eq for d in (-1, 0, 1))
    for x, l in eq:
        assert (top * R) % (top - l) == 0 and (top * R) // (top - l) == lc.first_upper(x) == lc.recurrence(x)[0][1]
        assert lc.model(l, bits, x) == (False, 1) and lc.model(l - 1, bits, x)[1] > 1
    assert any(lc.model(l - 1, bits, x)[0] for x, l in eq)
    assert lc.model(0, bits, 0) == (False, 1)                                 # the one equality among the boundaries
    # one wave mixes short and long runs
    its = [it for _, it in want]
    assert all(len(set(its[g:g + 64])) >= 8 for g in range(0, len(its) - 64, 64))
    hist = Counter(its)
    print(f"leader cases, {bits} bits: {len(cases)} cases, largest err * x has {max_ex.bit_length()} bits, "
          f"{len(neg)} values of x with a negative acc' - e, {flips} boundaries that flip")
    print("  iterations: " + " ".join(f"{k}:{v}" for k, v in sorted(hist.items())))


@pytest.mark.parametrize("bits", [256, 512])
def test_oracle_parity(oracle, bits):
    check = oracle.check_leader if bits == 256 else oracle.check_leader512
    for (x, l), want in zip(lc.cases(bits), lc.expected(bits)):
        assert check(l.to_bytes(bits // 8, "big"), R, -x) == want, (x, hex(l))


@pytest.fixture(scope="module")
def twin():
    from praos_hip import cpu
    c = cpu.CpuContext()
    yield c
    c.close()


def test_twin_parity(twin):
    from praos_hip import abi
    cases, want = lc.cases(256), lc.expected(256)
    for x in sorted({x for x, _ in cases}):
        rows = [(l, w[0]) for (xx, l), w in zip(cases, want) if xx == x]
        got = twin.check_leader(arr([l.to_bytes(32, "big") for l, _ in rows], 32),
                                arr([R.to_bytes(16, "little")] * len(rows), 16), abi.params(c_raw=-x))
        assert [bool(g) for g in got] == [w for _, w in rows], x


def _sig(vals):
    return arr([int(v).to_bytes(16, "little") for v in vals], 16)


def test_twin_range_limit(twin):
    from praos_hip import abi
    one = arr([bytes(32)], 32)
    for x in (0, 1, 16 * R - 1, 16 * R):
        for exact in (True, False):
            s, c = lc.pair_for(x, exact)
            got = twin.check_leader(one, _sig([s]), abi.params(c_raw=c))
            assert bool(got[0]) == lc.model(0, 256, x)[0], (x, exact)
    for s, c in (lc.pair_for(16 * R + 1, True), lc.pair_for(16 * R + 1, False), (R, 1), (2 ** 128 - 1, -2 ** 127)):
        with pytest.raises(abi.PraosError, match="rc=-2"):
            twin.check_leader(one, _sig([s]), abi.params(c_raw=c))


def test_host_range_limit_in_set_epoch():
    """praos_set_epoch of libpraos_hip computes x per pool on the host (pool_tables_build), so a
    context without a device shows the limit: 16 R accepted, 16 R + 1 rejected with the message."""
    from praos_hip import abi
    c = abi.Context(abi.HOST_ONLY)
    try:
        pool = lambda s: [(b"\x01" * 28, b"\x02" * 32, s)]
        for x in (0, 1, 16 * R - 1, 16 * R):
            for exact in (True, False):
                s, cr = lc.pair_for(x, exact)
                c.set_epoch(b"\x07" * 32, pool(s), abi.params(c_raw=cr))
        for s, cr in (lc.pair_for(16 * R + 1, True), lc.pair_for(16 * R + 1, False), (R, 1), (2 ** 128 - 1, -2 ** 127)):
            with pytest.raises(abi.PraosError, match=r"rc=-2: sigma \* activeSlotLog out of range \(x_raw > 16 \* 10\^34\)"):
                c.set_epoch(b"\x07" * 32, pool(s), abi.params(c_raw=cr))
    finally:
        c.close()
