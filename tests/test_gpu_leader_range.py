"""GPU: the leader check over the whole range of x the host accepts (0 .. 16 R): the cases of
leader_cases.py (validated on the CPU by test_leader_cases.py) through praos_debug_leader and
praos_debug_leader512, decisions and Taylor iteration counts equal to the Python model's; the
host's range limit of x in praos_check_leader and praos_set_epoch."""
import numpy as np
import pytest

import leader_cases as lc
from helpers import arr, b2b

pytestmark = pytest.mark.gpu
R = lc.R


def _run(ctx, bits, cases):
    fn = ctx.debug_leader if bits == 256 else ctx.debug_leader512
    res, it = fn(arr([l.to_bytes(bits // 8, "big") for _, l in cases], bits // 8),
                 arr([x.to_bytes(16, "little") for x, _ in cases], 16))
    return [(bool(r), int(i)) for r, i in zip(res, it)]


@pytest.mark.parametrize("bits", [256, 512])
def test_leader_range(ctx, bits):
    cases, want = lc.cases(bits), lc.expected(bits)
    got = _run(ctx, bits, cases)
    bad = [(x / R, hex(l), g, w) for (x, l), g, w in zip(cases, got, want) if g != w]
    assert not bad, (len(bad), bad[:4])
    assert _run(ctx, bits, cases[:1]) == want[:1]                             # one lane
    assert _run(ctx, bits, cases[:65]) == want[:65]                           # one lane in a second wave


def _sig(vals):
    return arr([int(v).to_bytes(16, "little") for v in vals], 16)


LS = [0, 1, 2 ** 255, 2 ** 256 - 2 ** 32, 2 ** 256 - 1, int(0.864665 * 2 ** 256), int(0.99 * 2 ** 256)]


def test_check_leader_range_limit(ctx):
    from praos_hip import abi
    ls = arr([l.to_bytes(32, "big") for l in LS], 32)
    for x in (0, 1, 16 * R - 1, 16 * R):
        for exact in (True, False):
            s, c = lc.pair_for(x, exact)
            got = ctx.check_leader(ls, _sig([s] * len(LS)), abi.params(c_raw=c))
            assert [bool(g) for g in got] == [lc.model(l, 256, x)[0] for l in LS], (x, exact)
    # 16 R + 1 (exact and by the ceiling), c > 0, a quotient beyond 128 bits; one bad item among good ones
    for s, c in (lc.pair_for(16 * R + 1, True), lc.pair_for(16 * R + 1, False), (R, 1), (2 ** 128 - 1, -2 ** 127)):
        with pytest.raises(abi.PraosError, match="rc=-2: x out of range"):
            ctx.check_leader(ls, _sig([R // 2] * (len(LS) - 1) + [s]), abi.params(c_raw=c))
    # c = 0: x = 0 and nobody leads, whatever the stake
    got = ctx.check_leader(ls, _sig([0, 1, R // 2, R, 2 * R, 2 ** 127, 2 ** 128 - 1]), abi.params(c_raw=0))
    assert not got.any() and not any(lc.model(l, 256, 0)[0] for l in LS)


def test_set_epoch_range_limit(ctx):
    """A pool at x = 16 R is accepted and decided as the model decides; a pool at 16 R + 1 fails
    praos_set_epoch with its message and leaves no epoch (praos_hip.h's contract, held by
    test_chainstate.py); the next praos_set_epoch makes the context usable again."""
    from fractions import Fraction
    from praos_hip import abi, fixed
    c_raw = fixed.active_slot_log(Fraction(1, 20))
    p = abi.params(c_raw=c_raw)
    eta0 = b2b(b"range")
    H, pools, _ = ctx.synthesize(64, 3, p, eta0, b"\x21" * 32, first_slot=500, slot_stride=5, body_len=200,
                                 corrupt_per_10000=0)
    s16, c16 = lc.pair_for(16 * R, False)
    p16 = abi.params(c_raw=c16)
    ok_pools = [(h, v, s16) for h, v in pools]
    ctx.set_epoch(eta0, ok_pools, p16)
    out = ctx.verify_headers(H)
    lead = [lc.model(int.from_bytes(bytes(l), "big"), 256, 16 * R)[0] for l in out["leader"]]
    assert [not (int(b) & abi.BIT_LEADER) for b in out["bits"]] == lead and all(int(i) >= 0 for i in out["pool_idx"])
    s17, c17 = lc.pair_for(16 * R + 1, False)
    assert c17 == c16 - 1
    bad_pools = [(h, v, R // 2) for h, v in pools[:2]] + [(pools[2][0], pools[2][1], s17)]   # one pool over the limit
    with pytest.raises(abi.PraosError, match=r"rc=-2: sigma \* activeSlotLog out of range \(x_raw > 16 \* 10\^34\)"):
        ctx.set_epoch(eta0, bad_pools, abi.params(c_raw=c17))
    with pytest.raises(abi.PraosError, match="rc=-4"):
        ctx.verify_headers(H)
    ctx.set_epoch(eta0, ok_pools, p16)
    again = ctx.verify_headers(H)
    assert np.array_equal(again["bits"], out["bits"]) and np.array_equal(again["leader"], out["leader"])
