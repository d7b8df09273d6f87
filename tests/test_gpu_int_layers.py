"""GPU: the integer routines under every verdict (praos_debug_int, and praos_debug_sc_reduce for
sc_reduce512), one item per lane, bit-exact against Python integers over the case lists of
int_cases.py (validated on the CPU by test_int_cases.py)."""
import numpy as np
import pytest

import int_cases as ic

pytestmark = pytest.mark.gpu
L, R = ic.L, ic.R


def _same(got, want, inputs):
    got = ic.unpack(got)
    assert len(got) == len(want)
    bad = [(hex(i) if isinstance(i, int) else [hex(v) for v in i], hex(g), hex(w))
           for i, g, w in zip(inputs, got, want) if g != w]
    assert not bad, (len(bad), bad[:3])


def test_sc_reduce512(ctx):
    xs = ic.reduce512_cases()
    _same(ctx.debug_sc_reduce(ic.pack(xs, 64)), [x % L for x in xs], xs)


def test_sc_reduce256(ctx):
    xs = ic.reduce256_cases()
    _same(ctx.debug_int(0, ic.pack(xs)), [x % L for x in xs], xs)


def test_sc_muladd(ctx):
    ts = ic.muladd_cases()
    got = ctx.debug_int(1, ic.pack([a for a, _, _ in ts]), ic.pack([b for _, b, _ in ts]), ic.pack([c for _, _, c in ts]))
    _same(got, [(a * b + c) % L for a, b, c in ts], ts)


def test_sc_is_canonical(ctx):
    xs = ic.canonical_cases()
    _same(ctx.debug_int(2, ic.pack(xs)), [int(x < L) for x in xs], xs)


@pytest.mark.parametrize("op", [3, 4, 5, 6])
def test_sc_recode(ctx, op):
    xs = ic.recode_cases(op)
    got = ctx.debug_int(op, ic.pack(xs))
    _same(got, [ic.recode_expected(op, s) for s in xs], xs)
    bias = ic.RECODERS[op][2]
    for s, w in zip(xs, ic.unpack(got)):                                      # what the consumers rely on
        ds = ic.digits(op, w)
        assert all(-bias <= d < bias for d in ds) and ic.digits_value(op, ds) == s, hex(s)


def test_fx_div_R(ctx):
    xs = ic.div_R_cases()
    _same(ctx.debug_int(7, ic.pack(xs)), [x // R for x in xs], xs)


def test_mp_div_small(ctx):
    cs = ic.div_small_cases()
    got = ctx.debug_int(8, ic.pack([a for a, _ in cs]), ic.pack([k for _, k in cs]))
    _same(got, [a // k for a, k in cs], cs)


def test_argument_errors(ctx):
    from praos_hip import abi
    one = ic.pack([1])
    for args in ((9, one), (-1, one), (1, one), (1, one, one), (8, one), (3, ic.pack([2 ** 253])), (4, ic.pack([1, 2 ** 254])),
                 (5, ic.pack([2 ** 255])), (6, ic.pack([2 ** 128])), (8, ic.pack([5]), ic.pack([1])),
                 (8, ic.pack([5, 5]), ic.pack([2, 65536]))):
        with pytest.raises(abi.PraosError, match="rc=-2: praos_debug_int"):
            ctx.debug_int(*args)
    assert ctx.debug_int(0, np.zeros((0, 32), np.uint8)).shape == (0, 32)
    # n = 1 and n = 65: one lane, and one lane in a second block
    xs = ic.reduce256_cases()[:65]
    _same(ctx.debug_int(0, ic.pack(xs[:1])), [xs[0] % L], xs[:1])
    _same(ctx.debug_int(0, ic.pack(xs)), [x % L for x in xs], xs)
