"""GPU CRC-32 over variable-length spans (k_crc32.hip through praos_crc32) against zlib.crc32:
every short length at every start alignment, the sizes around the powers of two and around
the kernel's tile, one long span among many tiny ones (tile-list prefix sums), overlapping
spans, a span ending at the last byte of an arena of odd length, constant data, n = 0, the
argument check, and repeatability."""
import zlib

import numpy as np
import pytest

from praos_hip import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    return np.random.default_rng(0xC4C32).integers(0, 256, size=(1 << 20) + 77, dtype=np.uint8)


def _check(ctx, arena, off, ln):
    got = ctx.crc32(arena, off, ln)
    raw = arena.tobytes() if isinstance(arena, np.ndarray) else bytes(arena)
    want = np.array([zlib.crc32(raw[o:o + n]) for o, n in zip(off, ln)], np.uint32)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(off[i]), int(ln[i]), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]
    return got


def test_every_short_length_at_every_alignment(ctx, data):
    off, ln = [], []
    for a in range(16):
        for n in range(301):
            off.append(1024 + a + 17 * n)
            ln.append(n)
    got = _check(ctx, data, off, ln)
    assert all(int(got[301 * a]) == 0 for a in range(16))      # len 0 -> 0


def test_sizes_around_powers_of_two_and_tiles(ctx, data):
    lens = [x for k in range(8, 18) for x in ((1 << k) - 1, 1 << k, (1 << k) + 1)]
    for t in abi.CRC_TILE:
        lens += [t - 1, t, t + 1, 2 * t - 1, 2 * t + 1, 3 * t]
    off = [(37 * i) % 61 for i in range(len(lens))]
    _check(ctx, data, off, lens)
    _check(ctx, data, [o + 3 for o in off], lens)


def test_one_long_span_among_tiny_ones(ctx, data):
    r = np.random.default_rng(5)
    ln = [int(x) for x in r.integers(1, 65, size=1000)]
    off = [int(x) for x in r.integers(0, len(data) - 64, size=1000)]
    ln.insert(613, 200_000)
    off.insert(613, 12345)
    _check(ctx, data, off, ln)


def test_overlapping_and_identical_spans(ctx, data):
    off = [100, 100, 100, 101, 50, 0, 100, 20_000, 20_001]
    ln = [5000, 5000, 40_000, 4999, 100, 60_000, 5000, 33_000, 33_000]
    got = _check(ctx, data, off, ln)
    assert got[0] == got[1] == got[6]


def test_span_ending_at_the_last_byte_of_an_odd_arena(ctx, data):
    for total in (1000 + 13, 16384 + 5, 40_001, 7):
        arena = np.ascontiguousarray(data[:total])
        assert total % 16
        off = [0, total - 1, total - min(total, 300), max(0, total - 16385), total]
        ln = [total, 1, min(total, 300), total - max(0, total - 16385), 0]
        _check(ctx, arena, off, ln)


def test_constant_data(ctx):
    for v in (0, 0xFF):
        arena = np.full(70_001 + 9, v, np.uint8)
        _check(ctx, arena, [0, 9, 3], [70_001, 70_001, 70_001])


def test_no_spans(ctx, data):
    assert len(ctx.crc32(data, [], [])) == 0
    assert len(ctx.crc32(np.zeros(0, np.uint8), [], [])) == 0


def test_out_of_range_span_is_an_argument_error(ctx, data):
    arena = np.ascontiguousarray(data[:1000])
    for off, ln in (([0, 990], [10, 11]), ([1001], [0]), ([2 ** 40], [1]), ([5], [0xFFFFFFFF])):
        with pytest.raises(abi.PraosError, match=f"rc={abi.E_ARG}"):
            ctx.crc32(arena, off, ln)
    _check(ctx, arena, [0, 990, 1000], [10, 10, 0])


def test_same_call_twice(ctx, data):
    r = np.random.default_rng(6)
    ln = [int(x) for x in r.integers(0, 90_000, size=200)]
    off = [int(x) for x in r.integers(0, len(data) - 90_000, size=200)]
    a = ctx.crc32(data, off, ln)
    b = ctx.crc32(data, off, ln)
    assert (a == b).all()
    _check(ctx, data, off, ln)
