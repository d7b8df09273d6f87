"""GPU: the BlockFetch dedup's compare kernel alone (k_blockfetch.hip span_equal_wave through
praos_debug_span_equal) against `bytes ==`.

Two spans of one arena at arbitrary, different offsets.  Lengths 0 to 4097 and one of 70,001;
every pair of start offsets (0..15) x (0..15) at the lengths up to 257; a difference planted at
the first byte, at the last byte and on each side of every edge the kernel has -- the first
16-byte boundary of span a, every vector (PRAOS_SPAN_EQ_VEC), wave step (PRAOS_SPAN_EQ_WAVE) and
tile (PRAOS_SPAN_EQ_TILE) boundary after it, the start of the last partial tile, of the last
vector and of the tail bytes -- all derived from the header's constants; the byte before and the
byte after the two spans always differ and must not matter; spans that touch both ends of the
arena, the same span twice, overlapping spans."""
import numpy as np
import pytest

from praos_hip import abi

pytestmark = pytest.mark.gpu

VEC, WAVE, TILE = abi.SPAN_EQ_VEC, abi.SPAN_EQ_WAVE, abi.SPAN_EQ_TILE
SMALL = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257)
LARGE = (1023, 1024, 1025, 4095, 4096, 4097, 70001)
FEW_OFFSETS = ((0, 0), (0, 1), (5, 0), (15, 15), (3, 11), (8, 8), (1, 15))


def edges(length, a_off):
    """the byte positions of a span of `length` bytes starting a_off past a 16-byte boundary at which
    the kernel changes from one load, lane, step or tile to the next: both sides of each"""
    pre = min(length, -a_off % VEC)
    rem = length - pre
    nvec = rem // VEC
    marks = {0, pre, pre + nvec * VEC}                          # first byte, first vector, the tail bytes
    for unit in (VEC, WAVE, TILE):
        k = rem // unit
        marks |= {pre + m * unit for m in (1, 2, k - 1, k) if 0 < m * unit <= rem}
    full = nvec // (TILE // VEC) * (TILE // VEC)                # vectors in whole tiles
    marks |= {pre + full * VEC, pre + (nvec - nvec % 64) * VEC}  # the partial tile, its last wave step
    out = set()
    for m in marks:
        out |= {m - 1, m}
    return sorted(p for p in out | {length - 1} if 0 <= p < length)


class Arena:
    """pairs of spans laid out behind each other, each span between two guard bytes that differ
    between the two spans of a pair"""

    def __init__(self, seed):
        self.r = np.random.default_rng(seed)
        self.pool = self.r.integers(0, 256, max(LARGE) + 64, dtype=np.uint8)
        self.parts, self.pos, self.a, self.b, self.ln = [], 0, [], [], []

    def _place(self, data, phase, guard, lead=True):
        pad = (phase - (self.pos + (1 if lead else 0))) % VEC
        self.parts.append(np.full(pad, 0xEE, np.uint8))
        self.pos += pad
        if lead:
            self.parts.append(np.array([guard], np.uint8))
            self.pos += 1
        at = self.pos
        assert at % VEC == phase
        self.parts += [data, np.array([guard ^ 0xFF], np.uint8)]
        self.pos += len(data) + 1
        return at

    def pair(self, length, oa, ob, diff=None, lead=True):
        data = self.pool[(oa + 3 * ob) % 32:][:length].copy()
        other = data.copy()
        if diff is not None:
            other[diff] ^= 1 << int(self.r.integers(8))
        self.a.append(self._place(data, oa, 0x11, lead))
        self.b.append(self._place(other, ob, 0x22))
        self.ln.append(length)

    def run(self, ctx, drop_last_guard=False):
        arena = np.concatenate(self.parts)
        if drop_last_guard:
            arena = arena[:-1]
        raw = arena.tobytes()
        want = [int(raw[a:a + n] == raw[b:b + n]) for a, b, n in zip(self.a, self.b, self.ln)]
        got = ctx.debug_span_equal(raw, self.a, self.b, self.ln).tolist()
        return got, want, raw


def test_every_offset_pair_at_the_small_lengths(ctx):
    A = Arena(1)
    n_diff = 0
    for length in SMALL:
        for oa in range(VEC):
            for ob in range(VEC):
                A.pair(length, oa, ob)
                for p in sorted({0, length - 1, length // 2} if length else ()):
                    A.pair(length, oa, ob, diff=p)
                    n_diff += 1
    got, want, _ = A.run(ctx)
    assert got == want and want.count(0) == n_diff and want.count(1) == len(SMALL) * VEC * VEC


def test_every_edge_at_the_small_lengths(ctx):
    A = Arena(2)
    for length in SMALL[1:]:
        for oa, ob in FEW_OFFSETS:
            for p in edges(length, oa):
                A.pair(length, oa, ob, diff=p)
    got, want, _ = A.run(ctx)
    assert got == want and set(want) == {0}


@pytest.mark.parametrize("length", LARGE)
def test_large_lengths_at_every_edge(ctx, length):
    A = Arena(length)
    offs = FEW_OFFSETS if length < 70000 else FEW_OFFSETS[:4]
    for oa, ob in offs:
        A.pair(length, oa, ob)
        for p in edges(length, oa):
            A.pair(length, oa, ob, diff=p)
    got, want, _ = A.run(ctx)
    assert got == want and want.count(1) == len(offs) and want.count(0) > 10 * len(offs)


def test_the_edges_are_the_kernels(ctx):
    """the positions `edges` names cover both sides of every boundary of the geometry in the header"""
    assert (VEC, WAVE, TILE) == (16, 1024, 4096) and WAVE == 64 * VEC and TILE % WAVE == 0
    e = edges(70001, 5)
    pre = 11
    for want in (0, pre - 1, pre, pre + VEC - 1, pre + VEC, pre + WAVE - 1, pre + WAVE, pre + TILE - 1, pre + TILE,
                 pre + 17 * TILE - 1, pre + 17 * TILE, pre + 68 * WAVE - 1, pre + 68 * WAVE, 70000):
        assert want in e, want
    assert (70001 - pre) // VEC * VEC + pre in e and edges(5, 14) == [0, 1, 2, 4]


def test_spans_at_both_ends_of_the_arena_and_on_each_other(ctx):
    A = Arena(3)
    A.pair(300, 0, 7, lead=False)                # span a starts at byte 0 of the arena
    A.pair(2000, 9, 4, diff=1999)
    A.pair(4097, 2, 13)                          # span b ends at the arena's last byte (the guard is dropped)
    got, want, raw = A.run(ctx, drop_last_guard=True)
    assert A.a[0] == 0 and A.b[-1] + A.ln[-1] == len(raw)
    assert got == want == [1, 0, 1]
    # one span twice; spans that overlap (equal only where the bytes repeat); the empty span at the end
    z = bytes(5000)
    arena = raw + z
    base = len(raw)
    a = [A.a[1], base, base + 1, 3, len(arena), 0]
    b = [A.a[1], base + 1, base + 18, 4, len(arena), len(arena)]
    ln = [2000, 4000, 4900, 1000, 0, 0]
    got = ctx.debug_span_equal(arena, a, b, ln).tolist()
    assert got == [int(arena[x:x + n] == arena[y:y + n]) for x, y, n in zip(a, b, ln)] == [1, 1, 1, 0, 1, 1]
    # a span outside the arena is refused before anything runs
    with pytest.raises(abi.PraosError):
        ctx.debug_span_equal(arena, [0], [len(arena) - 3], [4])
