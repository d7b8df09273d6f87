"""GPU: the row set of the wire calls alone (k_wire.hip's k_hdr_* kernels through api_internal.hpp's
RowSet and praos_debug_row_set) against a dict.

The features reach these kernels only with Blake2b digests as keys, which never collide in a home
slot on purpose.  Here the keys are chosen: every size around a wave, a block and the scan's 1,024
partial sums; one class and n classes; 257 keys in one home slot, and in the table's last slot so
that the probe chain wraps; the tag as part of the key; items that stay out of the set between
items that are in it; the reversed input; 1,026 block counts for k_hdr_scan (two per lane); and
the numbering without a set, with a limit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_ROW = 0xFFFFFFFF
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
N_SCAN = 256 * 1025 + 1            # 1,026 blocks of 256 items: k_hdr_scan sums two counts per lane


def model(flag, tag, key, tag_mask=0xFFFFFFFF, dedup=True, limit=None):
    """rows in order of first appearance: (tag, key) -> first index, as a dict"""
    first, rows = {}, []
    for i in range(len(flag)):
        if dedup:
            inside = flag[i] == 0 and tag[i] < 32 and (tag_mask >> int(tag[i])) & 1
            k = (int(tag[i]), key[i].tobytes())
        else:
            inside, k = flag[i] == 0 and (limit is None or i < limit), i
        rows.append(first.setdefault(k, len(first)) if inside else NO_ROW)
    return rows, len(first)


def check(ctx, flag, tag, key, **kw):
    got, total = ctx.debug_row_set(flag, tag, key, **kw)
    want, want_total = model(flag, tag, key, **kw)
    assert total == want_total
    assert got.tolist() == want
    return got


def distinct_keys(rng, n):
    key = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    key[:, 8:12] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)     # no two alike
    return key


def mixed(rng, n):
    """keys drawn from a pool a third of n, under four tags"""
    pool = distinct_keys(rng, n // 3 + 1)
    return np.zeros(n, np.uint8), rng.integers(0, 4, n).astype(np.uint8), pool[rng.integers(0, len(pool), n)]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_trivial_classes(ctx, n):
    rng = np.random.default_rng(n)
    check(ctx, *mixed(rng, n))
    zero = np.zeros(n, np.uint8)
    same = check(ctx, zero, zero, np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (n, 1)))
    assert same.tolist() == [0] * n
    each = check(ctx, zero, zero, distinct_keys(rng, n))
    assert each.tolist() == list(range(n))


@pytest.mark.parametrize("tag,word", [(3, 0x12345678), (0, 0xFFFFFFFF)], ids=["one_home_slot", "wraps_past_the_last_slot"])
def test_one_home_slot(ctx, tag, word):
    """257 distinct keys with one first word and one tag: one home slot, a probe chain of 257.
    Tag 0 and a first word of all ones: the home slot is the table's last (any power of two), so the
    chain goes on at slot 0."""
    n = 257
    rng = np.random.default_rng(word & 0xFFFF)
    key = distinct_keys(rng, n)
    key[:, 0:4] = np.frombuffer(np.uint32(word).tobytes(), np.uint8)
    zero = np.zeros(n, np.uint8)
    got = check(ctx, zero, np.full(n, tag, np.uint8), key)
    assert got.tolist() == list(range(n))
    # each of them twice, the copies in another order: still 257 rows, every copy on its first's row
    order = rng.permutation(n)
    got = check(ctx, np.zeros(2 * n, np.uint8), np.full(2 * n, tag, np.uint8), np.concatenate([key, key[order]]))
    assert got[n:].tolist() == order.tolist()


def test_tag_is_part_of_the_key(ctx):
    rng = np.random.default_rng(7)
    key = np.repeat(distinct_keys(rng, 50), 2, axis=0)
    tag = np.tile(np.array([2, 5], np.uint8), 50)
    got = check(ctx, np.zeros(100, np.uint8), tag, key)
    assert got.tolist() == list(range(100))


def test_excluded_items_get_no_row_and_shift_nothing(ctx):
    n = 600
    rng = np.random.default_rng(11)
    flag, tag, key = mixed(rng, n)
    bad_flag, bad_tag = rng.random(n) < 0.2, rng.random(n) < 0.15
    flag[bad_flag] = rng.choice(np.array([1, 2, 7, 255], np.uint8), int(bad_flag.sum()))
    tag[bad_tag] = rng.choice(np.array([32, 33, 64, 255], np.uint8), int(bad_tag.sum()))
    got = check(ctx, flag, tag, key, tag_mask=0b1011)              # tags 0, 1, 3: tag 2 is outside the mask
    excluded = (flag != 0) | (tag >= 32) | (tag == 2)
    assert excluded.sum() > 100 and (got[excluded] == NO_ROW).all() and (got[~excluded] != NO_ROW).all()
    # the items that stayed keep their order: the same rows as the set of those items alone
    keep = ~excluded
    alone, _ = ctx.debug_row_set(flag[keep], tag[keep], key[keep], tag_mask=0b1011)
    assert got[keep].tolist() == alone.tolist()


def test_reversed_input(ctx):
    rng = np.random.default_rng(13)
    flag, tag, key = mixed(rng, 700)
    flag[::7] = 1
    check(ctx, flag, tag, key)
    check(ctx, flag[::-1].copy(), tag[::-1].copy(), key[::-1].copy())


@pytest.mark.parametrize("repeated", [False, True], ids=["distinct", "each_key_twice"])
def test_large_scan(ctx, repeated):
    """n = 256 * 1025 + 1 items: 1,026 block counts, so each lane of k_hdr_scan sums two (per = 2)"""
    n = N_SCAN
    rng = np.random.default_rng(17)
    if repeated:
        half = (n + 1) // 2
        idx = rng.permutation(np.concatenate([np.arange(half), np.arange(n - half)]))
        key = distinct_keys(rng, half)[idx]
    else:
        key = distinct_keys(rng, n)
    zero = np.zeros(n, np.uint8)
    got, total = ctx.debug_row_set(zero, zero, key)
    if repeated:
        want, want_total = model(zero, zero, key)
    else:
        want, want_total = list(range(n)), n
    assert total == want_total
    assert np.array_equal(got, np.array(want, np.uint32))


@pytest.mark.parametrize("limit", [None, 0, 1, 255, 256, 300, 777, 5000])
def test_dedup_off(ctx, limit):
    """every item with flag 0 below the limit is its own row, equal keys or not; the items at or
    past the limit get none"""
    n = 777
    rng = np.random.default_rng(19)
    flag, tag, key = mixed(rng, n)
    flag[rng.random(n) < 0.3] = 1
    got = check(ctx, flag, tag, key, dedup=False, limit=limit)
    if limit is not None and limit < n:
        assert (got[limit:] == NO_ROW).all()
