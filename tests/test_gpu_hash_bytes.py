"""GPU: the hashes over stored bytes (praos_debug_hash_bytes) at every length residue and offset
alignment, bytewise against hashlib.  The case lists and what they cover: hash_cases.py,
test_hash_cases.py."""
import hashlib

import numpy as np
import pytest

import hash_cases as hc
from helpers import b2b
from praos_hip import abi

pytestmark = pytest.mark.gpu


def _same(out, want, what):
    got = [bytes(o) for o in out]
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (what, len(bad), bad[:8])


def test_b2b256_range(ctx):
    """Kind 0: every length 0..400 at every offset residue, 3,208 items in one launch."""
    arena, off, ln = hc.range_cases()
    out = ctx.debug_hash_bytes(0, arena, off, ln)
    _same(out, [b2b(m) for m in hc.range_messages()], "b2b256_range")


@pytest.mark.parametrize("npre", [0, 1, 2])
def test_b2b256_pre(ctx, npre):
    """Kind 1: the same ranges behind npre literal bytes that differ from the bytes they replace."""
    arena, off, ln, aux, msgs = hc.pre_cases(npre)
    out = ctx.debug_hash_bytes(1, arena, off, ln, aux=aux)
    _same(out, [b2b(m) for m in msgs], f"b2b256_pre npre={npre}")


@pytest.mark.parametrize("name", [c["name"] for c in hc.seg_cases()])
def test_seg_hash(ctx, name):
    """Kind 2: k_seg_hash itself; an inactive slot's 32 bytes stay zero."""
    case = next(c for c in hc.seg_cases() if c["name"] == name)
    out = ctx.debug_hash_bytes(2, case["arena"], case["seg_off"], case["seg_len"], aux=case["nseg"])
    msgs = hc.seg_messages(case)
    assert len(out) == 4 * case["n"]
    act = np.array([m is not None for m in msgs])
    assert not out[~act].any(), name
    _same(out[act], [b2b(m) for m in msgs if m is not None], name)


def test_stream_sha512(ctx):
    """Kind 3: Hs<true> fed by the product's loop, then the SHA-512 finalisation."""
    arena, items = hc.stream_cases()
    first, count, parts = hc.stream_tables(items)
    out = ctx.debug_hash_bytes(3, arena, first, count, parts=parts)
    _same(out, [hashlib.sha512(m).digest() for m in hc.stream_messages()], "Hs<true>")


def test_stream_blake2b(ctx):
    """Kind 4: Hs<false> over the same part lists, ended by compress(true)."""
    arena, items = hc.stream_cases()
    first, count, parts = hc.stream_tables(items)
    out = ctx.debug_hash_bytes(4, arena, first, count, parts=parts)
    _same(out, [b2b(m) for m in hc.stream_messages()], "Hs<false>")


def test_bad_arguments_launch_nothing(ctx):
    """A range past the arena, a literal prefix before offset 0, a part longer than the arena:
    PRAOS_E_ARG, and the context still works."""
    arena = hc.nonzero_bytes(9, 64)
    one = lambda v, t: np.array([v], t)
    bad = [(0, one(60, np.uint64), one(5, np.uint32), None, None),
           (1, one(1, np.uint64), one(5, np.uint32), np.array([[2, 1, 1, 0]], np.uint8), None),
           (2, np.array([0, 0, 0, 64], np.uint64), np.array([1, 1, 1, 1], np.uint32), np.array([4], np.uint8), None),
           (3, one(0, np.uint64), one(1, np.uint32), None, np.array([[0, 65]], np.uint64)),
           (4, one(0, np.uint64), one(1, np.uint32), None, np.array([[7, hc.LIT | 9]], np.uint64)),
           (4, one(1, np.uint64), one(1, np.uint32), None, np.array([[0, 8]], np.uint64))]
    for kind, off, ln, aux, parts in bad:
        with pytest.raises(abi.PraosError, match=f"rc={abi.E_ARG}"):
            ctx.debug_hash_bytes(kind, arena, off, ln, aux=aux, parts=parts)
    out = ctx.debug_hash_bytes(0, arena, one(59, np.uint64), one(5, np.uint32))
    assert bytes(out[0]) == b2b(arena[59:64])
