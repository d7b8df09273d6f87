"""GPU: the key-witness check over an ImmutableDB directory
(praos_hip.witnesses.verify_immutable_witnesses), three chunks.

The chunks are written by immutable.write_immutable from chunk_corpus blocks (linked, signed
headers) whose segments are txwit_corpus transactions: every witness genuinely signed, but for
two planted bad ones (a VKey witness in the first chunk, a bootstrap witness in the third).  The
per-block tuples, the totals and the failing list equal what the blocks were built to hold, for
the whole directory and with `limit` cutting inside the second chunk."""
import numpy as np
import pytest

import block_integrity as bi
import chunk_corpus as cc
import tx_corpus as tc
import txwit_corpus as wc
from helpers import rng
from praos_hip import immutable, witnesses

pytestmark = pytest.mark.gpu
SPKP = 129600
CHUNK_SLOTS = 100
SLOTS = [3, 40, 99, 100, 101, 150, 200, 250, 299]
# (block, transaction, witness in row order, damage): the planted bad witnesses
PLANTED = {(2, 2, 1): "S", (7, 0, 3): "R"}


def build_db(path):
    """-> per block: slot, block_no, the transactions' (n_vkey, n_boot) and the failing witnesses"""
    r = rng(78)
    g = wc.Gen(4242)
    blocks, prev = [], None
    for k, slot in enumerate(SLOTS):
        era = (6, 3, 5, 7, 2, 4)[k % 6]
        four = era >= 5
        b = cc.Block(r, SPKP, era, slot, k, prev)
        shape = [(2, 0), (1, 1), (3, 0), (0, 0), (2, 2)][:(3, 0, 5, 1, 4)[k % 5]]
        if k == 7:
            shape = [(2, 2)]
        txs = [g.tx(nv, nb, four=four, keys=(0, 2) if j % 2 else None, map_indef=j % 3 == 1,
                    damage={w: d for (bk, t, w), d in PLANTED.items() if (bk, t) == (k, j)})
               for j, (nv, nb) in enumerate(shape)]
        n = len(txs)
        segs = [tc.seq(4, [t[0] for t in txs], n % 2 == 1), tc.seq(4, [t[1] for t in txs], False),
                tc.seq(5, [(tc.hd(0, 0), tc.bstr(r, 11))] if n else [], False)]
        if four:
            segs.append(tc.seq(4, [tc.hd(0, n - 1)] if n else [], False))
        b.segs = segs
        b.f["body_size"] = sum(map(len, segs))
        b.f["body_hash"] = bi._b2b(b"".join(bi._b2b(s) for s in segs))
        b.sign()
        bad = [(j, w, 0 if w < shape[j][0] else 2) for j, t in enumerate(txs) for w, ok in enumerate(t[2]) if not ok]
        blocks.append({"slot": slot, "block_no": k, "obj": b, "shape": shape, "bad": bad})
        prev = b.header_hash
    arena, off, _ = cc.layout([x["obj"].bytes for x in blocks])
    immutable.write_immutable(str(path), np.frombuffer(arena, np.uint8),
                              np.array(off, np.uint64) + np.uint64(immutable.HEADER_OFFSET),
                              np.array([len(x["obj"].header) for x in blocks], np.uint32),
                              [x["slot"] for x in blocks], [x["obj"].header_hash for x in blocks], CHUNK_SLOTS)
    return blocks


def expected(blocks, limit):
    bl = blocks if limit is None else blocks[:limit]
    rows = [witnesses.BlockWitnesses(x["slot"], x["block_no"], len(x["shape"]), sum(a + b for a, b in x["shape"]),
                                     len(x["bad"]), 0) for x in bl]
    failing = [(x["slot"], j, w, kind) for x in bl for j, w, kind in x["bad"]]
    tot = witnesses.WitnessTotals(len(bl), sum(r.n_tx for r in rows), sum(r.n_wit for r in rows),
                                  sum(r.n_bad for r in rows), 0, failing)
    return rows + [tot]


def test_directory_totals_and_failing_list(ctx, tmp_path):
    path = tmp_path / "immutable"
    path.mkdir()
    blocks = build_db(path)
    assert len({x["slot"] // CHUNK_SLOTS for x in blocks}) == 3
    assert [(x["block_no"], x["bad"]) for x in blocks if x["bad"]] == [(2, [(2, 1, 0)]), (7, [(0, 3, 2)])]
    first = sum(1 for x in blocks if x["slot"] < CHUNK_SLOTS)
    in_first_two = sum(1 for x in blocks if x["slot"] < 2 * CHUNK_SLOTS)
    for limit in (None, first + 2):
        assert limit is None or first < limit < in_first_two
        got = list(witnesses.verify_immutable_witnesses(ctx, str(path), SPKP, limit=limit))
        assert got == expected(blocks, limit)
    whole = expected(blocks, None)[-1]
    assert whole.bad == 2 and whole.wits > 30 and len(whole.failing) == 2
    assert expected(blocks, first + 2)[-1].bad == 1
