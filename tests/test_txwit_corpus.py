"""CPU: the key-witness corpus (txwit_corpus.py) holds what it was built to hold, and the model
(tx_witness_model.py) alone marks ok every witness the generator meant valid and not ok every one
it meant invalid -- so the GPU test cannot pass by agreeing with a wrong model."""
import pytest

import tx_witness_model as wm
import txwit_corpus as wc


@pytest.fixture(scope="module")
def corp():
    cases = wc.corpus()
    arena, off, ln = wc.layout(cases)
    return cases, arena, off, ln, wm.verify_blocks(arena, off, ln, byron=True)


def rows_of(corp, name):
    cases, _, _, _, (B, T, W) = corp
    i = [c.name for c in cases].index(name)
    return i, range(B["tx_first"][i], B["tx_first"][i + 1])


def test_model_agrees_with_the_generators_intent(corp):
    cases, _, _, _, (B, T, W) = corp
    n_valid = n_invalid = 0
    for i, c in enumerate(cases):
        rows = range(B["tx_first"][i], B["tx_first"][i + 1])
        if c.want is None:
            assert B["status"][i] != 0 and len(rows) == 0, c.name
            continue
        assert B["status"][i] == 0 and len(rows) == len(c.want), c.name
        for p, want in zip(rows, c.want):
            w0, w1 = T["wit_first"][p], T["wit_first"][p + 1]
            if want == "skipped":
                assert T["status"][p] == wm.SKIPPED and w0 == w1, c.name
            elif want == "shape":
                assert T["status"][p] == wm.SHAPE and w0 == w1, c.name
            else:
                assert T["status"][p] == wm.OK, c.name
                assert [bool(x) for x in W["ok"][w0:w1]] == want, c.name
                assert W["kind"][w0:w1] == [0] * T["n_vkey"][p] + [2] * T["n_boot"][p], c.name
                n_valid += sum(want)
                n_invalid += len(want) - sum(want)
    assert n_valid > 800 and n_invalid > 60
    assert 200 <= len(T["block"]) <= 600 and 1000 <= len(W["tx"]) <= 2000


def test_witness_counts(corp):
    _, _, _, _, (B, T, W) = corp
    per_tx = [T["n_vkey"][p] + T["n_boot"][p] for p in range(len(T["block"]))]
    for n in wc.WIT_COUNTS:
        assert n in per_tx, n
    i, rows = rows_of(corp, "cross_slices")
    assert B["n_wit"][i] == 250 and len(rows) == 5 and B["n_bad"][i] == 5
    i, rows = rows_of(corp, "count_65")
    assert (T["n_vkey"][rows[0]], T["n_boot"][rows[0]]) == (40, 25)


def test_key_presence_and_forms(corp):
    cases, arena, off, _, (B, T, W) = corp
    tags = set().union(*(c.tags for c in cases))
    for t in ("key0_only", "key2_only", "both_02", "both_20", "neither", "key0_twice", "wit_not_map", "map_indef",
              "map_def", "arr_indef", "arr_def", "item_indef", "item_def", "tag0", "tag2", "wide_key0", "other_before",
              "other_between", "other_after", "cross_slices", "valid", "in_s4", "swapped", "forged_small_a",
              "forged_small_r", "odd_keys", "txi_shape", "txi_decode", "byron_ebb", "byron_main", "random",
              *("count_%d" % n for n in wc.WIT_COUNTS), *("dmg_" + d for d in wc.DAMAGE),
              *("mut_" + m for m in wc.SHAPE_MUTATIONS), *("tag_%s" % t for t in (2, 3, 4, 5, 6, 7, "bare3", "bare4"))):
        assert t in tags, t
    i, rows = rows_of(corp, "keys_presence")
    assert [(T["n_vkey"][p], T["n_boot"][p]) for p in rows] == [(2, 0), (0, 2), (2, 2), (2, 3), (0, 0), (0, 0), (0, 0)]
    p = rows[3]      # key 2 first in the map: the key-0 items still come first
    ks = W["key_off"][T["wit_first"][p]:T["wit_first"][p + 1]]
    assert W["kind"][T["wit_first"][p]:T["wit_first"][p + 1]] == [0, 0, 2, 2, 2] and max(ks[:2]) > min(ks[2:])
    # key 0 twice: the second is not read (each row has the first key's count, none is SHAPE)
    i, rows = rows_of(corp, "key0_twice")
    assert [(T["n_vkey"][p], T["status"][p]) for p in rows] == [(2, 0), (1, 0), (1, 0)]
    blk = cases[i].bytes
    assert blk.count(b"\x00\x82\x82\x58\x20") + blk.count(b"\x00\x81\x82\x58\x20") >= 3
    i, rows = rows_of(corp, "not_a_map")
    assert [T["n_vkey"][p] for p in rows] == [1, 0, 0] and [T["status"][p] for p in rows] == [0, 0, 0]
    i, rows = rows_of(corp, "odd_keys")
    assert [(T["n_vkey"][p], T["n_boot"][p], T["status"][p]) for p in rows] == [(2, 1, 0), (1, 2, 0), (0, 0, 0)]
    i, rows = rows_of(corp, "wide_key0")
    assert b"\x18\x00" in cases[i].bytes and [T["n_vkey"][p] for p in rows] == [2, 1]


def test_shape_rules_one_per_case(corp):
    cases, _, _, _, (B, T, W) = corp
    for m in wc.SHAPE_MUTATIONS:
        i, rows = rows_of(corp, "shape_" + m)
        assert [T["status"][p] for p in rows] == [wm.OK, wm.SHAPE, wm.OK], m
        assert B["n_shape"][i] == 1 and B["n_bad"][i] == 0 and B["n_wit"][i] == 4, m
    i, rows = rows_of(corp, "shape_after_good_key0")
    assert [T["status"][p] for p in rows] == [wm.SHAPE, wm.OK] and B["n_wit"][i] == 1


def test_signatures_blocks_and_byron(corp):
    cases, arena, off, ln, (B, T, W) = corp
    i, rows = rows_of(corp, "signatures")
    assert [T["n_bad"][p] for p in rows] == [0, 1, 1, 1, 1, 1, 1, 1, 1] and B["n_bad"][i] == 8
    for fam in ("small_a", "small_r"):
        i, rows = rows_of(corp, "forged_" + fam)
        assert [T["n_bad"][p] for p in rows] == [1, 0]
    i, rows = rows_of(corp, "swapped")
    assert [T["n_bad"][p] for p in rows] == [1, 1, 0]
    assert B["status"][[c.name for c in cases].index("txi_shape")] == 2
    assert B["status"][[c.name for c in cases].index("txi_decode")] == 1
    # Byron off: the Byron blocks have no rows, the others are as before
    B0, T0, W0 = wm.verify_blocks(arena, off, ln, byron=False)
    byr = [i for i, c in enumerate(cases) if "byron" in c.tags]
    assert len(byr) == 3 and all(B0["status"][i] == 1 and B0["n_tx"][i] == 0 for i in byr)
    assert len(T0["block"]) == len(T["block"]) - 4 and W0["ok"] == W["ok"]
    assert sum(1 for s in T["status"] if s == wm.SKIPPED) == 4
    assert sum(1 for c in cases if "random" in c.tags) == 50
