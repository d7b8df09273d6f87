"""CPU: the transaction corpus (tx_corpus.py) holds everything the index's tests rely on.

Asserted through the model's output wherever the model can see it (counts, lengths, statuses,
sums), and through the generator's tags for the forms the model's output does not name (which
head was definite)."""
import pytest

import tx_corpus as tc
import tx_index_model as tm


@pytest.fixture(scope="module")
def corp():
    cases = tc.corpus()
    arena, off, ln = tc.layout(cases)
    return cases, arena, off, ln, tm.index_blocks(arena, off, ln, byron=True)


def test_seeded_and_sized(corp):
    cases, arena, _, _, _ = corp
    assert [c.bytes for c in cases] == [c.bytes for c in tc.corpus()]
    assert 150 <= len(cases) <= 250 and len(arena) < 2_000_000
    assert len({c.name for c in cases}) == len(cases)


def test_every_listed_thing_occurs(corp):
    cases, arena, off, ln, (st, rw) = corp
    tags = set().union(*(c.tags for c in cases))
    by = {c.name: i for i, c in enumerate(cases)}
    ok = [i for i in range(len(cases)) if st["status"][i] == tm.OK]
    # era tags, bare blocks, Byron main blocks and EBBs, all indexed
    for t in (2, 3, 4, 5, 6, 7, "bare3", "bare4"):
        assert st["status"][by[f"era_{t}"]] == tm.OK and st["n_tx"][by[f"era_{t}"]] == 3
    assert arena[off[by["era_bare3"]]] == 0x84 and arena[off[by["era_bare4"]]] == 0x85
    assert st["status"][by["byron_ebb"]] == tm.OK and st["n_tx"][by["byron_ebb"]] == 0
    assert {st["n_tx"][i] for i, c in enumerate(cases) if "byron_main" in c.tags} >= {0, 1, 2, 64, 65}
    # transaction counts, body lengths, output counts
    assert set(tc.TX_COUNTS) <= {st["n_tx"][i] for i in ok}
    assert set(tc.BODY_LENS) <= set(rw["body_len"]) and max(rw["body_len"]) > 0xffff
    assert set(tc.OUT_COUNTS) <= set(rw["n_out"])
    # definite and indefinite forms: segments, body map, outputs array, redeemers, nested items
    for k in (1, 2, 3, 4):
        assert {f"indef_s{k}", f"def_s{k}"} <= tags
    assert {"body_indef", "body_def", "outs_indef", "outs_def", "nested_indef", "wide_key", "no_key1"} <= tags
    assert {"red_array_def", "red_array_indef", "red_map_def", "red_map_indef"} <= tags
    first_bytes = {arena[o] for o in rw["body_off"]}
    assert 0xbf in first_bytes and any(0xa0 <= b <= 0xbb for b in first_bytes)
    # auxiliary data absent, out of order, for all; invalid lists empty, partial, full
    def rows_of(name):
        i = by[name]
        return range(st["tx_first"][i], st["tx_first"][i + 1])
    assert [rw["aux_len"][q] for q in rows_of("aux_absent")] == [0] * 5
    assert [rw["aux_len"][q] > 0 for q in rows_of("aux_out_of_order")] == [True, False, True, False, True]
    au = [rw["aux_off"][q] for q in rows_of("aux_out_of_order") if rw["aux_len"][q]]
    assert au != sorted(au)
    assert all(rw["aux_len"][q] > 0 for q in rows_of("aux_all"))
    assert rw["aux_len"][rows_of("aux_repeated")[1]] == 9          # the later of the two entries
    assert [rw["is_valid"][q] for q in rows_of("invalid_empty")] == [1] * 5
    assert [rw["is_valid"][q] for q in rows_of("invalid_partial")] == [0, 1, 1, 0, 1]
    assert [rw["is_valid"][q] for q in rows_of("invalid_full")] == [0] * 5
    # steps at 2^32 and near 2^64: a row's sum wraps, and so does a block's
    for form in ("array", "map"):
        for v in ("00", "10", "11"):
            q = rows_of(f"redeemers_{form}_{v}")
            assert rw["ex_steps"][q[0]] == sum(tc.STEPS) % (1 << 64) and sum(tc.STEPS) >= 1 << 64
            assert rw["ex_steps"][q[1]] == 1 and rw["ex_steps"][q[2]] == 0 and rw["ex_steps"][q[3]] == 0
            i = by[f"redeemers_{form}_{v}"]
            assert st["ex_steps"][i] == sum(rw["ex_steps"][k] for k in q) % (1 << 64)
    assert 1 << 32 in tc.STEPS
    assert [rw["ex_steps"][q] for q in rows_of("key5_in_three_segments")] == [0, 0]
    assert [rw["ex_steps"][q] for q in rows_of("witness_not_map")] == [0]
    # the shape mutations, one per case, and the blocks that do not decode
    for m in tc.SHAPE_MUTATIONS:
        i = by["shape_" + m]
        assert st["status"][i] == tm.SHAPE and st["n_tx"][i] == 0 and st["txs_size"][i] == 0, m
    for name in ("byron_tx_not_array", "byron_outs_not_array"):
        assert st["status"][by[name]] == tm.SHAPE
    for name in ("truncated", "wrong_tag", "header_arity", "byron_truncated"):
        assert st["status"][by[name]] == tm.DECODE
    assert all(st["status"][i] == tm.OK for i, c in enumerate(cases)
               if not (c.name.startswith("shape_") or c.tags & {"truncated", "decode", "byron_decode", "mut_byron_tx",
                                                                  "mut_byron_outs"}))
    # a mutated block is one intact block away from OK: the same builder without the mutation indexes
    assert st["tx_first"][-1] == len(rw["block"]) > 1000
