"""CPU: the wire-transaction corpus (gentx_corpus.py) holds every case the GPU tests rely on, and
the model (gentx_model.py) marks every item and every witness as the generator meant it."""
import gentx_corpus as gc
import gentx_model as gm

NEEDED = (
    "txwit", "era_1", "era_2", "era_3", "era_4", "era_5", "era_6", "dup2_adjacent", "dup3_adjacent", "dup65_adjacent",
    "dup_far", "same_body", "two_eras", "shape_arr2", "shape_arr5", "shape_three_under_4", "shape_four_under_3",
    "shape_indef_count", "shape_indef_no_break", "shape_valid_f6", "shape_valid_01", "shape_trailing_inside",
    "shape_not_array", "shape_truncated", "shape_empty", "shape_body_not_map", "shape_key5", "shape_twice",
    "key5_unread_era3", "trailing", "syntax_tag23", "syntax_indef_bytes", "syntax_outer", "syntax_era_word8",
    "syntax_short", "syntax_empty", "era_7", "era_255", "range", "wide_wrapper", "wide_inner", "indef_inner",
    "aux_null", "aux_present", "is_valid_false", "red_array", "red_map", "units_2p32", "units_wrap", "units_indef",
    "units_none", "body_len_1", "body_len_128", "body_len_129", "body_len_256", "body_len_5000", "byron_0", "byron_1", "byron_2", "byron_3", "byron_4", "byron_other")


def run():
    items = gc.corpus()
    arena, off, ln = gc.layout(items)
    return items, arena, gm.verify(arena, off.tolist(), ln.tolist())


def test_every_case_occurs():
    items = gc.corpus()
    tags = set().union(*(it.tags for it in items))
    assert [t for t in NEEDED if t not in tags] == []
    assert {it.status for it in items} == set(range(7))
    assert len(items) > max(gc.COUNTS) and gc.COUNTS == (0, 1, 63, 64, 65, 257)
    # the witness walk's own cases came along with the blocks' transactions
    for t in ("mut_key_31", "tag0", "tag2", "map_indef", "arr_indef", "item_indef", "key0_twice", "count_300",
              "forged_small_a", "dmg_S+L"):
        assert t in tags, t


def test_the_model_marks_every_item_and_witness_as_meant():
    items, arena, (I, T, W) = run()
    assert I["status"] == [it.status for it in items]
    for k, it in enumerate(items):
        row = I["row"][k]
        assert (row == gm.NO_ROW) == (it.want is None), it.name
        if it.want is None:
            continue
        if it.want == "shape":
            assert T["wstatus"][row] == 1 and T["wit_first"][row] == T["wit_first"][row + 1], it.name
        else:
            got = W["ok"][T["wit_first"][row]:T["wit_first"][row + 1]]
            assert T["wstatus"][row] == 0 and got == [1 if v else 0 for v in it.want], it.name
        assert I["era"][k] == T["era"][row]
    assert len(W["tx"]) > 1000 and 0 in W["ok"] and 1 in T["wstatus"]
    byr = [k for k, it in enumerate(items) if it.status == gc.BYRON]
    assert [I["byron_kind"][k] for k in byr] == [0, 1, 2, 3]
    assert all(I["payload_len"][k] == len(items[k].bytes) - 4 for k in byr)


def test_rows_follow_first_appearance_and_classes():
    items, arena, (I, T, W) = run()
    first = {}
    for k, it in enumerate(items):
        if it.status == gc.OK:
            key = (I["era"][k], it.bytes)
            first.setdefault(key, k)
            assert T["item"][I["row"][k]] == first[key], it.name
    assert T["item"] == sorted(first.values()) and len(first) < sum(it.status == gc.OK for it in items)
    by = {it.name: k for k, it in enumerate(items)}
    # the same body under two witness sets: one tx_id, two rows
    a, b = I["row"][by["same_body_0"]], I["row"][by["same_body_1"]]
    assert a != b and T["tx_id"][a] == T["tx_id"][b]
    # the same inner bytes under two era indices: two rows
    for x, y in (("two_eras_1", "two_eras_2"), ("two_eras_4", "two_eras_6")):
        a, b = I["row"][by[x]], I["row"][by[y]]
        assert a != b and T["tx_id"][a] == T["tx_id"][b] and T["size"][a] == T["size"][b]
    # the far copy shares the row of the first
    for k in (2, 3, 65):
        assert I["row"][by[f"dup{k}_far"]] == I["row"][by[f"dup{k}_0"]]
    # the redeemers' sums
    M = 1 << 64
    for form in ("array", "map"):
        r = I["row"][by[f"red_{form}_2p32"]]
        assert (T["ex_mem"][r], T["ex_steps"][r]) == (1 << 32, 1 << 32)
        r = I["row"][by[f"red_{form}_wrap"]]
        assert (T["ex_mem"][r], T["ex_steps"][r]) == ((M - 1 + 7 + (1 << 63)) % M, (M - 5 + 9 + (1 << 63)) % M)
        r = I["row"][by[f"red_{form}_indef"]]
        assert (T["ex_mem"][r], T["ex_steps"][r]) == (8, 10)
    for bl in gc.BODY_LENS:
        assert T["body_len"][I["row"][by[f"body_len_{bl}"]]] == bl
    r = I["row"][by["not_valid"]]
    assert T["is_valid"][r] == 0
    r = I["row"][by["aux_null"]]
    assert T["aux_len"][r] == 0 and T["aux_off"][r] == 0
    r = I["row"][by["wide_inner_4"]]
    assert T["size"][r] == 1 + T["body_len"][r] + T["wit_len"][r] + 1      # the head's width is not counted


def test_without_dedup_every_ok_item_is_a_row():
    items = gc.corpus()
    arena, off, ln = gc.layout(items)
    I, T, W = gm.verify(arena, off.tolist(), ln.tolist(), dedup=False)
    ok = [k for k, it in enumerate(items) if it.status == gc.OK]
    assert T["item"] == ok and [I["row"][k] for k in ok] == list(range(len(ok)))
