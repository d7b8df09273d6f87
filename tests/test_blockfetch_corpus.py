"""CPU: the wire-block corpus (blockfetch_corpus.py) says what it means to say.

Every case the tests of praos_verify_fetched_blocks rely on occurs, and the model alone gives each
item the verdict and each range the status the generator meant, with Byron on and off."""
import blockfetch_corpus as fc
import blockfetch_model as fm

WANT_TAGS = ("good_all", "good_again", "dup2", "dup3", "dup65", "deviant", "deviant_other", "deviant_again",
             "envelope_wide", "wrong_hash", "wrong_slot", "flip_s1", "flip_s2", "flip_s3", "flip_s4", "too_many",
             "too_few", "bare", "decode", "not_reached", "fault_tag_23", "fault_indef_bytes", "fault_trailing_outside",
             "trailing_inside", "fault_truncated", "range", "fault_disk_tag_8", "fault_disk_tag_255", "fault_no_array",
             "wide_tag", "wide_len", "wide_both", "byron_ok", "byron_ebb_ok", "byron_main_ok", "byron_random",
             "byron_root_2", "byron_root_1", "byron_root_0", "byron_decode", "ebb_slot")


def test_every_case_occurs():
    R = fc.corpus()
    items = [it for g in R for it in g.items]
    assert len(items) >= 260 and R is fc.corpus()
    tags = set().union(*(it.tags for it in items))
    assert not [t for t in WANT_TAGS if t not in tags]
    names = {g.name for g in R}
    assert {"empty_range", "no_items", "too_few"} <= names
    assert {it.verdict for it in items} == {0, 1, 2, 3, 4, 5, 6, 255}
    assert {g.status for g in R} == {fc.COMPLETE, fc.FAILED, fc.TOO_FEW}
    by = {g.name: g for g in R}
    assert not by["empty_range"].items and not by["empty_range"].points and by["empty_range"].status == fc.COMPLETE
    assert not by["no_items"].items and len(by["no_items"].points) == 2 and by["no_items"].status == fc.TOO_FEW
    assert sum(1 for it in items if it.bytes == by["dup65"].items[0].bytes) >= 65
    assert len(by["dup2"].items) == 2 and by["dup2"].items[0].bytes == by["dup2"].items[1].bytes
    # the deviants are D's length and differ from it and from each other; the first comes twice
    d, d1, d2, d1b = (by[k].items[0].bytes for k in ("dup3_0", "deviant_1", "deviant_2", "deviant_1_again"))
    assert len({d, d1, d2}) == 3 and len(d) == len(d1) == len(d2) and d1 == d1b


def test_the_model_gives_every_item_the_verdict_meant():
    R = fc.corpus()
    arena, off, ln, ifirst, efirst, es, eh, items = fc.layout(R)
    for es_on in (fc.EPOCH_SLOTS, 0):
        I, G, W, *_ = fm.verify(arena, off, ln, ifirst, efirst, es, eh, byron_epoch_slots=es_on, witnesses=False)
        want = [it.verdict if es_on else it.verdict_off for it in items]
        assert [(it.name, v) for it, v, w in zip(items, I["verdict"], want) if v != w] == []
        assert G["status"] == [g.status if es_on else g.status_off for g in R]
        assert all(s == a for s, a in zip(G["stop"], G["accepted"]))
    # the rows: duplicates share one, a deviant has its own (also the second time), wide wrappers share
    I, G, W, *_ = fm.verify(arena, off, ln, ifirst, efirst, es, eh, byron_epoch_slots=fc.EPOCH_SLOTS, witnesses=False)
    row = {}
    for it, q in zip(items, I["row"]):
        row.setdefault(it.name + "|" + "+".join(sorted(it.tags)), []).append(q)
    pick = lambda tag: [q for it, q in zip(items, I["row"]) if tag in it.tags]
    assert len(set(pick("dup65"))) == 1 and len(set(pick("dup3"))) == 1 and len(set(pick("dup2"))) == 1
    assert pick("good_all") == pick("good_again") and len(set(pick("good_all"))) == len(pick("good_all"))
    dev = pick("deviant")
    assert len(dev) == 3 and len(set(dev)) == 3 and not set(dev) & set(pick("dup3"))
    assert len(set(pick("wide_tag") + pick("wide_len") + pick("wide_both"))) == 1
    assert pick("wide_tag")[0] == pick("good_all")[0]
    assert pick("envelope_wide")[0] not in pick("good_all")
    assert sorted(set(q for q in I["row"] if q != fm.NO_ROW)) == list(range(len(W["item"])))
    assert W["item"] == sorted(W["item"])        # rows in order of first appearance
    # without dedup every item that decodes is its own row
    I2, _, W2, *_ = fm.verify(arena, off, ln, ifirst, efirst, es, eh, byron_epoch_slots=fc.EPOCH_SLOTS, dedup=False,
                              witnesses=False)
    assert len(W2["item"]) == sum(q != fm.NO_ROW for q in I["row"]) and I2["verdict"] == I["verdict"]
