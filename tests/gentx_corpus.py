"""Wire transactions (GenTxs in the node-to-node encoding) for the TxSubmission tests (test
infrastructure; built on txwit_corpus and tx_corpus).

Seeded.  Every transaction of txwit_corpus's Shelley-based blocks is taken out of its block (by
tx_index_model's rows) and wrapped again as a wire item of the block's era; then one case for
everything praos_verify_gen_txs looks at: repeats of an item (adjacent and far apart), the same
body under another witness set, the same inner bytes under two era indices, every status and
every SHAPE rule, wider heads, the indefinite inner array, null and present aux, both redeemer
forms with units at 2^32 and wrapping 2^64, bodies of 1 to 5000 bytes around Blake2b's block
edges, and the Byron kinds.

corpus() -> list of Item(name, bytes, tags, status, want).  status: the PRAOS_WIRE_* / PRAOS_GTX_*
code meant; want: None for an item without a row, else "shape" (the witness set is outside the
shapes) or the list of its witnesses' intended validity in witness-row order.  An item tagged
"range" is laid out with a span that leaves the arena (layout)."""
from collections import namedtuple

import numpy as np

import tx_corpus as tc
import tx_index_model as tm
import txwit_corpus as wc
from tx_corpus import bstr, hd, seq

Item = namedtuple("Item", "name bytes tags status want")

OK, RANGE, SYNTAX, ERA, TRAILING, SHAPE, BYRON = 0, 1, 2, 3, 4, 5, 6
COUNTS = (0, 1, 63, 64, 65, 257)      # 257: one more than the workgroup
BODY_LENS = (1, 127, 128, 129, 255, 256, 257, 1023, 5000)


def wrap(era, inner):
    return b"\x82" + hd(0, era) + b"\xd8\x18" + hd(2, len(inner)) + inner


def tx_bytes(era, body, wits, aux=None, valid=True, indef=False, head=None):
    """[body, wits, aux / null] for era <= 3, [body, wits, isValid, aux / null] otherwise"""
    items = [body, wits] + ([b"\xf5" if valid else b"\xf4"] if era >= 4 else []) + [b"\xf6" if aux is None else aux]
    if head is not None:
        return head + b"".join(items)
    return seq(4, items, indef)


def exunits(mem, steps, indef=False):
    return seq(4, [hd(0, mem), hd(0, steps)], indef)


def redeemers(r, form, units, indef=False):
    if form == "array":
        return seq(4, [seq(4, [hd(0, 0), hd(0, k), bstr(r, 5), exunits(m, s, indef)], indef)
                       for k, (m, s) in enumerate(units)], indef)
    return seq(5, [(hd(4, 2) + hd(0, 0) + hd(0, k), seq(4, [bstr(r, 5), exunits(m, s, indef)], indef))
                   for k, (m, s) in enumerate(units)], indef)


def source_blocks():
    """txwit_corpus's Shelley-based blocks that have rows, in from_blocks' order"""
    return [c for c in wc.corpus() if c.want is not None and "byron" not in c.tags]


def from_blocks():
    """every transaction of txwit_corpus's Shelley-based blocks as a wire item of its era"""
    out = []
    for c in source_blocks():
        b = c.bytes
        st, rows = tm.index_block(b, 0, len(b))
        assert st == tm.OK and len(rows) == len(c.want), c.name
        tagged = b[0] == 0x82 and b[1] < 24
        four = tm.head(b, 2 if tagged else 0, len(b))[2] == 5
        era = b[1] - 1 if tagged else (5 if four else 3)
        assert (era >= 4) == four, c.name
        for t, (rw, want) in enumerate(zip(rows, c.want)):
            body = b[rw["body_off"]:rw["body_off"] + rw["body_len"]]
            wits = b[rw["wit_off"]:rw["wit_off"] + rw["wit_len"]]
            aux = b[rw["aux_off"]:rw["aux_off"] + rw["aux_len"]] if rw["aux_len"] else None
            out.append(Item(f"{c.name}.{t}", wrap(era, tx_bytes(era, body, wits, aux, bool(rw["is_valid"]))),
                            frozenset(c.tags | {"txwit", f"era_{era}", "aux_present" if aux else "aux_null"}), OK, want))
    return out


_CORPUS = {}


def corpus(seed=20251017):
    if seed in _CORPUS:
        return _CORPUS[seed]
    g = wc.Gen(seed)
    r = g.r
    out = from_blocks()
    base = list(out)

    def add(name, data, status, want, *tags):
        out.append(Item(name, data, frozenset(tags), status, want))

    def good(era, name, *tags, **kw):
        body, wits, want = g.tx(1, 0, four=era >= 4)
        add(name, wrap(era, tx_bytes(era, body, wits, **kw)), OK, want, *tags)

    # ---- the same item again: adjacent, and far apart (the far copies come at the end)
    reps = [(base[3], 2), (base[10], 3), (base[20], 65)]
    for it, k in reps:
        for j in range(k - 1):
            add(f"dup{k}_{j}", it.bytes, OK, it.want, f"dup{k}_adjacent", "dup")
    # ---- the same body under another witness set: the same tx_id, two rows
    body = tc.body(r)
    for k in range(2):
        _, wits, want = g.tx(1 + k, 0, four=True, body=body)
        add(f"same_body_{k}", wrap(5, tx_bytes(5, body, wits)), OK, want, "same_body")
    # ---- the same inner bytes under two era indices: two rows
    body, wits, want = g.tx(1, 1)
    for era in (1, 2):
        add(f"two_eras_{era}", wrap(era, tx_bytes(era, body, wits)), OK, want, "two_eras")
    body, wits, want = g.tx(2, 0, four=True)
    for era in (4, 6):
        add(f"two_eras_{era}", wrap(era, tx_bytes(era, body, wits)), OK, want, "two_eras")
    # ---- the SHAPE rules
    body, wits, want = g.tx(1, 0, four=True)
    add("arr2", wrap(3, seq(4, [body, wits], False)), SHAPE, None, "shape_arr2")
    add("arr5", wrap(5, seq(4, [body, wits, b"\xf5", b"\xf6", b"\xf6"], False)), SHAPE, None, "shape_arr5")
    add("three_under_4", wrap(4, seq(4, [body, wits, b"\xf6"], False)), SHAPE, None, "shape_three_under_4")
    add("four_under_3", wrap(3, seq(4, [body, wits, b"\xf5", b"\xf6"], False)), SHAPE, None, "shape_four_under_3")
    add("indef_three_under_4", wrap(4, seq(4, [body, wits, b"\xf6"], True)), SHAPE, None, "shape_indef_count")
    add("indef_no_break", wrap(5, b"\x9f" + body + wits + b"\xf5\xf6"), SHAPE, None, "shape_indef_no_break")
    add("valid_f6", wrap(5, seq(4, [body, wits, b"\xf6", b"\xf6"], False)), SHAPE, None, "shape_valid_f6")
    add("valid_01", wrap(5, seq(4, [body, wits, b"\x01", b"\xf6"], False)), SHAPE, None, "shape_valid_01")
    add("trailing_inside", wrap(5, tx_bytes(5, body, wits) + b"\x00"), SHAPE, None, "shape_trailing_inside")
    add("inner_not_array", wrap(5, seq(5, [(body, wits), (b"\xf5", b"\xf6")], False)), SHAPE, None, "shape_not_array")
    add("inner_truncated", wrap(5, tx_bytes(5, body, wits)[:-40]), SHAPE, None, "shape_truncated")
    add("inner_empty", wrap(5, b""), SHAPE, None, "shape_empty")
    add("body_not_map", wrap(5, tx_bytes(5, seq(4, [hd(0, 1)], False), wits)), SHAPE, None, "shape_body_not_map")
    add("body_not_map_3", wrap(2, tx_bytes(2, hd(0, 7), wits)), SHAPE, None, "shape_body_not_map")
    bad5 = seq(5, [(hd(0, 0), seq(4, [], False)), (hd(0, 5), hd(0, 9))], False)
    add("key5_uint", wrap(4, tx_bytes(4, body, bad5)), SHAPE, None, "shape_key5")
    add("key5_uint_era3", wrap(3, tx_bytes(3, body, bad5)), OK, [], "key5_unread_era3")     # eras 1..3: key 5 is not read
    bad5 = seq(5, [(hd(0, 5), seq(4, [seq(4, [hd(0, 0), hd(0, 0), hd(0, 0)], False)], False))], False)
    add("key5_arity", wrap(6, tx_bytes(6, body, bad5)), SHAPE, None, "shape_key5")
    # the two copies of a refused transaction: both SHAPE, no row between their neighbours'
    add("key5_arity_again", wrap(6, tx_bytes(6, body, bad5)), SHAPE, None, "shape_key5", "shape_twice")
    # ---- the wrapper's statuses
    whole = wrap(5, tx_bytes(5, body, wits))
    inner = tx_bytes(5, body, wits)
    add("trailing_outside", whole + b"\x00", TRAILING, None, "trailing")
    add("tag_23", b"\x82\x05\xd7" + hd(2, len(inner)) + inner, SYNTAX, None, "syntax_tag23")
    add("indef_bytes", b"\x82\x05\xd8\x18\x5f" + hd(2, len(inner)) + inner + b"\xff", SYNTAX, None, "syntax_indef_bytes")
    add("outer_3", b"\x83\x05\xd8\x18" + hd(2, len(inner)) + inner + b"\x00", SYNTAX, None, "syntax_outer")
    add("outer_indef", b"\x9f\x05\xd8\x18" + hd(2, len(inner)) + inner + b"\xff", SYNTAX, None, "syntax_outer")
    add("era_wide_256", b"\x82\x19\x01\x00\xd8\x18" + hd(2, len(inner)) + inner, SYNTAX, None, "syntax_era_word8")
    add("short_bytes", whole[:-1], SYNTAX, None, "syntax_short")
    add("empty", b"", SYNTAX, None, "syntax_empty")
    add("era_7", wrap(7, inner), ERA, None, "era_7")
    add("era_255", wrap(255, inner), ERA, None, "era_255")
    add("range", whole, RANGE, None, "range")
    # ---- wider heads: on the wrapper, on the inner array
    add("wide_wrapper", b"\x98\x02\x18\x05\xd9\x00\x18\x5a" + len(inner).to_bytes(4, "big") + inner, OK, want,
        "wide_wrapper")
    add("wide_inner_4", wrap(5, tx_bytes(5, body, wits, head=b"\x98\x04")), OK, want, "wide_inner")
    b3, w3, want3 = g.tx(1, 1)
    add("wide_inner_3", wrap(2, tx_bytes(2, b3, w3, head=b"\x99\x00\x03")), OK, want3, "wide_inner")
    # ---- the indefinite inner array; aux null and present; isValid false
    good(5, "indef_inner_4", "indef_inner", indef=True)
    good(1, "indef_inner_3", "indef_inner", indef=True, aux=bstr(r, 20))
    good(6, "aux_present", "aux_present", aux=seq(5, [(hd(0, 1), bstr(r, 33))], True))
    good(3, "aux_null", "aux_null")
    good(4, "not_valid", "is_valid_false", valid=False)
    # ---- body lengths around Blake2b's 128-byte blocks (tx_id), neighbours in one workgroup
    for bl in BODY_LENS:
        body, wits, want = g.tx(1, 0, four=True, body=tc.body(r, body_len=bl))
        add(f"body_len_{bl}", wrap(5, tx_bytes(5, body, wits)), OK, want, f"body_len_{bl}", "body_len")
    # ---- both redeemer forms; units at 2^32 and wrapping 2^64
    M = 1 << 64
    for form in ("array", "map"):
        for name, units, ind in (("2p32", [(1 << 32, 1 << 32)], False),
                                 ("wrap", [(M - 1, M - 5), (7, 9), (1 << 63, 1 << 63)], False),
                                 ("indef", [(3, 4), (5, 6)], True), ("none", [], False)):
            body, ws, want = g.tx(1, 0, four=True)
            # the witness set with key 5 put after key 0
            n = ws[0] & 31
            assert ws[0] >> 5 == 5 and n < 23
            ws = bytes([0xA0 | (n + 1)]) + ws[1:] + hd(0, 5) + redeemers(r, form, units, ind)
            add(f"red_{form}_{name}", wrap(6, tx_bytes(6, body, ws)), OK, want, f"red_{form}", f"units_{name}")
    # ---- Byron: kinds 0..3 unwrapped only; anything else is SYNTAX
    for kind in range(4):
        add(f"byron_{kind}", b"\x82\x00\x82" + hd(0, kind) + bstr(r, 40 + kind), BYRON, None, f"byron_{kind}")
    add("byron_4", b"\x82\x00\x82\x04" + bstr(r, 40), SYNTAX, None, "byron_4")
    add("byron_indef", b"\x82\x00\x9f\x00" + bstr(r, 40) + b"\xff", SYNTAX, None, "byron_other")
    add("byron_no_payload", b"\x82\x00\x82\x00", SYNTAX, None, "byron_other")
    add("byron_tag24", b"\x82\x00\xd8\x18" + hd(2, len(inner)) + inner, SYNTAX, None, "byron_other")
    # ---- the far copies
    for it, k in reps:
        add(f"dup{k}_far", it.bytes, OK, it.want, "dup_far", "dup")
    _CORPUS[seed] = out
    return out


def layout(items):
    """-> (arena u8, off u64, len u32); an item tagged "range" gets a span that leaves the arena"""
    off, p = [], 0
    for it in items:
        off.append(p)
        p += len(it.bytes)
    arena = np.frombuffer(b"".join(it.bytes for it in items) + bytes(8), np.uint8)
    off = np.array(off, np.uint64)
    ln = np.array([len(it.bytes) for it in items], np.uint32)
    for k, it in enumerate(items):
        if "range" in it.tags:
            off[k] = len(arena) - 5
    return arena, off, ln
