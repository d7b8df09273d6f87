"""Wire blocks (blocks in the node-to-node encoding) in ranges with their requested points, for the
BlockFetch tests (test infrastructure; built on txwit_corpus, block_corpus and byron_corpus).

Seeded.  txwit_corpus's 102 stored blocks carry the transactions and witnesses; a BlockFetch block
also needs a header that decodes and names its body, so every Shelley-based one is given
block_corpus's header over its own segments and, if it was bare, the envelope of an era of its
shape (the body hash holds, the point is the header's).  Two bare blocks, the block that does not
decode and tx_corpus's Byron blocks (random proofs) stay as they are: they are the cases without a row or with an invalid body.  byron_corpus adds a Byron
chain whose bodies hold, and blocks whose Merkle root alone fails.

Then one case for everything praos_verify_fetched_blocks looks at: the same block 2, 3 and 65
times, next to each other and ranges apart; deviants -- a twin differing in one body byte under
the same header, a second different one, the first one again (deviants are not classed among
themselves) and a twin differing only in the width of the envelope's head; every verdict and
range status; every wrapper fault; wider heads on the wrapper; Byron on and off.

corpus() -> list of Range(name, items, points, status, status_off): items a list of Item(name,
bytes, tags, verdict, verdict_off) -- the PRAOS_BF_* verdict meant after the fold with Byron on /
off -- points the (slot, header hash) pairs the range expects, status / status_off the range status
meant.  An item tagged "range" is laid out with a span that leaves the arena (layout)."""
import random
from collections import namedtuple

import block_corpus as bc
import block_integrity as bi
import byron_corpus as yc
import byron_model as bm
import cbor_header as ch
import txwit_corpus as wc
from tx_corpus import hd

Item = namedtuple("Item", "name bytes tags verdict verdict_off")
Range = namedtuple("Range", "name items points status status_off")
Blk = namedtuple("Blk", "name bytes point byron")     # a stored block and its point

(BF_OK, BF_WIRE, BF_DECODE, BF_WRONG_BLOCK, BF_INVALID_BODY, BF_TOO_MANY, BF_UNSUPPORTED,
 BF_NOT_REACHED) = 0, 1, 2, 3, 4, 5, 6, 255
COMPLETE, FAILED, TOO_FEW = 0, 1, 2
SPKP = 129600
EPOCH_SLOTS = yc.EPOCH_SLOTS
NOWHERE = (7, bytes(range(32)))      # the point asked of an item that has no header


def wrap(inner, tag24=b"\xd8\x18", head=None):
    return tag24 + (hd(2, len(inner)) if head is None else head) + inner


def point_of(blk):
    """(slot, header hash) of a stored Shelley-based block that decodes"""
    ok, ho, hl, _ = bi.split_block(blk, 0, len(blk))
    d = ch.decode_header(blk, ho, hl, allow_tpraos=True)
    assert ok and not d["status"] & ch.DEC_FAIL
    return d["fields"]["slot"], d["header_hash"]


def reheader(r, case):
    """txwit_corpus's block with a header that decodes and names its segments"""
    ok, _, _, segs = bi.split_block(case.bytes, 0, len(case.bytes))
    assert ok, case.name
    era = case.bytes[1] if case.bytes[:1] == b"\x82" else 4 if len(segs) == 3 else 6     # a bare block: an era of its shape
    blk, _, _ = bc.make_block(r, SPKP, era=era, segs=[case.bytes[o:o + n] for o, n in segs])
    return Blk(case.name, blk, point_of(blk), False)


def flip_in_segment(blk, k):
    """blk with one byte of segment k (1..) changed so that every span stays what it was"""
    ok, ho, hl, segs = bi.split_block(blk, 0, len(blk))
    o, n = segs[k - 1]
    for at in range(o + n - 1, o - 1, -1):
        v = bytearray(blk)
        v[at] ^= 0x01
        if bi.split_block(bytes(v), 0, len(v)) == (ok, ho, hl, segs):
            return bytes(v)
    raise ValueError("no byte of the segment can change")


_CORPUS = {}


def corpus(seed=20251021):
    if seed in _CORPUS:
        return _CORPUS[seed]
    r = random.Random(seed)
    good, odd = [], []
    for c in wc.corpus():
        if "byron" in c.tags:
            d = bm.parse_block(c.bytes, 0, len(c.bytes))
            odd.append((Blk(c.name, c.bytes, (bm.point_slot(d, EPOCH_SLOTS), d["header_hash"]), True), BF_INVALID_BODY
                        if not d["is_ebb"] else BF_OK))
        elif not bi.split_block(c.bytes, 0, len(c.bytes))[0]:
            odd.append((Blk(c.name, c.bytes, NOWHERE, False), BF_DECODE))
        else:
            if c.name in ("era_bare3", "era_bare4"):                              # as it is: no 2-array inside
                odd.append((Blk(c.name + "_as_is", c.bytes, NOWHERE, False), BF_WIRE))
            good.append(reheader(r, c))
    assert len(good) + len(odd) == 104 and len(good) == 98
    out = []

    def fold(vs):
        """the verdicts after the fold: the items after the first that is not OK are not reached"""
        res, stopped = [], False
        for v in vs:
            res.append(BF_NOT_REACHED if stopped else v)
            stopped = stopped or v != BF_OK
        return res

    def add(name, entries, points=None, tags=()):
        """entries: (item name, wire bytes, verdict before the fold, a Byron item, tags)"""
        points = [] if points is None else points
        von = [BF_TOO_MANY if j >= len(points) and e[2] != BF_WIRE else e[2] for j, e in enumerate(entries)]
        voff = [BF_UNSUPPORTED if e[3] and v not in (BF_WIRE, BF_TOO_MANY) else v for e, v in zip(entries, von)]
        st = []
        for vs in (von, voff):
            st.append(FAILED if any(v != BF_OK for v in vs) else TOO_FEW if len(vs) < len(points) else COMPLETE)
        items = [Item(e[0], e[1], frozenset(e[4]) | frozenset(tags), a, b)
                 for e, a, b in zip(entries, fold(von), fold(voff))]
        out.append(Range(name, items, list(points), st[0], st[1]))

    def ent(b, verdict=BF_OK, wire=None, name=None, tags=()):
        return (name or b.name, wrap(b.bytes) if wire is None else wire, verdict, b.byron, tags)

    def flips_everywhere(b):
        try:
            return len(bi.split_block(b.bytes, 0, len(b.bytes))[3]) == 4 and all(flip_in_segment(b.bytes, k) for k in (1, 2, 3, 4))
        except ValueError:
            return False
    A, B, C, D, E = good[:5]
    F = next(g for g in good if flips_everywhere(g))      # four segments, none of them empty
    # ---- every block that holds, in one range
    add("good_all", [ent(b) for b in good], [b.point for b in good], tags=["good_all"])
    # ---- the blocks without a row or with an invalid body, each between two that hold
    for b, v in odd:
        if b.byron:
            add("odd_" + b.name, [ent(b, v, tags=["byron_random"])], [b.point])
        else:
            add("odd_" + b.name, [ent(A), ent(b, v, tags=["bare" if v == BF_WIRE else "decode"]), ent(B)],
                [A.point, b.point, B.point], tags=["not_reached"])
    # ---- duplicates: a second peer's answer to the same request; 2 in one range, 3 in three ranges,
    # 65 with the one in good_all
    add("good_again", [ent(b) for b in good], [b.point for b in good], tags=["good_again"])
    add("dup2", [ent(B), ent(B)], [B.point, B.point], tags=["dup2"])
    for k in range(3):
        add(f"dup3_{k}", [ent(D)], [D.point], tags=["dup3"])
    add("dup65", [ent(C)] * 64, [C.point] * 64, tags=["dup65"])
    # ---- deviants under D's header: one body byte, another byte, the first again; E's envelope head widened
    d1, d2 = flip_in_segment(D.bytes, 1), flip_in_segment(D.bytes, 2)
    assert len({D.bytes, d1, d2}) == 3 and len(d1) == len(d2) == len(D.bytes)
    add("deviant_1", [ent(D, BF_INVALID_BODY, wrap(d1), tags=["deviant"])], [D.point])
    add("deviant_2", [ent(D, BF_INVALID_BODY, wrap(d2), tags=["deviant", "deviant_other"])], [D.point])
    add("deviant_1_again", [ent(D, BF_INVALID_BODY, wrap(d1), tags=["deviant", "deviant_again"])], [D.point])
    wide = b"\x98\x02" + E.bytes[1:]
    add("envelope_wide", [ent(E), ent(E, BF_OK, wrap(wide), tags=["envelope_wide"])], [E.point, E.point])
    # ---- verdicts
    slot, hh = A.point
    add("wrong_hash", [ent(A, BF_WRONG_BLOCK, tags=["wrong_hash"])], [(slot, bytes([hh[0] ^ 1]) + hh[1:])])
    add("wrong_slot", [ent(A, BF_WRONG_BLOCK, tags=["wrong_slot"])], [(slot + 1, hh)])
    for k in (1, 2, 3, 4):
        add(f"flip_s{k}", [ent(F, BF_INVALID_BODY, wrap(flip_in_segment(F.bytes, k)), tags=[f"flip_s{k}"])], [F.point])
    add("too_many", [ent(A), ent(B, tags=["too_many"])], [A.point])
    add("too_few", [ent(A)], [A.point, B.point], tags=["too_few"])
    add("empty_range", [], [], tags=["empty_range"])
    add("no_items", [], [A.point, B.point], tags=["no_items"])
    # ---- wrapper faults, each asked for A's point
    w = wrap(A.bytes)
    n8 = b"\x82\x08" + A.bytes[2:]
    n255 = b"\x82\x18\xff" + A.bytes[2:]
    faults = [("tag_23", b"\xd7" + w[2:]), ("tag_25", b"\xd8\x19" + w[2:]),
              ("indef_bytes", b"\xd8\x18\x5f" + hd(2, len(A.bytes)) + A.bytes + b"\xff"),
              ("text_string", b"\xd8\x18" + hd(3, len(A.bytes)) + A.bytes),
              ("trailing_outside", w + b"\x00"), ("truncated", w[:-5]), ("truncated_head", w[:3]), ("empty", b""),
              ("disk_tag_8", wrap(n8)), ("disk_tag_255", wrap(n255)), ("no_array", wrap(A.bytes[2:])),
              ("tag_not_uint", wrap(b"\x82\x20" + A.bytes[2:])), ("array_3", wrap(b"\x83" + A.bytes[1:])),
              ("array_indef", wrap(b"\x9f" + A.bytes[1:] + b"\xff"))]
    for name, raw in faults:
        add("fault_" + name, [ent(A, BF_WIRE, raw, name, tags=["fault_" + name])], [A.point])
    add("fault_range", [ent(A, BF_WIRE, w, "range", tags=["range"])], [A.point])
    add("trailing_inside", [ent(A, BF_DECODE, wrap(A.bytes + b"\x00"), tags=["trailing_inside"])], [A.point])
    # ---- wider heads on the wrapper: the same inner bytes, the same row
    n = len(A.bytes)
    add("wide_wrapper", [ent(A, wire=b"\xd9\x00\x18" + hd(2, n) + A.bytes, tags=["wide_tag"]),
                         ent(A, wire=b"\xd8\x18\x5a" + n.to_bytes(4, "big") + A.bytes, tags=["wide_len"]),
                         ent(A, wire=b"\xda\x00\x00\x00\x18\x5b" + n.to_bytes(8, "big") + A.bytes, tags=["wide_both"])],
        [A.point] * 3)
    # ---- Byron: a chain whose bodies hold; a Merkle root that alone fails, of 2 transactions and of 1
    chain = yc.make_chain(r, [[{"tx_sizes": (40, 300)}, {"tx_sizes": ()}, {"tx_sizes": (9,), "indef": True}], [{}]])
    bl = [Blk(f"byron_chain_{k}", b.bytes, (b.epoch * EPOCH_SLOTS + (0 if b.kind == 0 else b.sie), b.header_hash), True)
          for k, b in enumerate(chain)]
    add("byron_chain", [ent(b, tags=["byron_ok", "byron_ebb_ok" if chain[k].kind == 0 else "byron_main_ok"])
                        for k, b in enumerate(bl)], [b.point for b in bl])
    dlg = yc.Delegate(r)
    for ntx, v, tag in ((2, BF_UNSUPPORTED, "byron_root_2"), (1, BF_INVALID_BODY, "byron_root_1"),
                        (0, BF_UNSUPPORTED, "byron_root_0")):
        m = yc.Main(r, dlg, bytes(32), 5, 3, 77, tx_sizes=(30,) * ntx)
        m.bad_root = True
        m.sign()
        add(tag, [ent(Blk(tag, m.bytes, (5 * EPOCH_SLOTS + 3, m.header_hash), True), v, tags=[tag])],
            [(5 * EPOCH_SLOTS + 3, m.header_hash)])
    trunc = chain[1].bytes[:-4]
    add("byron_decode", [ent(Blk("byron_decode", trunc, NOWHERE, True), BF_DECODE, tags=["byron_decode"])], [NOWHERE])
    # an EBB asked for at another slot of its epoch: its slot is the epoch's first
    e0 = bl[0]
    add("ebb_slot", [ent(e0, BF_WRONG_BLOCK, tags=["ebb_slot"])], [(e0.point[0] + 1, e0.point[1])])
    assert sum(len(g.items) for g in out) >= 260
    _CORPUS[seed] = out
    return out


def layout(ranges, reverse=False, first=None):
    """-> (arena, off, len, item_first, exp_first, exp_slot, exp_hash [.][32] as bytes, items): the
    ranges' items back to back behind a few odd bytes; reverse: the ranges in the opposite order;
    first: only the first so many items, the ranges cut to them (their points kept)."""
    ranges = list(reversed(ranges)) if reverse else list(ranges)
    off, ln, parts, pos, items = [], [], [b"\x00\x01\x02"], 3, []
    item_first, exp_first, exp_slot, exp_hash = [0], [0], [], []
    for g in ranges:
        for it in g.items:
            if first is not None and len(items) >= first:
                break
            off.append(pos)
            ln.append(len(it.bytes))
            parts.append(it.bytes)
            pos += len(it.bytes)
            items.append(it)
        item_first.append(len(items))
        exp_first.append(exp_first[-1] + len(g.points))
        exp_slot += [s for s, _ in g.points]
        exp_hash += [h for _, h in g.points]
    arena = b"".join(parts)
    for k, it in enumerate(items):
        if "range" in it.tags:
            off[k] = len(arena) - len(it.bytes) + 1
    return arena, off, ln, item_first, exp_first, exp_slot, exp_hash, items
