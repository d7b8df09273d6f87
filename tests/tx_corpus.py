"""Stored blocks full of transactions for the transaction-index tests (test infrastructure).

Seeded and pure Python: no signatures, no hashes.  A header only has to pass the block split's
arity peek ([body of 15 / 10 items, kesSig]); a Byron header only has to have the shapes the
Byron split reads.  Everything the index looks at is chosen per case: the transaction count, the
body length (to the byte), definite or indefinite forms of s1..s4, of the body map, of the
outputs array and of both redeemer forms, indefinite items nested inside outputs, which
transactions have auxiliary data (and in which key order), which are listed invalid, the number
of outputs, the redeemers' steps, and one mutation that breaks the shape.

corpus() -> list of Case(name, bytes, tags); the tags name what a case was built to hold, and
tests/test_tx_corpus.py asserts (through the model's output, where the model can see it) that
each thing the issue lists occurs."""
import random
from collections import namedtuple

Case = namedtuple("Case", "name bytes tags")

TX_COUNTS = (0, 1, 2, 63, 64, 65, 300)
BODY_LENS = (1, 127, 128, 129, 255, 256, 257, 70000)
OUT_COUNTS = (0, 1, 23, 24, 25, 256)
STEPS = (1 << 32, (1 << 64) - 1, (1 << 64) - 5, 7)
SHAPE_MUTATIONS = ("s1_not_array", "s2_not_array", "s3_not_map", "s4_not_array", "s2_count", "s3_key_not_uint",
                   "s3_key_range", "s4_entry_not_uint", "s4_entry_range", "body_not_map", "key1_not_array",
                   "key5_neither", "key5_redeemer_arity", "key5_steps_not_uint")


def hd(mt, v):
    """the shortest head of major type mt with argument v"""
    if v < 24:
        return bytes([(mt << 5) | v])
    for ai, nb in ((24, 1), (25, 2), (26, 4), (27, 8)):
        if v < 1 << (8 * nb):
            return bytes([(mt << 5) | ai]) + v.to_bytes(nb, "big")
    raise ValueError(v)


def rb(r, n):
    return bytes(r.getrandbits(8) for _ in range(n)) if n < 64 else r.getrandbits(8 * n).to_bytes(n, "big")


def seq(mt, items, indef):
    """an array (mt 4) of items or a map (mt 5) of (key, value) pairs"""
    flat = b"".join(items) if mt == 4 else b"".join(k + v for k, v in items)
    return (bytes([(mt << 5) | 31]) + flat + b"\xff") if indef else (hd(mt, len(items)) + flat)


def bstr(r, n):
    return hd(2, n) + rb(r, n)


def filler(r, size):
    """one byte string item of exactly `size` bytes (size >= 1; 25, 258 and 65539 do not exist
    as one definite string: an array around a shorter one)"""
    assert size >= 1
    for n in (size - 1, size - 2, size - 3, size - 5):
        if n >= 0 and len(hd(2, n)) + n == size:
            return bstr(r, n)
    return b"\x81" + filler(r, size - 1)


def output(r, nested_indef=False):
    if nested_indef:     # [indefinite bytes, [indefinite array], indefinite map] inside an indefinite array
        return b"\x9f\x5f\x43" + rb(r, 3) + b"\x41\x00\xff\x9f\x01\x9f\xff\xff\xbf\x00\x01\xff\xff"
    return hd(4, 2) + bstr(r, 29) + hd(0, r.randrange(1, 1 << 40))


def body(r, n_out=1, body_len=None, indef=False, out_indef=False, nested=False, key1=True, wide_key=False):
    """a transaction body: {0: filler, 1: [outputs], 2: fee}, body_len bytes when given"""
    if body_len == 1:
        return b"\xa0"
    outs = seq(4, [output(r, nested) for _ in range(n_out)], out_indef)
    k1 = b"\x18\x01" if wide_key else hd(0, 1)        # a key in a wider head is the same key
    pairs = [(hd(0, 2), hd(0, r.randrange(1 << 20)))]
    if key1:
        pairs.insert(0, (k1, outs))
    if body_len is not None:
        base = len(seq(5, [(hd(0, 0), b"")] + pairs, indef))
        pairs.insert(0, (hd(0, 0), filler(r, body_len - base)))
    else:
        pairs.insert(0, (hd(0, 0), bstr(r, r.randrange(30, 60))))
    b = seq(5, pairs, indef)
    assert body_len is None or len(b) == body_len
    return b


def exunits(steps, indef=False):
    return seq(4, [hd(0, 1000), hd(0, steps)], indef)


def redeemers(r, form, steps, indef=False, inner_indef=False):
    if form == "array":
        return seq(4, [seq(4, [hd(0, 0), hd(0, k), bstr(r, 5), exunits(s, inner_indef)], inner_indef)
                       for k, s in enumerate(steps)], indef)
    return seq(5, [(hd(4, 2) + hd(0, 0) + hd(0, k), seq(4, [bstr(r, 5), exunits(s, inner_indef)], inner_indef))
                   for k, s in enumerate(steps)], indef)


def witness(r, red=None, indef=False, size=None):
    pairs = [(hd(0, 0), seq(4, [hd(4, 2) + bstr(r, 32) + bstr(r, 64)], False))]
    if size is not None:
        base = len(seq(5, [(hd(0, 0), b"")], indef))
        pairs = [(hd(0, 0), filler(r, size - base))]
    if red is not None:
        pairs.append((hd(0, 5), red))
    return seq(5, pairs, indef)


def header(r, arity):
    return hd(4, 2) + hd(4, arity) + b"".join(hd(0, r.randrange(24)) for _ in range(arity)) + bstr(r, 40)


def block(r, tag, bodies, wits, aux=(), invalid=(), indef=(), raw=None):
    """tag 2..7, or "bare3" / "bare4".  aux: (index, item) pairs in the order written; invalid:
    indices; indef: the segments (1..4) written in the indefinite form; raw: {segment: bytes}
    written instead of the built one."""
    four = tag == "bare4" or (isinstance(tag, int) and tag >= 5)
    segs = [seq(4, bodies, 1 in indef), seq(4, wits, 2 in indef),
            seq(5, [(hd(0, k), v) for k, v in aux], 3 in indef)]
    if four:
        segs.append(seq(4, [hd(0, k) for k in invalid], 4 in indef))
    for k, v in (raw or {}).items():
        segs[k - 1] = v
    arity = 10 if tag in ("bare3", "bare4") or tag >= 6 else 15
    inner = hd(4, 1 + len(segs)) + header(r, arity) + b"".join(segs)
    return inner if isinstance(tag, str) else hd(4, 2) + hd(0, tag) + inner


def byron_tx(r, n_out=1, indef=False, out_indef=False):
    ins = seq(4, [hd(4, 2) + hd(0, 0) + b"\xd8\x18" + bstr(r, 36)], indef)
    outs = seq(4, [hd(4, 2) + bstr(r, 30) + hd(0, r.randrange(1 << 30)) for _ in range(n_out)], out_indef)
    return seq(4, [ins, outs, hd(5, 0)], False)


def byron_wits(r):
    return hd(4, 1) + hd(4, 2) + hd(0, 0) + b"\xd8\x18" + bstr(r, 70)


def byron_main(r, txs, indef=False):
    """txs: (tx item, witnesses item) pairs"""
    proof = (hd(4, 4) + hd(4, 3) + hd(0, len(txs)) + bstr(r, 32) + bstr(r, 32) + hd(4, 2) + hd(0, 0) + bstr(r, 32) +
             bstr(r, 32) + bstr(r, 32))
    cert = hd(4, 4) + hd(0, 0) + bstr(r, 64) + bstr(r, 64) + bstr(r, 64)
    consensus = (hd(4, 4) + hd(4, 2) + hd(0, 3) + hd(0, 17) + bstr(r, 64) + hd(4, 1) + hd(0, 99) +
                 hd(4, 2) + hd(0, 2) + hd(4, 2) + cert + bstr(r, 64))
    hdr = hd(4, 5) + hd(0, 764824073) + bstr(r, 32) + proof + consensus + hd(4, 1) + hd(5, 0)
    txp = seq(4, [hd(4, 2) + t + w for t, w in txs], indef)
    bdy = hd(4, 4) + txp + hd(4, 0) + hd(4, 0) + hd(4, 0)
    return hd(4, 2) + hd(0, 1) + hd(4, 3) + hdr + bdy + hd(4, 1) + hd(5, 0)


def byron_ebb(r):
    hdr = (hd(4, 5) + hd(0, 764824073) + bstr(r, 32) + bstr(r, 32) + hd(4, 2) + hd(0, 3) + hd(4, 1) + hd(0, 98) +
           hd(4, 1) + hd(5, 0))
    return hd(4, 2) + hd(0, 0) + hd(4, 3) + hdr + hd(4, 0) + hd(4, 1) + hd(5, 0)


def corpus(seed=20240607):
    r = random.Random(seed)
    out = []

    def add(name, data, *tags):
        out.append(Case(name, data, frozenset(tags)))

    def simple(n, four, **kw):
        red = redeemers(r, "array", [3, 4]) if four else None
        return [body(r, **kw) for _ in range(n)], [witness(r, red) for _ in range(n)]

    # every era tag and the bare forms, a handful of plain transactions each
    for tag in (2, 3, 4, 5, 6, 7, "bare3", "bare4"):
        four = tag == "bare4" or (isinstance(tag, int) and tag >= 5)
        b, w = simple(3, four)
        add(f"era_{tag}", block(r, tag, b, w, aux=[(1, bstr(r, 20))], invalid=[2] if four else ()), f"tag_{tag}")
    # transaction counts at the wave and workgroup edges of the per-row kernel
    for n in TX_COUNTS:
        for tag, ind in ((6, ()), (3, (1, 2))) if n != 300 else ((7, (1, 2, 3, 4)),):
            four = tag >= 5
            b, w = simple(n, four)
            aux = [(k, bstr(r, 10 + k % 7)) for k in range(0, n, 3)]
            inv = list(range(1, n, 5)) if four else ()
            add(f"count_{n}_tag{tag}", block(r, tag, b, w, aux, inv, ind), f"count_{n}")
    # body lengths at the Blake2b block edges (the transactions of a block are of one size, and
    # of mixed sizes in the last two blocks)
    for ln in BODY_LENS:
        n = 1 if ln == 70000 else 3
        b = [body(r, body_len=ln, n_out=0 if ln < 127 else 2) for _ in range(n)]
        add(f"body_len_{ln}", block(r, 6, b, [witness(r) for _ in range(n)]), f"body_len_{ln}")
    mixed = [body(r, body_len=ln, n_out=1) for ln in (127, 257, 128, 5000, 129, 255, 256, 100)]
    add("body_len_mixed", block(r, 7, mixed, [witness(r, size=50 + 40 * k) for k in range(len(mixed))]), "mixed")
    add("body_len_mixed_indef", block(r, 5, mixed[::-1], [witness(r, indef=True) for _ in mixed], indef=(1, 2)),
        "mixed")
    # definite and indefinite forms of s1..s4, one segment at a time and all at once
    for ind in ((), (1,), (2,), (3,), (4,), (1, 2, 3, 4)):
        b, w = simple(4, True)
        add(f"indef_segs_{'_'.join(map(str, ind)) or 'none'}",
            block(r, 6, b, w, [(0, bstr(r, 9)), (3, hd(4, 0))], [1, 3], ind), *(f"indef_s{k}" for k in ind),
            *(f"def_s{k}" for k in (1, 2, 3, 4) if k not in ind))
    # the body map, the outputs array, nested indefinite items inside outputs, the wide key
    for bi, oi, nest, wide in ((True, False, False, False), (False, True, False, False), (True, True, True, False),
                               (False, False, False, True), (False, False, True, False)):
        b = [body(r, n_out=k + 1, indef=bi, out_indef=oi, nested=nest, wide_key=wide) for k in range(3)]
        add(f"body_forms_{int(bi)}{int(oi)}{int(nest)}{int(wide)}", block(r, 6, b, [witness(r) for _ in b]),
            *(["body_indef"] if bi else ["body_def"]), *(["outs_indef"] if oi else ["outs_def"]),
            *(["nested_indef"] if nest else []), *(["wide_key"] if wide else []))
    # output counts at the CBOR head widths, in both forms; no key 1 at all
    for k in OUT_COUNTS:
        for oi in (False, True):
            b = [body(r, n_out=k, out_indef=oi), body(r, n_out=1)]
            add(f"outs_{k}_{int(oi)}", block(r, 4, b, [witness(r), witness(r)]), f"outs_{k}")
    b = [body(r, key1=False), body(r, n_out=2)]
    add("no_key1", block(r, 6, b, [witness(r), witness(r)]), "no_key1")
    # auxiliary data: absent, out of order, for every transaction, a repeated key
    b, w = simple(5, True)
    add("aux_absent", block(r, 6, b, w), "aux_absent")
    add("aux_out_of_order", block(r, 6, b, w, [(4, bstr(r, 5)), (0, hd(5, 0)), (2, bstr(r, 300))]), "aux_unordered")
    add("aux_all", block(r, 7, b, w, [(k, bstr(r, 3 + k)) for k in range(5)], indef=(3,)), "aux_all")
    add("aux_repeated", block(r, 6, b, w, [(1, bstr(r, 5)), (1, bstr(r, 8))]), "aux_repeated")
    # invalid lists: empty, partial, full
    add("invalid_empty", block(r, 6, b, w), "invalid_empty")
    add("invalid_partial", block(r, 5, b, w, invalid=[3, 0]), "invalid_partial")
    add("invalid_full", block(r, 7, b, w, invalid=[0, 1, 2, 3, 4], indef=(4,)), "invalid_full")
    # redeemers: both forms, definite and indefinite at both levels, steps at 2^32 and near 2^64
    for form in ("array", "map"):
        for ind, inner in ((False, False), (True, False), (True, True)):
            ws = [witness(r, redeemers(r, form, list(STEPS), ind, inner), indef=ind),
                  witness(r, redeemers(r, form, [(1 << 64) - 1, 2], ind, inner)),
                  witness(r, redeemers(r, form, [], ind)), witness(r)]
            bs = [body(r) for _ in ws]
            add(f"redeemers_{form}_{int(ind)}{int(inner)}", block(r, 7 if form == "map" else 5, bs, ws),
                f"red_{form}", f"red_{form}_{'indef' if ind else 'def'}", "steps_wrap")
    # a block of tags 2..4 whose witness sets carry a key 5: not looked at there
    ws = [witness(r, redeemers(r, "array", [11])), witness(r, hd(0, 9))]
    add("key5_in_three_segments", block(r, 3, [body(r), body(r)], ws), "key5_ignored")
    # a witness set that is no map: no key 5
    add("witness_not_map", block(r, 6, [body(r)], [hd(4, 0)]), "wit_not_map")

    # ---- the shape mutations, one per case, each beside an intact neighbour in the corpus
    def mut(name, **kw):
        b, w = simple(3, True)
        args = dict(tag=6, bodies=b, wits=w, aux=[(1, bstr(r, 6))], invalid=[2])
        args.update(kw)
        add("shape_" + name, block(r, **args), "mut_" + name)

    mut("s1_not_array", raw={1: hd(5, 0)})
    mut("s2_not_array", raw={2: hd(0, 3)})
    mut("s3_not_map", raw={3: hd(4, 0)})
    mut("s4_not_array", raw={4: hd(5, 0)})
    b, w = simple(3, True)
    mut("s2_count", bodies=b, wits=w[:2])
    mut("s3_key_not_uint", raw={3: hd(5, 1) + hd(3, 1) + b"a" + hd(0, 0)})
    mut("s3_key_range", aux=[(3, bstr(r, 4))])
    mut("s4_entry_not_uint", raw={4: hd(4, 1) + hd(1, 0)})
    mut("s4_entry_range", invalid=[3])
    mut("body_not_map", bodies=[body(r), hd(4, 2) + hd(0, 1) + hd(4, 0), body(r)])
    mut("key1_not_array", bodies=[body(r), seq(5, [(hd(0, 1), hd(5, 0))], False), body(r)])
    mut("key5_neither", wits=[witness(r), witness(r), witness(r, hd(0, 9))])
    mut("key5_redeemer_arity", wits=[witness(r, hd(4, 1) + hd(4, 3) + hd(0, 0) + hd(0, 0) + exunits(5)),
                                     witness(r), witness(r)])
    mut("key5_steps_not_uint", wits=[witness(r), witness(r, hd(5, 1) + hd(0, 0) + hd(4, 2) + hd(0, 0) +
                                                         hd(4, 2) + hd(0, 1) + hd(1, 4)), witness(r)])
    # ---- seeded random blocks: every choice above drawn independently
    for k in range(100):
        tag = r.choice((2, 3, 4, 5, 6, 7, "bare3", "bare4"))
        four = tag == "bare4" or (isinstance(tag, int) and tag >= 5)
        n = r.choice((0, 1, 2, 3, 5, 8, 13))
        bs = [body(r, n_out=r.choice((0, 1, 2, 3, 30)), indef=r.random() < .3, out_indef=r.random() < .3,
                   nested=r.random() < .2, key1=r.random() < .9, wide_key=r.random() < .1,
                   body_len=r.choice((None, None, 1500 + r.randrange(400)))) for _ in range(n)]
        ws = [witness(r, redeemers(r, r.choice(("array", "map")), [r.getrandbits(r.choice((8, 33, 64)))
                                                                    for _ in range(r.randrange(4))],
                                   r.random() < .3, r.random() < .3) if four and r.random() < .6 else None,
                      indef=r.random() < .3) for _ in range(n)]
        keys = r.sample(range(n), r.randrange(n + 1))
        inv = r.sample(range(n), r.randrange(n + 1)) if four else ()
        ind = tuple(q for q in (1, 2, 3, 4) if r.random() < .3)
        add(f"random_{k}", block(r, tag, bs, ws, [(q, bstr(r, r.randrange(40))) for q in keys], inv, ind), "random")
    # ---- blocks that do not decode
    b, w = simple(2, True)
    whole = block(r, 6, b, w)
    add("truncated", whole[:-7], "truncated")
    add("wrong_tag", hd(4, 2) + hd(0, 9) + whole[2:], "decode")
    tp = block(r, 5, b, w)
    assert tp[4] == 0x8f
    add("header_arity", tp[:4] + hd(4, 10) + tp[5:], "decode")
    # ---- Byron
    add("byron_ebb", byron_ebb(r), "byron_ebb")
    for n, ind in ((0, False), (1, False), (2, True), (65, False), (64, True)):
        txs = [(byron_tx(r, 1 + k % 3, indef=ind, out_indef=ind and k % 2 == 0), byron_wits(r)) for k in range(n)]
        add(f"byron_main_{n}_{int(ind)}", byron_main(r, txs, ind), "byron_main", f"byron_count_{n}")
    add("byron_outs_24", byron_main(r, [(byron_tx(r, 24), byron_wits(r))]), "byron_main")
    add("byron_tx_not_array", byron_main(r, [(byron_tx(r), byron_wits(r)), (hd(5, 0), byron_wits(r))]),
        "mut_byron_tx")
    add("byron_outs_not_array", byron_main(r, [(hd(4, 3) + hd(4, 0) + hd(5, 0) + hd(5, 0), byron_wits(r))]),
        "mut_byron_outs")
    add("byron_truncated", byron_main(r, [(byron_tx(r), byron_wits(r))])[:-3], "byron_decode")
    return out


def layout(cases):
    """-> (arena bytes, offsets, lengths): the blocks back to back behind a few odd bytes"""
    off, pos, parts = [], 3, [b"\x00\x01\x02"]
    for c in cases:
        off.append(pos)
        parts.append(c.bytes)
        pos += len(c.bytes)
    return b"".join(parts), off, [len(c.bytes) for c in cases]
