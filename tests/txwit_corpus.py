"""Stored blocks whose transactions carry signed key witnesses, for the key-witness tests (test
infrastructure; built on tx_corpus's block builder).

Seeded and pure Python but for the signer (oracle.ed25519_sign).  A transaction's witnesses sign
its txId = Blake2b-256 of the body bytes, so the bodies are drawn first and the witness sets
built over them.  Everything the witness walk looks at is chosen per case: the number of VKey and
bootstrap witnesses, which of keys 0 and 2 the map holds and in which order, the definite or
indefinite form of the map, of the two arrays and of the items, tag 258, a wider head for key 0,
other keys around the two, one mutation that breaks the shape, and what is wrong with a signature.

corpus() -> list of Case(name, bytes, tags, want).  want: None for a block without rows (the
index does not give it any), else per transaction "skipped" (Byron), "shape", or the list of the
witnesses' intended validity in witness-row order (key-0 items, then key-2 items)."""
import hashlib
import random
from collections import namedtuple

import ec_model as em
import forged_cases as fc
import oracle
import tx_corpus as tc
from tx_corpus import bstr, hd, seq

Case = namedtuple("Case", "name bytes tags want")

WIT_COUNTS = (0, 1, 2, 63, 64, 65, 300)
DAMAGE = ("R", "S", "A", "S+L", "other_tx")
SHAPE_MUTATIONS = ("v0_not_array", "v2_not_array", "tag_not_258", "arity_1", "arity_3", "arity_3_indef", "boot_arity_3",
                   "boot_arity_5", "key_31", "key_33", "sig_63", "key_indef_bytes", "sig_text")
L = em.L


def tx_id(body):
    return hashlib.blake2b(body, digest_size=32).digest()


def flip(b, bit):
    v = bytearray(b)
    v[bit // 8] ^= 1 << (bit % 8)
    return bytes(v)


class Gen:
    def __init__(self, seed):
        self.r = random.Random(seed)
        self.seeds = [tc.rb(self.r, 32) for _ in range(12)]
        self.pks = [oracle.ed25519_pk(s) for s in self.seeds]

    def sign(self, body, damage=None):
        """-> (key, sig, meant valid): a witness over body's txId, damaged as asked"""
        r = self.r
        k = r.randrange(len(self.seeds))
        key, sig = self.pks[k], oracle.ed25519_sign(self.seeds[k], tx_id(body))
        if damage is None:
            return key, sig, True
        if damage == "R":
            sig = flip(sig, r.randrange(255))
        elif damage == "S":
            sig = sig[:32] + flip(sig[32:], r.randrange(250))
        elif damage == "A":
            key = flip(key, r.randrange(255))
        elif damage == "S+L":
            sig = sig[:32] + (int.from_bytes(sig[32:], "little") + L).to_bytes(32, "little")
        elif damage == "other_tx":       # a valid signature by the same key, of another transaction
            sig = oracle.ed25519_sign(self.seeds[k], tx_id(body + b"\x00"))
        else:
            raise ValueError(damage)
        return key, sig, False

    def item(self, kind, key, sig, indef=False):
        parts = [hd(2, 32) + key, hd(2, 64) + sig]
        if kind == 2:
            parts += [bstr(self.r, 32), self.r.choice((hd(5, 0), bstr(self.r, self.r.randrange(40)),
                                                      b"\xbf\x01\x9f\x02\xff\xff"))]
        return seq(4, parts, indef)

    def other(self, key, four):
        """the value of another key of the witness set (1 scripts, 3, 4 data, 5 redeemers)"""
        if key == 5:
            return tc.redeemers(self.r, "array", [7]) if four else hd(0, 9)
        return seq(4, [bstr(self.r, self.r.randrange(1, 30))], self.r.random() < .5)

    def tx(self, nv=1, nb=0, keys=None, four=False, map_indef=False, arr_indef=False, item_indef=False, tag0=False,
           tag2=False, wide0=False, extra=(), dup0=False, damage=(), not_map=False, mutate=None, body=None):
        """-> (body, witness set, want).  keys: which of 0 and 2 the map holds, in map order
        (default: those with witnesses, 0 first); extra: (position, key) with position "before",
        "between" or "after"; damage: {witness index in row order: kind}."""
        r = self.r
        body = tc.body(r) if body is None else body
        damage = dict(damage)
        if keys is None:
            keys = tuple(k for k, n in ((0, nv), (2, nb)) if n)
        if not_map:
            return body, seq(4, [self.item(0, *self.sign(body)[:2])], False), []
        wits = {0: [self.sign(body, damage.get(j)) for j in range(nv if 0 in keys else 0)],
                2: [self.sign(body, damage.get(nv + j)) for j in range(nb if 2 in keys else 0)]}
        want = [w[2] for w in wits[0]] + [w[2] for w in wits[2]]
        vals = {}
        for k in keys:
            v = seq(4, [self.item(k, key, sig, item_indef) for key, sig, _ in wits[k]], arr_indef)
            vals[k] = b"\xd9\x01\x02" + v if (tag0 if k == 0 else tag2) else v
        if mutate:
            vals, want = self.mutated(mutate, body, vals, keys), "shape"
        pairs = [(k, b"\x18\x00" if (k == 0 and wide0) else hd(0, k), vals[k]) for k in keys]

        def pair(k):     # another key: an unsigned integer, or (bytes) the encoded key itself
            return (k, self.other(1, four)) if isinstance(k, bytes) else (hd(0, k), self.other(k, four))
        out = [pair(k) for pos, k in extra if pos == "before"]
        for n, (k, kh, v) in enumerate(pairs):
            out.append((kh, v))
            if n == 0:
                out += [pair(k2) for pos, k2 in extra if pos == "between"]
        out += [pair(k) for pos, k in extra if pos == "after"]
        if dup0 and 0 in keys:        # a second key 0: not read (read, it would be a witness more, or a SHAPE)
            out.append((hd(0, 0), r.choice((hd(0, 7), seq(4, [self.item(0, *self.sign(body)[:2])], False)))))
        return body, seq(5, out, map_indef), want

    def mutated(self, name, body, vals, keys):
        r = self.r
        key, sig, _ = self.sign(body)
        good = self.item(0, key, sig)
        v = dict(vals)
        if name == "v0_not_array":
            v[0] = hd(0, 5)
        elif name == "v2_not_array":
            v[2] = seq(5, [(hd(0, 1), good)], False)
        elif name == "tag_not_258":
            v[0] = b"\xd9\x01\x03" + seq(4, [good], False)
        elif name == "arity_1":
            v[0] = seq(4, [good, seq(4, [hd(2, 32) + key], False)], False)
        elif name == "arity_3":
            v[0] = seq(4, [seq(4, [hd(2, 32) + key, hd(2, 64) + sig, hd(0, 1)], False)], False)
        elif name == "arity_3_indef":
            v[0] = seq(4, [seq(4, [hd(2, 32) + key, hd(2, 64) + sig, hd(0, 1)], True)], True)
        elif name == "boot_arity_3":
            v[2] = seq(4, [seq(4, [hd(2, 32) + key, hd(2, 64) + sig, bstr(r, 32)], False)], False)
        elif name == "boot_arity_5":
            v[2] = seq(4, [hd(4, 5) + self.item(2, key, sig)[1:] + hd(0, 0)], False)
        elif name == "key_31":
            v[0] = seq(4, [seq(4, [hd(2, 31) + key[:31], hd(2, 64) + sig], False)], False)
        elif name == "key_33":
            v[0] = seq(4, [good, seq(4, [hd(2, 33) + key + b"\x00", hd(2, 64) + sig], False)], False)
        elif name == "sig_63":
            v[0] = seq(4, [seq(4, [hd(2, 32) + key, hd(2, 63) + sig[:63]], False)], False)
        elif name == "key_indef_bytes":
            v[0] = seq(4, [seq(4, [b"\x5f" + hd(2, 32) + key + b"\xff", hd(2, 64) + sig], False)], False)
        elif name == "sig_text":
            v[0] = seq(4, [seq(4, [hd(2, 32) + key, hd(3, 64) + bytes(65 + b % 26 for b in sig)], False)], False)
        else:
            raise ValueError(name)
        return v


def forged(g, family):
    """(body, key, sig) of a forged witness whose group equation holds over the body's txId, so
    that only libsodium's encoding predicates reject it (forged_cases.py): a small-order key, or a
    small-order R under a mixed-order key.  The body is redrawn until the challenge fits."""
    r = g.r
    if family == "small_a":
        a_enc = next(e for e in fc.torsion_encodings() if em.order(fc.lenient_decode(e)) == 4)
        k = r.randrange(1, L)
        r_enc = em.encode(em.mul(k, em.B_AFF))
        while True:
            body = tc.body(r)
            if fc.hram(r_enc, a_enc, tx_id(body)) % 4 == 0:
                sig = r_enc + k.to_bytes(32, "little")
                break
    else:
        a = r.randrange(1, L)
        a_enc = em.encode(em.add(em.mul(a, em.B_AFF), em.affine_to_ext(fc.T8)))
        sig = None
        while sig is None:
            body = tc.body(r)
            for j, pt in enumerate(fc.TORSION):
                r_enc = em.encode_affine(pt)
                h = fc.hram(r_enc, a_enc, tx_id(body))
                if j == (-h) % 8:
                    sig = r_enc + (h * a % L).to_bytes(32, "little")
                    break
    assert fc.ed_equation_holds(a_enc, tx_id(body), sig), family
    return body, a_enc, sig


_CORPUS = {}


def corpus(seed=20250930):
    if seed in _CORPUS:
        return _CORPUS[seed]
    g = Gen(seed)
    r = g.r
    out = []

    def add(name, tag, txs, *tags, aux=(), invalid=(), indef=(), want=True):
        """txs: (body, witness set, want) triples"""
        data = tc.block(r, tag, [t[0] for t in txs], [t[1] for t in txs], aux, invalid, indef)
        out.append(Case(name, data, frozenset(tags), [t[2] for t in txs] if want else None))

    def is_four(tag):
        return tag == "bare4" or (isinstance(tag, int) and tag >= 5)

    # ---- witness counts at the wave edges, one transaction each beside a small neighbour
    for n in WIT_COUNTS:
        nv, nb = (40, 25) if n == 65 else (n, 0)
        add(f"count_{n}", 6, [g.tx(nv, nb, four=True, damage={n // 2: "R"} if n > 1 else {}), g.tx(1, four=True)],
            f"count_{n}")
    # one block whose transactions together cross several slices of 64 and of 100 witnesses
    add("cross_slices", 7, [g.tx(50 - k, k, four=True, damage={7 * k: "S"}) for k in range(5)], "cross_slices")
    # ---- which keys the map holds
    add("keys_presence", 3, [g.tx(2, 0), g.tx(0, 2), g.tx(2, 2), g.tx(2, 3, keys=(2, 0)), g.tx(0, 0, extra=[("after", 1)]),
                             g.tx(0, 0, keys=()), g.tx(0, 0, keys=(0, 2))],
        "key0_only", "key2_only", "both_02", "both_20", "neither", "empty_map", "empty_arrays")
    add("key0_twice", 4, [g.tx(2, 0, dup0=True), g.tx(1, 1, dup0=True), g.tx(1, 0, dup0=True, map_indef=True)],
        "key0_twice")
    add("not_a_map", 6, [g.tx(1, four=True), g.tx(not_map=True), (tc.body(r), hd(0, 3), [])], "wit_not_map")
    # ---- the forms
    for mi, ai, ii in ((False, False, False), (True, False, False), (False, True, False), (False, False, True),
                       (True, True, True)):
        add(f"forms_{int(mi)}{int(ai)}{int(ii)}", 5,
            [g.tx(2, 2, four=True, map_indef=mi, arr_indef=ai, item_indef=ii, damage={1: "A", 3: "R"}),
             g.tx(1, 0, four=True, map_indef=mi, arr_indef=ai, item_indef=ii)],
            *(["map_indef"] if mi else ["map_def"]), *(["arr_indef"] if ai else ["arr_def"]),
            *(["item_indef"] if ii else ["item_def"]))
    add("tag_258", 7, [g.tx(2, 0, four=True, tag0=True), g.tx(0, 2, four=True, tag2=True),
                       g.tx(1, 1, four=True, tag0=True, tag2=True, arr_indef=True), g.tx(1, 1, tag0=True, keys=(2, 0))],
        "tag0", "tag2")
    add("wide_key0", 6, [g.tx(2, 1, four=True, wide0=True), g.tx(1, 0, four=True, wide0=True, map_indef=True)], "wide_key0")
    add("other_keys", 6, [g.tx(1, 1, four=True, extra=[("before", 1), ("between", 3), ("after", 4), ("after", 5)]),
                          g.tx(1, 1, four=True, keys=(2, 0), extra=[("before", 5), ("between", 1), ("after", 3)]),
                          g.tx(2, 0, four=True, extra=[("before", 4), ("after", 5)], map_indef=True)],
        "other_before", "other_between", "other_after")
    add("other_keys_three_segments", 3, [g.tx(1, 1, extra=[("before", 1), ("between", 5), ("after", 4)])], "other_3seg")
    # ---- the SHAPE rules, one per case, each between intact neighbours
    for m in SHAPE_MUTATIONS:
        keys = (0, 2) if m.startswith(("v2", "boot")) else None
        add("shape_" + m, 6, [g.tx(1, 1, four=True), g.tx(1, 1 if keys else 0, keys=keys, four=True, mutate=m),
                              g.tx(2, 0, four=True)], "mut_" + m)
    # a SHAPE under key 2 after a well-formed key 0: no witness rows at all
    add("shape_after_good_key0", 4, [g.tx(2, 1, keys=(0, 2), mutate="boot_arity_3"), g.tx(1, 0)], "mut_after_good")
    # ---- what is wrong with a signature; one transaction listed invalid, still checked
    txs = [g.tx(1, 0, four=True)] + [g.tx(1, 0, four=True, damage={0: d}) for d in DAMAGE]
    txs += [g.tx(1, 1, four=True, damage={1: d}) for d in ("R", "S+L")] + [g.tx(2, 0, four=True, damage={1: "S"})]
    add("signatures", 7, txs, "valid", *("dmg_" + d for d in DAMAGE), "in_s4", invalid=[0, 8])
    # a valid witness moved to another transaction: both transactions' witnesses swapped
    b1, b2 = tc.body(r), tc.body(r)
    (_, w1, _), (_, w2, _) = g.tx(1, 0, body=b1), g.tx(1, 0, body=b2)
    add("swapped", 3, [(b1, w2, [False]), (b2, w1, [False]), g.tx(1, 0)], "swapped")
    # forged witnesses whose equation holds, each with its control
    for fam in ("small_a", "small_r"):
        body, key, sig = forged(g, fam)
        ws = seq(5, [(hd(0, 0), seq(4, [g.item(0, key, sig)], False))], False)
        add("forged_" + fam, 6, [(body, ws, [False]), g.tx(1, 0, four=True)], "forged_" + fam)
    # ---- eras and bare blocks
    for tag in (2, 3, 4, 5, 6, 7, "bare3", "bare4"):
        f = is_four(tag)
        add(f"era_{tag}", tag, [g.tx(1, 0, four=f), g.tx(1, 1, four=f, damage={0: "R"}), g.tx(0, 0, four=f, keys=())],
            f"tag_{tag}", invalid=[1] if f else ())
    # ---- blocks without rows: TXI SHAPE, DECODE
    txs = [g.tx(1, 0, four=True) for _ in range(3)]
    out.append(Case("txi_shape", tc.block(r, 6, [t[0] for t in txs], [t[1] for t in txs[:2]]), frozenset(["txi_shape"]),
                    None))
    whole = tc.block(r, 6, [t[0] for t in txs], [t[1] for t in txs])
    out.append(Case("txi_decode", whole[:-9], frozenset(["txi_decode"]), None))
    # ---- Byron
    out.append(Case("byron_ebb", tc.byron_ebb(r), frozenset(["byron", "byron_ebb"]), []))
    for n in (1, 3):
        txs = [(tc.byron_tx(r, 1 + k), tc.byron_wits(r)) for k in range(n)]
        out.append(Case(f"byron_main_{n}", tc.byron_main(r, txs), frozenset(["byron", "byron_main"]), ["skipped"] * n))
    # ---- seeded random blocks: every choice above drawn independently
    for k in range(50):
        tag = r.choice((2, 3, 4, 5, 6, 7, "bare3", "bare4"))
        f = is_four(tag)
        txs = []
        for _ in range(r.choice((0, 1, 2, 2, 3, 4))):
            nv, nb = r.choice((0, 1, 1, 2, 3, 5)), r.choice((0, 0, 1, 2))
            keys = [q for q, n in ((0, nv), (2, nb)) if n or r.random() < .2]
            r.shuffle(keys)
            extra = [(r.choice(("before", "between", "after")), q) for q in (1, 3, 4, 5) if r.random() < .25]
            dmg = {j: r.choice(DAMAGE) for j in range(nv + nb) if r.random() < .2}
            mut = r.choice(SHAPE_MUTATIONS) if r.random() < .06 else None
            if mut and mut.startswith(("v2", "boot")) and 2 not in keys:
                keys.append(2)
            if mut and not mut.startswith(("v2", "boot")) and 0 not in keys:
                keys.insert(0, 0)
            txs.append(g.tx(nv, nb, keys=tuple(keys), four=f, map_indef=r.random() < .3, arr_indef=r.random() < .3,
                            item_indef=r.random() < .3, tag0=r.random() < .2, tag2=r.random() < .2,
                            wide0=r.random() < .15, extra=extra, dup0=r.random() < .1, damage=dmg, mutate=mut))
        n = len(txs)
        add(f"random_{k}", tag, txs, "random", aux=[(q, bstr(r, 9)) for q in r.sample(range(n), r.randrange(n + 1))],
            invalid=r.sample(range(n), r.randrange(n + 1)) if f else (),
            indef=tuple(q for q in (1, 2, 3, 4) if r.random() < .3))
    # ---- keys of the map that are no unsigned integers: a text string, an indefinite byte string, an
    # array, a negative integer (-1 and -3: not keys 0 and 2)
    odd = [("before", b"\x61a"), ("before", b"\x5f\x41\x00\xff"), ("between", b"\x20"), ("between", b"\x82\x00\x02"),
           ("after", b"\x22")]
    add("odd_keys", 6, [g.tx(2, 1, four=True, extra=odd), g.tx(1, 2, four=True, keys=(2, 0), extra=odd, map_indef=True),
                        g.tx(0, 0, keys=(), extra=odd)], "odd_keys")
    _CORPUS[seed] = out
    return out


layout = tc.layout
