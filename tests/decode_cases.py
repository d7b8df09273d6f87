"""Stored-header cases for the decoder (k_decode.hip) at every head, width and length
(test infrastructure, pure Python).

A header is laid out as a list of items [name, major type, argument, payload]; `enc`
writes it with any of the five head widths per item (its own head encoder `head_w`, not
the oracle's), so a case is stated as "this header, but ...".  Both eras: the 10-field
Praos HeaderBody (21 heads) and the 15-field TPraos BHBody (22 heads).

Every generator returns (arena, off, len, names).  A name ends in "=>" and what the case
claims: a status in hex ("=>0x20"), or "?" where only the oracle says (first bytes, era
selection).  tests/test_decode_cases.py holds the claims against oracle/cbor_header.py;
tests/test_gpu_decode_cases.py holds the kernel against the same oracle.

Headers follow each other in the arena with no gap (the offsets take every residue mod 8
anyway), so a decoder that reads beyond its `end` reads the next header's bytes."""
import cbor_header as ch
from helpers import rbytes, rng

FORMS = (0, 24, 25, 26, 27)         # additional info of the five head widths; 0 = in the first byte
NBYTES = {24: 1, 25: 2, 26: 4, 27: 8}
INT_FIELDS = ("block_no", "slot", "body_size", "n", "c0", "prot_major", "prot_minor")
EDGE_VALUES = (0, 23, 24, 255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32, (1 << 64) - 1)
OUTSIDE_BODY = ("outer", "kes_sig")  # heads outside the signed body: their width is not the body's
U64 = (1 << 64) - 1


def shortest(value):
    for ai, lim in ((0, 24), (24, 1 << 8), (25, 1 << 16), (26, 1 << 32), (27, 1 << 64)):
        if value < lim:
            return ai
    raise ValueError(value)


def forms_for(value):
    """The widths that can hold `value`, shortest first."""
    return FORMS[FORMS.index(shortest(value)):]


def head_w(mt, value, ai=None):
    """CBOR head of major type mt with argument `value` in the width `ai` (None: shortest)."""
    ai = shortest(value) if ai is None else ai
    if ai == 0:
        assert value < 24
        return bytes([(mt << 5) | value])
    return bytes([(mt << 5) | ai]) + value.to_bytes(NBYTES[ai], "big")


def base_fields(multi, tp, seed=26):
    """multi False: every integer below 24 (one-byte heads); True: multi-byte integers."""
    r = rng(seed + 2 * multi + tp)
    ints = (dict(block_no=1 << 20, slot=1 << 30, body_size=70000, n=300, c0=25, prot_major=7, prot_minor=2)
            if multi else dict(block_no=1, slot=2, body_size=3, n=4, c0=5, prot_major=6, prot_minor=7))
    f = {"prev_hash": rbytes(r, 32), "cold_vk": rbytes(r, 32), "vrf_vk": rbytes(r, 32), "vrf_out": rbytes(r, 64),
         "vrf_proof": rbytes(r, 80), "body_hash": rbytes(r, 32), "hot_vk": rbytes(r, 32), "ocert_sig": rbytes(r, 64),
         "kes_sig": rbytes(r, 448)}
    if tp:
        f["leader_out"], f["leader_proof"] = rbytes(r, 64), rbytes(r, 80)
    f.update(ints)
    return f


def items(f, tp):
    """The header of fields f as [name, mt, argument, payload] items; a null prev_hash is the
    raw item [name, None, None, b'\\xf6']."""
    def u(k):
        return [k, 0, f[k], b""]

    def b(k):
        return [k, 2, len(f[k]), f[k]]

    def a(k, n):
        return [k, 4, n, b""]
    prev = ["prev_hash", None, None, b"\xf6"] if f["prev_hash"] is None else b("prev_hash")
    it = [a("outer", 2), a("body", 15 if tp else 10), u("block_no"), u("slot"), prev, b("cold_vk"), b("vrf_vk"),
          a("vrf", 2), b("vrf_out"), b("vrf_proof")]
    if tp:
        it += [a("leader", 2), b("leader_out"), b("leader_proof")]
    it += [u("body_size"), b("body_hash")]
    if not tp:
        it.append(a("ocert", 4))
    it += [b("hot_vk"), u("n"), u("c0"), b("ocert_sig")]
    if not tp:
        it.append(a("pv", 2))
    return it + [u("prot_major"), u("prot_minor"), b("kes_sig")]


def enc(its, widths=None):
    """-> (bytes, {name: offset of its head}).  widths: {name: ai}, or one ai for every head
    that can hold it ('widest': 27 everywhere)."""
    out, at = bytearray(), {}
    for name, mt, val, payload in its:
        at[name] = len(out)
        if mt is not None:
            ai = widths.get(name) if isinstance(widths, dict) else widths
            out += head_w(mt, val, ai)
        out += payload
    return bytes(out), at


def header(f, tp, widths=None):
    return enc(items(f, tp), widths)[0]


def pack(cases):
    """[(bytes, name)] -> (arena, off, len, names), the headers back to back."""
    off, ln, pos = [], [], 0
    for h, _ in cases:
        off.append(pos)
        ln.append(len(h))
        pos += len(h)
    return b"".join(h for h, _ in cases), off, ln, [n for _, n in cases]


def claim(name):
    """The status a case's name claims, or None."""
    s = name.rsplit("=>", 1)[1]
    return None if s == "?" else int(s, 16)


# ---- (a) first bytes ----
def first_bytes(multi, tp):
    """Each head's first byte replaced by each of the 256 values, and a tag-2 byte in front of
    each head."""
    f = base_fields(multi, tp)
    h, at = enc(items(f, tp))
    cases = []
    for name, p in at.items():
        for v in range(256):
            g = bytearray(h)
            g[p] = v
            cases.append((bytes(g), f"a/{name}/{v:02x}=>" + ("0x0" if v == h[p] else "?")))
    for name, p in at.items():
        cases.append((h[:p] + b"\xc2" + h[p:], f"a/{name}/tag=>{ch.DEC_UNSUPPORTED:#x}"))
    return pack(cases)


# ---- (b) widths ----
def _width_claim(name, ai, value):
    wide = ai != shortest(value)
    return ch.DEC_NONCANONICAL if wide and name not in OUTSIDE_BODY else 0


def widths(multi, tp):
    """Each head in each of the widths that hold its argument; all heads at their widest."""
    f = base_fields(multi, tp)
    its = items(f, tp)
    cases = []
    for name, mt, val, _ in its:
        for ai in forms_for(val):
            cases.append((enc(its, {name: ai})[0], f"b/{name}/ai{ai}=>{_width_claim(name, ai, val):#x}"))
    cases.append((enc(its, 27)[0], f"b/all/ai27=>{ch.DEC_NONCANONICAL:#x}"))
    return pack(cases)


def body_width_cases(tp):
    """(head name, ai) of every wider form of every head inside the body (multi-byte base)."""
    return [(name, ai) for name, _, val, _ in items(base_fields(True, tp), tp) if name not in OUTSIDE_BODY
            for ai in forms_for(val)[1:]]


# ---- (c) values ----
def max_fields(tp):
    """Every integer at its maximum at once: the longest canonical body."""
    f = base_fields(True, tp)
    f.update(block_no=U64, slot=U64, body_size=(1 << 32) - 1, n=U64, c0=U64, prot_major=ch.MAX_PROT_MAJOR,
             prot_minor=U64)
    return f


def values(tp):
    f = base_fields(True, tp)
    its = items(f, tp)
    cases = []
    for k in INT_FIELDS:
        for v in EDGE_VALUES:
            over = (k == "body_size" and v > (1 << 32) - 1) or (k == "prot_major" and v > ch.MAX_PROT_MAJOR)
            g = items(dict(f, **{k: v}), tp)
            for ai in forms_for(v):
                st = ch.DEC_OVERFLOW if over else ch.DEC_NONCANONICAL if ai != shortest(v) else 0
                cases.append((enc(g, {k: ai})[0], f"c/{k}/{v:#x}/ai{ai}=>{st:#x}"))
    for j, (name, mt, val, payload) in enumerate(its):
        for d in (-1, 1):
            g = [list(x) for x in its]
            if mt == 4:
                g[j][2] = val + d
                st = ch.DEC_SYNTAX
            elif mt == 2:
                g[j][2], g[j][3] = val + d, (payload + b"\x5a")[:val + d]
                st = ch.DEC_SIZE
            else:
                continue
            cases.append((enc(g)[0], f"c/{name}/len{d:+d}=>{st:#x}"))
    cases.append((header(max_fields(tp), tp), "c/max_ints=>0x0"))
    cases.append((header(f, tp), "c/prev_32=>0x0"))
    null = items(dict(f, prev_hash=None), tp)
    cases.append((enc(null)[0], "c/prev_null=>0x0"))
    for b in (0xF7, 0xF5):
        g = [list(x) for x in null]
        g[4][3] = bytes([b])
        cases.append((enc(g)[0], f"c/prev_{b:02x}=>{ch.DEC_SYNTAX:#x}"))
    return pack(cases)


# ---- (d) lengths ----
def lengths(tp):
    """A header (canonical, then with every head at its widest) with a copy of itself directly
    behind it, at each of the 8 alignments: the spans (off, k) for k = 0 .. length + 8; then
    the cuts inside heads with a wrong argument; then the spans around the arena's end.  The
    arena's last header ends on its last byte."""
    f = base_fields(True, tp)
    arena, off, ln, names = bytearray(), [], [], []
    for wide in (False, True):
        h = header(f, tp, 27 if wide else None)
        ok = ch.DEC_NONCANONICAL if wide else 0
        for al in range(8):
            arena += bytes((al - len(arena)) % 8)
            at = len(arena)
            assert at % 8 == al
            arena += h + h
            for k in range(len(h) + 9):
                st = ch.DEC_SYNTAX if k < len(h) else ok if k == len(h) else ch.DEC_TRAILING
                off.append(at)
                ln.append(k)
                names.append(f"d/{'wide' if wide else 'canon'}/al{al}/k{k}=>{st:#x}")
    h = header(f, tp)
    # cuts inside the argument of a head that, read to its end, gives another verdict: an
    # integer over its limit (OVERFLOW), a string one byte too long (SIZE), a tag
    # (UNSUPPORTED).  The argument's bytes lie behind `end`, so a decoder that reads a head
    # without looking at `end` reports that verdict where the span is only cut short (SYNTAX).
    its = items(f, tp)
    wrong = []
    for k, v in (("body_size", 1 << 32), ("prot_major", ch.MAX_PROT_MAJOR + 1)):
        g = items(dict(f, **{k: v}), tp)
        wrong += [(enc(g, {k: ai}), k, ai, ch.DEC_OVERFLOW) for ai in forms_for(v) if ai]
    for j, (name, mt, val, payload) in enumerate(its):
        if mt == 2:
            g = [list(x) for x in its]
            g[j][2], g[j][3] = val + 1, payload + b"\x5a"
            wrong += [(enc(g, {name: ai}), name, ai, ch.DEC_SIZE) for ai in forms_for(val + 1) if ai]
    for name in ("slot", "kes_sig"):
        p = enc(its)[1][name]
        for ai in FORMS[1:]:
            wrong.append(((h[:p] + head_w(6, 2, ai) + h[p:], {name: p}), name, f"tag{ai}", ch.DEC_UNSUPPORTED))
    for (hb, at_), name, ai, st in wrong:
        at, p = len(arena), at_[name]
        arena += hb + h
        nb = NBYTES[ai if isinstance(ai, int) else int(ai[3:])]
        for k in list(range(p + 1, p + 1 + nb)) + [len(hb)]:
            off.append(at)
            ln.append(k)
            names.append(f"d/cut/{name}/ai{ai}/k{k}=>{ch.DEC_SYNTAX if k < len(hb) else st:#x}")
    arena += h
    last, end = len(arena) - len(h), len(arena)
    for o, n, what, st in ((last, len(h), "last_exact", 0), (last, len(h) + 1, "last_plus1", ch.DEC_RANGE),
                           (end, 0, "empty_at_end", ch.DEC_SYNTAX), (end, 1, "one_at_end", ch.DEC_RANGE),
                           (end + 1, 0, "off_beyond", ch.DEC_RANGE), (end + 1, len(h), "off_beyond_len", ch.DEC_RANGE),
                           (1 << 63, len(h), "off_2^63", ch.DEC_RANGE), (U64, 0xFFFFFFFF, "off_len_max", ch.DEC_RANGE),
                           (0, 0xFFFFFFFF, "len_max", ch.DEC_RANGE)):
        off.append(o)
        ln.append(n)
        names.append(f"d/end/{what}=>{st:#x}")
    return bytes(arena), off, ln, names


# ---- (e) era selection ----
ARITIES = (9, 10, 11, 14, 15, 16)


def eras():
    """Body arities 9, 10, 11, 14, 15, 16, each over a 10-field and over a 15-field layout.
    What a case decodes to depends on the mode, so the names claim nothing."""
    cases = []
    for tp in (False, True):
        its = items(base_fields(True, tp), tp)
        for n in ARITIES:
            g = [list(x) for x in its]
            g[1][2] = n
            cases.append((enc(g)[0], f"e/{'15' if tp else '10'}fields/arity{n}=>?"))
    return pack(cases)


# ---- genuine KES signatures over the canonical body (for the verify paths) ----
def signed_fields(tp, spkp, seed=2600):
    """Multi-byte base whose KES signature is genuine: hot_vk = kes_vk(seed), signed over the
    canonical body at t = kp - c0.  -> fields (with 'kes_sig')."""
    import oracle as orc
    r = rng(seed + tp)
    f = base_fields(True, tp)
    kseed = rbytes(r, 32)
    kp = f["slot"] // spkp
    f.update(hot_vk=orc.kes_vk(kseed), c0=kp - 3)
    body = ch.encode_tpraos_body(f) if tp else ch.encode_body(f)
    f["kes_sig"] = orc.kes_sign(kseed, 3, body)
    return f


def genuine_wide(tp, spkp):
    """The signed header canonical, then with each wider form of each body head, then with all
    heads at their widest.  -> (arena, off, len, names)."""
    f = signed_fields(tp, spkp)
    its = items(f, tp)
    cases = [(enc(its)[0], "g/canonical=>0x0")]
    for name, _, val, _ in its:
        if name not in OUTSIDE_BODY:
            for ai in forms_for(val)[1:]:
                cases.append((enc(its, {name: ai})[0], f"g/{name}/ai{ai}=>{ch.DEC_NONCANONICAL:#x}"))
    cases.append((enc(its, 27)[0], f"g/all/ai27=>{ch.DEC_NONCANONICAL:#x}"))
    return pack(cases)
