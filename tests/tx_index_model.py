"""The transaction index restated sequentially in plain Python (the independent checker of
k_txindex.hip; semantics: DESIGN section 29, include/praos_hip.h).

Shares no code with the library or the oracle: its own CBOR walk (recursive, where the device's
is a counter and a stack) and hashlib.  One block at a time, one transaction at a time.

A stored Shelley-based block is [tag 2..7, [header, s1, s2, s3 (, s4)]] or the bare inner array;
s1 = array of bodies, s2 = array of witness sets, s3 = map index -> auxiliary data, s4 = array of
the invalid transactions' indices.  A Byron item is a definite array whose first element is the
unsigned integer 0 (EBB) or 1 (main block); it is indexed only with byron=True and is DECODE
otherwise, never a bare Shelley-based block."""
import hashlib

OK, DECODE, SHAPE = 0, 1, 2
MAX_INDEF = 16          # nested indefinite-length items the block split accepts
M64 = (1 << 64) - 1
STATS = ("status", "n_tx", "txs_size", "n_out", "ex_steps", "tx_first")
ROWS = ("block", "body_off", "body_len", "wit_off", "wit_len", "aux_off", "aux_len", "size", "n_out", "ex_steps",
        "is_valid", "tx_id")


class Bad(Exception):
    """not well-formed CBOR (or not the envelope): the block does not decode"""


class Shape(Exception):
    """well-formed, but not the shape of a block of transactions"""


def head(buf, p, end):
    """-> (major type, additional info, argument or None when indefinite, next)"""
    if p >= end:
        raise Bad
    ib = buf[p]
    mt, ai = ib >> 5, ib & 31
    p += 1
    if ai < 24:
        return mt, ai, ai, p
    if ai <= 27:
        nb = 1 << (ai - 24)
        if nb > end - p:
            raise Bad
        return mt, ai, int.from_bytes(buf[p:p + nb], "big"), p + nb
    if ai == 31 and mt in (2, 3, 4, 5, 7):
        return mt, ai, None, p
    raise Bad


def skip(buf, p, end, depth=0):
    """-> the offset after the ONE well-formed item at p"""
    if p >= end or buf[p] == 0xFF:
        raise Bad
    mt, ai, arg, p = head(buf, p, end)
    if mt <= 1:
        return p
    if mt in (2, 3):
        if arg is not None:
            if arg > end - p:
                raise Bad
            return p + arg
        if depth == MAX_INDEF:
            raise Bad
        while True:
            if p >= end:
                raise Bad
            if buf[p] == 0xFF:
                return p + 1
            m2, _, a2, p = head(buf, p, end)
            if m2 != mt or a2 is None or a2 > end - p:
                raise Bad
            p += a2
    if mt in (4, 5):
        if arg is not None:
            for _ in range(arg * (2 if mt == 5 else 1)):
                p = skip(buf, p, end, depth)
            return p
        if depth == MAX_INDEF:
            raise Bad
        while True:
            if p >= end:
                raise Bad
            if buf[p] == 0xFF:
                return p + 1
            p = skip(buf, p, end, depth + 1)
    if mt == 6:
        return skip(buf, p, end, depth)
    if ai == 24 and arg < 32:
        raise Bad
    return p


def is_byron_item(buf, off, end):
    try:
        mt, _, n, p = head(buf, off, end)
        if mt != 4 or n is None or n < 1:
            return False
        mt, _, k, p = head(buf, p, end)
        return mt == 0 and k <= 1
    except Bad:
        return False


def split_shelley(buf, off, end):
    """-> the spans [(start, end)] of s1..s3|s4; raises Bad"""
    mt, _, n, p = head(buf, off, end)
    if mt != 4 or n is None:
        raise Bad
    arity = 0
    if n == 2:
        mt, _, tag, p = head(buf, p, end)
        if mt != 0 or not 2 <= tag <= 7:
            raise Bad
        mt, _, n, p = head(buf, p, end)
        if mt != 4 or n is None or n != (4 if tag <= 4 else 5):
            raise Bad
        arity = 15 if tag <= 5 else 10
    elif n not in (4, 5):
        raise Bad
    if arity:       # the header is [body, kesSig] and the body has the era's arity
        mt, _, a2, q = head(buf, p, end)
        if mt != 4 or a2 != 2:
            raise Bad
        mt, _, ab, q = head(buf, q, end)
        if mt != 4 or ab != arity:
            raise Bad
    spans = []
    for _ in range(n):
        s = p
        p = skip(buf, p, end)
        spans.append((s, p))
    if p != end:
        raise Bad
    return spans[1:]


def _uint(buf, p, end, limit=M64):
    mt, _, v, p = head(buf, p, end)
    if mt != 0 or v > limit:
        raise Bad
    return v, p


def _list(buf, p, end, n):
    mt, _, v, p = head(buf, p, end)
    if mt != 4 or v is None or v != n:
        raise Bad
    return p


def _bytes(buf, p, end, n):
    mt, _, v, p = head(buf, p, end)
    if mt != 2 or v is None or v != n or n > end - p:
        raise Bad
    return p + n


def split_byron(buf, off, end):
    """A Byron item -> None (EBB) or the txPayload span of a main block; raises Bad.  The
    envelope and header shapes are the ones the Byron block split accepts."""
    _, _, n, p = head(buf, off, end)
    _, _, kind, p = head(buf, p, end)
    if n != 2:
        raise Bad
    p = _list(buf, p, end, 3)
    ho, he = p, skip(buf, p, end)
    bo, be = he, skip(buf, he, end)
    if skip(buf, be, end) != end:
        raise Bad
    p = _list(buf, ho, he, 5)
    _, p = _uint(buf, p, he, 0xFFFFFFFF)
    p = _bytes(buf, p, he, 32)
    if kind == 0:
        p = _bytes(buf, p, he, 32)
        p = _list(buf, p, he, 2)
        _, p = _uint(buf, p, he)
        p = _list(buf, p, he, 1)
        _, p = _uint(buf, p, he)
        if skip(buf, p, he) != he:
            raise Bad
        return None
    p = _list(buf, p, he, 4)
    p = _list(buf, p, he, 3)
    _, p = _uint(buf, p, he)
    p = _bytes(buf, p, he, 32)
    p = _bytes(buf, p, he, 32)
    p = skip(buf, p, he)
    p = _bytes(buf, p, he, 32)
    p = _bytes(buf, p, he, 32)
    p = _list(buf, p, he, 4)
    p = _list(buf, p, he, 2)
    _, p = _uint(buf, p, he)
    _, p = _uint(buf, p, he, 0xFFFF)
    p = _bytes(buf, p, he, 64)
    p = _list(buf, p, he, 1)
    _, p = _uint(buf, p, he)
    p = _list(buf, p, he, 2)
    t, p = _uint(buf, p, he)
    if t != 2:
        raise Bad
    p = _list(buf, p, he, 2)
    p = _list(buf, p, he, 4)
    _, p = _uint(buf, p, he)
    for _ in range(4):
        p = _bytes(buf, p, he, 64)
    if skip(buf, p, he) != he:
        raise Bad
    # body = [txPayload, ssc, dlg, upd]; txPayload = a list of [tx, witnesses]
    p = _list(buf, bo, be, 4)
    ts = p
    mt, _, cnt, p = head(buf, p, be)
    if mt != 4:
        raise Bad
    k = 0
    while (cnt is None and p < be and buf[p] != 0xFF) or (cnt is not None and k < cnt):
        p = _list(buf, p, be, 2)
        p = skip(buf, skip(buf, p, be), be)
        k += 1
    if cnt is None:
        if p >= be:
            raise Bad
        p += 1
    te = p
    for _ in range(3):
        p = skip(buf, p, be)
    if p != be:
        raise Bad
    return ts, te


# ---- the walks over well-formed items: anything unexpected is a Shape

def _items(buf, s, e, want):
    """The top-level item spans of the array (want 4) or map (want 5: keys and values in turn)
    at [s, e)."""
    try:
        mt, _, n, p = head(buf, s, e)
    except Bad:
        raise Shape
    if mt != want:
        raise Shape
    out = []
    try:
        if n is None:
            while True:
                if p >= e:
                    raise Shape
                if buf[p] == 0xFF:
                    break
                q = skip(buf, p, e)
                out.append((p, q))
                p = q
        else:
            for _ in range(n * (2 if want == 5 else 1)):
                q = skip(buf, p, e)
                out.append((p, q))
                p = q
    except Bad:
        raise Shape
    return out


def _count(buf, s, e):
    """items of the array at [s, e); a definite head is taken at its word"""
    try:
        mt, _, n, _ = head(buf, s, e)
    except Bad:
        raise Shape
    if mt != 4:
        raise Shape
    return n if n is not None else len(_items(buf, s, e, 4))


def _as_uint(buf, s, e):
    try:
        mt, _, v, p = head(buf, s, e)
    except Bad:
        raise Shape
    if mt != 0 or p != e:
        raise Shape
    return v


def _pairs(buf, s, e):
    """(key span, value span) of the map at [s, e), in order; an odd item at the end of an
    indefinite map is a Shape when the walk reaches it"""
    it = _items(buf, s, e, 5)
    for k in range(0, len(it), 2):
        if k + 1 >= len(it):
            raise Shape
        yield it[k], it[k + 1]


def _first_key(buf, s, e, want):
    """the value span under the first unsigned key `want` of the map at [s, e), or None.
    The walk stops at the key, as the device's does: what follows it is not looked at."""
    try:
        mt, _, n, p = head(buf, s, e)
        if mt != 5:
            raise Shape
        k = 0
        while True:
            if n is None:
                if p >= e:
                    raise Shape
                if buf[p] == 0xFF:
                    return None
            elif k == n:
                return None
            ke = skip(buf, p, e)
            kmt, _, kv, kq = head(buf, p, e)
            if kmt == 0 and kv == want:
                return ke, skip(buf, ke, e)
            p = skip(buf, ke, e)
            k += 1
    except Bad:
        raise Shape


def _exunits(buf, s, e):
    it = _items(buf, s, e, 4)
    if len(it) != 2:
        raise Shape
    _as_uint(buf, *it[0])
    return _as_uint(buf, *it[1])


def _redeemer_steps(buf, s, e):
    try:
        mt = head(buf, s, e)[0]
    except Bad:
        raise Shape
    total = 0
    if mt == 4:
        for rs, re_ in _items(buf, s, e, 4):
            it = _items(buf, rs, re_, 4)
            if len(it) != 4:
                raise Shape
            total += _exunits(buf, *it[3])
    elif mt == 5:
        for _, (vs, ve) in _pairs(buf, s, e):
            it = _items(buf, vs, ve, 4)
            if len(it) != 2:
                raise Shape
            total += _exunits(buf, *it[1])
    else:
        raise Shape
    return total & M64


def _tx_id(buf, s, e):
    return hashlib.blake2b(bytes(buf[s:e]), digest_size=32).digest()


def shelley_rows(buf, segs):
    """-> the rows of one Shelley-based block; raises Shape"""
    bodies = _items(buf, *segs[0], 4)
    n = _count(buf, *segs[0])
    if _count(buf, *segs[1]) != n:
        raise Shape
    wits = _items(buf, *segs[1], 4)
    aux = {}
    for (ks, ke), v in _pairs(buf, *segs[2]):
        k = _as_uint(buf, ks, ke)
        if k >= n:
            raise Shape
        aux[k] = v              # a repeated key: the later entry stands
    invalid = set()
    if len(segs) == 4:
        for s, e in _items(buf, *segs[3], 4):
            k = _as_uint(buf, s, e)
            if k >= n:
                raise Shape
            invalid.add(k)
    rows = []
    for t in range(n):
        (bs, be), (ws, we) = bodies[t], wits[t]
        v = _first_key(buf, bs, be, 1)
        n_out = _count(buf, *v) if v else 0
        steps = 0
        if len(segs) == 4:
            try:
                is_map = head(buf, ws, we)[0] == 5
            except Bad:
                raise Shape
            v = _first_key(buf, ws, we, 5) if is_map else None
            steps = _redeemer_steps(buf, *v) if v else 0
        a = aux.get(t)
        alen = a[1] - a[0] if a else 0
        rows.append({"body_off": bs, "body_len": be - bs, "wit_off": ws, "wit_len": we - ws,
                     "aux_off": a[0] if a else 0, "aux_len": alen,
                     "size": 1 + (be - bs) + (we - ws) + (alen if a else 1), "n_out": n_out, "ex_steps": steps,
                     "is_valid": 0 if t in invalid else 1, "tx_id": _tx_id(buf, bs, be)})
    return rows


def byron_rows(buf, ts, te):
    rows = []
    for s, e in _items(buf, ts, te, 4):
        pair = _items(buf, s, e, 4)
        (bs, be), (ws, we) = pair
        tx = _items(buf, bs, be, 4)
        if len(tx) < 2:
            raise Shape
        rows.append({"body_off": bs, "body_len": be - bs, "wit_off": ws, "wit_len": we - ws, "aux_off": 0,
                     "aux_len": 0, "size": e - s, "n_out": _count(buf, *tx[1]), "ex_steps": 0, "is_valid": 1,
                     "tx_id": _tx_id(buf, bs, be)})
    return rows


def index_block(buf, off, length, byron=False):
    """-> (status, rows) of one stored block"""
    end = off + length
    if off > len(buf) or length > len(buf) - off:
        return DECODE, []
    try:
        if is_byron_item(buf, off, end):
            if not byron:
                return DECODE, []
            span = split_byron(buf, off, end)
            return OK, ([] if span is None else byron_rows(buf, *span))
        return OK, shelley_rows(buf, split_shelley(buf, off, end))
    except Bad:
        return DECODE, []
    except Shape:
        return SHAPE, []


def index_blocks(buf, off, length, byron=False):
    """-> (stats, rows): dicts of lists named as the library's arrays (STATS, ROWS)"""
    st = {k: [] for k in STATS}
    rw = {k: [] for k in ROWS}
    total = 0
    for i, (o, ln) in enumerate(zip(off, length)):
        status, rows = index_block(buf, int(o), int(ln), byron)
        st["status"].append(status)
        st["n_tx"].append(len(rows))
        st["txs_size"].append(sum(r["size"] for r in rows))
        st["n_out"].append(sum(r["n_out"] for r in rows))
        st["ex_steps"].append(sum(r["ex_steps"] for r in rows) & M64)
        st["tx_first"].append(total)
        total += len(rows)
        for r in rows:
            rw["block"].append(i)
            for k in ROWS[1:]:
                rw[k].append(r[k])
    st["tx_first"].append(total)
    return st, rw
