"""praos_verify_gen_txs restated sequentially in plain Python (the independent checker of
k_gentx.hip; semantics: DESIGN section 32, include/praos_hip.h).

Its own walk of the wire wrapper and of the inner array, tx_index_model's item walk for what is
inside, tx_witness_model's witness walk with oracle.ed25519_verify for the signatures, hashlib
for the hashes.  One item at a time; the distinct transactions are found by comparing the era
index and the inner bytes themselves (the library compares their Blake2b-256)."""
import hashlib

import oracle
import tx_index_model as tm
import tx_witness_model as wm

OK, RANGE, SYNTAX, ERA, TRAILING, SHAPE, BYRON = 0, 1, 2, 3, 4, 5, 6
NO_ROW = 0xFFFFFFFF
PER_TX_OVERHEAD = 4
M64 = (1 << 64) - 1
ITEMS = ("status", "era", "row", "byron_kind", "payload_off", "payload_len")
TXS = ("item", "era", "body_off", "body_len", "wit_off", "wit_len", "aux_off", "aux_len", "size", "in_block_size",
       "ex_mem", "ex_steps", "is_valid", "tx_id", "wstatus", "n_vkey", "n_boot", "n_bad", "wit_first")
WITS = wm.WITS


class Syntax(Exception):
    pass


def _whead(buf, p, e, want):
    """one definite head of major type `want`, any width -> (argument, next)"""
    if p >= e:
        raise Syntax
    ib = int(buf[p])
    p += 1
    if ib >> 5 != want:
        raise Syntax
    ai = ib & 31
    if ai < 24:
        return ai, p
    if ai > 27:
        raise Syntax
    nb = 1 << (ai - 24)
    if nb > e - p:
        raise Syntax
    return int.from_bytes(buf[p:p + nb], "big"), p + nb


def unwrap(buf, off, length, n_eras=7):
    """-> (status, era, byron kind, inner / payload offset, length)"""
    era = 0xFF
    if off > len(buf) or length > len(buf) - off:
        return RANGE, era, 0xFF, 0, 0
    e = off + length
    try:
        v, p = _whead(buf, off, e, 4)
        if v != 2:
            raise Syntax
        v, p = _whead(buf, p, e, 0)
        if v > 0xFF:
            raise Syntax
        era = v
        if era >= n_eras:
            return ERA, era, 0xFF, 0, 0
        if era == 0:
            v, p = _whead(buf, p, e, 4)
            if v != 2:
                raise Syntax
            kind, p = _whead(buf, p, e, 0)
            if kind > 3 or p >= e:
                raise Syntax
            return BYRON, era, kind, p, e - p
        v, p = _whead(buf, p, e, 6)
        if v != 24:
            raise Syntax
        v, p = _whead(buf, p, e, 2)
        if v > e - p:
            raise Syntax
        return (OK if p + v == e else TRAILING), era, 0xFF, p, v
    except Syntax:
        return SYNTAX, era, 0xFF, 0, 0


def _exunits(buf, s, e):
    it = tm._items(buf, s, e, 4)
    if len(it) != 2:
        raise tm.Shape
    return tm._as_uint(buf, *it[0]), tm._as_uint(buf, *it[1])


def redeemer_units(buf, s, e):
    """-> (mem, steps) summed mod 2^64 over both redeemer forms"""
    try:
        mt = tm.head(buf, s, e)[0]
    except tm.Bad:
        raise tm.Shape
    mem = steps = 0
    if mt == 4:
        for rs, re_ in tm._items(buf, s, e, 4):
            it = tm._items(buf, rs, re_, 4)
            if len(it) != 4:
                raise tm.Shape
            m, st = _exunits(buf, *it[3])
            mem, steps = mem + m, steps + st
    elif mt == 5:
        for _, (vs, ve) in tm._pairs(buf, s, e):
            it = tm._items(buf, vs, ve, 4)
            if len(it) != 2:
                raise tm.Shape
            m, st = _exunits(buf, *it[1])
            mem, steps = mem + m, steps + st
    else:
        raise tm.Shape
    return mem & M64, steps & M64


def split(buf, era, s, e):
    """the transaction in the inner bytes [s, e) -> dict of the row's fields; raises tm.Shape"""
    want = 3 if era <= 3 else 4
    try:
        mt, _, n, p = tm.head(buf, s, e)
        if mt != 4 or (n is not None and n != want):
            raise tm.Shape
        b0 = p
        w0 = tm.skip(buf, b0, e)
        p = w1 = tm.skip(buf, w0, e)
        valid = 1
        if want == 4:
            if p >= e or buf[p] not in (0xF4, 0xF5):
                raise tm.Shape
            valid = 1 if int(buf[p]) == 0xF5 else 0
            p += 1
        x0 = p
        x1 = p = tm.skip(buf, x0, e)
        if n is None:
            if p >= e or buf[p] != 0xFF:
                raise tm.Shape
            p += 1
        if p != e:
            raise tm.Shape
        if buf[b0] >> 5 != 5:
            raise tm.Shape
        mem = steps = 0
        if era >= 4 and tm.head(buf, w0, w1)[0] == 5:
            v = tm._first_key(buf, w0, w1, 5)
            if v:
                mem, steps = redeemer_units(buf, *v)
    except tm.Bad:
        raise tm.Shape
    null = x1 - x0 == 1 and buf[x0] == 0xF6
    size = 1 + (w0 - b0) + (w1 - w0) + (x1 - x0)
    return {"body_off": b0, "body_len": w0 - b0, "wit_off": w0, "wit_len": w1 - w0, "aux_off": 0 if null else x0,
            "aux_len": 0 if null else x1 - x0, "size": size, "in_block_size": size + PER_TX_OVERHEAD, "ex_mem": mem,
            "ex_steps": steps, "is_valid": valid, "tx_id": hashlib.blake2b(bytes(buf[b0:w0]), digest_size=32).digest()}


def verify(buf, off, length, n_eras=7, dedup=True):
    """-> (items, txs, wits): dicts of lists named as the library's arrays"""
    buf = bytes(buf)
    I = {k: [] for k in ITEMS}
    T = {k: [] for k in TXS}
    W = {k: [] for k in WITS}
    rows = {}
    for i, (o, ln) in enumerate(zip(off, length)):
        st, era, kind, p, n = unwrap(buf, int(o), int(ln), n_eras)
        row = NO_ROW
        if st == OK:
            key = (era, bytes(buf[p:p + n])) if dedup else i
            if key in rows:
                row = rows[key]
            else:
                try:
                    r = split(buf, era, p, p + n)
                except tm.Shape:
                    r = None
                rows[key] = row = NO_ROW if r is None else len(T["item"])
                if r is not None:
                    _add_row(buf, T, W, i, era, r)
            if row == NO_ROW:
                st = SHAPE
        I["status"].append(st)
        I["era"].append(era)
        I["row"].append(row)
        I["byron_kind"].append(kind)
        I["payload_off"].append(p if st == BYRON else 0)
        I["payload_len"].append(n if st == BYRON else 0)
    T["wit_first"].append(len(W["tx"]))
    return I, T, W


def _add_row(buf, T, W, i, era, r):
    row = len(T["item"])
    ws = r["wit_off"]
    wstatus, vk, bt = wm.OK, [], []
    try:
        vk, bt = wm.witness_set(buf, ws, ws + r["wit_len"])
    except wm.Shape:
        wstatus = wm.SHAPE
    bad = 0
    T["wit_first"].append(len(W["tx"]))
    for kind, items in ((0, vk), (2, bt)):
        for key_at, sig_at in items:
            key, sig = bytes(buf[key_at:key_at + 32]), bytes(buf[sig_at:sig_at + 64])
            ok = 1 if oracle.ed25519_verify(key, r["tx_id"], sig) else 0
            bad += 1 - ok
            W["tx"].append(row)
            W["kind"].append(kind)
            W["key_off"].append(key_at)
            W["sig_off"].append(sig_at)
            W["ok"].append(ok)
            W["key_hash"].append(hashlib.blake2b(key, digest_size=28).digest() if kind == 0 else bytes(28))
    T["item"].append(i)
    T["era"].append(era)
    for k in ("body_off", "body_len", "wit_off", "wit_len", "aux_off", "aux_len", "size", "in_block_size", "ex_mem",
              "ex_steps", "is_valid", "tx_id"):
        T[k].append(r[k])
    T["wstatus"].append(wstatus)
    T["n_vkey"].append(len(vk))
    T["n_boot"].append(len(bt))
    T["n_bad"].append(bad)
