"""The key-witness check restated sequentially in plain Python (the independent checker of
k_txwit.hip; semantics: DESIGN section 30, include/praos_hip.h).

On top of tx_index_model for the rows (witness-set span, tx_id), with its own walk of the witness
set, oracle.ed25519_verify for the signature and hashlib for the key hash.  One transaction at a
time, one witness at a time.

The witness set is a map (definite or indefinite, keys in any head width).  The value under the
first key 0 is the VKey witnesses, items [vkey, sig]; the value under the first key 2 the
bootstrap witnesses, items [vkey, sig, chain_code, attributes]; either may sit in tag 258.  The
walk ends when both keys have been seen or the map ends."""
import hashlib

import oracle
import tx_index_model as tm

OK, SHAPE, SKIPPED = 0, 1, 2
BLOCKS = ("status", "n_tx", "n_wit", "n_bad", "n_shape", "tx_first")
TXS = ("block", "status", "n_vkey", "n_boot", "n_bad", "tx_id", "wit_first")
WITS = ("tx", "kind", "key_off", "sig_off", "ok", "key_hash")


class Shape(Exception):
    """a witness set outside the shapes: the transaction has no witness rows"""


def _bytes_at(buf, p, e, n):
    """a definite byte string of exactly n bytes at p -> (offset of its bytes, next)"""
    mt, _, v, p = tm.head(buf, p, e)
    if mt != 2 or v is None or v != n or n > e - p:
        raise Shape
    return p, p + n


def wit_items(buf, p, e, arity):
    """the value of key 0 (arity 2) or key 2 (arity 4) at p -> ([(key offset, sig offset)], next)"""
    mt, _, arg, p = tm.head(buf, p, e)
    if mt == 6:
        if arg != 258:
            raise Shape
        mt, _, arg, p = tm.head(buf, p, e)
    if mt != 4:
        raise Shape
    out = []
    while True:
        if arg is None:
            if p >= e:
                raise Shape
            if buf[p] == 0xFF:
                p += 1
                break
        elif len(out) == arg:
            break
        mt, _, n, p = tm.head(buf, p, e)
        if mt != 4 or (n is not None and n != arity):
            raise Shape
        key_at, p = _bytes_at(buf, p, e, 32)
        sig_at, p = _bytes_at(buf, p, e, 64)
        for _ in range(arity - 2):
            p = tm.skip(buf, p, e)
        if n is None:
            if p >= e or buf[p] != 0xFF:
                raise Shape
            p += 1
        out.append((key_at, sig_at))
    return out, p


def witness_set(buf, s, e):
    """-> (VKey items, bootstrap items) of the witness set at [s, e); raises Shape"""
    try:
        mt, _, n, p = tm.head(buf, s, e)
        if mt != 5:
            return [], []
        seen = {}
        k = 0
        while len(seen) < 2:
            if n is None:
                if p >= e:
                    raise Shape
                if buf[p] == 0xFF:
                    break
            elif k == n:
                break
            kmt, _, kv, kq = tm.head(buf, p, e)
            if kmt == 0 and kv in (0, 2) and kv not in seen:
                seen[kv], p = wit_items(buf, kq, e, 2 if kv == 0 else 4)
            else:
                p = tm.skip(buf, tm.skip(buf, p, e), e)
            k += 1
        return seen.get(0, []), seen.get(2, [])
    except tm.Bad:
        raise Shape


def verify_blocks(buf, off, length, byron=False):
    """-> (blocks, txs, wits): dicts of lists named as the library's arrays"""
    st, rw = tm.index_blocks(buf, off, length, byron)
    B = {k: [] for k in BLOCKS}
    T = {k: [] for k in TXS}
    W = {k: [] for k in WITS}
    B["status"], B["n_tx"], B["tx_first"] = st["status"], st["n_tx"], st["tx_first"]
    for i, (o, ln) in enumerate(zip(off, length)):
        n_wit = n_bad = n_shape = 0
        is_byron = tm.is_byron_item(buf, int(o), int(o) + int(ln))
        for p in range(st["tx_first"][i], st["tx_first"][i + 1]):
            ws, tx_id = rw["wit_off"][p], rw["tx_id"][p]
            status, vk, bt = OK, [], []
            if is_byron:
                status = SKIPPED
            else:
                try:
                    vk, bt = witness_set(buf, ws, ws + rw["wit_len"][p])
                except Shape:
                    status = SHAPE
            bad = 0
            T["wit_first"].append(len(W["tx"]))
            for kind, items in ((0, vk), (2, bt)):
                for key_at, sig_at in items:
                    key, sig = bytes(buf[key_at:key_at + 32]), bytes(buf[sig_at:sig_at + 64])
                    ok = 1 if oracle.ed25519_verify(key, tx_id, sig) else 0
                    bad += 1 - ok
                    W["tx"].append(p)
                    W["kind"].append(kind)
                    W["key_off"].append(key_at)
                    W["sig_off"].append(sig_at)
                    W["ok"].append(ok)
                    W["key_hash"].append(hashlib.blake2b(key, digest_size=28).digest() if kind == 0 else bytes(28))
            T["block"].append(i)
            T["status"].append(status)
            T["n_vkey"].append(len(vk))
            T["n_boot"].append(len(bt))
            T["n_bad"].append(bad)
            T["tx_id"].append(tx_id)
            n_wit += len(vk) + len(bt)
            n_bad += bad
            n_shape += status == SHAPE
        B["n_wit"].append(n_wit)
        B["n_bad"].append(n_bad)
        B["n_shape"].append(n_shape)
    T["wit_first"].append(len(W["tx"]))
    return B, T, W
