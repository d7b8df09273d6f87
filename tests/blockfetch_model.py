"""praos_verify_fetched_blocks restated sequentially in plain Python (the independent checker of
k_blockfetch.hip; semantics: DESIGN section 35, include/praos_hip.h).

Its own walk of the wire wrapper; oracle/block_integrity.py and oracle/cbor_header.py for the
split, the header fields and hashTxSeq of a Shelley-based block, byron_model for a Byron one;
tx_witness_model (over tx_index_model) for the transactions and their key witnesses.  One item at
a time.  The distinct blocks are found by comparing the bytes themselves, under the library's
rule stated exactly: items that split and decode are classed by (disk tag, header hash, inner
length); the representative of a class is its lowest item; every other member is compared byte
for byte with the representative -- equal, it shares the representative's row; not equal, it gets
a row of its own, and such deviants are not classed further among themselves.  Rows are numbered
in order of first appearance of their lowest item."""
import hashlib

import block_integrity as bi
import byron_model as bm
import cbor_header as ch
import tx_witness_model as wm

OK, RANGE, SYNTAX, ERA, TRAILING = 0, 1, 2, 3, 4
(BF_OK, BF_WIRE, BF_DECODE, BF_WRONG_BLOCK, BF_INVALID_BODY, BF_TOO_MANY, BF_UNSUPPORTED,
 BF_NOT_REACHED) = 0, 1, 2, 3, 4, 5, 6, 255
COMPLETE, FAILED, TOO_FEW = 0, 1, 2
NO_ROW = 0xFFFFFFFF
ITEMS = ("status", "tag", "verdict", "row")
RANGES = ("stop", "accepted", "status")
ROWS = ("item", "tag", "is_ebb", "slot", "block_no", "header_hash", "prev_hash", "hdr_off", "hdr_len", "blk_off",
        "blk_len", "body_hash", "bits", "which")


def b2b(m):
    return hashlib.blake2b(bytes(m), digest_size=32).digest()


class _No(Exception):
    pass


def _head(buf, p, e, want):
    """a definite head of major type `want` at p, of any width -> (argument, next)"""
    if p >= e:
        raise _No
    ib = buf[p]
    if ib >> 5 != want:
        raise _No
    ai, p = ib & 31, p + 1
    if ai < 24:
        return ai, p
    if ai > 27:
        raise _No
    nb = 1 << (ai - 24)
    if e - p < nb:
        raise _No
    return int.from_bytes(buf[p:p + nb], "big"), p + nb


def unwrap(buf, off, length, n_eras=7):
    """-> (status, disk tag, inner offset, inner length); the span of an OK or ERA item, else 0, 0"""
    if off > len(buf) or length > len(buf) - off:
        return RANGE, 0xFF, 0, 0
    e = off + length
    try:
        t, p = _head(buf, off, e, 6)
        if t != 24:
            raise _No
        n, p = _head(buf, p, e, 2)
        if n > e - p or n >> 32:
            raise _No
        if p + n != e:
            return TRAILING, 0xFF, 0, 0
        k, q = _head(buf, p, e, 4)
        if k != 2:
            raise _No
        tag, _ = _head(buf, q, e, 0)
    except _No:
        return SYNTAX, 0xFF, 0, 0
    return (ERA if tag > n_eras else OK), min(tag, 0xFE), p, n


def header_of(buf, tag, off, length, epoch_slots):
    """The stored block buf[off:off+length] of disk tag `tag` -> dict of the row's header columns
    and what the body check needs, or None when the envelope or the header does not decode."""
    if tag <= 1:
        if not epoch_slots:
            return None
        try:
            d = bm.parse_block(buf, off, length)
        except bm.Bad:
            return None
        if d is None:
            return None
        return {"is_ebb": d["is_ebb"], "slot": bm.point_slot(d, epoch_slots), "block_no": d["block_no"],
                "header_hash": d["header_hash"], "prev_hash": d["prev_hash"] or bytes(32), "hdr_off": d["hoff"],
                "hdr_len": d["hlen"], "byron": d}
    ok, ho, hl, segs = bi.split_block(buf, off, length)
    if not ok:
        return None
    h = ch.decode_header(buf, ho, hl, allow_tpraos=True)
    if h["status"] & ch.DEC_FAIL:
        return None
    f = h["fields"]
    return {"is_ebb": 0, "slot": f["slot"], "block_no": f["block_no"], "header_hash": h["header_hash"],
            "prev_hash": f["prev_hash"] or bytes(32), "hdr_off": ho, "hdr_len": hl, "segs": segs,
            "claimed": f["body_hash"]}


def body_check(buf, hd):
    """-> (bits, which, body hash as computed)"""
    if "byron" in hd:
        d = hd["byron"]
        w = 0 if d["is_ebb"] else bm.body_which(buf, d)
        return (bi.BLK_BODY_HASH if w else 0), w, bytes(32)
    bh = bi.hash_tx_seq(buf, hd["segs"])
    return (0 if bh == hd["claimed"] else bi.BLK_BODY_HASH), 0, bh


def verify(buf, off, length, item_first, exp_first, exp_slot, exp_hash, n_eras=7, byron_epoch_slots=0, dedup=True,
           witnesses=True):
    """-> (items, ranges, rows, blocks, txs, wits): dicts of lists named as the library's arrays
    (the last three None without witnesses)"""
    buf = bytes(buf)
    n = len(off)
    I = {k: [] for k in ITEMS}
    R = {k: [] for k in ROWS}
    heads, rep_of, row_ntx = [], {}, []
    for i in range(n):
        st, tag, p, ln = unwrap(buf, int(off[i]), int(length[i]), n_eras)
        hd = header_of(buf, tag, p, ln, byron_epoch_slots) if st == OK else None
        heads.append(hd)
        row = NO_ROW
        if hd is not None:
            key = (tag, hd["header_hash"], ln) if dedup else i
            rep = rep_of.setdefault(key, i)
            rp = R["blk_off"][I["row"][rep]] if rep != i else p
            if rep != i and buf[p:p + ln] == buf[rp:rp + ln]:
                row = I["row"][rep]
            else:
                row = len(R["item"])
                bits, which, bh = body_check(buf, hd)
                for k, v in (("item", i), ("tag", tag), ("blk_off", p), ("blk_len", ln), ("body_hash", bh),
                             ("bits", bits), ("which", which)):
                    R[k].append(v)
                for k in ("is_ebb", "slot", "block_no", "header_hash", "prev_hash", "hdr_off", "hdr_len"):
                    R[k].append(hd[k])
                row_ntx.append(len(hd["byron"].get("pairs", ())) if "byron" in hd else None)
        I["status"].append(st)
        I["tag"].append(tag)
        I["row"].append(row)
    # ---- verdicts, then the fold per range
    G = {k: [] for k in RANGES}
    I["verdict"] = [None] * n
    for r in range(len(item_first) - 1):
        i0, i1 = int(item_first[r]), int(item_first[r + 1])
        e0, points = int(exp_first[r]), int(exp_first[r + 1]) - int(exp_first[r])
        stop = i1 - i0
        for j in range(i1 - i0):
            i = i0 + j
            row, tag, hd = I["row"][i], I["tag"][i], heads[i]
            if I["status"][i] != OK:
                v = BF_WIRE
            elif j >= points:
                v = BF_TOO_MANY
            elif tag <= 1 and not byron_epoch_slots:
                v = BF_UNSUPPORTED
            elif row != NO_ROW and tag == 1 and bm.root_unpinned(R["bits"][row], R["which"][row], row_ntx[row]):
                v = BF_UNSUPPORTED
            elif row == NO_ROW:
                v = BF_DECODE
            elif hd["slot"] != int(exp_slot[e0 + j]) or hd["header_hash"] != bytes(exp_hash[e0 + j]):
                v = BF_WRONG_BLOCK
            elif R["bits"][row]:
                v = BF_INVALID_BODY
            else:
                v = BF_OK
            if j > stop:
                v = BF_NOT_REACHED
            elif v != BF_OK and stop == i1 - i0:
                stop = j
            I["verdict"][i] = v
        G["stop"].append(stop)
        G["accepted"].append(stop)
        G["status"].append(FAILED if stop < i1 - i0 else TOO_FEW if i1 - i0 < points else COMPLETE)
    if not witnesses:
        return I, G, R, None, None, None
    B, T, W = wm.verify_blocks(buf, R["blk_off"], R["blk_len"], byron=bool(byron_epoch_slots))
    return I, G, R, B, T, W
