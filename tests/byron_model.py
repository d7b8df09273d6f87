"""The Byron storage rules restated in plain Python (the independent checker of k_byron.hip).

Stored form (Byron/Ledger/Serialisation.hs:165-177): an EBB is 82 00 83 <hdr> <body> <extra>, a
main block 82 01 83 <hdr> <body> <extra>; headerOffset 3, headerSize = the header item's length.
Header hash = Blake2b-256(82 0k || header item), k = 0 EBB / 1 main block.
  main header = [pm, prev(bytes32), proof, consensus, extra]
    proof     = [[nTx, txRoot(32), witHash(32)], sscProof, dlgHash(32), updHash(32)]
    consensus = [[epoch, slotInEpoch], issuerXPub(64), [difficulty],
                 [2, [[certEpoch, issuerXPub, delegateXPub, certSig(64)], sig(64)]]]
  EBB header  = [pm, prev(bytes32), bodyProof(bytes32), [epoch, [difficulty]], extra]
verifyHeaderIntegrity (Byron/Ledger/Integrity.hs:21-53, PBFT.hs:55-75): EBB True; main block
pm == configured pm and Ed25519 over "01" || issuerXPub || 09 || CBOR(pm) || 85 || the stored
prev, proof, slot-id, difficulty and extra items, under the first 32 bytes of delegateXPub.
blockMatchesHeader (Block.hs:161-162): EBB True; main block the five comparisons of
body_which().  The Merkle root for n = 0 and n >= 2 follows the published Byron rule and is
pinned by no reference file; parse_chunk therefore answers UNSUPPORTED where it alone fails.

Uses hashlib and the oracle's ed25519_verify; imports chunk_model for the Shelley side of a
mixed chunk and for the result layout."""
import hashlib
import zlib

import numpy as np

import block_integrity as bi
import chunk_model as cm
import oracle as orc

OK, ERR_READ, ERR_CORRUPT, ERR_HASH_MISMATCH, UNSUPPORTED = 0, 1, 2, 3, 4
BLK_DECODE, BLK_BODY_HASH, BLK_PBFT_SIG, BLK_PM = 0x01, 0x04, 0x08, 0x10
W_DLG, W_UPD, W_NTX, W_WIT, W_ROOT = 1, 2, 4, 8, 16
M64 = (1 << 64) - 1


def b2b(m):
    return hashlib.blake2b(m, digest_size=32).digest()


class Bad(Exception):
    pass


def _uint(buf, p, end, limit):
    mt, _, v, p = bi._head(buf, p, end)
    if mt != 0 or v > limit:
        raise Bad
    return v, p


def _list(buf, p, end, n):
    mt, _, v, p = bi._head(buf, p, end)
    if mt != 4 or v is None or v != n:
        raise Bad
    return p


def _bytes(buf, p, end, n):
    """a definite byte string of exactly n bytes -> (offset of the raw bytes, next)"""
    mt, _, v, p = bi._head(buf, p, end)
    if mt != 2 or v is None or v != n or n > end - p:
        raise Bad
    return p, p + n


def _item(buf, p, end):
    return p, bi.cbor_skip(buf, p, end)


def parse_block(buf, off, length):
    """A stored Byron block -> dict of fields and spans (absolute offsets), or None when it is
    not [0|1, ...] at all; raises Bad when it is but does not decode."""
    end = off + length
    try:
        mt, _, v, p = bi._head(buf, off, end)
        if mt != 4 or v is None or v < 1:
            return None
        mt, _, kind, p = bi._head(buf, p, end)
        if mt != 0 or kind > 1:
            return None
        if v != 2:
            raise Bad
        p = _list(buf, p, end, 3)
        ho, he = _item(buf, p, end)
        bo, be = _item(buf, he, end)
        xo, xe = _item(buf, be, end)
        if xe != end:
            raise Bad
        d = {"kind": kind, "is_ebb": int(kind == 0), "hoff": ho, "hlen": he - ho,
             "header_hash": b2b(bytes([0x82, kind]) + bytes(buf[ho:he]))}
        p = _list(buf, ho, he, 5)
        d["pm"], p = _uint(buf, p, he, 0xFFFFFFFF)
        prev_s = p
        q, p = _bytes(buf, p, he, 32)
        d["prev_span"] = (prev_s, p)
        prev = bytes(buf[q:q + 32])
        if kind == 0:
            _, p = _bytes(buf, p, he, 32)
            p = _list(buf, p, he, 2)
            epoch, p = _uint(buf, p, he, M64)
            p = _list(buf, p, he, 1)
            d["block_no"], p = _uint(buf, p, he, M64)
            _, p = _item(buf, p, he)
            if p != he:
                raise Bad
            d.update(epoch=epoch, slot_in_epoch=0, prev_hash=None if epoch == 0 else prev)
            return d
        d["prev_hash"] = prev
        proof_s = p
        p = _list(buf, p, he, 4)
        p = _list(buf, p, he, 3)
        d["ntx"], p = _uint(buf, p, he, M64)
        d["tx_root"], p = _bytes(buf, p, he, 32)
        d["wit_hash"], p = _bytes(buf, p, he, 32)
        _, p = _item(buf, p, he)
        d["dlg_hash"], p = _bytes(buf, p, he, 32)
        d["upd_hash"], p = _bytes(buf, p, he, 32)
        d["proof_span"] = (proof_s, p)
        p = _list(buf, p, he, 4)
        sid = p
        p = _list(buf, p, he, 2)
        d["epoch"], p = _uint(buf, p, he, M64)
        d["slot_in_epoch"], p = _uint(buf, p, he, 0xFFFF)
        d["slotid_span"] = (sid, p)
        d["issuer"], p = _bytes(buf, p, he, 64)
        ds = p
        p = _list(buf, p, he, 1)
        d["block_no"], p = _uint(buf, p, he, M64)
        d["diff_span"] = (ds, p)
        p = _list(buf, p, he, 2)
        tag, p = _uint(buf, p, he, M64)
        if tag != 2:
            raise Bad
        p = _list(buf, p, he, 2)
        p = _list(buf, p, he, 4)
        _, p = _uint(buf, p, he, M64)
        _, p = _bytes(buf, p, he, 64)
        d["delegate"], p = _bytes(buf, p, he, 64)
        _, p = _bytes(buf, p, he, 64)
        d["sig"], p = _bytes(buf, p, he, 64)
        xs = p
        _, p = _item(buf, p, he)
        d["extra_span"] = (xs, p)
        if p != he:
            raise Bad
        # body = [txPayload, ssc, dlg, upd]; txPayload = a list of [tx, witnesses]
        p = _list(buf, bo, be, 4)
        mt, _, n, q = bi._head(buf, p, be)
        if mt != 4:
            raise Bad
        pairs = []
        while (n is None and q < be and buf[q] != 0xFF) or (n is not None and len(pairs) < n):
            q = _list(buf, q, be, 2)
            ts, q = _item(buf, q, be)
            ws, q2 = _item(buf, q, be)
            pairs.append(((ts, q), (ws, q2)))
            q = q2
        if n is None:
            if q >= be:
                raise Bad
            q += 1
        d["pairs"] = pairs
        d["txp_span"] = (p, q)
        d["ssc_span"] = _item(buf, q, be)
        d["dlg_span"] = _item(buf, d["ssc_span"][1], be)
        d["upd_span"] = _item(buf, d["dlg_span"][1], be)
        if d["upd_span"][1] != be:
            raise Bad
        return d
    except bi._Bad:
        raise Bad


def point_slot(d, epoch_slots):
    return (d["epoch"] * epoch_slots + d["slot_in_epoch"]) & M64


def cbor_uint(v):
    for ai, nb in ((24, 1), (25, 2), (26, 4), (27, 8)):
        if v < 24:
            return bytes([v])
        if v < 1 << (8 * nb):
            return bytes([ai]) + v.to_bytes(nb, "big")
    raise ValueError


def signed_message(buf, d):
    sp = lambda k: bytes(buf[d[k][0]:d[k][1]])
    return (b"01" + bytes(buf[d["issuer"]:d["issuer"] + 64]) + b"\x09" + cbor_uint(d["pm"]) + b"\x85" +
            sp("prev_span") + sp("proof_span") + sp("slotid_span") + sp("diff_span") + sp("extra_span"))


def merkle_root(leaves):
    """Byron's MerkleTree root over leaf hashes: node = H(01 || l || r), split at the largest power
    of two below n, empty tree = H("")."""
    n = len(leaves)
    if n == 0:
        return b2b(b"")
    if n == 1:
        return leaves[0]
    k = 1 << ((n - 1).bit_length() - 1)
    return b2b(b"\x01" + merkle_root(leaves[:k]) + merkle_root(leaves[k:]))


def body_which(buf, d):
    """The failing comparisons of blockMatchesHeader as W_* bits (0: the body matches)."""
    h = lambda o: bytes(buf[o:o + 32])
    sp = lambda s: bytes(buf[s[0]:s[1]])
    w = 0
    if h(d["dlg_hash"]) != b2b(sp(d["dlg_span"])):
        w |= W_DLG
    if h(d["upd_hash"]) != b2b(sp(d["upd_span"])):
        w |= W_UPD
    if d["ntx"] != len(d["pairs"]):
        w |= W_NTX
    if h(d["wit_hash"]) != b2b(b"\x9f" + b"".join(sp(ws) for _, ws in d["pairs"]) + b"\xff"):
        w |= W_WIT
    if h(d["tx_root"]) != merkle_root([b2b(b"\x00" + sp(ts)) for ts, _ in d["pairs"]]):
        w |= W_ROOT
    return w


_cache = {}


def integrity(blk, pm):
    """(PRAOS_BLK_* bits, which) of one stored block: praos_verify_byron_integrity's answer."""
    blk = bytes(blk)
    key = (hashlib.sha256(blk).digest(), pm)
    if key not in _cache:
        _cache[key] = _integrity(blk, pm)
    return _cache[key]


def _integrity(blk, pm):
    try:
        d = parse_block(blk, 0, len(blk))
    except Bad:
        d = None
    if d is None:
        return BLK_DECODE, 0
    if d["is_ebb"]:
        return 0, 0
    bits = 0
    if d["pm"] != pm:
        bits |= BLK_PM
    key = blk[d["delegate"]:d["delegate"] + 32]
    if not orc.ed25519_verify(key, signed_message(blk, d), blk[d["sig"]:d["sig"] + 64]):
        bits |= BLK_PBFT_SIG
    w = body_which(blk, d)
    if w:
        bits |= BLK_BODY_HASH
    return bits, w


def root_unpinned(bits, which, ntx):
    """The one verdict this validator leaves to the reference: only the unpinned Merkle root fails."""
    return bits == BLK_BODY_HASH and which == W_ROOT and ntx != 1


def _one_block(data, o, e):
    try:
        if parse_block(data, o, e - o) is not None:
            return True
    except Bad:
        return False
    return bi.split_block(data, o, e - o)[0]


def rescanned_from(data, block_off, m):
    """chunk_model.rescanned_from where a Byron block that decodes confirms its candidate too."""
    L = len(data)
    k = 0
    if block_off is not None:
        while k < m and block_off[k] < L and (block_off[0] == 0 if k == 0 else block_off[k] > block_off[k - 1]):
            k += 1
    full = m > 0 and k == m
    ncand = m if full else max(k - 1, 0)
    for j in range(ncand):
        o = int(block_off[j])
        e = int(block_off[j + 1]) if j + 1 < m else L
        if not _one_block(data, o, e):
            return o
    return L if full else (int(block_off[k - 1]) if k else 0)


def parse_chunk(data, expected_crc=None, byron=None, spkp=129600, block_off=None):
    """chunk_model.parse_chunk with Byron items decoded when byron = (epoch_slots, pm); also
    returns is_ebb per yielded block.  byron=None is chunk_model's answer."""
    if byron is None:
        return cm.parse_chunk(data, expected_crc, spkp, block_off)
    es, pm = byron
    data = bytes(data)
    exp = [] if expected_crc is None else [int(x) for x in expected_crc]
    L = len(data)
    res = {"outcome": OK, "integrity_bits": 0, "blocks": 0, "checked": 0, "truncate_at": L,
           "rescanned_from": rescanned_from(data, block_off, len(exp)), "err_slot": 0,
           "err_hash": bytes(32), "expected_prev": bytes(32), "actual_prev": bytes(32), "actual_prev_is_genesis": 0}
    rows = []
    pos, i, last_hash = 0, 0, None
    while pos < L:
        res["truncate_at"] = pos
        try:
            end = bi.cbor_skip(data, pos, L)
        except bi._Bad:
            res["outcome"] = ERR_READ
            break
        try:
            d = parse_block(data, pos, end - pos)
        except Bad:
            res["outcome"] = ERR_READ
            break
        if d is None:     # a Shelley-based block: chunk_model's rules
            ok, ho, hl, _ = bi.split_block(data, pos, end - pos)
            dh = cm.ch.decode_header(data, ho, hl, allow_tpraos=True) if ok else None
            if not ok or dh["status"] & cm.ch.DEC_FAIL:
                res["outcome"] = ERR_READ
                break
            f = dh["fields"]
            d = {"hoff": ho, "hlen": hl, "header_hash": dh["header_hash"], "prev_hash": f["prev_hash"],
                 "block_no": f["block_no"], "is_ebb": 0}
            slot = entry_slot = f["slot"]
            bits, which, ntx = cm._integrity(data[pos:end], spkp), 0, 1
        else:
            slot = point_slot(d, es)
            entry_slot = d["epoch"] if d["is_ebb"] else slot
            bits, which = integrity(data[pos:end], pm)
            ntx = len(d.get("pairs", [0]))
        crc = zlib.crc32(data[pos:end])
        trusted = i < len(exp) and crc == exp[i]
        if not trusted:
            res["checked"] += 1
            if bits:
                if root_unpinned(bits, which, ntx):
                    res["outcome"] = UNSUPPORTED
                else:
                    res.update(outcome=ERR_CORRUPT, integrity_bits=bits, err_slot=slot, err_hash=d["header_hash"])
                break
        if i > 0 and d["prev_hash"] != last_hash:
            res.update(outcome=ERR_HASH_MISMATCH, err_slot=slot, err_hash=d["header_hash"], expected_prev=last_hash,
                       actual_prev=d["prev_hash"] or bytes(32), actual_prev_is_genesis=int(d["prev_hash"] is None))
            break
        rows.append((pos.to_bytes(8, "big") + (d["hoff"] - pos).to_bytes(2, "big") + d["hlen"].to_bytes(2, "big") +
                     crc.to_bytes(4, "big") + d["header_hash"] + entry_slot.to_bytes(8, "big"),
                     d["block_no"], d["prev_hash"] or bytes(32), int(d["prev_hash"] is None),
                     -1 if trusted else 0, d["is_ebb"]))
        last_hash = d["header_hash"]
        pos, i = end, i + 1
    else:
        res["truncate_at"] = L
    res["blocks"] = len(rows)
    col = lambda k, dt: np.array([r[k] for r in rows], dt)
    res.update(entries=b"".join(r[0] for r in rows), block_no=col(1, np.uint64),
               prev_hash=np.frombuffer(b"".join(r[2] for r in rows), np.uint8).reshape(-1, 32),
               prev_is_genesis=col(3, np.uint8), integrity=col(4, np.int8), is_ebb=col(5, np.uint8))
    return res
