"""parseChunkFile restated in Python (the independent checker of praos_validate_chunk).

Built only from what the oracle already has: block_integrity.cbor_skip (the block boundaries:
block i starts where block i-1 ended and is the one CBOR item there), split_block and
verify_block_integrity, cbor_header.decode_header, zlib.crc32.  Sequential, block by block,
as Storage/ImmutableDB/Impl/Parser.hs:92-197 runs: read, then checkEntries (trusted by its
CRC or verifyBlockIntegrity), then checkIfHashesLineUp; the first offending block ends it.
The result has the keys of praos_hip.abi.Context.validate_chunk."""
import hashlib
import zlib

import numpy as np

import block_integrity as bi
import cbor_header as ch

OK, ERR_READ, ERR_CORRUPT, ERR_HASH_MISMATCH, UNSUPPORTED = 0, 1, 2, 3, 4
_integrity_cache = {}


def _integrity(blk, spkp):
    key = (hashlib.sha256(blk).digest(), spkp)
    if key not in _integrity_cache:
        _integrity_cache[key] = bi.verify_block_integrity(blk, 0, len(blk), spkp)[0]
    return _integrity_cache[key]


def _is_byron(buf, p, end):
    """[0, ...] / [1, ...]: a definite-length array whose first element is the integer 0 or 1."""
    try:
        mt, _, arg, q = bi._head(buf, p, end)
        if mt != 4 or arg is None or arg < 1:
            return False
        mt, _, v, _ = bi._head(buf, q, end)
        return mt == 0 and v <= 1
    except bi._Bad:
        return False


def rescanned_from(data, block_off, m):
    """Where the host walk starts: the first index candidate that is not exactly one block
    envelope (the last one runs to the end of the file), the first offset that cannot be a
    candidate's end, 0 without usable hints; len(data) when every candidate holds."""
    L = len(data)
    k = 0
    if block_off is not None:
        while k < m and block_off[k] < L and (block_off[0] == 0 if k == 0 else block_off[k] > block_off[k - 1]):
            k += 1
    full = m > 0 and k == m
    ncand = m if full else max(k - 1, 0)
    rs = L if full else (int(block_off[k - 1]) if k else 0)
    for j in range(ncand):
        o = int(block_off[j])
        e = int(block_off[j + 1]) if j + 1 < m else L
        if not bi.split_block(data, o, e - o)[0]:
            return o
    return rs


def parse_chunk(data, expected_crc=None, spkp=129600, block_off=None):
    data = bytes(data)
    exp = [] if expected_crc is None else [int(x) for x in expected_crc]
    L = len(data)
    res = {"outcome": OK, "integrity_bits": 0, "blocks": 0, "checked": 0, "truncate_at": L,
           "rescanned_from": rescanned_from(data, block_off, len(exp)), "err_slot": 0, "err_hash": bytes(32),
           "expected_prev": bytes(32), "actual_prev": bytes(32), "actual_prev_is_genesis": 0}
    entries, block_no, prev_hash, prev_gen, integ = [], [], [], [], []
    pos, i, last_hash = 0, 0, None
    while pos < L:
        res["truncate_at"] = pos
        try:
            end = bi.cbor_skip(data, pos, L)
        except bi._Bad:
            res["outcome"] = ERR_READ
            break
        ok, ho, hl, _ = bi.split_block(data, pos, end - pos)
        d = ch.decode_header(data, ho, hl, allow_tpraos=True) if ok else None
        if not ok or d["status"] & ch.DEC_FAIL:
            res["outcome"] = UNSUPPORTED if _is_byron(data, pos, end) else ERR_READ
            break
        f = d["fields"]
        crc = zlib.crc32(data[pos:end])
        trusted = i < len(exp) and crc == exp[i]
        if not trusted:
            res["checked"] += 1
            bits = _integrity(data[pos:end], spkp)
            if bits:
                res.update(outcome=ERR_CORRUPT, integrity_bits=bits, err_slot=f["slot"], err_hash=d["header_hash"])
                break
        if i > 0 and f["prev_hash"] != last_hash:             # None (GenesisHash) never equals a hash
            res.update(outcome=ERR_HASH_MISMATCH, err_slot=f["slot"], err_hash=d["header_hash"],
                       expected_prev=last_hash, actual_prev=f["prev_hash"] or bytes(32),
                       actual_prev_is_genesis=int(f["prev_hash"] is None))
            break
        entries.append(pos.to_bytes(8, "big") + (ho - pos).to_bytes(2, "big") + hl.to_bytes(2, "big") +
                       crc.to_bytes(4, "big") + d["header_hash"] + f["slot"].to_bytes(8, "big"))
        block_no.append(f["block_no"])
        prev_hash.append(f["prev_hash"] or bytes(32))
        prev_gen.append(int(f["prev_hash"] is None))
        integ.append(-1 if trusted else 0)
        last_hash = d["header_hash"]
        pos, i = end, i + 1
    else:
        res["truncate_at"] = L
    res["blocks"] = len(entries)
    res.update(entries=b"".join(entries), block_no=np.array(block_no, np.uint64),
               prev_hash=np.frombuffer(b"".join(prev_hash), np.uint8).reshape(-1, 32),
               prev_is_genesis=np.array(prev_gen, np.uint8), integrity=np.array(integ, np.int8))
    return res


def assert_same(got, want, skip=()):
    """Every field of res and out."""
    for k, w in want.items():
        if k in skip:
            continue
        g = got[k]
        if isinstance(w, np.ndarray):
            assert g.shape == w.shape and (g == w).all(), k
        else:
            assert g == w, (k, g, w)
    assert set(got) == set(want)
