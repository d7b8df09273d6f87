"""BlockFetch client side: the blocks several peers send, held against the requested points, each
distinct one checked once on the device (Context.verify_fetched_blocks).

wrap_block / unwrap_block are the node-to-node encoding of a block in plain Python (the rules of
wire_scan.hpp's wire_block_unwrap restated); verify_fetched lays the peers' answers out in one
arena, one range per request, makes the one call and hands every request its results back."""
from collections import namedtuple

import numpy as np

from . import abi
from .txsubmission import _head

N_ERAS = 7     # the highest disk tag of the reference's CardanoBlock (Conway)
WIRE_OK, WIRE_RANGE, WIRE_SYNTAX, WIRE_ERA, WIRE_TRAILING = 0, 1, 2, 3, 4

Request = namedtuple("Request", "verdicts accepted blocks status")
Block = namedtuple("Block", "slot block_no hash n_tx n_wit n_bad n_shape")


def wrap_block(block_bytes):
    """The wire form of a stored block [diskTag, ...]: #6.24(bytes), the shortest heads."""
    block_bytes = bytes(block_bytes)
    return b"\xd8\x18" + _head(2, len(block_bytes)) + block_bytes


def _rd(buf, p, e, want):
    """one definite head of major type `want`, any width -> (argument, next) or None"""
    if p >= e or buf[p] >> 5 != want:
        return None
    ai = buf[p] & 31
    p += 1
    if ai < 24:
        return ai, p
    if ai > 27 or (1 << (ai - 24)) > e - p:
        return None
    nb = 1 << (ai - 24)
    return int.from_bytes(buf[p:p + nb], "big"), p + nb


def unwrap_block(buf, off=0, length=None, n_eras=N_ERAS):
    """-> (status, disk tag, inner offset, inner length) of the wire block buf[off:off+length].
    The tag's and the byte string's heads at any width, tag 24, a definite byte string; bytes
    after it: TRAILING.  The inner bytes start with a definite array head of 2 and an unsigned
    integer, the disk tag (SYNTAX otherwise); a tag above n_eras is ERA.  The tag reads 0xff until
    it is seen and 0xfe above 0xfe; the span is that of an OK or ERA item, else (0, 0)."""
    length = len(buf) - off if length is None else length
    if off > len(buf) or length > len(buf) - off:
        return WIRE_RANGE, 0xFF, 0, 0
    e = off + length
    h = _rd(buf, off, e, 6)
    if h is None or h[0] != 24:
        return WIRE_SYNTAX, 0xFF, 0, 0
    h = _rd(buf, h[1], e, 2)
    if h is None or h[0] > e - h[1] or h[0] > 0xFFFFFFFF:
        return WIRE_SYNTAX, 0xFF, 0, 0
    n, p = h
    if p + n != e:
        return WIRE_TRAILING, 0xFF, 0, 0
    a = _rd(buf, p, e, 4)
    t = _rd(buf, a[1], e, 0) if a is not None and a[0] == 2 else None
    if t is None:
        return WIRE_SYNTAX, 0xFF, 0, 0
    return (WIRE_ERA if t[0] > n_eras else WIRE_OK), min(t[0], 0xFE), p, n


def verify_fetched(ctx, peers, n_eras=N_ERAS, byron_epoch_slots=0, witnesses=True, max_lanes=0):
    """peers: a list of peers, each a list of requests (points, blocks): points the (slot, 32-byte
    header hash) pairs of the requested headers in order, blocks the wire blocks the peer sent in
    answer, in arrival order.  Returns (results, n_distinct): results[p][q] is the Request of peer
    p's request q -- the PRAOS_BF_* verdict of each block, how many were accepted (the blocks
    before the first that is not BF_OK), per accepted block a Block (slot, block_no, header hash,
    and with witnesses its transaction count, witness count, witnesses that do not verify and
    transactions whose witness set is outside the shapes; None without) and the range status
    (BF_RANGE_*); n_distinct is the number of distinct blocks, each checked once whoever sent it."""
    reqs = [rq for p in peers for rq in p]
    items = [bytes(b) for _, blocks in reqs for b in blocks]
    ln = np.array([len(b) for b in items], np.uint32)
    off = np.zeros(len(items), np.uint64)
    if len(items):
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(items), np.uint8)
    item_first = np.cumsum([0] + [len(blocks) for _, blocks in reqs], dtype=np.uint64)
    exp_first = np.cumsum([0] + [len(points) for points, _ in reqs], dtype=np.uint64)
    points = [pt for pts, _ in reqs for pt in pts]
    exp_slot = np.array([s for s, _ in points], np.uint64)
    exp_hash = np.frombuffer(b"".join(bytes(h) for _, h in points), np.uint8).reshape(-1, 32)
    I, G, R, B, _, _, (n_rows, _, _) = ctx.verify_fetched_blocks(
        arena, off, ln, item_first, exp_first, exp_slot, exp_hash, n_eras=n_eras, byron_epoch_slots=byron_epoch_slots,
        dedup=True, witnesses=witnesses, max_lanes=max_lanes)
    out, r = [], 0
    for p in peers:
        res = []
        for _ in p:
            i0, acc = int(item_first[r]), int(G["accepted"][r])
            blocks = []
            for i in range(i0, i0 + acc):
                q = int(I["row"][i])
                w = (int(B["n_tx"][q]), int(B["n_wit"][q]), int(B["n_bad"][q]), int(B["n_shape"][q])) if B else (None,) * 4
                blocks.append(Block(int(R["slot"][q]), int(R["block_no"][q]), bytes(R["header_hash"][q]), *w))
            res.append(Request([int(v) for v in I["verdict"][i0:int(item_first[r + 1])]], acc, blocks, int(G["status"][r])))
            r += 1
        out.append(res)
    return out, n_rows
