"""TxSubmission inbound side: the transactions several peers offer, each distinct one checked once
on the device before the mempool sees it (Context.verify_gen_txs).

wrap_gen_tx builds the node-to-node encoding of a transaction; verify_inbound lays the peers'
items out in one arena, makes the one call and hands every peer its items' results back."""
from collections import namedtuple

import numpy as np

from . import abi

TxResult = namedtuple("TxResult", "status tx_id in_block_size ex_mem ex_steps witnesses_ok")


def _head(mt, v):
    if v < 24:
        return bytes([(mt << 5) | v])
    for ai, nb in ((24, 1), (25, 2), (26, 4), (27, 8)):
        if v < 1 << (8 * nb):
            return bytes([(mt << 5) | ai]) + v.to_bytes(nb, "big")
    raise ValueError(v)


def wrap_gen_tx(era, tx_bytes):
    """The wire GenTx of era index `era`: [era, #6.24(tx_bytes)] for a Shelley-based era, tx_bytes
    the ledger's transaction ([body, wits, aux] / [body, wits, isValid, aux]); for Byron (era 0)
    [0, tx_bytes] with tx_bytes the [kind, payload] pair as encodeByronGenTx writes it."""
    tx_bytes = bytes(tx_bytes)
    if era == 0:
        return b"\x82\x00" + tx_bytes
    return b"\x82" + _head(0, era) + b"\xd8\x18" + _head(2, len(tx_bytes)) + tx_bytes


def verify_inbound(ctx, peers, n_eras=7, max_lanes=0):
    """peers: a list of lists of wire transactions (bytes).  Returns (results, n_distinct):
    results[p][k] is the TxResult of peer p's item k -- status (PRAOS_WIRE_* / PRAOS_GTX_*) and,
    for an item with a row, tx_id, in_block_size, ex_mem, ex_steps and whether the transaction's
    witness set has the shapes and every key witness verifies (None otherwise); n_distinct is the
    number of distinct transactions, each verified once whoever offered it."""
    items = [bytes(t) for p in peers for t in p]
    ln = np.array([len(t) for t in items], np.uint32)
    off = np.zeros(len(items), np.uint64)
    if len(items):
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(items), np.uint8)
    I, T, _, (n_rows, _) = ctx.verify_gen_txs(arena, off, ln, n_eras=n_eras, dedup=True, max_lanes=max_lanes)
    out, k = [], 0
    for p in peers:
        res = []
        for _ in p:
            st, row = int(I["status"][k]), int(I["row"][k])
            if row == abi.GTX_NO_ROW:
                res.append(TxResult(st, None, None, None, None, None))
            else:
                ok = int(T["wstatus"][row]) == abi.TXW_OK and int(T["n_bad"][row]) == 0
                res.append(TxResult(st, bytes(T["tx_id"][row]), int(T["in_block_size"][row]), int(T["ex_mem"][row]),
                                    int(T["ex_steps"][row]), ok))
            k += 1
        out.append(res)
    return out, n_rows
