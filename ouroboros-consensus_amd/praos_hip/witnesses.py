"""The signature check of every transaction's key witnesses over an ImmutableDB directory, one
GPU pass per chunk.

What a `db-analyser --validate-all-blocks` style revalidation spends per witness on the CPU:
applyBlockLedgerResult with asoValidation = STS.ValidateAll (Shelley/Ledger/Ledger.hs:335-352)
verifies every VKey and bootstrap witness of a block as an Ed25519 signature over its
transaction's txId; reapplyBlockLedgerResult (:354-373) skips it.  Per chunk file the bytes go to
the device twice over one read, as analysis.analyse_immutable sends them: Context.validate_chunk
(parseChunkFile: slot and block number of every block of the valid prefix) and
Context.verify_tx_witnesses (the transaction index and the witness check over the same bytes).

Signature validity only: which keys had to sign (witsVKeyNeeded) needs the ledger state, and
Byron transactions are skipped."""
import os
from collections import namedtuple

import numpy as np

from . import abi
from .immutable import ENTRY, chunk_report, read_index

BlockWitnesses = namedtuple("BlockWitnesses", "slot block_no n_tx n_wit n_bad n_shape")
# failing: (slot, transaction index in its block, witness index in its transaction, kind 0 / 2)
WitnessTotals = namedtuple("WitnessTotals", "blocks txs wits bad shape failing")


def chunk_witnesses(ctx, data, crc, off, slots_per_kes_period, byron=None):
    """One chunk file -> (parse result, slots, block numbers, is_ebb, per-block, per-transaction and
    per-witness arrays of Context.verify_tx_witnesses) over validate_chunk's valid prefix."""
    res = ctx.validate_chunk(data, crc, off, slots_per_kes_period, byron=byron)
    n = res["blocks"]
    e = np.frombuffer(res["entries"], np.uint8).reshape(n, ENTRY)
    boff = e[:, 0:8].copy().view(">u8").reshape(-1).astype(np.uint64)
    blen = np.diff(np.append(boff, np.uint64(res["truncate_at"]))).astype(np.uint32)
    B, T, W, _ = ctx.verify_tx_witnesses(data, boff, blen, byron=byron is not None)
    if n and (B["status"] != abi.TXI_OK).any():
        k = int(np.nonzero(B["status"] != abi.TXI_OK)[0][0])
        raise abi.PraosError(f"block {k} of the chunk passed validation but its transactions do not index "
                             f"(status {int(B['status'][k])})")
    slot = e[:, 48:56].copy().view(">u8").reshape(-1).astype(np.uint64)
    is_ebb = res["is_ebb"] if "is_ebb" in res else np.zeros(n, np.uint8)
    return res, slot, res["block_no"], is_ebb, B, T, W


def verify_immutable_witnesses(ctx, path, slots_per_kes_period, byron=None, limit=None):
    """Generator: one BlockWitnesses(slot, block_no, n_tx, n_wit, n_bad, n_shape) per block of the
    database at `path`, in chain order, then a WitnessTotals as the last item: the sums and the
    failing witnesses as (slot, transaction index in the block, witness index in the transaction,
    kind).  byron: None or (epoch_slots, protocol_magic), as validate_immutable takes it (Byron
    transactions are skipped: no witnesses, none failing); limit: the first N blocks.  An EBB's
    slot is its epoch's first.  Stops, as the reference's validation would truncate, after the
    valid prefix of the first chunk that has an error or does not fit its predecessor."""
    chunks = sorted(int(f[:5]) for f in os.listdir(path) if f.endswith(".chunk"))
    left = limit
    tot = [0, 0, 0, 0, 0]
    failing = []
    tip = None
    for c in chunks:
        if left is not None and left <= 0:
            break
        data = np.fromfile(os.path.join(path, f"{c:05d}.chunk"), np.uint8)
        sec, crc, off = read_index(path, c)
        res, slot, block_no, is_ebb, B, T, W = chunk_witnesses(ctx, data, crc, off, slots_per_kes_period, byron)
        row, tip = chunk_report(c, res, sec, tip)
        n = res["blocks"] if row["fits"] else 0
        if left is not None:
            n = min(n, left)
            left -= n
        slots = [int(slot[i]) * (int(byron[0]) if is_ebb[i] else 1) for i in range(n)]
        for i in range(n):
            yield BlockWitnesses(slots[i], int(block_no[i]), int(B["n_tx"][i]), int(B["n_wit"][i]), int(B["n_bad"][i]),
                                 int(B["n_shape"][i]))
        tot[0] += n
        for k, name in enumerate(("n_tx", "n_wit", "n_bad", "n_shape")):
            tot[1 + k] += int(B[name][:n].sum())
        for w in np.nonzero(W["ok"] == 0)[0]:
            p = int(W["tx"][w])
            i = int(T["block"][p])
            if i < n:
                failing.append((slots[i], p - int(B["tx_first"][i]), int(w) - int(T["wit_first"][p]), int(W["kind"][w])))
        if row["outcome"] != 0 or not row["fits"]:
            break
    yield WitnessTotals(*tot, failing)
