"""db-analyser's ledger-free analyses over an ImmutableDB directory, one GPU pass per chunk.

The six analyses of Cardano/Tools/DBAnalyser/Analysis.hs that need no ledger state
(:112-119, :240-329, :385-395): ShowSlotBlockNo, CountTxOutputs, ShowBlockHeaderSize,
ShowBlockTxsSize, ShowEBBs and CountBlocks.  Per chunk file the bytes go to the device twice
over one read: Context.validate_chunk (parseChunkFile: slot, block number, header size, hash,
prevHash and the EBB flag of every block of the valid prefix) and Context.index_block_txs (the
transaction index: transaction count, sizes and output count per block).  analyse_immutable
yields the lines the reference's tracer prints, `instance Show (TraceEvent blk)` (:190-233),
tab-separated, and ends with the analysis' result.

Show instances from outside the reference tree are written as their packages derive them
(DESIGN section 29 lists them as unpinned): BlockNo n, SlotNo n, GenesisHash / BlockHash <hex>;
a header hash is OneEraHash's hex (HardFork/Combinator/AcrossEras.hs:146-147); sizes and
counts are plain numbers."""
import os

import numpy as np

from . import abi
from .immutable import ENTRY, chunk_report, read_index

ANALYSES = ("ShowSlotBlockNo", "CountTxOutputs", "ShowBlockHeaderSize", "ShowBlockTxsSize", "ShowEBBs", "CountBlocks")


class ResultMaxHeaderSize(int):
    """ShowBlockHeaderSize's AnalysisResult"""


class ResultCountBlock(int):
    """CountBlocks' AnalysisResult"""


def chunk_blocks(ctx, data, crc, off, slots_per_kes_period, byron=None):
    """One chunk file -> (parse result, per-block dict): validate_chunk's valid prefix with, per
    block, slot, block_no, header_size, hash, prev (None = GenesisHash), is_ebb and the
    transaction statistics n_tx, txs_size, n_out of the index over the same bytes."""
    res = ctx.validate_chunk(data, crc, off, slots_per_kes_period, byron=byron)
    n = res["blocks"]
    e = np.frombuffer(res["entries"], np.uint8).reshape(n, ENTRY)
    boff = e[:, 0:8].copy().view(">u8").reshape(-1).astype(np.uint64)
    blen = np.diff(np.append(boff, np.uint64(res["truncate_at"]))).astype(np.uint32)
    st, _ = ctx.index_block_txs(data, boff, blen, byron=byron is not None, rows=False, cap=0)
    if n and (st["status"] != abi.TXI_OK).any():
        k = int(np.nonzero(st["status"] != abi.TXI_OK)[0][0])
        raise abi.PraosError(f"block {k} of the chunk passed validation but its transactions do not index "
                             f"(status {int(st['status'][k])})")
    is_ebb = res["is_ebb"] if "is_ebb" in res else np.zeros(n, np.uint8)
    blocks = {"slot": e[:, 48:56].copy().view(">u8").reshape(-1).astype(np.uint64),
              "block_no": res["block_no"], "header_size": e[:, 10:12].copy().view(">u2").reshape(-1).astype(np.uint16),
              "hash": [bytes(h) for h in e[:, 16:48]],
              "prev": [None if g else bytes(p) for p, g in zip(res["prev_hash"], res["prev_is_genesis"])],
              "is_ebb": is_ebb, "n_tx": st["n_tx"], "txs_size": st["txs_size"], "n_out": st["n_out"]}
    return res, blocks


def _chain_hash(h):
    return "GenesisHash" if h is None else "BlockHash " + h.hex()


def analyse_immutable(ctx, path, analysis, slots_per_kes_period, byron=None, limit=None, known_ebbs=None):
    """Generator: the trace lines of one analysis over the database at `path`, in chain order,
    from "Started <analysis>" to "Done", then the result (a ResultMaxHeaderSize, a
    ResultCountBlock, or None) as the last item.  byron: None or (epoch_slots, protocol_magic),
    as validate_immutable takes it; limit: the first N blocks (db-analyser's Limit);
    known_ebbs: {hash: prev hash or None} for ShowEBBs' `Known` column (default empty: the
    mainnet table is the caller's to supply).  An EBB's slot is its epoch's first
    (epoch * epoch_slots).  Stops, as the reference's validation would truncate, after the valid
    prefix of the first chunk that has an error or does not fit its predecessor."""
    if analysis not in ANALYSES:
        raise ValueError(f"unknown analysis {analysis!r}: one of {', '.join(ANALYSES)}")
    known_ebbs = known_ebbs or {}
    yield "Started " + analysis
    chunks = sorted(int(f[:5]) for f in os.listdir(path) if f.endswith(".chunk"))
    left = limit
    cumulative = counted = max_header = 0
    tip = None
    for c in chunks:
        if left is not None and left <= 0:
            break
        data = np.fromfile(os.path.join(path, f"{c:05d}.chunk"), np.uint8)
        sec, crc, off = read_index(path, c)
        res, b = chunk_blocks(ctx, data, crc, off, slots_per_kes_period, byron)
        row, tip = chunk_report(c, res, sec, tip)
        n = res["blocks"] if row["fits"] else 0
        if left is not None:
            n = min(n, left)
            left -= n
        for i in range(n):
            slot = int(b["slot"][i])
            if b["is_ebb"][i]:
                slot *= int(byron[0])           # the entry of an EBB carries its epoch number
            bn, sn = f"BlockNo {int(b['block_no'][i])}", f"SlotNo {slot}"
            counted += 1
            if analysis == "ShowSlotBlockNo":
                yield f"{bn}\t{sn}"
            elif analysis == "CountTxOutputs":
                cumulative += int(b["n_out"][i])
                yield f"{bn}\t{sn}\tcumulative: {cumulative}\tcount: {int(b['n_out'][i])}"
            elif analysis == "ShowBlockHeaderSize":
                max_header = max(max_header, int(b["header_size"][i]))
                yield f"{bn}\t{sn}\theader size: {int(b['header_size'][i])}"
            elif analysis == "ShowBlockTxsSize":
                yield (f"{sn}\tNum txs in block = {int(b['n_tx'][i])}\t"
                       f"Total size of txs in block = {int(b['txs_size'][i])}")
            elif analysis == "ShowEBBs" and b["is_ebb"][i]:
                h, prev = b["hash"][i], b["prev"][i]
                known = h in known_ebbs and known_ebbs[h] == prev
                yield f"EBB: {h.hex()}\tPrev: {_chain_hash(prev)}\tKnown: {known}"
        if row["outcome"] != 0 or not row["fits"]:
            break
    result = None
    if analysis == "ShowBlockHeaderSize":
        yield f"Maximum encountered header size = {max_header}"
        result = ResultMaxHeaderSize(max_header)
    elif analysis == "CountBlocks":
        yield f"Counted {counted} blocks."
        result = ResultCountBlock(counted)
    yield "Done"
    yield result
