"""GPU: db-analyser's ledger-free analyses (praos_hip.analysis.analyse_immutable) over a small
ImmutableDB directory of three chunks.

The Shelley-based chunks are written by immutable.write_immutable from chunk_corpus blocks
(linked, signed headers) whose segments are tx_corpus transactions; with `byron` set the first
chunk holds an EBB and Byron main blocks (byron_corpus, their txPayload from tx_corpus).  For
each of the six analyses the lines equal the lines formed here from the blocks' own fields and
the model's per-block values (tx_index_model.py), for the whole directory and with `limit`
cutting inside the second chunk."""
import numpy as np
import pytest

import block_integrity as bi
import byron_corpus as bc
import chunk_corpus as cc
import tx_corpus as tc
import tx_index_model as tm
from helpers import rbytes, rng
from praos_hip import analysis, immutable

pytestmark = pytest.mark.gpu
SPKP = 129600
CHUNK_SLOTS = 100
BYRON = (bc.EPOCH_SLOTS, bc.PM)


def tx_block(r, era, slot, block_no, prev, n_tx):
    """a chunk_corpus block whose segments are tx_corpus transactions (re-signed)"""
    b = cc.Block(r, SPKP, era, slot, block_no, prev)
    four = era >= 5
    bodies = [tc.body(r, n_out=j % 4, out_indef=j % 2 == 1) for j in range(n_tx)]
    wits = [tc.witness(r, tc.redeemers(r, "array", [5, 6]) if four else None) for _ in range(n_tx)]
    segs = [tc.seq(4, bodies, n_tx % 2 == 1), tc.seq(4, wits, False),
            tc.seq(5, [(tc.hd(0, 0), tc.bstr(r, 11))] if n_tx else [], False)]
    if four:
        segs.append(tc.seq(4, [tc.hd(0, n_tx - 1)] if n_tx else [], False))
    b.segs = segs
    b.f["body_size"] = sum(map(len, segs))
    b.f["body_hash"] = bi._b2b(b"".join(bi._b2b(s) for s in segs))
    return b.sign()


def build_db(path, byron):
    """-> the blocks in chain order as dicts: slot, block_no, header_size, hash, prev, is_ebb, bytes"""
    r = rng(77)
    blocks, prev, bno = [], None, 0
    if byron:
        dlg = bc.Delegate(r)
        ebb = bc.EBB(r, rbytes(r, 32), 0, 0)
        blocks.append({"slot": 0, "block_no": 0, "obj": ebb, "prev": None, "is_ebb": 1})
        prev = ebb.header_hash
        for k in range(4):
            bno += 1
            m = bc.Main(r, dlg, prev, 0, 3 * k, bno)
            m.txs = [(tc.byron_tx(r, 1 + j), tc.byron_wits(r)) for j in range(k)]
            m.sign()
            blocks.append({"slot": 3 * k, "block_no": bno, "obj": m, "prev": prev, "is_ebb": 0})
            prev = m.header_hash
        bno += 1
    first = len(blocks)
    slots = [CHUNK_SLOTS + 7, 130, 131, 199, 200, 244, 260, 299] if byron else [3, 40, 99, 100, 101, 150, 200, 250, 299]
    for k, slot in enumerate(slots):
        b = tx_block(r, (6, 3, 5, 7, 2, 4)[k % 6], slot, bno, prev, (2, 0, 5, 1, 3)[k % 5])
        blocks.append({"slot": slot, "block_no": bno, "obj": b, "prev": prev, "is_ebb": 0})
        prev, bno = b.header_hash, bno + 1
    sh = blocks[first:]
    arena, off, _ = cc.layout([x["obj"].bytes for x in sh])
    immutable.write_immutable(str(path), np.frombuffer(arena, np.uint8),
                              np.array(off, np.uint64) + np.uint64(immutable.HEADER_OFFSET),
                              np.array([len(x["obj"].header) for x in sh], np.uint32),
                              [x["slot"] for x in sh], [x["obj"].header_hash for x in sh], CHUNK_SLOTS)
    if byron:       # the Byron chunk, written as it is stored; no index (every block is checked)
        (path / "00000.chunk").write_bytes(b"".join(x["obj"].bytes for x in blocks[:first]))
        (path / "00000.secondary").unlink()
    for x in blocks:
        blob = x["obj"].bytes
        st, _ = tm.index_blocks(blob, [0], [len(blob)], byron=bool(byron))
        assert st["status"] == [tm.OK]
        x.update(hash=x["obj"].header_hash, header_size=len(x["obj"].header), n_tx=st["n_tx"][0],
                 txs_size=st["txs_size"][0], n_out=st["n_out"][0])
    return blocks


def expected(blocks, name, limit):
    bl = blocks if limit is None else blocks[:limit]
    out, cum = ["Started " + name], 0
    for x in bl:
        bn, sn = f"BlockNo {x['block_no']}", f"SlotNo {x['slot']}"
        if name == "ShowSlotBlockNo":
            out.append(f"{bn}\t{sn}")
        elif name == "CountTxOutputs":
            cum += x["n_out"]
            out.append(f"{bn}\t{sn}\tcumulative: {cum}\tcount: {x['n_out']}")
        elif name == "ShowBlockHeaderSize":
            out.append(f"{bn}\t{sn}\theader size: {x['header_size']}")
        elif name == "ShowBlockTxsSize":
            out.append(f"{sn}\tNum txs in block = {x['n_tx']}\tTotal size of txs in block = {x['txs_size']}")
        elif name == "ShowEBBs" and x["is_ebb"]:
            prev = "GenesisHash" if x["prev"] is None else "BlockHash " + x["prev"].hex()
            out.append(f"EBB: {x['hash'].hex()}\tPrev: {prev}\tKnown: True")
    result = None
    if name == "ShowBlockHeaderSize":
        result = max([x["header_size"] for x in bl], default=0)
        out.append(f"Maximum encountered header size = {result}")
    elif name == "CountBlocks":
        result = len(bl)
        out.append(f"Counted {result} blocks.")
    return out + ["Done", result]


@pytest.fixture(scope="module", params=[None, BYRON], ids=["shelley", "byron"])
def db(request, tmp_path_factory):
    path = tmp_path_factory.mktemp("txdb") / "immutable"
    path.mkdir()
    return str(path), request.param, build_db(path, request.param)


@pytest.mark.parametrize("name", analysis.ANALYSES)
def test_analysis_lines(ctx, db, name):
    path, byron, blocks = db
    known = {x["hash"]: x["prev"] for x in blocks if x["is_ebb"]}
    assert len({x["slot"] // CHUNK_SLOTS for x in blocks}) == 3
    in_first_two = sum(1 for x in blocks if x["slot"] < 2 * CHUNK_SLOTS)
    first = sum(1 for x in blocks if x["slot"] < CHUNK_SLOTS)
    for limit in (None, first + 2):
        assert limit is None or first < limit < in_first_two
        got = list(analysis.analyse_immutable(ctx, path, name, SPKP, byron=byron, limit=limit, known_ebbs=known))
        want = expected(blocks, name, limit)
        assert got == want
        assert type(got[-1]) is {"ShowBlockHeaderSize": analysis.ResultMaxHeaderSize,
                                 "CountBlocks": analysis.ResultCountBlock}.get(name, type(None))
    if name == "ShowEBBs" and byron:
        got = list(analysis.analyse_immutable(ctx, path, name, SPKP, byron=byron))
        assert len(got) == 4 and got[1].endswith("\tKnown: False")        # the default table is empty
    if name == "CountTxOutputs":
        assert sum(x["n_out"] for x in blocks) > 10 and any(x["n_out"] == 0 for x in blocks)
