"""ImmutableDB directories of synthetic chains (db-synthesizer analogue) for the replay
driver (praos_replay_immutable).

On-disk layout written (ouroboros-consensus Storage/ImmutableDB/Impl):
  NNNNN.chunk      the stored blocks of chunk N back to back (chunk.pack_chunk layout:
                   [6, [header, [], [], {}, []]]);
  NNNNN.secondary  one 56-byte big-endian Entry per block (Index/Secondary.hs:93-128):
                   blockOffset u64, headerOffset u16, headerSize u16, checksum u32
                   (CRC32 of the block bytes), headerHash 32, blockOrEBB = slot u64;
  NNNNN.primary    version byte 1, then u32 BE secondary offsets, one per relative slot
                   plus one (Index/Primary.hs:104-160; relative slot 0 is the EBB slot).
A block of slot s lives in chunk s // chunk_slots (ChunkInfo with a uniform chunk size).

make_multi_epoch_chain forges a linked chain across several epochs: per epoch the
first-leader-wins schedule under that epoch's nonce (praos_leader_schedule), signed
with hbPrev = headerHash of the previous block and consecutive block numbers, and the
next epoch nonce taken from the chain state folded over the epoch (tickChainDepState:
candidate ⭒ lastEpochBlock, Praos.hs:407-431).
"""
import hashlib
import os
import zlib

import numpy as np

from . import chains
from .chunk import HEADER_OFFSET, pack_chunk

ENTRY = 56


def write_immutable(path, arena, off, length, slots, header_hash, chunk_slots):
    """arena/off/length: pack_chunk output (off/length = the headers inside their blocks).
    Returns the number of chunk files written."""
    os.makedirs(path, exist_ok=True)
    n = len(off)
    slots = np.asarray(slots, np.uint64)
    bstart = off.astype(np.int64) - HEADER_OFFSET
    bend = np.append(bstart[1:], len(arena)) if n else bstart
    chunk_of = (slots // np.uint64(chunk_slots)).astype(np.int64)
    last = int(chunk_of[-1]) if n else -1
    for c in range(last + 1):
        rows = np.nonzero(chunk_of == c)[0]
        data, sec = bytearray(), bytearray()
        prim = [0] * (chunk_slots + 2)
        for i in rows:
            blk = arena[bstart[i]:bend[i]].tobytes()
            sec += (len(data).to_bytes(8, "big") + HEADER_OFFSET.to_bytes(2, "big") +
                    int(length[i]).to_bytes(2, "big") + zlib.crc32(blk).to_bytes(4, "big") +
                    bytes(header_hash[i]) + int(slots[i]).to_bytes(8, "big"))
            data += blk
            rel = 1 + int(slots[i]) - c * chunk_slots        # relative slot (0 = EBB)
            prim[rel + 1] = len(sec)
        for k in range(1, len(prim)):                        # empty slots repeat the offset
            prim[k] = max(prim[k], prim[k - 1])
        with open(os.path.join(path, f"{c:05d}.chunk"), "wb") as f:
            f.write(data)
        with open(os.path.join(path, f"{c:05d}.secondary"), "wb") as f:
            f.write(sec)
        with open(os.path.join(path, f"{c:05d}.primary"), "wb") as f:
            f.write(b"\x01" + b"".join(x.to_bytes(4, "big") for x in prim))
    return last + 1


def read_secondary(path, chunk):
    """Entries of one secondary index as a list of dicts (for tests and tools)."""
    raw = open(os.path.join(path, f"{chunk:05d}.secondary"), "rb").read()
    out = []
    for k in range(0, len(raw), ENTRY):
        e = raw[k:k + ENTRY]
        out.append({"block_offset": int.from_bytes(e[0:8], "big"), "header_offset": int.from_bytes(e[8:10], "big"),
                    "header_size": int.from_bytes(e[10:12], "big"), "checksum": int.from_bytes(e[12:16], "big"),
                    "header_hash": e[16:48], "slot": int.from_bytes(e[48:56], "big")})
    return out


def _combine(a, b):
    if a is None:
        return b
    if b is None:
        return a
    return hashlib.blake2b(a + b, digest_size=32).digest()


def make_multi_epoch_chain(ctx, cfg, epochs, epoch_length, stability_window, tpraos=False, extra_entropy=None,
                           progress=None, schedules=None, stakes=None):
    """A linked chain over `epochs` epochs of `epoch_length` slots from slot 0 (Origin,
    GenesisHash, epoch 0 nonce = cfg["eta0"]).  Returns dict(arena, off, len, slots,
    header_hash, pools, params, nonces (per epoch), state (after the last
    block, as Context.update_chain_dep_state keeps it)).  tpraos=True: a Shelley..Alonzo
    chain (TPraos leader schedule and BHeaders, stored as Alonzo blocks, era tag 5; the
    TPraos nonce rules with TICKN's extra_entropy).  schedules: {epoch: (slots, pools)} used
    instead of the leader-schedule search for those epochs (e.g. epoch 0 of the C5 / tp chain
    from its shipped schedule, which was searched under the same seed, stake and nonce).
    stakes: a function epoch -> per-pool Fixed E34 stake (0 = the pool is not in that epoch's
    PoolDistr), so the stake distribution changes between epochs as the ledger's NEWEPOCH makes
    it (the leader schedule of epoch e is searched under epoch e's stake); the result then has
    "views": [(epoch, pool list)] -- the LedgerView's PoolDistr per epoch."""
    sig0 = chains.stake(cfg["npools"], cfg["stake_offset"])
    views, used = [], []
    p = chains.params(cfg)
    st = {"last_slot": None, "counters": {}, "evolving": cfg["eta0"], "candidate": cfg["eta0"],
          "epoch_nonce": cfg["eta0"], "lab": None, "leb": None}
    ei = (0, 0, epoch_length, stability_window)
    eta = cfg["eta0"]
    parts, nonces, slots_all, hh_all = [], [], [], []
    prev, block_no, pool_list = None, 0, None
    for e in range(epochs):
        if e > 0:
            eta = _combine(st["candidate"], st["leb"])      # the tick into epoch e
            if tpraos:
                eta = _combine(eta, extra_entropy)          # TICKN
        nonces.append(eta)
        sig = list(stakes(e)) if stakes else sig0
        if schedules and e in schedules:
            sl, pl = schedules[e]
            keep = (sl >= e * epoch_length) & (sl < (e + 1) * epoch_length)
            sl, pl = sl[keep].astype(np.uint64), pl[keep].astype(np.uint32)
        elif cfg.get("round_robin"):
            # f = 1 (every pool a leader in every slot, checkLeaderNatValue's f == 1 case):
            # a block in every slot, forged by the pools in turn -- a dense chain of the C5
            # shape (432k headers per 432k-slot epoch) without the 26e9-evaluation search
            assert cfg["f"] == 1, "round_robin schedules are leader-valid only for f = 1"
            sl = np.arange(e * epoch_length, (e + 1) * epoch_length, dtype=np.uint64)
            pl = (sl % cfg["npools"]).astype(np.uint32)
        else:
            lead = ctx.leader_schedule(cfg["seed"], sig, p, eta, e * epoch_length, epoch_length, tpraos=tpraos)
            idx = np.nonzero(lead >= 0)[0]
            sl = (e * epoch_length + idx).astype(np.uint64)
            pl = lead[idx].astype(np.uint32)
        n = len(sl)
        used.append((sl, pl))
        H, keys, _ = ctx.synthesize(n, cfg["npools"], p, eta, cfg["seed"], body_len=0, schedule=(sl, pl),
                                    block_no0=block_no, link=True, prev0=prev, tpraos=tpraos)
        pool_list = [(h, v, s) for (h, v), s in zip(keys, sig) if s > 0]
        views.append((e, pool_list))
        # fold the clean chain to learn the next nonce (the generator's own ledger)
        ctx.set_epoch(eta, pool_list, p)
        o = ctx.verify_tpraos_headers(H) if tpraos else ctx.verify_headers(H)
        prev_hash = np.zeros((n, 32), np.uint8)
        gen = np.zeros(n, np.uint8)
        if prev is None:
            gen[0] = 1
        else:
            prev_hash[0] = np.frombuffer(prev, np.uint8)
        prev_hash[1:] = H["header_hash"][:-1]
        if tpraos:
            _, _, stop, _ = ctx.tpraos_update_chain_dep_state(H, o, prev_hash, st, ei, prev_is_genesis=gen,
                                                              extra_entropy=extra_entropy)
        else:
            _, stop, _ = ctx.update_chain_dep_state(H, o, prev_hash, st, ei, prev_is_genesis=gen)
        if stop != n:
            raise RuntimeError(f"epoch {e}: generated header {stop} does not validate")
        parts.append(H)
        slots_all.append(sl)
        hh_all.append(H["header_hash"])
        prev = bytes(H["header_hash"][-1])
        block_no += n
        if progress:
            progress(e, n)
    # one stored-bytes arena over all epochs
    arenas, offs, lens, base = [], [], [], 0
    for H in parts:
        a, o_, l_ = pack_chunk(H, era_tag=5 if tpraos else 6)
        arenas.append(a)
        offs.append(o_ + np.uint64(base))
        lens.append(l_)
        base += len(a)
    return {"arena": np.concatenate(arenas), "off": np.concatenate(offs), "len": np.concatenate(lens),
            "slots": np.concatenate(slots_all), "header_hash": np.concatenate(hh_all), "pools": pool_list,
            "params": p, "nonces": nonces, "state": st,
            "epoch_info": ei, "views": views, "schedules": used}


def read_index(path, chunk):
    """(.secondary bytes or None, checksums, block offsets) of one chunk; an index file whose
    size is no multiple of the entry size counts as missing, as the reference treats an
    invalid index."""
    p = os.path.join(path, f"{chunk:05d}.secondary")
    if not os.path.exists(p):
        return None, None, None
    raw = open(p, "rb").read()
    if len(raw) % ENTRY:
        return None, None, None
    e = np.frombuffer(raw, np.uint8).reshape(-1, ENTRY)
    crc = e[:, 12:16].copy().view(">u4").reshape(-1).astype(np.uint32)
    off = e[:, 0:8].copy().view(">u8").reshape(-1).astype(np.uint64)
    return raw, crc, off


def chunk_report(chunk, res, sec, prev_tip):
    """One row of validate_immutable from a parse result (Context.validate_chunk's dict):
    the cross-chunk fit (Validation.hs:389-399: the first block's prevHash against the tip
    before this chunk, None = Origin), the outcome, and whether the rebuilt entries are the
    secondary file's bytes (Validation.hs:412-420).  Returns (row, tip after the chunk)."""
    fits = True
    if res["blocks"]:
        if prev_tip is None:
            fits = bool(res["prev_is_genesis"][0])
        else:
            fits = not res["prev_is_genesis"][0] and bytes(res["prev_hash"][0]) == prev_tip
    row = {"chunk": chunk, "outcome": res["outcome"], "blocks": res["blocks"], "checked": res["checked"],
           "truncate_at": res["truncate_at"], "integrity_bits": res["integrity_bits"], "fits": fits,
           "entries_match": sec is not None and res["entries"] == sec, "entries": res["entries"]}
    tip = res["entries"][-40:-8] if res["blocks"] else prev_tip
    return row, tip


def validate_immutable(ctx, path, slots_per_kes_period, parse=None, byron=None):
    """validateAllChunks over NNNNN.chunk / NNNNN.secondary (Validation.hs:150-260): one
    praos_validate_chunk call per chunk file, in order, with the index's checksums and block
    offsets when the index is there.  Returns one chunk_report row per chunk; stops after the
    first chunk that has an error or does not fit its predecessor, where the reference
    truncates.  parse: the parser (default ctx.validate_chunk), for checkers.  byron: None, or
    (epoch_slots, protocol_magic) for a database that starts at genesis (without it the first
    Byron chunk is UNSUPPORTED)."""
    parse = parse or (lambda data, crc, off: ctx.validate_chunk(data, crc, off, slots_per_kes_period, byron=byron))
    chunks = sorted(int(f[:5]) for f in os.listdir(path) if f.endswith(".chunk"))
    rows, tip = [], None
    for c in chunks:
        data = np.fromfile(os.path.join(path, f"{c:05d}.chunk"), np.uint8)
        sec, crc, off = read_index(path, c)
        row, tip = chunk_report(c, parse(data, crc, off), sec, tip)
        rows.append(row)
        if row["outcome"] != 0 or not row["fits"]:
            break
    return rows


def validate_byron_headers(ctx, path, params, delegs, state=None, tip=None):
    """Byron header validation (validateHeader: the envelope, then PBFT updateChainDepState) over
    a database directory, one verify + fold per chunk (Context.validate_pbft_headers), state and tip
    carried across chunks.  Header spans come from the secondary index (blockOffset + headerOffset,
    headerSize); the EBB flag from the stored block's two prefix bytes (82 00 an EBB, 82 01 a main
    block: the nested context of Byron/Ledger/Serialisation.hs).  params: Context.pbft_params;
    delegs: [(genesis key hash, delegate key hash)], one delegation map per call (the caller splits
    at a re-delegation).  Stops at the first invalid header.  Returns a dict: headers (validated),
    stop (None, or (chunk, index in the chunk, verdict, aux) of the first invalid header), tip and
    state (those before it), rows (per chunk: chunk, headers, chain_stop)."""
    chunks = sorted(int(f[:5]) for f in os.listdir(path) if f.endswith(".chunk"))
    state = list(state or ())
    out = {"headers": 0, "stop": None, "rows": []}
    for c in chunks:
        data = np.fromfile(os.path.join(path, f"{c:05d}.chunk"), np.uint8)
        ents = read_secondary(path, c)
        if not ents:
            continue
        off = np.array([e["block_offset"] + e["header_offset"] for e in ents], np.uint64)
        ln = np.array([e["header_size"] for e in ents], np.uint32)
        boff = np.array([e["block_offset"] for e in ents], np.int64)
        if (boff + 2 > len(data)).any():
            raise ValueError(f"chunk {c}: a block offset of the secondary index is outside the chunk file")
        is_ebb = (data[boff + 1] == 0).astype(np.uint8)
        _, v, aux, stop, tip, state = ctx.validate_pbft_headers(data, off, ln, is_ebb, params, delegs, tip, state)
        out["rows"].append({"chunk": c, "headers": len(ents), "chain_stop": stop})
        out["headers"] += stop
        if stop != len(ents):
            out["stop"] = (c, stop, int(v[stop]), int(aux[stop]))
            break
    out["tip"], out["state"] = tip, state
    return out
