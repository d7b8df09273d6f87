"""Headers in the node-to-node encoding (what a ChainSync client receives).

Pure Python: ``wrap`` / ``unwrap`` of the wire wrapper, the rules of csrc/wire_scan.hpp restated
(the tests hold the two equal over a mutation corpus).

  Shelley-based eras   [eraIndex, #6.24(bytes)]              (decodeNS + CBOR-in-CBOR)
  Byron (era 0)        [0, [[kind, sizeHint], #6.24(bytes)]]   (kind 0 = EBB, 1 = main header)

GPU: ``unwrap_wire_headers(ctx, ...)`` (praos_unwrap_wire_headers) and ``validate_candidates(ctx,
...)`` (praos_validate_candidates), also reachable as ``Context.unwrap_wire_headers`` /
``Context.validate_candidates``; ``validate_candidates_pbft`` (praos_validate_candidates_pbft) is the
same call for fragments of Byron headers, ``validate_candidates_tpraos``
(praos_validate_candidates_tpraos) for fragments of TPraos headers.
"""
import ctypes

import numpy as np

from . import abi
from .abi import u8p, u32p, u64p

WIRE_OK, WIRE_RANGE, WIRE_SYNTAX, WIRE_ERA, WIRE_TRAILING = range(5)
NOT_BYRON = 0xFF
N_ERAS = 7                      # the reference's CardanoBlock: Byron .. Conway
PRAOS_ERAS = (1 << 5) | (1 << 6)
V_DOESNT_FIT = 25
V_NOT_REACHED = 255
NO_ROW = 0xFFFFFFFF


def head(major, value, width=0):
    """One CBOR head; width 0 = shortest, else the total size in bytes (1, 2, 3, 5 or 9)."""
    if width == 0:
        width = 1 if value < 24 else 2 if value < 256 else 3 if value < 65536 else 5 if value < 1 << 32 else 9
    if width == 1:
        assert value < 24
        return bytes([major << 5 | value])
    nb = {2: 1, 3: 2, 5: 4, 9: 8}[width]
    return bytes([major << 5 | {1: 24, 2: 25, 4: 26, 8: 27}[nb]]) + value.to_bytes(nb, "big")


def wrap(era, header, byron_kind=None, size_hint=0):
    """The wire item of a header's bytes.  Byron (era 0) needs byron_kind (0 EBB / 1 main) and the hint."""
    inner = head(6, 24) + head(2, len(header)) + bytes(header)
    if era == 0:
        return head(4, 2) + head(0, 0) + head(4, 2) + head(4, 2) + head(0, byron_kind) + head(0, size_hint) + inner
    return head(4, 2) + head(0, era) + inner


def _head(buf, pos, end, want):
    if pos >= end:
        return None
    ib = buf[pos]
    pos += 1
    if ib >> 5 != want:
        return None
    ai = ib & 31
    if ai < 24:
        return ai, pos
    if ai > 27:
        return None
    nb = 1 << (ai - 24)
    if nb > end - pos:
        return None
    return int.from_bytes(buf[pos:pos + nb], "big"), pos + nb


def unwrap(buf, pos=0, length=None, n_eras=N_ERAS):
    """(status, era, byron_kind, size_hint, off, len) of the wire item buf[pos:pos+length]; off / len
    are the inner header's span in buf (0, 0 unless the status is OK or TRAILING)."""
    length = len(buf) - pos if length is None else length
    if pos > len(buf) or length > len(buf) - pos:
        return (WIRE_RANGE, 0xFF, NOT_BYRON, 0, 0, 0)
    end = pos + length
    era, kind, hint = 0xFF, NOT_BYRON, 0

    def bad():
        return (WIRE_SYNTAX, era, kind, hint, 0, 0)
    r = _head(buf, pos, end, 4)
    if r is None or r[0] != 2:
        return bad()
    r = _head(buf, r[1], end, 0)
    if r is None or r[0] > 0xFF:
        return bad()
    era, p = r
    if era >= n_eras:
        return (WIRE_ERA, era, kind, hint, 0, 0)
    if era == 0:
        for _ in range(2):
            r = _head(buf, p, end, 4)
            if r is None or r[0] != 2:
                return bad()
            p = r[1]
        r = _head(buf, p, end, 0)
        if r is None or r[0] > 1:
            return bad()
        k, p = r
        r = _head(buf, p, end, 0)
        if r is None or r[0] > 0xFFFFFFFF:
            return bad()
        kind, hint, p = k, r[0], r[1]
    r = _head(buf, p, end, 6)
    if r is None or r[0] != 24:
        return bad()
    r = _head(buf, r[1], end, 2)
    if r is None or r[0] > end - r[1]:
        return bad()
    n, p = r
    return (WIRE_OK if p + n == end else WIRE_TRAILING, era, kind, hint, p, n)


# ---- the C ABI (include/praos_hip.h)
class WireOut(ctypes.Structure):
    _fields_ = [("status", u8p), ("era", u8p), ("byron_kind", u8p), ("size_hint", u32p), ("off", u64p),
                ("len", u32p), ("header_hash", u8p)]


class CandidatesIn(ctypes.Structure):
    _fields_ = [("items", abi.HeaderBytes), ("n_eras", ctypes.c_uint32), ("praos_eras", ctypes.c_uint32),
                ("view_end_slot", ctypes.c_uint64), ("ei", abi.EpochInfo), ("max_major_pv", ctypes.c_uint64),
                ("lv_prot_major", ctypes.c_uint64), ("max_header_size", ctypes.c_uint64),
                ("max_body_size", ctypes.c_uint64)]


class Fragment(ctypes.Structure):
    _fields_ = [("tip_is_origin", ctypes.c_int32), ("tip_slot", ctypes.c_uint64), ("tip_block_no", ctypes.c_uint64),
                ("tip_hash", ctypes.c_uint8 * 32), ("state", abi.ChainState), ("chain_stop", ctypes.c_size_t),
                ("processed", ctypes.c_size_t)]


class Fragments(ctypes.Structure):
    _fields_ = [("k", ctypes.c_size_t), ("frag_first", ctypes.POINTER(ctypes.c_size_t)),
                ("frag", ctypes.POINTER(Fragment))]


class CandidatesOut(ctypes.Structure):
    _fields_ = [("wire_status", u8p), ("row", u32p), ("verdict", u8p), ("rows_cap", ctypes.c_size_t),
                ("n_rows", ctypes.c_size_t), ("rows", abi.Out), ("dec", abi.Decoded), ("eta_idx", u8p),
                ("etas", ctypes.POINTER(abi.Nonce)), ("n_etas", ctypes.c_uint32), ("stats", ctypes.c_uint64 * 5)]


class TPraosCandidatesIn(ctypes.Structure):
    _fields_ = [("items", abi.HeaderBytes), ("n_eras", ctypes.c_uint32), ("tpraos_eras", ctypes.c_uint32),
                ("view_end_slot", ctypes.c_uint64), ("ei", abi.EpochInfo), ("max_major_pv", ctypes.c_uint64),
                ("lv_prot_major", ctypes.c_uint64), ("max_header_size", ctypes.c_uint64),
                ("max_body_size", ctypes.c_uint64), ("extra_entropy", ctypes.POINTER(abi.Nonce))]


class TPraosCandidatesOut(ctypes.Structure):
    _fields_ = [("wire_status", u8p), ("row", u32p), ("verdict", u8p), ("failures", abi.u16p),
                ("rows_cap", ctypes.c_size_t), ("n_rows", ctypes.c_size_t), ("rows", abi.TPOut), ("dec", abi.Decoded),
                ("leader_out", u8p), ("leader_proof", u8p), ("eta_idx", u8p), ("etas", ctypes.POINTER(abi.Nonce)),
                ("n_etas", ctypes.c_uint32), ("stats", ctypes.c_uint64 * 5)]


class PbftCandidatesIn(ctypes.Structure):
    _fields_ = [("items", abi.HeaderBytes), ("n_eras", ctypes.c_uint32), ("n_delegs", ctypes.c_uint32),
                ("view_end_slot", ctypes.c_uint64), ("params", abi.PbftParams), ("delegs", u8p)]


class PbftFragment(ctypes.Structure):
    _fields_ = [("tip", abi.PbftTip), ("state", abi.PbftStateC), ("chain_stop", ctypes.c_size_t),
                ("processed", ctypes.c_size_t)]


class PbftFragments(ctypes.Structure):
    _fields_ = [("k", ctypes.c_size_t), ("frag_first", ctypes.POINTER(ctypes.c_size_t)),
                ("frag", ctypes.POINTER(PbftFragment))]


class PbftCandidatesOut(ctypes.Structure):
    _fields_ = [("wire_status", u8p), ("row", u32p), ("verdict", u8p), ("aux", u64p), ("rows_cap", ctypes.c_size_t),
                ("n_rows", ctypes.c_size_t), ("rows", abi.PbftOut), ("row_is_ebb", u8p), ("stats", ctypes.c_uint64 * 4)]


STATS = ("items", "unwrapped", "distinct_headers", "rows", "extra_rows")
PBFT_STATS = ("items", "unwrapped", "distinct_headers", "sig_verifies")


def unwrap_wire_headers(ctx, arena, off, length, n_eras=N_ERAS, header_hash=True):
    """praos_unwrap_wire_headers over the wire items arena[off[i]:off[i]+len[i]]: a dict of arrays
    status, era, byron_kind, size_hint, off, len (the inner spans, into the same arena) and
    header_hash."""
    arena, off, length = ctx._chunk(arena, off, length)
    n = len(off)
    hb = ctx.header_bytes_struct(arena, off, length)
    O = {"status": np.zeros(n, np.uint8), "era": np.zeros(n, np.uint8), "byron_kind": np.zeros(n, np.uint8),
         "size_hint": np.zeros(n, np.uint32), "off": np.zeros(n, np.uint64), "len": np.zeros(n, np.uint32)}
    if header_hash:
        O["header_hash"] = np.zeros((n, 32), np.uint8)
    o = WireOut(abi.ptr(O["status"]), abi.ptr(O["era"]), abi.ptr(O["byron_kind"]), abi.ptr(O["size_hint"], u32p),
                abi.ptr(O["off"], u64p), abi.ptr(O["len"], u32p), abi.ptr(O.get("header_hash")))
    ctx.check(ctx.L.praos_unwrap_wire_headers(ctx.h, ctypes.byref(hb), n_eras, ctypes.byref(o)))
    return O


def validate_candidates(ctx, arena, off, length, frag_first, fragments, epoch_info, limits, view_end_slot=(1 << 64) - 1,
                        n_eras=N_ERAS, praos_eras=0, rows_cap=None, counter_cap=None, rows_out=True):
    """praos_validate_candidates.  fragments: one dict per fragment with "tip" (None = Origin, or (slot,
    block_no, hash32)) and "state" (the dict Context.update_chain_dep_state takes); both are updated
    in place and "chain_stop" / "processed" are added.  limits: (max_major_pv, lv_prot_major,
    max_header_size, max_body_size).  Returns a dict: wire_status, row, verdict (per item); n_rows,
    rows (praos_out arrays), dec (decoded columns), eta_idx (per row, cut to n_rows); etas (list of
    None / 32 bytes); stats.  A PraosError carries n_rows / n_etas of a refused call as attributes."""
    arena, off, length = ctx._chunk(arena, off, length)
    n, k = len(off), len(fragments)
    ff = (ctypes.c_size_t * (k + 1))(*[int(x) for x in frag_first])
    cin = CandidatesIn()
    cin.items = ctx.header_bytes_struct(arena, off, length)
    cin.n_eras, cin.praos_eras, cin.view_end_slot = n_eras, praos_eras, view_end_slot
    cin.ei = abi.EpochInfo(*epoch_info)
    cin.max_major_pv, cin.lv_prot_major, cin.max_header_size, cin.max_body_size = limits
    fr = (Fragment * max(k, 1))()
    keep = []
    for j, f in enumerate(fragments):
        tip = f["tip"]
        fr[j].tip_is_origin = int(tip is None)
        if tip is not None:
            fr[j].tip_slot, fr[j].tip_block_no = tip[0], tip[1]
            ctypes.memmove(fr[j].tip_hash, bytes(tip[2]), 32)
        nj = int(frag_first[j + 1]) - int(frag_first[j])
        cap = len(f["state"].get("counters", {})) + nj if counter_cap is None else counter_cap
        st, hk, cv = abi._state_struct(f["state"], cap)
        fr[j].state = st
        keep.append((hk, cv))
    fs = Fragments(k, ff, fr)
    cap = n if rows_cap is None else rows_cap
    ra = max(cap, 1) if rows_out else 0
    R = {"wire_status": np.zeros(n, np.uint8), "row": np.zeros(n, np.uint32), "verdict": np.zeros(n, np.uint8),
         "eta_idx": np.zeros(max(cap, 1), np.uint8)}
    out = CandidatesOut()
    out.wire_status, out.row, out.verdict = abi.ptr(R["wire_status"]), abi.ptr(R["row"], u32p), abi.ptr(R["verdict"])
    out.rows_cap = cap
    out.eta_idx = abi.ptr(R["eta_idx"])
    etas = (abi.Nonce * 256)()
    out.etas = etas
    if rows_out:
        R["rows"] = ctx.alloc_out(ra)
        out.rows = ctx.out_struct(R["rows"])
        R["dec"], out.dec = ctx.alloc_decoded(ra)
    rc = ctx.L.praos_validate_candidates(ctx.h, ctypes.byref(cin), ctypes.byref(fs), ctypes.byref(out))
    if rc != 0:
        msg = ctx.L.praos_last_error(ctx.h)
        e = abi.PraosError(f"praos rc={rc}: {msg.decode() if msg else ''}")
        e.rc, e.n_rows, e.n_etas = rc, int(out.n_rows), int(out.n_etas)
        raise e
    nr = int(out.n_rows)
    R["n_rows"] = nr
    R["eta_idx"] = R["eta_idx"][:nr]
    if rows_out:
        R["rows"] = {a: v[:nr] for a, v in R["rows"].items()}
        R["dec"] = {a: v[:nr] for a, v in R["dec"].items()}
    R["etas"] = [None if etas[e].neutral else bytes(etas[e].hash) for e in range(int(out.n_etas))]
    R["stats"] = dict(zip(STATS, (int(x) for x in out.stats)))
    for j, f in enumerate(fragments):
        f["tip"] = None if fr[j].tip_is_origin else (int(fr[j].tip_slot), int(fr[j].tip_block_no), bytes(fr[j].tip_hash))
        hk, cv = keep[j]
        new = abi._state_from_struct(fr[j].state, hk, cv)
        f["state"].clear()
        f["state"].update(new)
        f["chain_stop"], f["processed"] = int(fr[j].chain_stop), int(fr[j].processed)
    return R


TPRAOS_ERAS = (1 << 1) | (1 << 2) | (1 << 3) | (1 << 4)


def validate_candidates_tpraos(ctx, arena, off, length, frag_first, fragments, epoch_info, limits,
                               view_end_slot=(1 << 64) - 1, extra_entropy=None, n_eras=N_ERAS, tpraos_eras=0,
                               rows_cap=None, counter_cap=None, rows_out=True):
    """praos_validate_candidates_tpraos: validate_candidates for fragments of TPraos headers (wire
    indices 1 to 4).  extra_entropy: TICKN's (None = NeutralNonce, or 32 bytes).  Returns what
    validate_candidates returns, with failures (u16 per item) added, rows the praos_tpraos_out arrays
    (bits, pool_idx, beta_eta, beta_leader, nonce) and dec the TPraos decode (signed_body at
    TP_SIGNED_STRIDE, leader_out / leader_proof added)."""
    arena, off, length = ctx._chunk(arena, off, length)
    n, k = len(off), len(fragments)
    ff = (ctypes.c_size_t * (k + 1))(*[int(x) for x in frag_first])
    cin = TPraosCandidatesIn()
    cin.items = ctx.header_bytes_struct(arena, off, length)
    cin.n_eras, cin.tpraos_eras, cin.view_end_slot = n_eras, tpraos_eras, view_end_slot
    cin.ei = abi.EpochInfo(*epoch_info)
    cin.max_major_pv, cin.lv_prot_major, cin.max_header_size, cin.max_body_size = limits
    xe = None
    if extra_entropy is not None:
        xe = ctx.nonce_array([extra_entropy])
        cin.extra_entropy = xe
    fr = (Fragment * max(k, 1))()
    keep = []
    for j, f in enumerate(fragments):
        tip = f["tip"]
        fr[j].tip_is_origin = int(tip is None)
        if tip is not None:
            fr[j].tip_slot, fr[j].tip_block_no = tip[0], tip[1]
            ctypes.memmove(fr[j].tip_hash, bytes(tip[2]), 32)
        nj = int(frag_first[j + 1]) - int(frag_first[j])
        cap = len(f["state"].get("counters", {})) + nj if counter_cap is None else counter_cap
        st, hk, cv = abi._state_struct(f["state"], cap)
        fr[j].state = st
        keep.append((hk, cv))
    fs = Fragments(k, ff, fr)
    cap = n if rows_cap is None else rows_cap
    ra = max(cap, 1) if rows_out else 0
    R = {"wire_status": np.zeros(n, np.uint8), "row": np.zeros(n, np.uint32), "verdict": np.zeros(n, np.uint8),
         "failures": np.zeros(n, np.uint16), "eta_idx": np.zeros(max(cap, 1), np.uint8)}
    out = TPraosCandidatesOut()
    out.wire_status, out.row, out.verdict = abi.ptr(R["wire_status"]), abi.ptr(R["row"], u32p), abi.ptr(R["verdict"])
    out.failures = abi.ptr(R["failures"], abi.u16p)
    out.rows_cap = cap
    out.eta_idx = abi.ptr(R["eta_idx"])
    etas = (abi.Nonce * 256)()
    out.etas = etas
    if rows_out:
        R["rows"], out.rows = ctx.tp_out(ra)
        R["dec"], out.dec = ctx.alloc_decoded(ra, abi.TP_SIGNED_STRIDE)
        R["dec"]["leader_out"], R["dec"]["leader_proof"] = np.zeros((ra, 64), np.uint8), np.zeros((ra, 80), np.uint8)
        out.leader_out, out.leader_proof = abi.ptr(R["dec"]["leader_out"]), abi.ptr(R["dec"]["leader_proof"])
    rc = ctx.L.praos_validate_candidates_tpraos(ctx.h, ctypes.byref(cin), ctypes.byref(fs), ctypes.byref(out))
    if rc != 0:
        msg = ctx.L.praos_last_error(ctx.h)
        e = abi.PraosError(f"praos rc={rc}: {msg.decode() if msg else ''}")
        e.rc, e.n_rows, e.n_etas = rc, int(out.n_rows), int(out.n_etas)
        raise e
    nr = int(out.n_rows)
    R["n_rows"] = nr
    R["eta_idx"] = R["eta_idx"][:nr]
    if rows_out:
        R["rows"] = {a: v[:nr] for a, v in R["rows"].items()}
        R["dec"] = {a: v[:nr] for a, v in R["dec"].items()}
    R["etas"] = [None if etas[e].neutral else bytes(etas[e].hash) for e in range(int(out.n_etas))]
    R["stats"] = dict(zip(STATS, (int(x) for x in out.stats)))
    for j, f in enumerate(fragments):
        f["tip"] = None if fr[j].tip_is_origin else (int(fr[j].tip_slot), int(fr[j].tip_block_no), bytes(fr[j].tip_hash))
        hk, cv = keep[j]
        new = abi._state_from_struct(fr[j].state, hk, cv)
        f["state"].clear()
        f["state"].update(new)
        f["chain_stop"], f["processed"] = int(fr[j].chain_stop), int(fr[j].processed)
    del xe
    return R


def validate_candidates_pbft(ctx, arena, off, length, frag_first, fragments, params, delegs,
                             view_end_slot=(1 << 64) - 1, n_eras=N_ERAS, rows_cap=None, delegate_hash=False, rows_out=True):
    """praos_validate_candidates_pbft.  fragments: one dict per fragment with "tip" (None = Origin, or
    (slot, block_no, hash32, is_ebb)) and "state" (the window's signers, oldest first, as (slot,
    genesis key hash 28)), as Context.pbft_update_chain_dep_state takes them; both are replaced by
    those at the fragment's stop and "chain_stop" / "processed" are added.  params:
    Context.pbft_params; delegs: list of (genesis key hash 28, delegate key hash 28).  Returns a dict:
    wire_status, row, verdict, aux (per item); n_rows, rows (the praos_pbft_out columns) and
    row_is_ebb, cut to n_rows (rows_out=False: no per-row output is asked for); stats.  A PraosError
    carries n_rows of a refused call as an attribute."""
    arena, off, length = ctx._chunk(arena, off, length)
    n, k = len(off), len(fragments)
    ff = (ctypes.c_size_t * (k + 1))(*[int(x) for x in frag_first])
    d = ctx._pbft_delegs(delegs)
    cin = PbftCandidatesIn()
    cin.items = ctx.header_bytes_struct(arena, off, length)
    cin.n_eras, cin.n_delegs, cin.view_end_slot, cin.params = n_eras, len(d), view_end_slot, params
    cin.delegs = abi.ptr(d)
    fr = (PbftFragment * max(k, 1))()
    keep = []
    for j, f in enumerate(fragments):
        tip, state = f["tip"], list(f["state"])
        fr[j].tip.origin = 1
        if tip is not None:
            fr[j].tip.origin, fr[j].tip.slot, fr[j].tip.block_no, fr[j].tip.is_ebb = 0, int(tip[0]), int(tip[1]), int(bool(tip[3]))
            ctypes.memmove(fr[j].tip.hash, bytes(tip[2]), 32)
        cap = max(int(params.window_size), len(state), 1)
        ss, sh = np.zeros(cap, np.uint64), np.zeros((cap, 28), np.uint8)
        for q, (s, g) in enumerate(state):
            ss[q] = s
            sh[q] = np.frombuffer(bytes(g), np.uint8)
        fr[j].state = abi.PbftStateC(cap, len(state), abi.ptr(ss, u64p), abi.ptr(sh))
        keep.append((ss, sh))
    fs = PbftFragments(k, ff, fr)
    cap = n if rows_cap is None else rows_cap
    ra = max(cap, 1) if rows_out else 0
    R = {"wire_status": np.zeros(n, np.uint8), "row": np.zeros(n, np.uint32), "verdict": np.zeros(n, np.uint8),
         "aux": np.zeros(n, np.uint64), "row_is_ebb": np.zeros(ra, np.uint8)}
    R["rows"] = {name: np.zeros((ra,) + shp, dt) for name, dt, shp in abi.PBFT_OUT_FIELDS
                 if rows_out and (delegate_hash or name != "delegate_hash")}
    out = PbftCandidatesOut()
    out.wire_status, out.row, out.verdict = abi.ptr(R["wire_status"]), abi.ptr(R["row"], u32p), abi.ptr(R["verdict"])
    out.aux = abi.ptr(R["aux"], u64p)
    out.rows_cap = cap
    out.rows = ctx._pbft_out(R["rows"])
    out.row_is_ebb = abi.ptr(R["row_is_ebb"]) if rows_out else None
    rc = ctx.L.praos_validate_candidates_pbft(ctx.h, ctypes.byref(cin), ctypes.byref(fs), ctypes.byref(out))
    if rc != 0:
        msg = ctx.L.praos_last_error(ctx.h)
        e = abi.PraosError(f"praos rc={rc}: {msg.decode() if msg else ''}")
        e.rc, e.n_rows = rc, int(out.n_rows)
        raise e
    nr = int(out.n_rows)
    R["n_rows"] = nr
    R["rows"] = {a: v[:nr] for a, v in R["rows"].items()}
    R["row_is_ebb"] = R["row_is_ebb"][:nr]
    R["stats"] = dict(zip(PBFT_STATS, (int(x) for x in out.stats)))
    for j, f in enumerate(fragments):
        t = fr[j].tip
        ss, sh = keep[j]
        f["tip"] = None if t.origin else (int(t.slot), int(t.block_no), bytes(t.hash), int(t.is_ebb))
        f["state"] = [(int(ss[q]), bytes(sh[q])) for q in range(int(fr[j].state.n))]
        f["chain_stop"], f["processed"] = int(fr[j].chain_stop), int(fr[j].processed)
    return R


abi.Context.unwrap_wire_headers = unwrap_wire_headers
abi.Context.validate_candidates_tpraos = validate_candidates_tpraos
abi.Context.validate_candidates_pbft = validate_candidates_pbft
abi.Context.validate_candidates = validate_candidates
