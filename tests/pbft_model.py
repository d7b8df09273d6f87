"""Byron header validation restated in plain, sequential Python (the independent checker of
k_pbft.hip and praos_pbft.hip).

  hashVerKey        Blake2b-224(SHA3-256(58 40 || xpub64))                    (hashlib)
  decode            byron_model.parse_block's header shapes, the header wrapped as a block with an
                    empty body; is_ebb picks the shape, as the stored block's prefix does
  signature         the oracle's Ed25519 under the first 32 bytes of delegateXPub over "01" ||
                    issuerXPub || 09 || CBOR(configured pm) || 85 || the stored prev, proof,
                    slot-id, difficulty and extra items (Byron/Ledger/PBFT.hs:43-69)
  fold              validateEnvelope (HeaderValidation.hs:297-344, Byron instance
                    Byron/Ledger/HeaderValidation.hs:39-75), then PBFT updateChainDepState
                    (Protocol/PBFT.hs:320-353) with append (Protocol/PBFT/State.hs:206-228)
  codec             encodePBftState / decodePBftState (Protocol/PBFT/State.hs:277-305)
"""
import hashlib

import block_integrity as bi
import byron_model as bm
import oracle as orc

BIT_DECODE, BIT_SIG, BIT_NOT_DELEGATE = 1, 2, 4
V_OK, V_INPUT, V_ENV_BLOCK_NO, V_ENV_SLOT_NO, V_ENV_PREV_HASH = 0, 12, 13, 14, 15
V_INVALID_SIG, V_INVALID_SLOT, V_NOT_DELEGATE, V_EXCEEDED, V_EBB_IN_SLOT = 20, 21, 22, 23, 24
M64 = (1 << 64) - 1


def key_hash(xpub64):
    return hashlib.blake2b(hashlib.sha3_256(b"\x58\x40" + bytes(xpub64)).digest(), digest_size=28).digest()


def decode_header(hdr, is_ebb, epoch_slots):
    """One stored header -> dict of the columns, or None when it does not decode."""
    hdr = bytes(hdr)
    try:
        if bi.cbor_skip(hdr, 0, len(hdr)) != len(hdr):
            return None
    except bi._Bad:
        return None
    body = b"\x80" if is_ebb else b"\x84\x80\x80\x80\x80"
    blk = bytes([0x82, 0 if is_ebb else 1, 0x83]) + hdr + body + b"\x80"
    try:
        d = bm.parse_block(blk, 0, len(blk))
    except bm.Bad:
        return None
    if d is None:
        return None
    d["blk"] = blk
    d["slot"] = bm.point_slot(d, epoch_slots)
    return d


def signed_message(d, pm):
    blk = d["blk"]
    sp = lambda k: blk[d[k][0]:d[k][1]]
    return (b"01" + blk[d["issuer"]:d["issuer"] + 64] + b"\x09" + bm.cbor_uint(pm) + b"\x85" +
            sp("prev_span") + sp("proof_span") + sp("slotid_span") + sp("diff_span") + sp("extra_span"))


_sig_cache = {}


def verify_header(hdr, is_ebb, epoch_slots, pm, delegs):
    """praos_verify_pbft_headers' answer for one header: dict of bits, gk_idx, slot, block_no,
    prev_hash, prev_is_genesis, header_hash, delegate_hash.  delegs: [(genesis hash, delegate hash)]"""
    z = {"bits": BIT_DECODE, "gk_idx": -1, "slot": 0, "block_no": 0, "prev_hash": bytes(32), "prev_is_genesis": 0,
         "header_hash": bytes(32), "delegate_hash": bytes(28)}
    d = decode_header(hdr, is_ebb, epoch_slots)
    if d is None:
        return z
    z.update(bits=0, slot=d["slot"], block_no=d["block_no"], prev_hash=d["prev_hash"] or bytes(32),
             prev_is_genesis=int(d["prev_hash"] is None), header_hash=d["header_hash"])
    if is_ebb:
        return z
    blk = d["blk"]
    xpub = blk[d["delegate"]:d["delegate"] + 64]
    kh = key_hash(xpub)
    z["delegate_hash"] = kh
    for k, (_, dh) in enumerate(delegs):
        if bytes(dh) == kh:
            z["gk_idx"] = k
    if z["gk_idx"] < 0:
        z["bits"] |= BIT_NOT_DELEGATE
    msg, sig = signed_message(d, pm), blk[d["sig"]:d["sig"] + 64]
    key = (xpub[:32], msg, sig)
    if key not in _sig_cache:
        _sig_cache[key] = bool(orc.ed25519_verify(xpub[:32], msg, sig))
    if not _sig_cache[key]:
        z["bits"] |= BIT_SIG
    return z


def fold(rows, is_ebb, window_size, threshold, epoch_slots, delegs, tip=None, state=()):
    """praos_pbft_update_chain_dep_state.  rows: verify_header dicts; tip: None or (slot, block_no,
    hash, is_ebb); state: [(slot, genesis hash)] oldest first.  Returns (verdicts, aux, chain_stop,
    tip, state) with tip and state those at chain_stop."""
    win = [(int(s), bytes(g)) for s, g in state]
    verdicts, aux, stop, at_stop = [], [], len(rows), None
    for i, (h, ebb) in enumerate(zip(rows, is_ebb)):
        v, a = _one(h, bool(ebb), tip, win, window_size, threshold, epoch_slots, delegs)
        if v == V_OK:
            if not ebb:
                gk = bytes(delegs[h["gk_idx"]][0])
                full = len(win) == window_size          # the size before the append
                win = win + [(h["slot"], gk)]
                if full:
                    win = win[1:]
            tip = (h["slot"], h["block_no"], bytes(h["header_hash"]), int(bool(ebb)))
        elif at_stop is None:
            stop, at_stop = i, (tip, list(win))
        verdicts.append(v)
        aux.append(a)
    if at_stop is not None:
        tip, win = at_stop
    return verdicts, aux, stop, tip, win


def _one(h, ebb, tip, win, window_size, threshold, epoch_slots, delegs):
    if h["bits"] & BIT_DECODE:
        return V_INPUT, 0
    if tip is None:
        exp_bno, min_slot = 0, 0
    else:
        t_slot, t_bno, _, t_ebb = tip
        exp_bno = t_bno if (not t_ebb and ebb) else (t_bno + 1) & M64
        min_slot = t_slot if (t_ebb and not ebb) else (t_slot + 1) & M64
    if h["block_no"] != exp_bno:
        return V_ENV_BLOCK_NO, exp_bno
    if not h["slot"] >= min_slot:
        return V_ENV_SLOT_NO, min_slot
    if tip is None:
        prev_ok = bool(h["prev_is_genesis"])
    else:
        prev_ok = not h["prev_is_genesis"] and bytes(h["prev_hash"]) == tip[2]
    if not prev_ok:
        return V_ENV_PREV_HASH, 0
    if ebb:
        return (V_EBB_IN_SLOT, h["slot"]) if h["slot"] % epoch_slots else (V_OK, 0)
    if h["bits"] & BIT_SIG:
        return V_INVALID_SIG, 0
    if win and h["slot"] < win[-1][0]:
        return V_INVALID_SLOT, 0
    if h["gk_idx"] < 0:
        return V_NOT_DELEGATE, 0
    gk = bytes(delegs[h["gk_idx"]][0])
    after = win + [(h["slot"], gk)]
    if len(win) == window_size:
        after = after[1:]
    n = sum(1 for _, g in after if g == gk)
    if n > threshold:
        return V_EXCEEDED, n
    return V_OK, 0


def state_encode(state):
    inv = {}
    for s, g in state:
        inv.setdefault(bytes(g), []).insert(0, int(s))          # newest first
    out = b"\x82\x01" + bi_head(5, len(inv))
    for g in sorted(inv):
        out += b"\x58\x1c" + g + b"\x9f" + b"".join(bm.cbor_uint(s) for s in inv[g]) + b"\xff"
    return out


def bi_head(mt, v):
    return bytes([(mt << 5) | bm.cbor_uint(v)[0]]) + bm.cbor_uint(v)[1:]


def state_decode(data):
    """[1, {hash: [slots]}] -> [(slot, hash)] sorted by slot, stable over (key order, stored order)"""
    data = bytes(data)
    assert data[:2] == b"\x82\x01"
    mt, _, n, p = bi._head(data, 2, len(data))
    assert mt == 5 and n is not None
    ents = []
    for _ in range(n):
        assert data[p:p + 2] == b"\x58\x1c"
        g = data[p + 2:p + 30]
        mt, _, cnt, p = bi._head(data, p + 30, len(data))
        assert mt == 4
        slots = []
        while (cnt is None and data[p] != 0xFF) or (cnt is not None and len(slots) < cnt):
            mt, _, s, p = bi._head(data, p, len(data))
            assert mt == 0
            slots.append(s)
        if cnt is None:
            p += 1
        ents.append((g, slots))
    assert p == len(data)
    ents.sort(key=lambda e: e[0])
    flat = [(s, g) for g, slots in ents for s in slots]
    return sorted(flat, key=lambda x: x[0])
