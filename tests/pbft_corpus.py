"""Byron header chains with several delegates (test infrastructure), built from byron_corpus.Main /
EBB: Main takes its delegate per block.  Headers are what the secondary index slices out of the
stored blocks (block.header), with the is_ebb byte of each."""
import numpy as np

import byron_corpus as bc
import pbft_model as pm

EPOCH_SLOTS = bc.EPOCH_SLOTS
PM = bc.PM


def delegation(r, delegates):
    """[(genesis key hash, delegate key hash)] for delegates: the genesis key is the delegate's
    issuer key, as in a heavy delegation certificate."""
    return [(pm.key_hash(d.issuer), pm.key_hash(d.xpub)) for d in delegates]


def make_chain(r, per_epoch, pick, epochs=3, genesis=True, prev=None, epoch0=0, difficulty0=0, slot_step=1, fit=None):
    """epochs x (one EBB + per_epoch main blocks); main block k of the chain is signed by
    pick(k) (a byron_corpus.Delegate) in slot-in-epoch j * slot_step.  The first EBB has the genesis
    hash as prev (genesis=True: epoch0 must be 0 for GenesisHash) or `prev`.  fit: {k: target} sets the
    signed message's length of main block k so that (64 + len) % 128 == target."""
    out, diff, k = [], difficulty0, 0
    prev = prev if prev is not None else bytes(r.getrandbits(8) for _ in range(32))
    for e in range(epochs):
        ebb = bc.EBB(r, prev, epoch0 + e, diff)
        out.append(ebb)
        prev = ebb.header_hash
        for j in range(per_epoch):
            diff += 1
            b = bc.Main(r, pick(k), prev, epoch0 + e, j * slot_step, diff)
            if fit and k in fit:
                b.fit_message(fit[k], base=64)
            out.append(b)
            prev = b.header_hash
            k += 1
    return out


def columns(blocks):
    """(arena u8[], off u64[], len u32[], is_ebb u8[]) of the blocks' headers, back to back with
    a few bytes between them (a header need not start on a word boundary)."""
    arena, off, ln = bytearray(), [], []
    for i, b in enumerate(blocks):
        arena += bytes(i % 5)
        off.append(len(arena))
        ln.append(len(b.header))
        arena += b.header
    return (np.frombuffer(bytes(arena), np.uint8).copy(), np.array(off, np.uint64), np.array(ln, np.uint32),
            np.array([int(b.kind == 0) for b in blocks], np.uint8))


def model_rows(blocks, delegs, epoch_slots=EPOCH_SLOTS, pm_cfg=PM, is_ebb=None):
    is_ebb = [int(b.kind == 0) for b in blocks] if is_ebb is None else is_ebb
    return [pm.verify_header(b.header, e, epoch_slots, pm_cfg, delegs) for b, e in zip(blocks, is_ebb)]


def rows_to_columns(rows):
    """model rows -> the column dict of Context.verify_pbft_headers"""
    n = len(rows)
    H = {"bits": np.array([r["bits"] for r in rows], np.uint8), "gk_idx": np.array([r["gk_idx"] for r in rows], np.int32),
         "slot": np.array([r["slot"] for r in rows], np.uint64),
         "block_no": np.array([r["block_no"] for r in rows], np.uint64),
         "prev_is_genesis": np.array([r["prev_is_genesis"] for r in rows], np.uint8)}
    for name, w in (("prev_hash", 32), ("header_hash", 32), ("delegate_hash", 28)):
        H[name] = np.frombuffer(b"".join(bytes(r[name]) for r in rows), np.uint8).reshape(n, w).copy()
    return H
