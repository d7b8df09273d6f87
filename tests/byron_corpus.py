"""A small Byron forger for the chunk-validation tests (test infrastructure).

EBBs and main blocks in their stored form (byron_model's shapes), all main blocks signed by one
delegate key: the PBFT signature is the oracle's Ed25519 over byron_model.signed_message, the
proof's dlgHash / updHash / nTx / witHash / txRoot are computed from the block's own body, so a
forged block passes verifyBlockIntegrity.  Chosen per block: the number of transactions and
their sizes, a definite or indefinite txPayload list, and the length of an attribute in the
header's extra data (which sets the length of the signed message).  Blocks keep their parts,
so one can be re-signed with other fields."""
import cbor_header as ch
import oracle as orc
from helpers import rbytes

import byron_model as bm

H = ch._head
PM = 764824073
EPOCH_SLOTS = 40


def item(r, size):
    """One well-formed CBOR item of exactly `size` bytes."""
    if size == 1:
        return b"\x00"
    for n in (size - 1, size - 2, size - 3):
        if n >= 0 and len(H(2, n)) + n == size:
            return H(2, n) + rbytes(r, n)
    return b"\x81" + item(r, size - 1)


class Delegate:
    def __init__(self, r):
        self.seed = rbytes(r, 32)
        self.xpub = orc.ed25519_pk(self.seed) + rbytes(r, 32)       # key || chain code
        self.issuer = rbytes(r, 64)
        self.cert = H(4, 4) + H(0, 0) + H(2, 64) + self.issuer + H(2, 64) + self.xpub + H(2, 64) + rbytes(r, 64)


class Main:
    kind = 1

    def __init__(self, r, dlg, prev, epoch, sie, difficulty, tx_sizes=(), indef=False, attr_len=0, pm=PM):
        self.dlg, self.pm, self.prev, self.epoch, self.sie, self.difficulty = dlg, pm, prev, epoch, sie, difficulty
        self.txs = [(item(r, s), H(4, 1) + H(2, 9) + rbytes(r, 9)) for s in tx_sizes]
        self.indef, self.attr_len = indef, attr_len
        self.attr = rbytes(r, 700)
        self.ssc = H(4, 2) + H(0, 0) + H(2, 12) + rbytes(r, 12)
        self.ssc_proof = H(4, 3) + H(0, 0) + H(2, 32) + rbytes(r, 32) + H(2, 32) + rbytes(r, 32)
        self.dlg_payload = b"\x9f\xff" if indef else H(4, 0)
        self.upd = H(4, 2) + H(4, 0) + H(4, 0)
        self.extra_proof = rbytes(r, 32)
        self.block_extra = H(4, 1) + H(5, 0)
        self.bad_root = False       # sign over a txRoot that is not the body's (everything else holds)
        self.sign()

    def tx_payload(self):
        pairs = b"".join(H(4, 2) + t + w for t, w in self.txs)
        return (b"\x9f" + pairs + b"\xff") if self.indef else (H(4, len(self.txs)) + pairs)

    def extra(self):
        return (H(4, 4) + H(4, 3) + H(0, 1) + H(0, 0) + H(0, 0) + H(4, 2) + H(3, 4) + b"test" + H(0, 7) +
                H(5, 1) + H(0, 0) + H(2, self.attr_len) + self.attr[:self.attr_len] + H(2, 32) + self.extra_proof)

    def sign(self, sig=None):
        """(Re)build the bytes from the parts: proof from the body, signature over the message."""
        wit = bm.b2b(b"\x9f" + b"".join(w for _, w in self.txs) + b"\xff")
        root = bm.merkle_root([bm.b2b(b"\x00" + t) for t, _ in self.txs])
        if self.bad_root:
            root = bytes([root[0] ^ 0x10]) + root[1:]
        self.proof = (H(4, 4) + H(4, 3) + H(0, len(self.txs)) + H(2, 32) + root + H(2, 32) + wit + self.ssc_proof +
                      H(2, 32) + bm.b2b(self.dlg_payload) + H(2, 32) + bm.b2b(self.upd))
        prev_item = H(2, 32) + self.prev
        slotid = H(4, 2) + H(0, self.epoch) + H(0, self.sie)
        diff = H(4, 1) + H(0, self.difficulty)
        self.message = (b"01" + self.dlg.issuer + b"\x09" + bm.cbor_uint(self.pm) + b"\x85" + prev_item + self.proof +
                        slotid + diff + self.extra())
        self.sig = orc.ed25519_sign(self.dlg.seed, self.message) if sig is None else sig
        consensus = (H(4, 4) + slotid + H(2, 64) + self.dlg.issuer + diff +
                     H(4, 2) + H(0, 2) + H(4, 2) + self.dlg.cert + H(2, 64) + self.sig)
        self.header = H(4, 5) + H(0, self.pm) + prev_item + self.proof + consensus + self.extra()
        self.body = H(4, 4) + self.tx_payload() + self.ssc + self.dlg_payload + self.upd
        self.bytes = H(4, 2) + H(0, 1) + H(4, 3) + self.header + self.body + self.block_extra
        self.header_hash = bm.b2b(b"\x82\x01" + self.header)
        return self

    def fit_message(self, target, mod=128, base=0):
        """Choose attr_len so that (base + len(signed message)) % mod == target."""
        for n in range(600):
            self.attr_len = n
            self.sign(sig=bytes(64))
            if (base + len(self.message)) % mod == target:
                return self.sign()
        raise ValueError("no attribute length fits")


class EBB:
    kind = 0

    def __init__(self, r, prev, epoch, difficulty, n_ids=3, pm=PM):
        self.pm, self.prev, self.epoch, self.difficulty = pm, prev, epoch, difficulty
        self.ids = [rbytes(r, 28) for _ in range(n_ids)]
        self.sign()

    def sign(self):
        self.body = H(4, len(self.ids)) + b"".join(H(2, 28) + i for i in self.ids)
        self.header = (H(4, 5) + H(0, self.pm) + H(2, 32) + self.prev + H(2, 32) + bm.b2b(self.body) +
                       H(4, 2) + H(0, self.epoch) + H(4, 1) + H(0, self.difficulty) + H(4, 1) + H(5, 0))
        self.bytes = H(4, 2) + H(0, 0) + H(4, 3) + self.header + self.body + H(4, 1) + H(5, 0)
        self.header_hash = bm.b2b(b"\x82\x00" + self.header)
        return self


def make_chain(r, plan, dlg=None, genesis=None, epoch0=0, difficulty0=0, prev=None):
    """plan: per epoch a list of main-block keyword dicts (tx_sizes, indef, attr_len, fit=(target, base));
    every epoch opens with an EBB that shares slot epoch * EPOCH_SLOTS with its first main block.
    An EBB keeps the difficulty of the block before it, a main block adds one."""
    dlg = dlg or Delegate(r)
    out, diff = [], difficulty0
    prev = prev if prev is not None else (genesis or rbytes(r, 32))
    for e, mains in enumerate(plan):
        ebb = EBB(r, prev, epoch0 + e, diff, n_ids=mains[0].get("ebb_ids", 3) if mains else 3)
        out.append(ebb)
        prev = ebb.header_hash
        for k, kw in enumerate(mains):
            diff += 1
            b = Main(r, dlg, prev, epoch0 + e, k, diff, kw.get("tx_sizes", ()), kw.get("indef", False),
                     kw.get("attr_len", 0))
            if "fit" in kw:
                b.fit_message(kw["fit"][0], base=kw["fit"][1])
            out.append(b)
            prev = b.header_hash
    return out
