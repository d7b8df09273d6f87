"""Linked block chains for the chunk-validation tests (test infrastructure).

block_corpus.make_block's recipe (the oracle's encoders and signers, body hash = hashTxSeq of
the block's own segments, KES signature over the canonical body at t = max(0, kp - c0)) with
prev_hash = Blake2b-256 of the previous block's header span and consecutive block numbers, so
a chain written back to back is an intact chunk file.  Blocks keep their parts, so a block
can be re-signed with other fields; the test cases are mutations of one chain per module."""
import hashlib
import zlib

import block_corpus as bc
import block_integrity as bi
import cbor_header as ch
import oracle as orc
from helpers import rbytes

H = ch._head


class Block:
    def __init__(self, r, spkp, era, slot, block_no, prev, wrapped=True, pad=0):
        self.era, self.wrapped, self.spkp = era, wrapped, spkp
        self.tp = era in bi.TPRAOS_ERAS
        self.segs = bc.rand_segments(r, False, pad)
        self.seed = rbytes(r, 32)
        kp = slot // spkp
        self.f = {"block_no": block_no, "slot": slot, "prev_hash": prev, "cold_vk": rbytes(r, 32),
                  "vrf_vk": rbytes(r, 32), "vrf_out": rbytes(r, 64), "vrf_proof": rbytes(r, 80),
                  "body_size": sum(map(len, self.segs)),
                  "body_hash": bi._b2b(b"".join(bi._b2b(s) for s in self.segs)), "hot_vk": orc.kes_vk(self.seed),
                  "n": r.getrandbits(8), "c0": max(0, kp - r.randrange(3)), "ocert_sig": rbytes(r, 64),
                  "prot_major": 9 if not self.tp else era, "prot_minor": 0}
        if self.tp:
            self.f["leader_out"], self.f["leader_proof"] = rbytes(r, 64), rbytes(r, 80)
        self.sign()

    def sign(self):
        """(Re)build the bytes from the fields: header signed over the canonical body."""
        f = self.f
        body = ch.encode_tpraos_body(f) if self.tp else ch.encode_body(f)
        kp = f["slot"] // self.spkp
        kes = orc.kes_sign(self.seed, kp - f["c0"] if kp >= f["c0"] else 0, body)
        self.header = H(4, 2) + body + H(2, len(kes)) + kes
        inner = H(4, 1 + len(self.segs)) + self.header + b"".join(self.segs)
        self.bytes = (H(4, 2) + H(0, self.era) + inner) if self.wrapped else inner
        self.header_hash = hashlib.blake2b(self.header, digest_size=32).digest()
        return self

    def header_start(self):
        return self.bytes.index(self.header)


def make_chain(r, spkp, eras, pads=None, wrapped=True, slot0=1000):
    """Blocks of the given eras, linked; the first has a GenesisHash prev (None)."""
    out, prev = [], None
    for i, era in enumerate(eras):
        b = Block(r, spkp, era, slot0 + 20 * i + r.randrange(20), i, prev, wrapped, (pads or {}).get(i, 0))
        out.append(b)
        prev = b.header_hash
    return out


def layout(blobs):
    """-> (file bytes, offsets, CRCs) of the byte strings written back to back."""
    off, pos = [], 0
    for b in blobs:
        off.append(pos)
        pos += len(b)
    return b"".join(blobs), off, [zlib.crc32(b) for b in blobs]


def flip_segment_byte(blk):
    """One byte changed inside the segments so that the block is still one well-formed
    envelope: hashTxSeq no longer matches the header's body hash."""
    s0 = bc._seg_start(blk)
    for p in range(s0, len(blk)):
        m = blk[:p] + bytes([blk[p] ^ 0x01]) + blk[p + 1:]
        try:
            if bi.cbor_skip(m, 0, len(m)) == len(m) and bi.split_block(m, 0, len(m))[0]:
                return m
        except bi._Bad:
            pass
    raise ValueError("no flippable segment byte")


def flip_kes_byte(blk, k=7):
    i = blk.rfind(b"\x59\x01\xc0", 0, bc._seg_start(blk)) + 3 + k
    return blk[:i] + bytes([(blk[i] + 1) & 0xFF]) + blk[i + 1:]


def flip_header_byte(block):
    """A byte of the VRF proof: the header still decodes, its hash (and KES message) change."""
    blk = block.bytes
    i = blk.index(block.f["vrf_proof"]) + 11
    return blk[:i] + bytes([blk[i] ^ 0x40]) + blk[i + 1:]


def byron_item(r, n=60):
    return H(4, 2) + H(0, 0) + H(2, n) + rbytes(r, n)
