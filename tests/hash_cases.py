"""Case lists of the stored-byte hash self tests (praos_debug_hash_bytes, include/praos_hip.h).

Every arena is random non-zero bytes, so an item's neighbours are never zero and a byte that a
tail mask fails to clear changes the digest; the last item of every list ends on the arena's last
byte, so the loads past an item run into the 16 zero bytes the upload appends.  The lists are
inputs only: tests/test_hash_cases.py checks what they cover, tests/test_gpu_hash_bytes.py runs
them, both against hashlib."""
import functools

import numpy as np

NT = 256                      # lanes of a k_seg_hash workgroup
MAX_LEN = 400                 # kinds 0 and 1: every length 0 .. MAX_LEN at every offset residue
FINAL_FILLS = (1, 111, 112, 113, 119, 120, 127, 128)   # the stream's fill after the 0x80 byte
LIT = 1 << 63                 # part table: b = LIT | k marks a literal of k bytes


def nonzero_bytes(seed, n):
    return np.random.default_rng(seed).integers(1, 256, n, dtype=np.uint8).tobytes()


class Layout:
    """Hands out arena ranges at chosen offset residues; the arena ends with the last range."""

    def __init__(self, start=8):
        self.cur = start      # kind 1 needs two bytes before its first range

    def place(self, length, residue):
        off = self.cur + (residue - self.cur) % 8
        self.cur = off + length
        return off

    def arena(self, seed):
        return nonzero_bytes(seed, self.cur)


# ---- kinds 0 and 1: b2b256_range, b2b256_pre

@functools.lru_cache(maxsize=None)
def range_cases():
    """(arena, off, len): every length 0..400 at every offset residue 0..7, 3,208 items.  The
    lengths start at 398 so the list ends with a ragged one (397 at residue 7)."""
    lay = Layout()
    off, ln = [], []
    for length in list(range(398, MAX_LEN + 1)) + list(range(398)):
        for residue in range(8):
            off.append(lay.place(length, residue))
            ln.append(length)
    return lay.arena(101), np.array(off, np.uint64), np.array(ln, np.uint32)


def range_messages():
    arena, off, ln = range_cases()
    return [arena[int(o):int(o) + int(n)] for o, n in zip(off, ln)]


@functools.lru_cache(maxsize=None)
def pre_cases(npre):
    """The same ranges with npre literal bytes in front, each the complement of the arena byte it
    replaces (never equal to it).  Returns (arena, off, len, aux (n, 4), messages)."""
    arena, off, ln = range_cases()
    aux = np.zeros((len(off), 4), np.uint8)
    msgs = []
    for i, (o, n) in enumerate(zip(off, ln)):
        o, n = int(o), int(n)
        pre = bytes(arena[o - npre + k] ^ 0xFF for k in range(npre))
        aux[i, 0] = npre
        aux[i, 1:1 + npre] = list(pre)
        msgs.append(pre + arena[o:o + n])
    return arena, off, ln, aux, msgs


# ---- kind 2: k_seg_hash

def _seg_case(name, seed, n, nseg, length_of):
    """length_of(k, i) -> (length, offset residue) of segment k of block i; only slots k < nseg[i]
    are placed.  Slot j = k * n + i sits in workgroup j // NT at lane j % NT."""
    lay = Layout()
    seg_off, seg_len = np.zeros(4 * n, np.uint64), np.zeros(4 * n, np.uint32)
    for k in range(4):
        for i in range(n):
            if k < nseg[i]:
                length, residue = length_of(k, i)
                seg_off[k * n + i] = lay.place(length, residue)
                seg_len[k * n + i] = length
    return {"name": name, "n": n, "arena": lay.arena(seed), "seg_off": seg_off, "seg_len": seg_len,
            "nseg": np.array(nseg, np.uint8)}


ROT_OTHERS = 16               # the rotation case: further active lanes per workgroup


@functools.lru_cache(maxsize=None)
def seg_cases():
    r = np.random.default_rng(202)
    ones, cases = [1] * NT, []
    # (a) lengths 0..255, then 256..511, lane t at offset residue t % 8
    cases.append(_seg_case("a_0_255", 210, NT, ones, lambda k, i: (i, i % 8)))
    cases.append(_seg_case("a_256_511", 211, NT, ones, lambda k, i: (256 + i, i % 8)))
    # (b) one long lane among short ones, at both ends of the first wave and of the workgroup (one
    # position per segment kind, so one launch holds the four workgroups); then the reverse
    at = (0, 63, 64, 255)
    cases.append(_seg_case("b_long_lane", 212, NT, [4] * NT, lambda k, i: (2000 if i == at[k] else 1, i % 8)))
    cases.append(_seg_case("b_short_lane", 213, NT, ones, lambda k, i: (1 if i == 128 else 2000, i % 8)))
    # (c) inactive lanes between active ones
    mixed = [int(x) for x in r.choice([0, 3, 4], NT)]
    lens_c = r.integers(0, 300, (4, NT))
    cases.append(_seg_case("c_nseg_mixed", 214, NT, mixed, lambda k, i: (int(lens_c[k, i]), (i + k) % 8)))
    # (d) 4n no multiple of the workgroup: one partial workgroup, and a full one plus four lanes
    cases.append(_seg_case("d_n1", 215, 1, [4], lambda k, i: ((0, 129, 128, 257)[k], 2 * k + 1)))
    lens_d = r.integers(0, 300, (4, 65))
    cases.append(_seg_case("d_n65", 216, 65, [4] * 65, lambda k, i: (int(lens_d[k, i]), (i + 3 * k) % 8)))
    # (e) every segment a whole number of message blocks
    cases.append(_seg_case("e_whole_blocks", 217, NT, [3] * NT, lambda k, i: (128 * (k + 1), i % 8)))
    # rotation: workgroup g (blocks 256 g ..) has its one longest segment (three message blocks) at
    # lane g and its one shortest (empty) at lane g + 1; ROT_OTHERS further lanes hold 1..127 bytes
    n = NT * NT
    nseg = np.zeros(n, np.uint8)
    length = {}
    for g in range(NT):
        length[g * NT + g] = 257
        length[g * NT + (g + 1) % NT] = 0
        for m in range(ROT_OTHERS):
            length.setdefault(g * NT + (g + 2 + 15 * m) % NT, 1 + (g + 29 * m) % 127)
    for i in length:
        nseg[i] = 1
    cases.append(_seg_case("rotation", 218, n, nseg, lambda k, i: (length[i], i % 8)))
    return cases


def seg_messages(case):
    """Expected input of every slot (None where inactive), segment-major."""
    n, arena = case["n"], case["arena"]
    out = []
    for j in range(4 * n):
        k, i = divmod(j, n)
        o, ln = int(case["seg_off"][j]), int(case["seg_len"][j])
        out.append(arena[o:o + ln] if k < case["nseg"][i] else None)
    return out


# ---- kinds 3 and 4: the register streams

@functools.lru_cache(maxsize=None)
def stream_cases():
    """(arena, items): an item is a list of parts, ("a", off, len) an arena range and ("l", bytes) a
    literal of 1..8 bytes."""
    lay = Layout()
    rot = [0]

    def rng_part(length):
        rot[0] += 1
        return ("a", lay.place(length, rot[0] % 8), length)

    lit_src = nonzero_bytes(300, 128 * 25 * 8)
    items, c = [], 0
    # at every fill 0..127: an arena part of 1..17 bytes and a literal of 1..8 bytes, after an arena
    # part of `fill` bytes (empty at fill 0) and before 0..20 more bytes, the tails in rotation
    for fill in range(128):
        for kind, length in [("a", k) for k in range(1, 18)] + [("l", k) for k in range(1, 9)]:
            it = [rng_part(fill)]
            it.append(rng_part(length) if kind == "a" else ("l", lit_src[8 * c:8 * c + length]))
            if c % 21:
                it.append(rng_part(c % 21))
            items.append(it)
            c += 1
    # totals that leave every named fill after the 0x80 byte, in one block and in two (fill 1 is
    # the empty message and a whole block, fill 128 is 127 and 255 bytes)
    for f in FINAL_FILLS:
        items.append([rng_part(f - 1)] if f > 1 else [])
        items.append([rng_part(64), ("l", lit_src[:8]), rng_part(f - 1 + 56)])
    # five blocks
    items.append([rng_part(300), ("l", lit_src[8:13]), rng_part(295)])
    return lay.arena(301), items


def stream_tables(items):
    """The item and part tables of praos_debug_hash_bytes kinds 3 and 4."""
    first, count, parts = [], [], []
    for it in items:
        first.append(len(parts))
        count.append(len(it))
        for p in it:
            if p[0] == "a":
                parts.append((p[1], p[2]))
            else:
                parts.append((int.from_bytes(p[1], "little"), LIT | len(p[1])))
    return np.array(first, np.uint64), np.array(count, np.uint32), np.array(parts, np.uint64).reshape(-1, 2)


def stream_messages():
    arena, items = stream_cases()
    return [b"".join(arena[p[1]:p[1] + p[2]] if p[0] == "a" else p[1] for p in it) for it in items]
