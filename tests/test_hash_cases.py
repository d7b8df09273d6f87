"""CPU: the case lists of the stored-byte hash self tests (hash_cases.py).  Every expected digest
is recomputed by a block-by-block Blake2b-256 and SHA-512 written out here and must equal
hashlib's (the reference the GPU tests compare with); the lists must cover what they are for."""
import hashlib
import struct

import hash_cases as hc

M64 = (1 << 64) - 1
B2B_IV = (0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1,
          0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179)
B2B_SIGMA = ((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15), (14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3),
             (11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4), (7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8),
             (9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13), (2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9),
             (12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11), (13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10),
             (6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5), (10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0))
B2B_MIX = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13),
           (3, 4, 9, 14))


def _ror(x, n):
    return ((x >> n) | (x << (64 - n))) & M64


def blake2b256(msg):
    """RFC 7693, unkeyed, 32-byte digest.  Returns (digest, number of compressions)."""
    h = list(B2B_IV)
    h[0] ^= 0x01010000 ^ 32
    nblk = max(1, (len(msg) + 127) // 128)
    for b in range(nblk):
        last = b + 1 == nblk
        m = struct.unpack("<16Q", msg[128 * b:128 * b + 128].ljust(128, b"\0"))
        v = h + list(B2B_IV)
        v[12] ^= len(msg) if last else 128 * (b + 1)
        if last:
            v[14] ^= M64
        for r in range(12):
            s = B2B_SIGMA[r % 10]
            for i, (a, b_, c, d) in enumerate(B2B_MIX):
                v[a] = (v[a] + v[b_] + m[s[2 * i]]) & M64
                v[d] = _ror(v[d] ^ v[a], 32)
                v[c] = (v[c] + v[d]) & M64
                v[b_] = _ror(v[b_] ^ v[c], 24)
                v[a] = (v[a] + v[b_] + m[s[2 * i + 1]]) & M64
                v[d] = _ror(v[d] ^ v[a], 16)
                v[c] = (v[c] + v[d]) & M64
                v[b_] = _ror(v[b_] ^ v[c], 63)
        h = [h[i] ^ v[i] ^ v[i + 8] for i in range(8)]
    return struct.pack("<4Q", *h[:4]), nblk


def _primes(n):
    out, c = [], 2
    while len(out) < n:
        if all(c % p for p in out):
            out.append(c)
        c += 1
    return out


def _root_frac(p, k):
    """the first 64 fractional bits of p^(1/k), by integer bisection"""
    lo, hi = 0, 1 << 70
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if mid ** k <= p << (64 * k) else (lo, mid)
    return lo & M64


SHA_K = [_root_frac(p, 3) for p in _primes(80)]
SHA_IV = [_root_frac(p, 2) for p in _primes(8)]


def sha512(msg):
    """FIPS 180-4.  Returns (digest, number of compressions)."""
    data = msg + b"\x80" + b"\0" * ((111 - len(msg)) % 128) + (8 * len(msg)).to_bytes(16, "big")
    h = list(SHA_IV)
    for b in range(0, len(data), 128):
        w = list(struct.unpack(">16Q", data[b:b + 128]))
        for t in range(16, 80):
            s0 = _ror(w[t - 15], 1) ^ _ror(w[t - 15], 8) ^ (w[t - 15] >> 7)
            s1 = _ror(w[t - 2], 19) ^ _ror(w[t - 2], 61) ^ (w[t - 2] >> 6)
            w.append((w[t - 16] + s0 + w[t - 7] + s1) & M64)
        a, b_, c, d, e, f, g, hh = h
        for t in range(80):
            t1 = (hh + (_ror(e, 14) ^ _ror(e, 18) ^ _ror(e, 41)) + ((e & f) ^ (~e & g)) + SHA_K[t] + w[t]) & M64
            t2 = ((_ror(a, 28) ^ _ror(a, 34) ^ _ror(a, 39)) + ((a & b_) ^ (a & c) ^ (b_ & c))) & M64
            a, b_, c, d, e, f, g, hh = (t1 + t2) & M64, a, b_, c, (d + t1) & M64, e, f, g
        h = [(x + y) & M64 for x, y in zip(h, (a, b_, c, d, e, f, g, hh))]
    return struct.pack(">8Q", *h), len(data) // 128


def _check_b2b(msgs):
    """every digest against hashlib; returns the set of block counts"""
    counts = set()
    for m in msgs:
        if m not in _checked:                                                 # kind 1 with npre = 0 repeats kind 0
            d, _checked[m] = blake2b256(m)
            assert d == hashlib.blake2b(m, digest_size=32).digest(), len(m)
        counts.add(_checked[m])
    return counts


_checked = {}


def _nonzero(arena):
    return 0 not in arena


def test_range_and_pre_cases():
    arena, off, ln = hc.range_cases()
    assert _nonzero(arena) and len(off) == 8 * 401 == 3208
    assert {(int(n), int(o) % 8) for o, n in zip(off, ln)} == {(n, r) for n in range(401) for r in range(8)}
    assert {(int(n) % 128, int(o) % 8) for o, n in zip(off, ln)} == {(n, r) for n in range(128) for r in range(8)}
    assert int(off[-1]) + int(ln[-1]) == len(arena) and ln[-1] % 8 != 0      # the last item ends the arena
    assert {1, 2, 3, 4} <= _check_b2b(hc.range_messages())
    for npre in (0, 1, 2):
        a2, off2, ln2, aux, msgs = hc.pre_cases(npre)
        assert a2 is arena and min(int(o) for o in off2) >= 2
        for o, n, x, m in zip(off2, ln2, aux, msgs):
            o, n = int(o), int(n)
            assert x[0] == npre and m == bytes(x[1:1 + npre]) + arena[o:o + n] and len(m) == n + npre
            assert all(m[k] != arena[o - npre + k] for k in range(npre))      # the literal differs from what it replaces
        assert any(n == 0 for n in ln2)                                       # len = 0 with every npre
        assert {1, 2, 3, 4} <= _check_b2b(msgs)


def test_seg_cases():
    longest, shortest, names = set(), set(), set()
    for case in hc.seg_cases():
        n, msgs = case["n"], hc.seg_messages(case)
        names.add(case["name"])
        assert _nonzero(case["arena"]) and len(msgs) == 4 * n
        ends = [int(o) + int(ln) for o, ln, m in zip(case["seg_off"], case["seg_len"], msgs) if m]
        assert max(ends) == len(case["arena"])
        _check_b2b([m for m in msgs if m is not None])
        for g in range(0, 4 * n, hc.NT):                                      # workgroup by workgroup
            act = [(len(m), t) for t, m in enumerate(msgs[g:g + hc.NT]) if m is not None]
            if not act:
                continue
            for j in range(g, min(g + hc.NT, 4 * n)):                         # lane t at offset residue t % 8
                assert msgs[j] is None or case["name"] in ("c_nseg_mixed", "d_n1", "d_n65") or \
                    int(case["seg_off"][j]) % 8 == (j % hc.NT) % 8
            lens = sorted(ln for ln, _ in act)
            if len(lens) > 1 and lens[-1] > lens[-2]:
                longest.add(max(act)[1])
            if len(lens) > 1 and lens[0] < lens[1]:
                shortest.add(min(act)[1])
    assert longest == shortest == set(range(hc.NT))
    by = {c["name"]: c for c in hc.seg_cases()}
    assert [int(x) for x in by["a_0_255"]["seg_len"][:256]] == list(range(256))
    assert [int(x) for x in by["a_256_511"]["seg_len"][:256]] == list(range(256, 512))
    assert sorted(int(x) for x in by["b_long_lane"]["seg_len"] if x > 1) == [2000] * 4
    assert [int(by["b_long_lane"]["seg_len"][256 * k + t]) for k, t in enumerate((0, 63, 64, 255))] == [2000] * 4
    assert sorted(int(x) for x in by["b_short_lane"]["seg_len"][:256])[:2] == [1, 2000]
    assert set(int(x) for x in by["c_nseg_mixed"]["nseg"]) == {0, 3, 4}
    nz = [int(x) > 0 for x in by["c_nseg_mixed"]["nseg"]]
    assert any(nz[i - 1] and not nz[i] and nz[i + 1] for i in range(1, 255))  # an inactive lane between active ones
    assert by["d_n1"]["n"] == 1 and by["d_n65"]["n"] == 65
    assert {int(x) for x in by["e_whole_blocks"]["seg_len"]} == {0, 128, 256, 384}


def test_stream_cases():
    arena, items = hc.stream_cases()
    msgs = hc.stream_messages()
    assert _nonzero(arena) and [] in items
    assert max(p[1] + p[2] for it in items for p in it if p[0] == "a") == len(arena)
    starts, splits, residues = set(), set(), set()
    for it in items:
        fill = 0
        for p in it:
            ln = p[2] if p[0] == "a" else len(p[1])
            assert p[0] == "a" or (1 <= ln <= 8 and 0 not in p[1])
            starts.add((p[0], fill % 128, ln))
            if p[0] == "a" and ln:
                residues.add(p[1] % 8)
            # the feeding loop: words of 8 bytes, then the rest; put() splits a word at the block's end
            for w in range(0, ln, 8):
                k, f = min(8, ln - w), (fill + w) % 128
                if f + k > 128:
                    splits.add(128 - f)
            fill += ln
    for fill in range(128):
        assert all(("a", fill, ln) in starts for ln in range(1, 18)), fill
        assert all(("l", fill, ln) in starts for ln in range(1, 9)), fill
    assert splits == set(range(1, 8)) and residues == set(range(8))
    assert {(len(m) + 1) % 128 or 128 for m in msgs} >= set(hc.FINAL_FILLS)
    for f in hc.FINAL_FILLS:                                                  # each in one block and in more
        assert {len(m) // 128 > 0 for m in msgs if ((len(m) + 1) % 128 or 128) == f} == {False, True}, f
    grid = items[:128 * 25]                                                   # 0..20 more bytes after the part
    assert {it[2][2] if len(it) == 3 else 0 for it in grid} == set(range(21))
    assert b"" in msgs and max((len(m) + 127) // 128 for m in msgs) == 5
    assert {1, 2, 5} <= _check_b2b(msgs)
    counts = set()
    for m in msgs:
        d, nblk = sha512(m)
        assert d == hashlib.sha512(m).digest(), len(m)
        counts.add(nblk)
    assert {1, 2, 3, 5} <= counts
    first, count, parts = hc.stream_tables(items)
    assert len(first) == len(items) and int(first[-1]) + int(count[-1]) == len(parts)
    assert all(int(b) < len(arena) or (int(b) ^ hc.LIT) in range(1, 9) for _, b in parts)
