"""Case lists of the integer self tests (praos_debug_int and praos_debug_sc_reduce,
include/praos_hip.h): scalars mod L, the signed-digit recoders and the Fixed E34 helpers of the
leader check.  Pure Python and deterministic; every expected value is a Python integer
expression.  test_int_cases.py checks the coverage each list claims, test_gpu_int_layers.py runs
the lists on the device."""
import functools
import random

import numpy as np

L = 2 ** 252 + 27742317777372353535851937790883648493
R = 10 ** 34
M128, M253, M256, M512 = 2 ** 128, 2 ** 253, 2 ** 256, 2 ** 512


def pack(values, nbytes=32):
    """(n, nbytes) uint8, little-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(nbytes, "little") for v in values), np.uint8).reshape(-1, nbytes).copy()


def unpack(a):
    return [int.from_bytes(bytes(row), "little") for row in a]


# ---------------------------------------------------------------- Barrett reductions
def barrett(x, m, k):
    """Barrett reduction with 32-bit words as the device states it (b = 2^32, m below b^k, x below
    b^2k): q3 = ((x >> 32 (k - 1)) * mu) >> 32 (k + 1), mu = floor(b^2k / m).  Returns (floor(x / m),
    x mod m, the number of final subtractions of m)."""
    assert 0 <= x < 1 << (64 * k) and 1 << (32 * (k - 1)) <= m < 1 << (32 * k)
    mu = (1 << (64 * k)) // m
    q3 = ((x >> (32 * (k - 1))) * mu) >> (32 * (k + 1))
    r = x - q3 * m
    subs = r // m
    assert 0 <= subs <= 2 and q3 + subs == x // m
    return q3 + subs, r - subs * m, subs


def reduce512_model(x):
    return barrett(x, L, 8)


def div_R_model(x):
    return barrett(x, R, 4)


def _word_powers(bits):
    """2^k around every word boundary below `bits`, and the top bits"""
    ks = {1, 2, bits - 1, bits - 2}
    for w in range(32, bits, 32):
        ks |= {w - 1, w, w + 1}
    return sorted(k for k in ks if 0 < k < bits)


def _barrett_cases(m, k, seed, n_random, subs_of):
    top = 1 << (64 * k)
    r = random.Random(seed)
    qmax = (top - 1) // m
    qs = [0, 1, 2, qmax, qmax - 1] + [1 << j for j in range(2, qmax.bit_length())]
    rs = [0, 1, m - 2, m - 1] + [1 << j for j in _word_powers(m.bit_length() - 1)]
    out = [min(q * m + rem, top - 1) for q in qs for rem in rs]
    # the words the quotient estimate reads (x >> 32 (k - 1)) all ones, the rest anything
    low = 1 << (32 * (k - 1))
    ones = (top - 1) - (low - 1)
    out += [ones | v for v in [0, 1, low - 1] + [r.getrandbits(32 * (k - 1)) for _ in range(20)]]
    out.append(top - 1)
    # multiples of m and their neighbours
    for j in list(range(1, 21)) + [r.randrange(1, qmax) for _ in range(200)]:
        out += [j * m - 1, j * m, j * m + 1]
    out += [r.getrandbits(r.randrange(1, 64 * k + 1)) for _ in range(n_random)]
    # both outcomes of the final conditional subtraction, at least 100 times each
    count = {0: 0, 1: 0, 2: 0}
    for x in out:
        count[subs_of(x)] += 1
    while count[0] < 100 or count[1] < 100:
        x = r.getrandbits(64 * k)
        out.append(x)
        count[subs_of(x)] += 1
    return out


@functools.lru_cache(None)
def reduce512_cases():
    """Inputs of sc_reduce512 (praos_debug_sc_reduce): 64-byte values"""
    return _barrett_cases(L, 8, 0x5c512, 2000, lambda x: reduce512_model(x)[2])


@functools.lru_cache(None)
def div_R_cases():
    """Inputs of fx_div_R (op 7): any 256-bit value"""
    return _barrett_cases(R, 4, 0xf8d17, 2000, lambda x: div_R_model(x)[2])


@functools.lru_cache(None)
def reduce256_cases():
    """Inputs of sc_reduce256 (op 0)"""
    r = random.Random(0x5c256)
    out = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 15 * L - 1, 15 * L, 15 * L + 1, M256 - 1, 2 ** 252, 2 ** 255 - 1]
    out += [q * L + rem for q in range(16) for rem in (0, 1, L - 1) if q * L + rem < M256]
    return out + [r.getrandbits(r.randrange(1, 257)) for _ in range(500)]


# ---------------------------------------------------------------- sc_muladd, sc_is_canonical
MULADD_EDGES = (0, 1, 2, L - 1, L, L + 1, 2 ** 252, 2 ** 255 - 1, 2 ** 256 - 1)


@functools.lru_cache(None)
def muladd_cases():
    """(a, b, c) of sc_muladd (op 1); expected (a b + c) % L"""
    r = random.Random(0x3a1add)
    out = [(a, b, c) for a in MULADD_EDGES for b in MULADD_EDGES for c in MULADD_EDGES]
    return out + [(r.getrandbits(256), r.getrandbits(256), r.getrandbits(256)) for _ in range(500)]


def _words(x):
    return [(x >> (32 * i)) & 0xffffffff for i in range(8)]


@functools.lru_cache(None)
def canonical_cases():
    """Inputs of sc_is_canonical (op 2); expected x < L"""
    r = random.Random(0xca7071)
    out = [0, 1, L - 1, L, L + 1, 2 ** 252, 2 ** 253, M256 - 1]
    for i in range(8):
        for d in (1, -1):
            w = _words(L)
            w[i] = (w[i] + d) & 0xffffffff                                   # the word alone, wrapping
            out.append(sum(v << (32 * j) for j, v in enumerate(w)))
            if 0 <= L + d * 2 ** (32 * i) < M256:                            # the integer, borrowing
                out.append(L + d * 2 ** (32 * i))
    return out + [r.randrange(2 * L) for _ in range(200)]


# ---------------------------------------------------------------- recoders
# op -> (digit bits, digit count, bias, scalar bound, output words)
RECODERS = {3: (4, 64, 8, M253, 8), 4: (8, 32, 128, M253, 8), 5: (16, 16, 32768, M253, 8), 6: (6, 22, 32, M128, 5)}


def _repeat(field_values, width, bound):
    """the fields repeated from bit 0 up, cut to the bound"""
    v, i = 0, 0
    while width * i < bound.bit_length():
        v |= field_values[i % len(field_values)] << (width * i)
        i += 1
    return v & (bound - 1)


@functools.lru_cache(None)
def recode_cases(op):
    """Scalars of sc_recode16 / 256 / 65536 (ops 3 .. 5, below 2^253) and sc_recode64 (op 6, below
    2^128): the carry of the recoding runs through every digit, or through none"""
    r = random.Random(0x12ec0de + op)
    bound = RECODERS[op][3]
    if op == 6:
        pats = [_repeat(f, 6, bound) for f in ((31,), (32,), (63, 31), (0, 32), (63, 63, 31), (0, 0, 32), (63,), (31, 32))]
        out = [0, 1, M128 - 1] + pats
    else:
        pats = [_repeat(f, w, bound) for f, w in (((7,), 4), ((8,), 4), ((0x7f,), 8), ((0x80,), 8), ((0x7fff,), 16),
                                                  ((0x8000,), 16), ((0xf,), 4), ((7, 8), 4))]
        out = [0, 1, L - 1, M253 - 1] + pats
    return out + [r.getrandbits(r.randrange(1, bound.bit_length())) for _ in range(300)]


def recode_expected(op, s):
    """the recoded register: s plus the bias in every digit"""
    width, count, bias, bound, _ = RECODERS[op]
    assert 0 <= s < bound
    return s + sum(bias << (width * i) for i in range(count))


def digits(op, w):
    """the signed digits the consumers read from the recoded register w"""
    width, count, bias, _, _ = RECODERS[op]
    return [((w >> (width * i)) & ((1 << width) - 1)) - bias for i in range(count)]


def digits_value(op, ds):
    width = RECODERS[op][0]
    return sum(d * 2 ** (width * i) for i, d in enumerate(ds))


# ---------------------------------------------------------------- mp_div_small
DIV_KS = tuple(range(2, 1002)) + (32768, 32769, 65535)


@functools.lru_cache(None)
def div_small_cases():
    """(a, k) of mp_div_small (op 8); expected a // k"""
    r = random.Random(0xd17)
    out = []
    for k in DIV_KS:
        q = r.getrandbits(240) | 1 << 239
        out += [(a, k) for a in (0, k - 1, k, M256 - 1, q * k + (k - 1), r.getrandbits(256))]
    return out
