"""CPU: the case lists of the integer self tests (int_cases.py) cover what they claim, checked on
the Python model alone.  Prints the case counts and the histograms of final subtractions of both
Barrett routines (pytest -s shows them; DESIGN.md quotes them)."""
from collections import Counter

import int_cases as ic

L, R = ic.L, ic.R


def test_constants():
    assert L == 2 ** 252 + 27742317777372353535851937790883648493 and R == 10 ** 34
    assert pow(2, L - 1, L) == 1 and L.bit_length() == 253 and R.bit_length() == 113


def _barrett_histogram(name, cases, model, m, top):
    hist = Counter()
    for x in cases:
        q, r, subs = model(x)
        assert 0 <= x < top and (q, r) == divmod(x, m)
        hist[subs] += 1
    print(f"{name}: {len(cases)} cases, final subtractions {dict(sorted(hist.items()))}")
    assert hist[0] >= 100 and hist[1] >= 100 and set(hist) <= {0, 1, 2}
    assert len(cases) < 20000
    return hist


def test_reduce512_cases():
    cases = ic.reduce512_cases()
    _barrett_histogram("sc_reduce512", cases, ic.reduce512_model, L, ic.M512)
    s = set(cases)
    qmax = (ic.M512 - 1) // L
    assert {0, 1, L - 2, L - 1, L, L + 1, 2 * L - 1, 2 * L, ic.M512 - 1, qmax * L, (qmax - 1) * L + L - 1} <= s
    assert all((1 << k) * L in s and (1 << k) * L + L - 1 in s for k in range(2, 260))
    assert sum(1 for x in cases if x >> 224 == 2 ** 288 - 1) >= 20           # top nine words all ones
    assert {x % L for x in cases} >= {0, 1, L - 2, L - 1} | {1 << k for k in (31, 32, 33, 223, 224, 225, 251)}
    assert len({x.bit_length() for x in cases}) >= 500                       # random bit lengths


def test_div_R_cases():
    cases = ic.div_R_cases()
    _barrett_histogram("fx_div_R", cases, ic.div_R_model, R, ic.M256)
    s = set(cases)
    qmax = (ic.M256 - 1) // R
    assert {0, 1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, ic.M256 - 1, qmax * R, qmax * R - 1} <= s
    assert all((1 << k) * R in s and (1 << k) * R + R - 1 in s for k in range(2, 143))
    assert sum(1 for x in cases if x >> 96 == 2 ** 160 - 1) >= 20            # top five words all ones
    assert max(x.bit_length() for x in cases) == 256


def test_reduce256_and_muladd_cases():
    assert {0, L - 1, L, L + 1, 15 * L, ic.M256 - 1} <= set(ic.reduce256_cases())
    assert all(0 <= x < ic.M256 for x in ic.reduce256_cases())
    cases = ic.muladd_cases()
    assert len(cases) == 729 + 500 and len(set(cases[:729])) == 729
    m = ic.M256 - 1
    assert (m, m, m) in cases and (0, 0, 0) in cases and (L, L, L) in cases
    assert all(0 <= v < ic.M256 for t in cases for v in t)
    assert m * m + m < ic.M512                                                # the largest a b + c fits sc_reduce512
    print(f"sc_reduce256: {len(ic.reduce256_cases())} cases; sc_muladd: {len(cases)} cases")


def test_canonical_cases():
    cases = ic.canonical_cases()
    s = set(cases)
    assert {0, 1, L - 1, L, L + 1, 2 ** 252, 2 ** 253, ic.M256 - 1} <= s
    lw = [(L >> (32 * i)) & 0xffffffff for i in range(8)]
    for i in range(8):                                                        # one word of L off by one, the others equal
        for d in (1, -1):
            assert any(all(((x >> (32 * j)) & 0xffffffff) == (lw[j] if j != i else (lw[i] + d) & 0xffffffff)
                           for j in range(8)) for x in cases), (i, d)
    # an input that differs from L only below the top word, on either side: a top-word compare alone decides it wrongly
    assert any(x >> 224 == L >> 224 and x > L for x in cases) and any(x >> 224 == L >> 224 and x < L for x in cases)
    assert 50 < sum(x < L for x in cases) < len(cases) - 50
    print(f"sc_is_canonical: {len(cases)} cases")


def test_recode_cases():
    for op, (width, count, bias, bound, nwords) in ic.RECODERS.items():
        cases = ic.recode_cases(op)
        assert {0, 1, bound - 1} <= set(cases) and all(0 <= s < bound for s in cases)
        carries = set()
        for s in cases:
            w = ic.recode_expected(op, s)
            assert w < 1 << (32 * nwords)
            ds = ic.digits(op, w)
            # what the consumers rely on: the signed digits are in the selectors' range and sum to s
            assert all(-bias <= d < bias for d in ds) and ic.digits_value(op, ds) == s
            assert w >> (width * count) == 0                                 # nothing above the last digit
            carries.add(sum(1 for d in ds if d < 0))
        assert {0, count - 1} <= carries or {0, count} <= carries, (op, sorted(carries))
        print(f"recoder op {op}: {len(cases)} cases, negative digits per scalar {min(carries)}..{max(carries)}")
    assert ic.RECODERS[3][:3] == (4, 64, 8) and ic.RECODERS[6][:3] == (6, 22, 32)
    assert L - 1 in ic.recode_cases(3) and 2 ** 128 - 1 in ic.recode_cases(6)


def test_div_small_cases():
    cases = ic.div_small_cases()
    assert len(cases) == 6 * 1003 and {k for _, k in cases} == set(range(2, 1002)) | {32768, 32769, 65535}
    for k in ic.DIV_KS:
        mine = [a for a, kk in cases if kk == k]
        assert {0, k - 1, k, ic.M256 - 1} <= set(mine)
        assert any(a % k == k - 1 and a.bit_length() >= 240 for a in mine)   # the largest remainder at every limb
    assert all(0 <= a < ic.M256 for a, _ in cases)
    print(f"mp_div_small: {len(cases)} cases")
