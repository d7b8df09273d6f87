"""Reference model of the device's field, group and scalar-multiplication layers in plain
Python integers.  It shares no code with the device or with the C oracle.

  * GF(2^255 - 19) and edwards25519 in extended integer coordinates with the complete
    addition law (valid for every pair of curve points, small-order ones included);
  * scalar multiplication by the INTEGER scalar (never reduced mod L: a base with a
    small-order component has an order that does not divide L);
  * RFC 8032 point encoding / decoding;
  * raw-representative helpers: coordinates (X, Y, Z, T) of a given affine point in which one
    coordinate is a chosen 256-bit value (the device works on any representative < 2^256);
  * a limb-level model of the device's product scanning (8 x 32-bit limbs, a 64-bit column
    accumulator plus a carry count) and of fe_reduce512's two folds, used only to check that
    the test inputs reach the rare carry paths.
"""
P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
M256 = 2 ** 256
D = (-121665 * pow(121666, P - 2, P)) % P
D2 = 2 * D % P
SQRTM1 = pow(2, (P - 1) // 4, P)


def inv(x):
    return pow(x % P, P - 2, P)


# ---------------------------------------------------------------- curve
def recover_x(y, sign):
    """x with x^2 = (y^2 - 1) / (d y^2 + 1) and x & 1 == sign, or None (RFC 8032 5.1.3)."""
    if y >= P:
        return None
    x2 = (y * y - 1) * inv(D * y * y + 1) % P
    if x2 == 0:
        return None if sign else 0
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P != 0:
        x = x * SQRTM1 % P
    if (x * x - x2) % P != 0:
        return None
    if (x & 1) != sign:
        x = P - x
    return x


def on_curve(x, y):
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def affine_to_ext(a):
    x, y = a
    return (x, y, 1, x * y % P)


IDENT = (0, 1, 1, 0)


def add(p, q):
    """Complete unified addition (a = -1, d non-square): add-2008-hwcd-3, no exceptions."""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = t1 * D2 % P * t2 % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def dbl(p):
    return add(p, p)


def neg(p):
    x, y, z, t = p
    return ((-x) % P, y, z, (-t) % P)


def to_affine(p):
    x, y, z, _ = p
    zi = inv(z)
    return (x * zi % P, y * zi % P)


def equal(p, q):
    return (p[0] * q[2] - q[0] * p[2]) % P == 0 and (p[1] * q[2] - q[1] * p[2]) % P == 0


def encode_affine(a):
    x, y = a
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def encode(p):
    return encode_affine(to_affine(p))


def decode(b):
    """RFC 8032 decoding: the affine point, or None."""
    v = int.from_bytes(b, "little")
    y, sign = v & (2 ** 255 - 1), v >> 255
    x = recover_x(y, sign)
    return None if x is None else (x, y)


BY = 4 * inv(5) % P
B_AFF = (recover_x(BY, 0), BY)
B = affine_to_ext(B_AFF)


def scalarmult(k, p):
    """[k]p for the integer k >= 0 (plain double and add)."""
    r = IDENT
    q = p
    while k:
        if k & 1:
            r = add(r, q)
        q = dbl(q)
        k >>= 1
    return r


class Mul:
    """[k]p for many k and one p: radix-16 tables (64 additions per scalar, k < 2^256)."""

    def __init__(self, p):
        self.tab = []
        q = p
        for _ in range(64):
            row = [IDENT, q]
            for _ in range(14):
                row.append(add(row[-1], q))
            self.tab.append(row)
            q = add(row[15], q)

    def __call__(self, k):
        assert 0 <= k < M256
        r = IDENT
        j = 0
        while k:
            d = k & 15
            if d:
                r = add(r, self.tab[j][d])
            k >>= 4
            j += 1
        return r


_MUL = {}


def mul(k, aff):
    """[k](affine point), the tables cached per base."""
    m = _MUL.get(aff)
    if m is None:
        m = _MUL[aff] = Mul(affine_to_ext(aff))
    return m(k)


def small_order_points():
    """Affine points of order 2, 4 and 8: the order-8 one is [L]R for the first curve point R
    (y = 2, 3, ...) whose cofactor part has full order."""
    o2 = (0, P - 1)
    o4 = (SQRTM1, 0)
    y = 2
    while True:
        x = recover_x(y, 0)
        if x is not None:
            t = to_affine(scalarmult(L, affine_to_ext((x, y))))
            if order(t) == 8:
                return o2, o4, t
        y += 1


def order(aff, limit=16):
    q = affine_to_ext(aff)
    r = q
    for n in range(1, limit + 1):
        if equal(r, IDENT):
            return n
        r = add(r, q)
    return None


# ---------------------------------------------------------------- raw representatives
def lift_max(v):
    """The largest representative of v mod p below 2^256 (v, v + p or v + 2p)."""
    v %= P
    while v + P < M256:
        v += P
    return v


def lifts(v):
    """Every representative of v mod p below 2^256."""
    v %= P
    out = []
    while v < M256:
        out.append(v)
        v += P
    return out


def p3_with_z(aff, z):
    """(X, Y, Z, T) canonical limbs of the affine point with the given Z (Z mod p != 0); Z keeps its raw value."""
    x, y = aff
    zz = z % P
    assert zz != 0
    return (x * zz % P, y * zz % P, z, x * y % P * zz % P)


def p3_force(aff, coord, raw):
    """Extended coordinates of the affine point whose coordinate `coord` (0 X, 1 Y, 2 Z, 3 T) is the
    raw 256-bit value `raw`: Z = raw / x (or / y, / xy).  Where the point cannot take that residue
    (the coordinate is 0 for every Z, or raw = 0 mod p for a non-zero coordinate) the point keeps
    Z = 1 and the coordinate takes its largest representative below 2^256 instead."""
    x, y = aff
    unit = (x, y, 1, x * y % P)[coord]
    r = raw % P
    if coord == 2:
        if r == 0:
            c = list(p3_with_z(aff, 1))
            c[2] = lift_max(1)
            return tuple(c)
        return p3_with_z(aff, raw)
    if unit == 0 or r == 0:
        c = list(p3_with_z(aff, 1))
        c[coord] = lift_max(c[coord])
        return tuple(c)
    c = list(p3_with_z(aff, r * inv(unit) % P))
    assert c[coord] == r
    c[coord] = raw
    return tuple(c)


def p1p1_with(aff, z, t):
    """((X : Z), (Y : T)) of the affine point: X = x Z, Y = y T."""
    x, y = aff
    assert z % P and t % P
    return (x * z % P, y * t % P, z, t)


def p1p1_force(aff, coord, raw):
    """p1p1 coordinates with coordinate `coord` (0 X, 1 Y, 2 Z, 3 T) forced to `raw` (as p3_force)."""
    x, y = aff
    r = raw % P
    if coord >= 2:
        if r == 0:
            c = list(p1p1_with(aff, 1, 1))
            c[coord] = lift_max(1)
            return tuple(c)
        c = list(p1p1_with(aff, raw if coord == 2 else 1, raw if coord == 3 else 1))
        c[coord] = raw
        return tuple(c)
    unit = (x, y)[coord]
    if unit == 0 or r == 0:
        c = list(p1p1_with(aff, 1, 1))
        c[coord] = lift_max(c[coord])
        return tuple(c)
    w = r * inv(unit) % P
    c = list(p1p1_with(aff, w if coord == 0 else 1, w if coord == 1 else 1))
    assert c[coord] == r
    c[coord] = raw
    return tuple(c)


def to_cached(p):
    x, y, z, t = p
    return ((y + x) % P, (y - x) % P, z % P, t * D2 % P)


def to_niels(aff):
    x, y = aff
    return ((y + x) % P, (y - x) % P, x * y % P * D2 % P)


# projective comparisons of device outputs (raw limbs, any representative) with affine points
def p1p1_is(c, aff):
    x, y = aff
    cx, cy, cz, ct = c
    return cz % P != 0 and ct % P != 0 and (cx - x * cz) % P == 0 and (cy - y * ct) % P == 0


def p2_is(c, aff):
    x, y = aff
    return c[2] % P != 0 and (c[0] - x * c[2]) % P == 0 and (c[1] - y * c[2]) % P == 0


def p3_is(c, aff):
    return p2_is(c, aff) and (c[3] * c[2] - c[0] * c[1]) % P == 0


def cached_is(c, aff):
    """(Y+X, Y-X, Z, 2dT) of some (X : Y : Z : T) equal to the affine point."""
    ypx, ymx, z, t2d = c
    x, y = aff
    return (z % P != 0 and (ypx - (y + x) * z) % P == 0 and (ymx - (y - x) * z) % P == 0
            and (t2d - D2 * x * y % P * z) % P == 0)


def niels_is(c, aff):
    ypx, ymx, xy2d = c[:3]
    x, y = aff
    return (ypx - (y + x)) % P == 0 and (ymx - (y - x)) % P == 0 and (xy2d - D2 * x * y) % P == 0


# ---------------------------------------------------------------- limb-level product model
def limbs(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def prod_scan(a, b, square=False):
    """Product scanning as the device runs it: column k accumulates a_i b_(k-i) into a 64-bit
    accumulator and counts its carry-outs; the next column starts from (acc >> 32) | (count << 32).
    square: only the cross products i < j (the device doubles them and adds the diagonal later).
    Returns (the 16 limbs t, carry count per column 0 .. 14)."""
    A, Bv = limbs(a), limbs(b)
    t = [0] * 16
    counts = [0] * 15
    acc = 0
    for k in range(15):
        cnt = 0
        for i in range(8):
            j = k - i
            if j < 0 or j > 7 or (square and j <= i):
                continue
            acc += A[i] * Bv[j]
            if acc >> 64:
                acc &= 2 ** 64 - 1
                cnt += 1
        counts[k] = cnt
        t[k] = acc & 0xFFFFFFFF
        acc = (acc >> 32) | (cnt << 32)
    t[15] = acc & 0xFFFFFFFF
    assert acc >> 32 == 0
    return t, counts


def square_finish(t, a):
    """2 * (cross products) + the diagonal squares, as fe_sq_finish: the 16 limbs of a^2."""
    v = sum(x << (32 * i) for i, x in enumerate(t)) * 2
    A = limbs(a)
    v += sum((A[i] * A[i]) << (64 * i) for i in range(8))
    assert v >> 512 == 0
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(16)]


def reduce512(t):
    """fe_reduce512: returns (result, k of the second fold, whether that fold carried out of limb 0)."""
    lo = sum(t[i] << (32 * i) for i in range(8))
    hi = sum(t[8 + i] << (32 * i) for i in range(8))
    s = lo + 38 * hi
    k = s >> 256
    assert k < 40
    r = s & (M256 - 1)
    r0 = (r & 0xFFFFFFFF) + 38 * k
    carried = r0 >> 32 != 0
    r = (r - (r & 0xFFFFFFFF)) + r0
    if r >> 256:
        r = (r & (M256 - 1)) + 38
        assert r < 2 ** 11
    return r, k, carried


def product_trace(a, b=None):
    """The model of one device product (b None: the squaring of a): (value, k, carried, carry counts)."""
    if b is None:
        t, counts = prod_scan(a, a, square=True)
        t = square_finish(t, a)
        want = a * a
    else:
        t, counts = prod_scan(a, b)
        want = a * b
    assert sum(x << (32 * i) for i, x in enumerate(t)) == want
    r, k, carried = reduce512(t)
    assert r % P == want % P
    return r, k, carried, counts
