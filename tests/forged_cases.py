"""Forged certificates whose group equation HOLDS, so that only an encoding predicate rejects
them: Ed25519 (OCert) signatures under small-order keys, with small-order R, and with S + k L;
draft-03 VRF proofs under small-order keys.  Each family has a control under an ordinary key.

The generator proves the first half with tests/ec_model.py: points are decoded leniently (y mod
p, the sign bit applied to x, as libsodium's ge25519_frombytes does) and the verification
equation is evaluated on integers WITHOUT the predicates.  The second half (every forged case is
rejected, every control accepted) is asserted of the C oracle and the CPU twin by
test_forged_cases.py and of the device by test_gpu_forged.py.  Pure Python and deterministic;
`oracle` is only used for the VRF suite's hash_to_curve."""
import hashlib
import random

import ec_model as em

P, L = em.P, em.L
M255 = 2 ** 255 - 1
IDENT_ENC = (1).to_bytes(32, "little")


def lenient_decode(b):
    """libsodium ge25519_frombytes: y = the low 255 bits mod p, x the root made to match the sign bit
    (x = 0 keeps 0).  The affine point, or None."""
    v = int.from_bytes(b, "little")
    y, sign = (v & M255) % P, v >> 255
    x = em.recover_x(y, 0)
    if x is None:
        return None
    return ((P - x) % P if sign else x, y)


def _torsion():
    _, _, t8 = em.small_order_points()
    pts = [em.to_affine(em.scalarmult(j, em.affine_to_ext(t8))) for j in range(8)]
    assert pts[0] == (0, 1) and [em.order(p) for p in pts] == [1, 8, 4, 8, 2, 8, 4, 8]
    return pts


TORSION = _torsion()                                     # TORSION[j] = [j] T8
T8 = TORSION[1]


def torsion_encodings():
    """Every 32-byte string that decodes leniently to a torsion point: the canonical encodings, x = 0
    under a set sign bit, and y + p where it fits 255 bits.  Sorted."""
    out = set()
    for x, y in TORSION:
        for yy in (y, y + P):
            if yy <= M255:
                out.add(yy | (x & 1) << 255)
                if x == 0:
                    out.add(yy | 1 << 255)
    return [v.to_bytes(32, "little") for v in sorted(out)]


def ocert_msg(hot_vk, n, c0):
    return hot_vk + n.to_bytes(8, "big") + c0.to_bytes(8, "big")


def hram(r_enc, a_enc, msg):
    return int.from_bytes(hashlib.sha512(r_enc + a_enc + msg).digest(), "little") % L


def ed_equation_holds(a_enc, msg, sig):
    """[S]B - [h]A re-encodes to the signature's R, with A decoded leniently and no predicate applied"""
    a = lenient_decode(a_enc)
    if a is None:
        return False
    s = int.from_bytes(sig[32:], "little")
    h = hram(sig[:32], a_enc, msg)
    ha = em.scalarmult(h, em.affine_to_ext(a))
    return em.encode(em.add(em.mul(s, em.B_AFF), em.neg(ha))) == sig[:32]


def _ed_case(family, name, forged, a_enc, hot, n, c0, sig):
    assert ed_equation_holds(a_enc, ocert_msg(hot, n, c0), sig), (family, name)
    return {"family": family, "name": name, "forged": forged, "cold_vk": a_enc, "hot_vk": hot, "n": n, "c0": c0,
            "sig": sig}


def _rb(r, n):
    return bytes(r.getrandbits(8) for _ in range(n))


def _genuine(r, family, name):
    a, k = r.randrange(1, L), r.randrange(1, L)
    a_enc, r_enc = em.encode(em.mul(a, em.B_AFF)), em.encode(em.mul(k, em.B_AFF))
    hot, n, c0 = _rb(r, 32), r.getrandbits(16), r.randrange(600)
    s = (k + hram(r_enc, a_enc, ocert_msg(hot, n, c0)) * a) % L
    return _ed_case(family, name, False, a_enc, hot, n, c0, r_enc + s.to_bytes(32, "little"))


_ED = []


def ed25519_cases():
    """OCert cases (dicts: family, name, forged, cold_vk, hot_vk, n, c0, sig)."""
    if _ED:
        return _ED
    r = random.Random(0xf02ced)
    out = []
    # small-order key A: R = [k]B, S = k, the message redrawn until [h]A is the identity
    tries = []
    for i, a_enc in enumerate(torsion_encodings()):
        order = em.order(lenient_decode(a_enc))
        k = r.randrange(1, L)
        r_enc = em.encode(em.mul(k, em.B_AFF))
        n, c0 = r.getrandbits(16), r.randrange(600)
        t = 0
        while True:
            t += 1
            hot = _rb(r, 32)
            if hram(r_enc, a_enc, ocert_msg(hot, n, c0)) % order == 0:
                break
        tries.append(t)
        out.append(_ed_case("small_a", f"A[{i}] order {order}", True, a_enc, hot, n, c0, r_enc + k.to_bytes(32, "little")))
    assert len(tries) == 14 and max(tries) <= 64
    out.append(_genuine(r, "small_a", "control"))
    # small-order R under the mixed-order key A = [a]B + T8: R = -[h mod 8] T8, S = h a
    a = r.randrange(1, L)
    a_enc = em.encode(em.add(em.mul(a, em.B_AFF), em.affine_to_ext(T8)))
    found = {}
    for _ in range(400):
        hot, n, c0 = _rb(r, 32), r.getrandbits(16), r.randrange(600)
        for j, pt in enumerate(TORSION):
            r_enc = em.encode_affine(pt)
            h = hram(r_enc, a_enc, ocert_msg(hot, n, c0))
            if j == (-h) % 8 and r_enc not in found:
                found[r_enc] = _ed_case("small_r", f"R = [{j}]T8", True, a_enc, hot, n, c0,
                                        r_enc + (h * a % L).to_bytes(32, "little"))
        if len(found) == 8:
            break
    out += [found[k] for k in sorted(found)]
    out.append(_genuine(r, "small_r", "control"))
    # S + k L under an ordinary key
    g = _genuine(r, "s_plus_kl", "control")
    s = int.from_bytes(g["sig"][32:], "little")
    k = 1
    while s + k * L < 2 ** 256:
        out.append(_ed_case("s_plus_kl", f"S + {k} L", True, g["cold_vk"], g["hot_vk"], g["n"], g["c0"],
                            g["sig"][:32] + (s + k * L).to_bytes(32, "little")))
        k += 1
    out.append(g)
    _ED.extend(out)
    return _ED


# ---------------------------------------------------------------- VRF (ECVRF-ED25519-SHA512-Elligator2, draft 03)
def _challenge(h_enc, gamma, u, v):
    g = em.encode_affine(gamma)
    return hashlib.sha512(b"\x04\x02" + h_enc + g + em.encode(u) + em.encode(v)).digest()[:16]


def vrf_equation_holds(oracle, y_enc, proof, alpha):
    """draft-03 verification on integers without the key validation"""
    y, gamma = lenient_decode(y_enc), lenient_decode(proof[:32])
    if y is None or gamma is None:
        return False
    h_enc = oracle.vrf_hash_to_curve(y_enc, alpha)
    h = em.affine_to_ext(em.decode(h_enc))
    c = int.from_bytes(proof[32:48], "little")
    s = int.from_bytes(proof[48:], "little") % L
    u = em.add(em.mul(s, em.B_AFF), em.neg(em.scalarmult(c, em.affine_to_ext(y))))
    v = em.add(em.scalarmult(s, h), em.neg(em.scalarmult(c, em.affine_to_ext(gamma))))
    return _challenge(h_enc, gamma, u, v) == proof[32:48]


def vrf_forge(oracle, y_enc, alpha, r):
    """A proof under the small-order key y_enc that satisfies the equations: Gamma the identity,
    U = [k]B, V = [k]H, k redrawn until the challenge c is a multiple of the key's order, s = k."""
    order = em.order(lenient_decode(y_enc))
    h_enc = oracle.vrf_hash_to_curve(y_enc, alpha)
    h = em.affine_to_ext(em.decode(h_enc))
    for _ in range(200):
        k = r.randrange(1, L)
        c = _challenge(h_enc, (0, 1), em.mul(k, em.B_AFF), em.scalarmult(k, h))
        if int.from_bytes(c, "little") % order == 0:
            proof = IDENT_ENC + c + k.to_bytes(32, "little")
            assert vrf_equation_holds(oracle, y_enc, proof, alpha)
            return proof
    raise AssertionError("no challenge divisible by the key's order")


def vrf_genuine(oracle, alpha, r):
    """(key, proof) of an ordinary key Y = [x]B: Gamma = [x]H, s = k + c x"""
    x, k = r.randrange(1, L), r.randrange(1, L)
    y_enc = em.encode(em.mul(x, em.B_AFF))
    h_enc = oracle.vrf_hash_to_curve(y_enc, alpha)
    h = em.affine_to_ext(em.decode(h_enc))
    gamma = em.to_affine(em.scalarmult(x, h))
    c = _challenge(h_enc, gamma, em.mul(k, em.B_AFF), em.scalarmult(k, h))
    s = (k + int.from_bytes(c, "little") * x) % L
    proof = em.encode_affine(gamma) + c + s.to_bytes(32, "little")
    assert vrf_equation_holds(oracle, y_enc, proof, alpha)
    return y_enc, proof


_VRF = []


def vrf_cases(oracle):
    """VRF cases (dicts: name, forged, vrf_vk, proof, alpha): one per torsion encoding, and a control."""
    if _VRF:
        return _VRF
    r = random.Random(0xf02cef)
    out = []
    for i, y_enc in enumerate(torsion_encodings()):
        alpha = _rb(r, 32)
        out.append({"name": f"Y[{i}] order {em.order(lenient_decode(y_enc))}", "forged": True, "vrf_vk": y_enc,
                    "proof": vrf_forge(oracle, y_enc, alpha, r), "alpha": alpha})
    alpha = _rb(r, 32)
    y_enc, proof = vrf_genuine(oracle, alpha, r)
    out.append({"name": "control", "forged": False, "vrf_vk": y_enc, "proof": proof, "alpha": alpha})
    _VRF.extend(out)
    return _VRF
