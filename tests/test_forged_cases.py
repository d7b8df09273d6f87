"""CPU: the forged certificates of forged_cases.py.  Their group equations hold on the integer
model (asserted by the generator as it builds them); here the families cover what they claim, and
the C oracle and the CPU twin reject every forged case and accept every control."""
import numpy as np
import pytest

import ec_model as em
import forged_cases as fc
from helpers import arr

P, L = em.P, em.L
# the two order-8 ordinates of libsodium's blocklist, from the curve: y8b = p - y8a
Y8 = sorted({y for (_, y) in fc.TORSION if y not in (0, 1, P - 1)})


def test_torsion_encodings(oracle):
    encs = fc.torsion_encodings()
    assert len(encs) == len(set(encs)) == 14
    ys = {int.from_bytes(e, "little") & fc.M255 for e in encs}
    assert ys == {0, 1, P - 1, P, P + 1} | set(Y8) and len(Y8) == 2 and sum(Y8) == P
    for e in encs:
        pt = fc.lenient_decode(e)
        assert pt in fc.TORSION and em.on_curve(*pt) and em.order(pt) in (1, 2, 4, 8)
        assert oracle.has_small_order(e) and oracle.decode_ok(e)
    assert {fc.lenient_decode(e) for e in encs} == set(fc.TORSION)
    # each of the four order-8 points once, the others under every spelling
    assert sorted(em.order(fc.lenient_decode(e)) for e in encs) == [1, 1, 1, 1, 2, 2, 4, 4, 4, 4, 8, 8, 8, 8]
    # no other y + p fits 255 bits, and the lenient decoder agrees with the strict one on canonical input
    assert all(y + P > fc.M255 for y in Y8 + [P - 1])
    assert fc.lenient_decode(em.encode_affine(em.B_AFF)) == em.B_AFF == em.decode(em.encode_affine(em.B_AFF))


def test_ed25519_families():
    cases = fc.ed25519_cases()
    fam = lambda f, forged=True: [c for c in cases if c["family"] == f and c["forged"] == forged]
    encs = fc.torsion_encodings()
    assert [c["cold_vk"] for c in fam("small_a")] == encs
    for c in fam("small_a"):                                                  # R and S are ordinary
        s = int.from_bytes(c["sig"][32:], "little")
        assert 0 < s < L and em.order(fc.lenient_decode(c["sig"][:32])) is None
    rs = {c["sig"][:32] for c in fam("small_r")}
    assert len(rs) == len(fam("small_r")) >= 4
    assert any(int.from_bytes(e, "little") & fc.M255 in Y8 for e in rs)
    for c in fam("small_r"):
        assert em.order(fc.lenient_decode(c["sig"][:32])) in (1, 2, 4, 8)
        assert em.order(fc.lenient_decode(c["cold_vk"])) is None              # the key itself passes the blocklist
        assert int.from_bytes(c["sig"][32:], "little") < L
        assert int.from_bytes(c["cold_vk"], "little") & fc.M255 < P
    ks = fam("s_plus_kl")
    g = fam("s_plus_kl", False)[0]
    s0 = int.from_bytes(g["sig"][32:], "little")
    assert [int.from_bytes(c["sig"][32:], "little") for c in ks] == [s0 + k * L for k in range(1, len(ks) + 1)]
    assert len(ks) >= 14 and s0 + (len(ks) + 1) * L >= 2 ** 256
    assert all(len(fam(f, False)) == 1 for f in ("small_a", "small_r", "s_plus_kl"))
    print(f"forged OCerts: {len(fam('small_a'))} small-order keys, {len(rs)} small-order R, {len(ks)} S + k L, 3 controls")


def test_ed25519_oracle_and_twin(oracle, twin):
    cases = fc.ed25519_cases()
    want = [not c["forged"] for c in cases]
    got = [oracle.ed25519_verify(c["cold_vk"], fc.ocert_msg(c["hot_vk"], c["n"], c["c0"]), c["sig"]) for c in cases]
    assert got == want
    ok = twin.verify_ocert(arr([c["cold_vk"] for c in cases], 32), arr([c["hot_vk"] for c in cases], 32),
                           np.array([c["n"] for c in cases], np.uint64), np.array([c["c0"] for c in cases], np.uint64),
                           arr([c["sig"] for c in cases], 64))
    assert [bool(x) for x in ok] == want


def test_vrf_oracle_and_twin(oracle, twin):
    cases = fc.vrf_cases(oracle)
    assert [c["vrf_vk"] for c in cases if c["forged"]] == fc.torsion_encodings()
    assert sum(not c["forged"] for c in cases) == 1
    for c in cases:
        assert fc.vrf_equation_holds(oracle, c["vrf_vk"], c["proof"], c["alpha"])
        assert c["forged"] == (int.from_bytes(c["proof"][32:48], "little") % (em.order(fc.lenient_decode(c["vrf_vk"])) or L) == 0
                               and c["proof"][:32] == fc.IDENT_ENC)
    want = [not c["forged"] for c in cases]
    assert [oracle.vrf_verify(c["vrf_vk"], c["proof"], c["alpha"]) is not None for c in cases] == want
    ok, beta = twin.verify_vrf(arr([c["vrf_vk"] for c in cases], 32), arr([c["proof"] for c in cases], 80),
                               arr([c["alpha"] for c in cases], 32))
    assert [bool(x) for x in ok] == want
    for c, b in zip(cases, beta):                                             # beta does not depend on the key
        assert bytes(b) == oracle.vrf_proof_to_hash(c["proof"])
    print(f"forged VRF proofs: {sum(c['forged'] for c in cases)} small-order keys, 1 control")


@pytest.fixture(scope="module")
def twin():
    from praos_hip import cpu
    c = cpu.CpuContext()
    yield c
    c.close()
