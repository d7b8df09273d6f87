"""The claims of tests/decode_cases.py held against the oracle (oracle/cbor_header.py): runs
anywhere.  The case counts are stated here, so a generator that silently shrinks fails."""
import pytest

import cbor_header as ch
import decode_cases as dc

ERAS = (False, True)
NHEADS = {False: 21, True: 22}


def _decode_all(cases, mode):
    arena, off, ln, names = cases
    return [ch.decode_header(arena, off[i], ln[i], allow_tpraos=mode) for i in range(len(off))]


def _hold(cases, res):
    """Every claimed status is the oracle's; every signed length is below its stride.  (The
    oracle itself asserts (signed == stored slice) == canon on every passing case.)"""
    for name, r in zip(cases[3], res):
        want = dc.claim(name)
        assert want is None or r["status"] == want, (name, hex(r["status"]))
        assert len(r["signed"]) < (ch.TP_SIGNED_STRIDE if r["tpraos"] else ch.SIGNED_STRIDE), name
        assert (r["fields"] is None) == bool(r["status"] & ch.DEC_FAIL)


def test_head_w_forms():
    assert dc.head_w(0, 23) == b"\x17" and dc.head_w(0, 24) == b"\x18\x18" and dc.head_w(2, 448) == b"\x59\x01\xc0"
    assert dc.head_w(4, 2, 26) == b"\x9a\x00\x00\x00\x02" and dc.head_w(0, 1 << 32) == b"\x1b" + (1 << 32).to_bytes(8, "big")
    for v in dc.EDGE_VALUES + (448, 70000):
        for mt in (0, 2, 4):
            assert dc.head_w(mt, v) == ch._head(mt, v)          # the shortest form is the oracle encoder's
            for ai in dc.forms_for(v):
                h = dc.head_w(mt, v, ai)
                assert len(h) == 1 + (dc.NBYTES[ai] if ai else 0) and h[0] >> 5 == mt
    assert [len(dc.forms_for(v)) for v in dc.EDGE_VALUES] == [5, 5, 4, 4, 3, 3, 2, 2, 1, 1]


@pytest.mark.parametrize("tp", ERAS)
def test_bases_are_the_oracle_encoders(tp):
    """The item layout encodes to the oracle's canonical header, in both eras and both bases."""
    for multi in (False, True):
        f = dc.base_fields(multi, tp)
        body = ch.encode_tpraos_body(f) if tp else ch.encode_body(f)
        h, at = dc.enc(dc.items(f, tp))
        assert h == ch._head(4, 2) + body + ch._head(2, 448) + f["kes_sig"]
        assert len(at) == NHEADS[tp]
        if not multi:                                            # every integer head is one byte
            assert all(h[at[k]] < 24 for k in dc.INT_FIELDS)


@pytest.mark.parametrize("tp", ERAS)
@pytest.mark.parametrize("multi", (False, True))
def test_first_bytes(multi, tp):
    cases = dc.first_bytes(multi, tp)
    names = cases[3]
    assert len(names) == NHEADS[tp] * 257 == (5397, 5654)[tp]
    res = _decode_all(cases, 2 if tp else False)
    _hold(cases, res)
    st = {}
    for name, r in zip(names, res):
        st.setdefault(name.split("/")[1], []).append(r["status"])
    assert len(st) == NHEADS[tp]
    for head, s in st.items():                                   # at each head: the original passes, some byte fails
        assert len(s) == 257 and s.count(0) >= 1 and any(x & ch.DEC_FAIL for x in s), head
    reached = {x for s in st.values() for x in s}
    if multi:
        assert {0, ch.DEC_SYNTAX, ch.DEC_SIZE, ch.DEC_UNSUPPORTED, ch.DEC_OVERFLOW} <= reached
    # the either-era mode (block batches) agrees wherever the body head still says 15 or 10
    res1 = _decode_all(cases, True)
    assert sum(a["status"] != b["status"] for a, b in zip(res, res1)) <= 2


@pytest.mark.parametrize("tp", ERAS)
@pytest.mark.parametrize("multi", (False, True))
def test_widths(multi, tp):
    cases = dc.widths(multi, tp)
    # one-byte base: 5 forms for every array and integer, 4 for every string but the KES
    # signature (3), plus the all-widest header
    assert len(cases[3]) == {(False, False): 96, (False, True): 99, (True, False): 84, (True, True): 87}[(multi, tp)]
    res = _decode_all(cases, 2 if tp else False)
    _hold(cases, res)
    h = dc.header(dc.base_fields(multi, tp), tp)
    canon = ch.decode_header(h, 0, len(h), allow_tpraos=tp)
    assert canon["status"] == 0
    for name, r in zip(cases[3], res):                            # wider forms never fail and sign the same bytes
        assert r["status"] in (0, ch.DEC_NONCANONICAL) and r["signed"] == canon["signed"], name
        assert {k: v for k, v in r["fields"].items()} == canon["fields"], name
    assert {dc.claim(n) for n in cases[3]} == {0, ch.DEC_NONCANONICAL}
    assert len(dc.body_width_cases(tp)) == (56, 58)[tp]


@pytest.mark.parametrize("tp", ERAS)
def test_values(tp):
    cases = dc.values(tp)
    assert len(cases[3]) == 7 * 30 + 2 * (NHEADS[tp] - 7) + 5 == (243, 245)[tp]
    res = _decode_all(cases, 2 if tp else False)
    _hold(cases, res)
    by = dict(zip(cases[3], res))
    assert {r["status"] for r in res} == {0, ch.DEC_NONCANONICAL, ch.DEC_OVERFLOW, ch.DEC_SYNTAX, ch.DEC_SIZE}
    for name, r in by.items():                                    # every integer comes back as written
        p = name.split("/")
        if len(p) == 4 and p[1] in dc.INT_FIELDS and r["fields"]:
            assert r["fields"][p[1]] == int(p[2], 16), name
    assert by["c/prev_null=>0x0"]["fields"]["prev_hash"] is None
    # the longest canonical bodies: 439 and 586 bytes
    assert len(by["c/max_ints=>0x0"]["signed"]) == (439, 586)[tp]


@pytest.mark.parametrize("tp", ERAS)
def test_lengths(tp):
    cases = dc.lengths(tp)
    arena, off, ln, names = cases
    f = dc.base_fields(True, tp)
    lc, lw = len(dc.header(f, tp)), len(dc.header(f, tp, 27))
    # payloads 816 (+144 TPraos) bytes; 46 (49) bytes of shortest heads, 9 per head at the widest
    assert (lc, lw) == ((816 + 46, 816 + 9 * 21), (960 + 49, 960 + 9 * 22))[tp]
    # every span length at 8 alignments, canonical and wide; the cuts inside wrong heads with
    # their uncut headers; the 9 spans around the arena's end
    assert len(names) == 8 * (lc + 9) + 8 * (lw + 9) + (235, 273)[tp] + 9 == (15324, 17762)[tp]
    cuts = [n for n in names if n.startswith("d/cut/")]
    assert len(cuts) == (235, 273)[tp] and sum(dc.claim(n) == ch.DEC_SYNTAX for n in cuts) == (187, 217)[tp]
    assert {dc.claim(n) for n in cuts} == {ch.DEC_SYNTAX, ch.DEC_OVERFLOW, ch.DEC_SIZE, ch.DEC_UNSUPPORTED}
    _hold(cases, _decode_all(cases, 2 if tp else False))
    assert {dc.claim(n) for n in names if not n.startswith("d/cut/")} == {
        0, ch.DEC_NONCANONICAL, ch.DEC_SYNTAX, ch.DEC_TRAILING, ch.DEC_RANGE}
    assert sorted({o % 8 for o in off[:-9]}) == list(range(8))
    assert off[-9] + ln[-9] == len(arena)                         # the last header ends on the arena's last byte
    # the bytes behind every span's header are a valid header
    assert arena[off[0] + lc:off[0] + 2 * lc] == arena[off[0]:off[0] + lc]


def test_eras():
    cases = dc.eras()
    assert len(cases[3]) == 12
    want = {False: {"e/10fields/arity10=>?"}, True: {"e/10fields/arity10=>?", "e/15fields/arity15=>?"},
            2: {"e/15fields/arity15=>?"}}
    for mode in (False, True, 2):
        res = _decode_all(cases, mode)
        _hold(cases, res)
        assert {n for n, r in zip(cases[3], res) if r["status"] == 0} == want[mode]
        assert all(r["status"] in (0, ch.DEC_SYNTAX) for r in res)
        assert all(r["tpraos"] == n.startswith("e/15") for n, r in zip(cases[3], res) if r["status"] == 0)


def test_every_status_bit_occurs():
    seen = set()
    for tp in ERAS:
        for g in (dc.first_bytes(True, tp), dc.widths(True, tp), dc.values(tp), dc.lengths(tp)):
            seen |= {r["status"] for r in _decode_all(g, 2 if tp else False)}
        assert seen >= {0, ch.DEC_RANGE, ch.DEC_SYNTAX, ch.DEC_SIZE, ch.DEC_UNSUPPORTED, ch.DEC_TRAILING,
                        ch.DEC_NONCANONICAL, ch.DEC_OVERFLOW}
        seen.clear()


def test_oracle_encoder_widths_and_make_block_wide(oracle):
    """The oracle's encoders take {head: 24..27} and give decode_cases' bytes; make_block's
    `wide` stores such a body under a signature over the canonical one, and its default
    leaves the block unchanged."""
    import random

    import block_corpus as bc
    import block_integrity as bi
    for tp in ERAS:
        f = dc.base_fields(True, tp)
        for name, ai in dc.body_width_cases(tp):
            body = (ch.encode_tpraos_body if tp else ch.encode_body)(f, {name: ai})
            assert ch._head(4, 2) + body + ch._head(2, 448) + f["kes_sig"] == dc.header(f, tp, {name: ai})
    for era in (5, 6):
        a, fa, _ = bc.make_block(random.Random(5), 129600, era=era)
        b, fb, _ = bc.make_block(random.Random(5), 129600, era=era, wide=())
        w, fw, _ = bc.make_block(random.Random(5), 129600, era=era, wide={"slot": 27, "vrf_out": 26, "body": 24})
        assert a == b and fa == fw and len(w) == len(a) + 4 + 3 + 1
        assert bi.verify_block_integrity(w, 0, len(w), 129600)[0] == 0
        i = w.index(fa["vrf_out"]) + 7
        bad = w[:i] + bytes([w[i] ^ 1]) + w[i + 1:]
        assert bi.verify_block_integrity(bad, 0, len(bad), 129600)[0] == bi.BLK_KES


def test_genuine_wide_headers_verify(oracle):
    for tp in ERAS:
        arena, off, ln, names = dc.genuine_wide(tp, 129600)
        assert len(names) == 1 + len(dc.body_width_cases(tp)) - 1 + 1      # c0 = 8282 has one form fewer than 25
        _hold((arena, off, ln, names), _decode_all((arena, off, ln, names), 2 if tp else False))
        for i in (0, 1, len(names) - 1):
            r = ch.decode_header(arena, off[i], ln[i], allow_tpraos=tp)
            f = r["fields"]
            assert oracle.kes_verify(f["hot_vk"], f["slot"] // 129600 - f["c0"], r["signed"], f["kes_sig"]) == 0
