"""Wire-header fixtures and the mutation corpus shared by the wire tests (host and GPU).

golden(): tests/golden/wire_headers.json (the reference's golden node-to-node headers).
corpus(): (bytes, n_eras) cases around two goldens (one Byron, one Shelley-based): every byte
incremented by one (the reference's Corruption.hs model), truncations at every length, trailing
bytes, heads widened to 2, 3, 5 and 9 bytes, indefinite lists and strings, tags 23 and 25, era 7
and era 255, and seeded random edits on top.
"""
import json
import os
import random

from praos_hip import wire

HERE = os.path.dirname(os.path.abspath(__file__))


def golden():
    return json.load(open(os.path.join(HERE, "golden", "wire_headers.json")))


def _heads(era, kind, hint, n):
    """The wrapper's heads as (major, value) in wire order; the last is the byte string's."""
    hs = [(4, 2), (0, era)]
    if era == 0:
        hs += [(4, 2), (4, 2), (0, kind), (0, hint)]
    return hs + [(6, 24), (2, n)]


def rebuild(era, kind, hint, header, widths=None, replace=None):
    """The wire item with head k at width widths[k] (0 = shortest) or replaced by raw bytes."""
    hs = _heads(era, kind, hint, len(header))
    out = b""
    for k, (mt, v) in enumerate(hs):
        if replace and k in replace:
            out += replace[k]
        else:
            out += wire.head(mt, v, (widths or {}).get(k, 0))
    return out + bytes(header)


def corpus(seed=20240607):
    G = golden()
    by = {h["name"]: h for h in G["headers"]}
    R = random.Random(seed)
    cases = []
    for name in ("Byron_regular", "Babbage"):
        g = by[name]
        raw = bytes.fromhex(g["wire"])
        _, era, kind, hint, off, ln = wire.unwrap(raw)
        hdr = raw[off:off + ln]
        nh = len(_heads(era, kind, hint, ln))
        cases.append(raw)
        # every byte incremented by one (mod 256)
        for p in range(len(raw)):
            cases.append(raw[:p] + bytes([(raw[p] + 1) & 0xFF]) + raw[p + 1:])
        # truncations at every length, trailing bytes
        for n in range(len(raw)):
            cases.append(raw[:n])
        for extra in (b"\x00", b"\xff", b"\x82\x05", bytes(9)):
            cases.append(raw + extra)
        # widened heads: each head alone at each width that holds its value, then all together
        for k, (mt, v) in enumerate(_heads(era, kind, hint, ln)):
            for w in (2, 3, 5, 9):
                if v < 1 << (8 * {2: 1, 3: 2, 5: 4, 9: 8}[w]):
                    cases.append(rebuild(era, kind, hint, hdr, {k: w}))
        for w in (3, 5, 9):
            cases.append(rebuild(era, kind, hint, hdr, {k: w for k in range(nh)}))
        # indefinite lists / string, reserved additional info, other tags, other eras
        lists = [k for k, (mt, _) in enumerate(_heads(era, kind, hint, ln)) if mt == 4]
        for k in lists:
            cases.append(rebuild(era, kind, hint, hdr, replace={k: b"\x9f"}) + b"\xff")
            cases.append(rebuild(era, kind, hint, hdr, replace={k: b"\x9f"}))
            cases.append(rebuild(era, kind, hint, hdr, replace={k: b"\x83"}))
            cases.append(rebuild(era, kind, hint, hdr, replace={k: b"\x81"}))
        cases.append(rebuild(era, kind, hint, hdr, replace={nh - 1: b"\x5f" + wire.head(2, ln)}) + b"\xff")
        cases.append(rebuild(era, kind, hint, hdr, replace={nh - 1: b"\x5f"}))
        cases.append(rebuild(era, kind, hint, hdr, replace={nh - 1: b"\x5c"}))
        cases.append(rebuild(era, kind, hint, hdr, replace={nh - 1: wire.head(3, ln)}))
        for tag in (23, 25, 24 + 256):
            cases.append(rebuild(era, kind, hint, hdr, replace={nh - 2: wire.head(6, tag)}))
        cases.append(rebuild(era, kind, hint, hdr, replace={nh - 2: b""}))
        for e in (7, 255, 256, 6, 1, 0):
            cases.append(rebuild(era, kind, hint, hdr, replace={1: wire.head(0, e)}))
            cases.append(rebuild(era, kind, hint, hdr, replace={1: wire.head(0, e, 9)}))
        cases.append(rebuild(era, kind, hint, hdr, replace={1: wire.head(1, 0)}))
        if era == 0:
            for kk in (0, 1, 2, 255):
                cases.append(rebuild(era, kind, hint, hdr, replace={4: wire.head(0, kk)}))
            for hh in (0, (1 << 32) - 1, 1 << 32, (1 << 64) - 1):
                cases.append(rebuild(era, kind, hint, hdr, replace={5: wire.head(0, hh)}))
        # seeded random edits of the wrapper region
        for _ in range(150):
            b = bytearray(raw)
            for _ in range(R.randint(1, 3)):
                b[R.randrange(min(len(b), off + 2))] = R.randrange(256)
            cases.append(bytes(b[:R.randint(max(1, off - 2), len(b))]) if R.random() < 0.3 else bytes(b))
    out = [(c, G["n_eras"]) for c in cases]
    # other n_eras over the goldens themselves
    for h in G["headers"]:
        for ne in (0, 1, 5, 6, 7, 8):
            out.append((bytes.fromhex(h["wire"]), ne))
    for d in G["disabled"]:
        out.append((bytes.fromhex(d["wire"]), G["n_eras"]))
    out.append((b"", G["n_eras"]))
    return out
