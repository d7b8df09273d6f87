"""praos_validate_chunk (parseChunkFile as one call) against the Python restatement in
tests/chunk_model.py: every field of the result and of the rebuilt entries.

One linked chain per module (tests/chunk_corpus.py): 24 wrapped blocks -- 8 Alonzo, 8 Babbage,
8 Conway, two of them ~70 KB, the first with a GenesisHash prev -- plus a bare 6-block chain;
the cases are mutations of it crossed with the state of the index (checksums) and of the
block-offset hints, which may change the time but never the outcome."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import chunk_corpus as cc
import chunk_model as cm
from helpers import rbytes
from praos_hip import abi, immutable

pytestmark = pytest.mark.gpu
SPKP = 129600
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "integration", "c", "ffi_harness")
SWEEP_SEED = 1


class Chain:
    def __init__(self):
        r = random.Random(0xC4A1)
        pads = {i: 40 + i for i in range(1, 24, 2)}
        pads.update({6: 70_000, 17: 69_000})
        self.blocks = cc.make_chain(r, SPKP, [5] * 8 + [6] * 8 + [7] * 8, pads)
        self.bare = cc.make_chain(r, SPKP, [6, 7, 5, 6, 7, 6], {2: 300}, wrapped=False)
        self.blobs = [b.bytes for b in self.blocks]
        self.data, self.off, self.crc = cc.layout(self.blobs)
        # block 12 re-signed with a random prev (same length: the later offsets stay)
        b = self.blocks[12]
        keep = b.f["prev_hash"]
        b.f["prev_hash"] = rbytes(r, 32)
        self.relinked12 = b.sign().bytes
        b.f["prev_hash"] = keep
        b.sign()
        assert b.bytes == self.blobs[12]
        self.byron = cc.byron_item(r)

    def file(self, **repl):
        """The chain with blocks replaced: file(b9=bytes) -> (data, offsets, CRCs of what is stored)."""
        blobs = list(self.blobs)
        for k, v in repl.items():
            blobs[int(k[1:])] = v
        return cc.layout(blobs)


@pytest.fixture(scope="module")
def chain():
    return Chain()


def _both(ctx, data, crc=None, off=None, skip=()):
    got = ctx.validate_chunk(data, crc, off, SPKP)
    want = cm.parse_chunk(data, crc, SPKP, off)
    cm.assert_same(got, want, skip)
    return got


def test_intact_chain(ctx, chain):
    g = _both(ctx, chain.data, chain.crc, chain.off)
    assert (g["outcome"], g["blocks"], g["checked"]) == (abi.CHUNK_OK, 24, 0)
    assert g["rescanned_from"] == len(chain.data) == g["truncate_at"]
    assert g["prev_is_genesis"][0] == 1 and (g["integrity"] == -1).all()
    assert list(g["block_no"]) == list(range(24))


def test_bare_chain(ctx, chain):
    data, off, crc = cc.layout([b.bytes for b in chain.bare])
    g = _both(ctx, data, crc, off)
    assert (g["outcome"], g["blocks"], g["checked"]) == (abi.CHUNK_OK, 6, 0)
    assert g["entries"][8:10] == b"\x00\x01"                    # headerOffset of a bare block
    g = _both(ctx, data)
    assert (g["outcome"], g["blocks"], g["checked"]) == (abi.CHUNK_OK, 6, 6)


def test_no_index(ctx, chain):
    g = _both(ctx, chain.data)
    assert (g["outcome"], g["blocks"], g["checked"], g["rescanned_from"]) == (abi.CHUNK_OK, 24, 24, 0)
    assert (g["integrity"] == 0).all()


def test_index_of_the_first_ten(ctx, chain):
    g = _both(ctx, chain.data, chain.crc[:10], chain.off[:10])
    assert (g["outcome"], g["blocks"], g["checked"]) == (abi.CHUNK_OK, 24, 14)
    assert g["rescanned_from"] == chain.off[9]                  # the last candidate has trailing items


def test_stale_crc_on_an_intact_block(ctx, chain):
    crc = list(chain.crc)
    crc[7] ^= 0x5A5A
    g = _both(ctx, chain.data, crc, chain.off)
    assert (g["outcome"], g["blocks"], g["checked"]) == (abi.CHUNK_OK, 24, 1)
    assert int.from_bytes(g["entries"][56 * 7 + 12:56 * 7 + 16], "big") == chain.crc[7]
    assert g["integrity"][7] == 0


def test_segment_byte_flip(ctx, chain):
    data, off, _ = chain.file(b9=cc.flip_segment_byte(chain.blobs[9]))
    g = _both(ctx, data, chain.crc, chain.off)
    assert (g["outcome"], g["integrity_bits"], g["blocks"]) == (abi.CHUNK_ERR_CORRUPT, abi.BLK_BODY_HASH, 9)
    assert g["truncate_at"] == chain.off[9] and g["err_hash"] == chain.blocks[9].header_hash
    assert g["err_slot"] == chain.blocks[9].f["slot"]


def test_kes_signature_byte_flip(ctx, chain):
    data, _, _ = chain.file(b9=cc.flip_kes_byte(chain.blobs[9]))
    g = _both(ctx, data, chain.crc, chain.off)
    assert (g["outcome"], g["integrity_bits"], g["blocks"]) == (abi.CHUNK_ERR_CORRUPT, abi.BLK_KES, 9)


def test_damage_under_a_matching_crc_is_trusted(ctx, chain):
    data, off, crc = chain.file(b9=cc.flip_segment_byte(chain.blobs[9]))
    g = _both(ctx, data, crc, off)                              # the reference trusts the CRC
    assert (g["outcome"], g["blocks"], g["checked"]) == (abi.CHUNK_OK, 24, 0)


def test_header_damage_under_a_matching_crc(ctx, chain):
    data, off, crc = chain.file(b9=cc.flip_header_byte(chain.blocks[9]))
    g = _both(ctx, data, crc, off)
    assert (g["outcome"], g["blocks"], g["truncate_at"]) == (abi.CHUNK_ERR_HASH_MISMATCH, 10, off[10])
    assert g["actual_prev"] == chain.blocks[9].header_hash and g["expected_prev"] != g["actual_prev"]


def test_relinked_block(ctx, chain):
    data, off, crc = chain.file(b12=chain.relinked12)
    g = _both(ctx, data, crc, off)
    assert (g["outcome"], g["blocks"], g["truncate_at"]) == (abi.CHUNK_ERR_HASH_MISMATCH, 12, off[12])
    assert g["expected_prev"] == chain.blocks[11].header_hash and g["actual_prev"] != g["expected_prev"]
    assert g["actual_prev_is_genesis"] == 0


def test_corrupt_comes_before_mismatch_in_one_block(ctx, chain):
    data, off, _ = chain.file(b12=cc.flip_segment_byte(chain.relinked12))
    g = _both(ctx, data, chain.crc, off)
    assert (g["outcome"], g["blocks"]) == (abi.CHUNK_ERR_CORRUPT, 12)


def test_the_earlier_error_wins(ctx, chain):
    data, off, _ = chain.file(b12=chain.relinked12, b15=cc.flip_segment_byte(chain.blobs[15]))
    crc = list(chain.crc)
    crc[12] = cc.zlib.crc32(chain.relinked12)
    g = _both(ctx, data, crc, off)
    assert (g["outcome"], g["blocks"]) == (abi.CHUNK_ERR_HASH_MISMATCH, 12)


def test_file_cut_inside_a_block(ctx, chain):
    cut = chain.off[20] + len(chain.blobs[20]) // 2
    g = _both(ctx, chain.data[:cut], chain.crc, chain.off)
    assert (g["outcome"], g["blocks"], g["truncate_at"]) == (abi.CHUNK_ERR_READ, 20, chain.off[20])
    _both(ctx, chain.data[:cut])


def test_stray_bytes_after_the_last_block(ctx, chain):
    data = chain.data + b"\x01\x02\x03\x04\x05\x06\x07"
    g = _both(ctx, data, chain.crc, chain.off)
    assert (g["outcome"], g["blocks"], g["truncate_at"]) == (abi.CHUNK_ERR_READ, 24, len(chain.data))
    assert g["rescanned_from"] == chain.off[23]


def test_byron_item_is_unsupported(ctx, chain):
    data, off, crc = chain.file(b3=chain.byron)
    g = _both(ctx, data, crc, off)
    assert (g["outcome"], g["blocks"], g["truncate_at"]) == (abi.CHUNK_UNSUPPORTED, 3, off[3])
    _both(ctx, data)


def test_empty_file(ctx):
    g = _both(ctx, b"")
    assert (g["outcome"], g["blocks"], g["truncate_at"]) == (abi.CHUNK_OK, 0, 0)
    _both(ctx, b"", [1, 2], [0, 5])


def test_small_capacity_reports_the_needed_count(ctx, chain):
    with pytest.raises(abi.PraosError, match=f"rc={abi.E_ARG}") as e:
        ctx.validate_chunk(chain.data, chain.crc, chain.off, SPKP, cap=23)
    assert e.value.needed == 24
    assert ctx.validate_chunk(chain.data, chain.crc, chain.off, SPKP, cap=24)["blocks"] == 24


def _hint_corruptions(off, size):
    shifted = list(off[:5]) + [o + 1 for o in off[5:]]
    first = [1] + list(off[1:])
    swapped = list(off)
    swapped[8], swapped[9] = swapped[9], swapped[8]
    beyond = list(off)
    beyond[14] = size + 10
    return {"shifted": shifted, "first": first, "swapped": swapped, "beyond": beyond}


def test_hints_never_change_the_outcome(ctx, chain):
    files = [(chain.data, chain.crc), (chain.file(b9=cc.flip_kes_byte(chain.blobs[9]))[0], chain.crc),
             (chain.file(b12=chain.relinked12)[0], chain.crc)]
    for data, crc in files:
        plain = cm.parse_chunk(data, crc, SPKP, None)
        for name, hint in _hint_corruptions(chain.off, len(data)).items():
            g = _both(ctx, data, crc, hint)
            cm.assert_same(g, plain, skip=("rescanned_from",))
            assert g["rescanned_from"] < len(data), name


def _sweep_cases(chain, seed):
    r = random.Random(seed)
    muts = ["intact", "seg", "kes", "relink", "cut", "stray", "byron", "trusted_damage", "header_damage"]
    out = []
    for _ in range(30):
        kind = r.choice(muts)
        i = r.choice([1, 3, 5, 9, 11, 13, 15, 19, 21, 23])
        repl = {"seg": lambda: {f"b{i}": cc.flip_segment_byte(chain.blobs[i])},
                "kes": lambda: {f"b{i}": cc.flip_kes_byte(chain.blobs[i], r.randrange(448))},
                "relink": lambda: {"b12": chain.relinked12},
                "byron": lambda: {f"b{i}": chain.byron},
                "trusted_damage": lambda: {f"b{i}": cc.flip_segment_byte(chain.blobs[i])},
                "header_damage": lambda: {f"b{i}": cc.flip_header_byte(chain.blocks[i])}}.get(kind, dict)()
        data, off, crc = chain.file(**repl)
        if kind in ("seg", "kes"):
            crc = list(chain.crc)                                # the index keeps the old checksum
        if kind == "cut":
            data = data[:off[i] + 1 + r.randrange(len(chain.blobs[i]) - 1)]
        if kind == "stray":
            data = data + rbytes(r, 1 + r.randrange(9))
        index = r.choice(["full", "none", "first10", "stale"])
        if index == "none":
            crc_in, off_in = None, None
        elif index == "first10":
            crc_in, off_in = crc[:10], off[:10]
        else:
            crc_in, off_in = list(crc), list(off)
            if index == "stale":
                crc_in[r.randrange(24)] ^= 1 + r.getrandbits(20)
        hint = r.choice(["good", "none", "shifted", "first", "swapped", "beyond"])
        if off_in is not None and hint == "none":
            off_in = None
        elif off_in is not None and hint != "good" and len(off_in) == 24:
            off_in = _hint_corruptions(off_in, len(data))[hint]
        out.append((kind, index, hint, data, crc_in, off_in))
    return out


def test_seeded_sweep(ctx, chain):
    cases = _sweep_cases(chain, SWEEP_SEED)
    models = [cm.parse_chunk(d, c, SPKP, o) for _, _, _, d, c, o in cases]
    seen = [m["outcome"] for m in models]
    for outcome in range(5):
        assert seen.count(outcome) >= 2, (outcome, seen)          # the seed covers every outcome twice
    for (kind, index, hint, d, c, o), want in zip(cases, models):
        got = ctx.validate_chunk(d, c, o, SPKP)
        cm.assert_same(got, want)
        cm.assert_same(got, cm.parse_chunk(d, c, SPKP, None), skip=("rescanned_from",))


@pytest.fixture(scope="module")
def immdb(ctx, tmp_path_factory):
    from fractions import Fraction
    from helpers import b2b
    cfg = dict(npools=20, stake_offset=1, f=Fraction(1, 2), slots_per_kes_period=SPKP, max_kes_evo=62,
               eta0=b2b(b"replay-genesis"), seed=b"\x2a" * 32)
    data = immutable.make_multi_epoch_chain(ctx, cfg, 2, 600, 200)
    path = str(tmp_path_factory.mktemp("immdb") / "immutable")
    n = immutable.write_immutable(path, data["arena"], data["off"], data["len"], data["slots"],
                                  data["header_hash"], 250)
    return path, n


def _model_report(path):
    return immutable.validate_immutable(None, path, SPKP, parse=lambda d, c, o: cm.parse_chunk(d, c, SPKP, o))


def test_synthesized_immutable_db(ctx, immdb):
    path, n = immdb
    rows = immutable.validate_immutable(ctx, path, SPKP)
    assert len(rows) == n >= 4
    for row in rows:
        assert row["outcome"] == abi.CHUNK_OK and row["fits"] and row["checked"] == 0
        assert row["entries_match"]
        assert row["entries"] == open(os.path.join(path, f"{row['chunk']:05d}.secondary"), "rb").read()
    assert rows == _model_report(path)


def test_damaged_immutable_db_matches_the_model(ctx, immdb, tmp_path):
    import shutil
    # a missing index: every block of that chunk takes the integrity check
    path = str(tmp_path / "a" / "immutable")
    shutil.copytree(immdb[0], path)
    os.remove(os.path.join(path, "00001.secondary"))
    rows = immutable.validate_immutable(ctx, path, SPKP)
    assert rows == _model_report(path)
    assert len(rows) >= 2 and not rows[1]["entries_match"] and rows[1]["checked"] >= 1
    # one block byte flipped under an intact index: the walk ends in that chunk
    path = str(tmp_path / "b" / "immutable")
    shutil.copytree(immdb[0], path)
    p = os.path.join(path, "00002.chunk")
    raw = bytearray(open(p, "rb").read())
    raw[len(raw) // 2] ^= 0x10
    open(p, "wb").write(bytes(raw))
    rows = immutable.validate_immutable(ctx, path, SPKP)
    assert rows == _model_report(path)
    assert rows[-1]["chunk"] == 2 and rows[-1]["outcome"] != abi.CHUNK_OK and rows[-1]["checked"] <= 1


def _harness(tmp_path, name, data, crc, off, entries=None):
    d = tmp_path / name
    d.mkdir()
    (d / "00000.chunk").write_bytes(bytes(data))
    if crc is not None:
        sec = b"".join(int(o).to_bytes(8, "big") + bytes(4) + int(c).to_bytes(4, "big") + bytes(40)
                       for o, c in zip(off, crc))
        (d / "00000.secondary").write_bytes(entries if entries is not None else sec)
    out = subprocess.run([HARNESS, "--validate-chunk", str(d), "0", str(SPKP)], check=True, capture_output=True,
                         text=True, timeout=120).stdout
    return json.loads(out.strip().splitlines()[-1])


def test_harness_phase_prints_what_the_binding_returns(ctx, chain, tmp_path):
    intact = ctx.validate_chunk(chain.data, chain.crc, chain.off, SPKP)
    bad = chain.file(b9=cc.flip_kes_byte(chain.blobs[9]))[0]
    cases = {"intact": (chain.data, chain.crc, chain.off, intact["entries"]), "kes": (bad, chain.crc, chain.off, None),
             "noindex": (chain.file(b12=chain.relinked12)[0], None, None, None)}
    for name, (data, crc, off, entries) in cases.items():
        g = ctx.validate_chunk(data, crc, off, SPKP)
        j = _harness(tmp_path, name, data, crc, off, entries)
        assert j["phase"] == "validate_chunk" and j["outcome"] == abi.CHUNK_OUTCOMES[g["outcome"]]
        for k in ("integrity_bits", "blocks", "checked", "truncate_at", "rescanned_from", "err_slot",
                  "actual_prev_is_genesis"):
            assert j[k] == g[k], (name, k)
        for k in ("err_hash", "expected_prev", "actual_prev", "entries"):
            assert bytes.fromhex(j[k]) == g[k], (name, k)
        assert j["block_no"] == [int(x) for x in g["block_no"]]
        assert j["integrity"] == [int(x) for x in g["integrity"]]
        assert j["entries_match"] == (name == "intact")
