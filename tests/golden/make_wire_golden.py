#!/usr/bin/env python3
"""Copy the reference's golden wire headers into a data fixture.

Run where the reference tree is present (the GPU box never needs it):
    python tests/golden/make_wire_golden.py
Writes tests/golden/wire_headers.json (data only, hex):
  headers   the distinct decodable Header_* files of golden/cardano/CardanoNodeToNodeVersion{5,6,7}
            (name, the versions that hold these bytes, the wire bytes, and what the wrapper says:
            era index, Byron kind and size hint), each checked here to unwrap to exactly the header
            item inside the matching golden/cardano/disk/Block_* file;
  disabled  the three files that hold the text "HardForkEncoderDisabledEra ..." instead of a header;
  disk      the header item of each disk block (name -> hex) and the block's disk tag.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "..", "ouroboros-consensus_amd")]
import cbor_min  # noqa: E402
from praos_hip import wire  # noqa: E402

REF = "/root/reference/ouroboros-consensus-cardano/golden/cardano"
VERSIONS = (5, 6, 7)
NAMES = ("Byron_EBB", "Byron_regular", "Shelley", "Allegra", "Mary", "Alonzo", "Babbage", "Conway")


def disk_header(block: bytes):
    """(disk tag, header item bytes) of a stored HardForkBlock: [tag, [header, ...]]."""
    top = cbor_min.decode(block)
    assert top.end == len(block) and len(top.value) == 2
    tag, inner = top.value
    return tag.value, inner.value[0].raw(block)


def main():
    disk = {}
    for name in NAMES:
        tag, hdr = disk_header(open(os.path.join(REF, "disk", "Block_" + name), "rb").read())
        disk[name] = {"disk_tag": tag, "header": hdr.hex()}
    headers, disabled, total = [], [], 0
    for name in NAMES:
        seen = {}
        for v in VERSIONS:
            raw = open(os.path.join(REF, f"CardanoNodeToNodeVersion{v}", "Header_" + name), "rb").read()
            if raw.startswith(b"HardForkEncoderDisabledEra"):
                disabled.append({"name": name, "version": v, "wire": raw.hex()})
                continue
            total += 1
            seen.setdefault(raw, []).append(v)
        for raw, vs in seen.items():
            status, era, kind, hint, off, ln = wire.unwrap(raw)
            assert status == wire.WIRE_OK, (name, vs, status)
            assert raw[off:off + ln] == bytes.fromhex(disk[name]["header"]), (name, vs)
            assert wire.wrap(era, raw[off:off + ln], kind, hint) == raw, (name, vs)
            headers.append({"name": name, "versions": vs, "wire": raw.hex(), "era": era, "byron_kind": kind,
                            "size_hint": hint})
    assert total == 21 and len(disabled) == 3, (total, len(disabled))
    out = {"n_eras": wire.N_ERAS, "headers": headers, "disabled": disabled, "disk": disk}
    with open(os.path.join(HERE, "wire_headers.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for h in headers:
        print(h["name"], h["versions"], "era", h["era"], "kind", h["byron_kind"], "hint", h["size_hint"],
              len(h["wire"]) // 2, "bytes; disk tag", disk[h["name"]]["disk_tag"])


if __name__ == "__main__":
    main()
