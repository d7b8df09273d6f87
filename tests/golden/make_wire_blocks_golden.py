#!/usr/bin/env python3
"""Copy the reference's golden wire blocks into a data fixture.

Run where the reference tree is present (the GPU box never needs it):
    python tests/golden/make_wire_blocks_golden.py
Writes tests/golden/wire_blocks.json (data only, hex):
  blocks   the distinct Block_* files of golden/cardano/CardanoNodeToNodeVersion{5,6,7} (name, the
           versions that hold these bytes, the wire bytes, the disk tag), each checked here to be
           exactly the wrapper #6.24(bytes) around the bytes of the matching
           golden/cardano/disk/Block_* file, and to wrap again to the same bytes.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "..", "ouroboros-consensus_amd")]
from praos_hip import blockfetch as bf  # noqa: E402

REF = "/root/reference/ouroboros-consensus-cardano/golden/cardano"
VERSIONS = (5, 6, 7)
NAMES = ("Byron_EBB", "Byron_regular", "Shelley", "Allegra", "Mary", "Alonzo", "Babbage", "Conway")


def main():
    blocks, total = [], 0
    for tag, name in enumerate(NAMES):
        disk = open(os.path.join(REF, "disk", "Block_" + name), "rb").read()
        seen = {}
        for v in VERSIONS:
            raw = open(os.path.join(REF, f"CardanoNodeToNodeVersion{v}", "Block_" + name), "rb").read()
            total += 1
            seen.setdefault(raw, []).append(v)
        for raw, vs in seen.items():
            status, t, off, ln = bf.unwrap_block(raw)
            assert (status, t) == (bf.WIRE_OK, tag), (name, vs, status, t)
            assert raw[:2] == b"\xd8\x18" and raw[2] in (0x58, 0x59) and off + ln == len(raw), (name, vs)
            assert raw[off:] == disk, (name, vs)
            assert bf.wrap_block(disk) == raw, (name, vs)
            blocks.append({"name": name, "versions": vs, "disk_tag": tag, "wire": raw.hex()})
    assert total == 24, total
    with open(os.path.join(HERE, "wire_blocks.json"), "w") as f:
        json.dump({"n_eras": bf.N_ERAS, "blocks": blocks}, f, indent=1)
        f.write("\n")
    for b in blocks:
        print(b["name"], b["versions"], "disk tag", b["disk_tag"], len(b["wire"]) // 2, "bytes")


if __name__ == "__main__":
    main()
