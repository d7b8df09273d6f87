#!/usr/bin/env python3
"""Copy the reference's Byron golden blocks into a data fixture.

Run where the reference tree is present (the GPU box never needs it):
    python tests/golden/make_byron_golden.py
Writes tests/golden/byron_blocks.json (data only, hex): the stored EBB and main block of
ouroboros-consensus-cardano/golden/byron/disk (87 and 862 bytes) and the serialised
HeaderHash of the main block (34 bytes).  The reference's golden tests compare these files
byte for byte, so the main block's PBFT signature and body proof are reference outputs; the
EBB's header hash is the main block's prevHash, so the two written back to back are a
two-block chunk that lines up.
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/ouroboros-consensus-cardano/golden/byron/disk"
FILES = {"ebb": "Block_EBB", "main": "Block_regular", "header_hash": "HeaderHash"}


def main():
    out = {k: open(os.path.join(REF, f), "rb").read().hex() for k, f in FILES.items()}
    out["protocol_magic"] = 55550001
    with open(os.path.join(HERE, "byron_blocks.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
