#!/usr/bin/env python3
"""Copy the reference's PBFT fixtures into a data file.

Run where the reference tree is present (the GPU box never needs it):
    python tests/golden/make_pbft_golden.py
Writes tests/golden/pbft_golden.json (data only, hex):
  * the one heavyDelegation entry of ouroboros-consensus-cardano/test/tools-test/disk/config/
    byron/genesis.json: its map key (the genesis key hash, hashVerKey of issuerPk), issuerPk and
    delegatePk (base64 in the file, 64 bytes each);
  * ouroboros-consensus-cardano/golden/byron/disk/ChainDepState, the serialised PBftState the
    reference's golden test compares byte for byte.
"""
import base64
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/ouroboros-consensus-cardano"


def main():
    g = json.load(open(os.path.join(REF, "test/tools-test/disk/config/byron/genesis.json")))
    (key_hash, d), = g["heavyDelegation"].items()
    out = {"genesis_key_hash": key_hash,
           "issuer_pk": base64.b64decode(d["issuerPk"]).hex(),
           "delegate_pk": base64.b64decode(d["delegatePk"]).hex(),
           "chain_dep_state": open(os.path.join(REF, "golden/byron/disk/ChainDepState"), "rb").read().hex()}
    with open(os.path.join(HERE, "pbft_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
