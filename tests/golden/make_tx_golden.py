#!/usr/bin/env python3
"""Copy the reference's golden blocks and transactions into a data fixture.

Run where the reference tree is present (the GPU box never needs it):
    python tests/golden/make_tx_golden.py
Writes tests/golden/tx_golden.json (data only, hex): from
ouroboros-consensus-cardano/golden/cardano/CardanoNodeToNodeVersion7 the files Block_<era>,
GenTx_<era> and GenTxId_<era> of the six Shelley-based eras, Block_Byron_regular,
Block_Byron_EBB and GenTx_Byron, each as it is on disk.  A Block_ file is the stored block
inside a tag-24 byte string; GenTx_<era> is [era index, tag-24 bytes of the transaction] and
GenTxId_<era> [era index, hash]; GenTx_Byron is [0, [0, [tx, witnesses]]].  Each golden block
holds the one transaction of its era's GenTx file.
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/ouroboros-consensus-cardano/golden/cardano/CardanoNodeToNodeVersion7"
ERAS = ("Shelley", "Allegra", "Mary", "Alonzo", "Babbage", "Conway")


def rd(name):
    return open(os.path.join(REF, name), "rb").read().hex()


def main():
    out = {"eras": {e: {"block": rd("Block_" + e), "gen_tx": rd("GenTx_" + e), "gen_tx_id": rd("GenTxId_" + e)}
                    for e in ERAS},
           "byron": {"main": rd("Block_Byron_regular"), "ebb": rd("Block_Byron_EBB"), "gen_tx": rd("GenTx_Byron")}}
    with open(os.path.join(HERE, "tx_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
