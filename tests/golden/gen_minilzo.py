#!/usr/bin/env python3
"""Record what minilzo answers on the inputs of tests/test_oracle_lzo.py, so that those tests also run where minilzo
cannot be built (oracle/_ref/libminilzo.so is compiled from the reference tree by oracle/Makefile).

Run where oracle/_ref/libminilzo.so exists (`make -C oracle`):   python tests/golden/gen_minilzo.py

Writes tests/golden/minilzo.json:
    datasets           one record per input of _datasets(), in order: its length and digest; minilzo's stream (length,
                       digest, and its bytes where they differ from the oracle's stream); the digest of the oracle's
                       stream, which minilzo decoded back to the input
    reference_vectors  the decoder cases of lzo.json minilzo decodes to the expected bytes
    quirk_238          minilzo's stream of test_238_byte_quirk's input
Only minilzo's outputs are stored (hex), nothing of its source.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import oracle_lib  # noqa: E402
from tests.conftest import golden_bytes  # noqa: E402
from tests.test_oracle_lzo import _datasets, quirk_238_input  # noqa: E402


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def main():
    m, orc = oracle_lib.load_minilzo(), oracle_lib.load()
    if m is None:
        sys.exit("oracle/_ref/libminilzo.so not built (needs the reference tree); the fixture is already committed")
    datasets = []
    for d in _datasets():
        st, z = orc.lzo_compress(d)
        zm = m.compress(d)
        assert st == 0 and m.decompress(z, len(d)) == (0, d) and orc.lzo_uncompress(zm, len(d)) == (0, d)
        r = {"n": len(d), "sha256": sha(d), "oracle_sha256": sha(z), "minilzo_len": len(zm), "minilzo_sha256": sha(zm)}
        if zm != z:
            r["minilzo"] = zm.hex()
        datasets.append(r)
    with open(os.path.join(HERE, "lzo.json")) as f:
        cases = json.load(f)
    agreed = []
    for case in cases:
        if case["status"] == 0:
            want = golden_bytes(case["out"])
            if m.decompress(golden_bytes(case["src"]), len(want)) == (0, want):
                agreed.append(case["name"])
    out = {"datasets": datasets, "reference_vectors": agreed, "quirk_238": m.compress(quirk_238_input()).hex()}
    with open(os.path.join(HERE, "minilzo.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("minilzo.json: %d datasets (%d streams stored), %d reference vectors" % (
        len(datasets), sum("minilzo" in r for r in datasets), len(agreed)))


if __name__ == "__main__":
    main()
