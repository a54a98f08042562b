#!/usr/bin/env python3
"""FastME ``-m N -s`` goldens (neighbour joining, then balanced SPR moves): what ``--spr`` (phyloformer_amd/bme.py::
bme_spr) is pinned against in tests/test_spr.py, so that the tests need no FastME binary.

Needs the built library (``format_phylip``) and a FastME 2.1.6 binary, whose path is the argument.  The matrices are the
reference's own pf.ckpt distances of the 20 test MSAs (tests/golden/e2e_testdata.npz) and the eight harder ones of
tests/helpers/spr_check.py::harder_cases; each is written with this build's ``format_phylip`` and its tree stored in
``tests/golden/fastme_nj_spr.json`` under the sha256 of that PHYLIP text, in ``fastme_nj_bnni.json``'s layout:

    {"<sha256 of the PHYLIP bytes>": {"source": "<where the matrix comes from>", "tree": "<Newick text FastME wrote>"}, ...}

FastME keeps NJ's own branch lengths when it performs no move.

    python tools/gen_golden_fastme_spr.py PATH/TO/fastme
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def matrices():
    """``(source, ids, float64 [P_n])`` of the 28 matrices."""
    from helpers import spr_check
    from phyloformer_amd import fasta
    msas = os.path.join(REPO, "data", "testdata", "msas")
    gold = np.load(os.path.join(REPO, "tests", "golden", "e2e_testdata.npz"))
    for name in sorted(os.listdir(msas)):
        _idx, ids = fasta.load_alignment(os.path.join(msas, name))
        yield f"e2e_testdata.npz:pf/{name[:-3]}", ids, gold[f"pf/{name[:-3]}"].astype(np.float64)
    for label, ids, vec in spr_check.harder_cases():
        yield f"tests/helpers/spr_check.py:{label}", ids, vec.astype(np.float64)


def main(fastme):
    from phyloformer_amd.hostio import format_phylip
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for source, ids, vec in matrices():
            text = format_phylip(vec, ids)
            src, dst = os.path.join(tmp, "m.phy"), os.path.join(tmp, "t.nwk")
            with open(src, "wb") as fh:
                fh.write(text)
            subprocess.run([fastme, "-i", src, "-o", dst, "-m", "N", "-s"], check=True, capture_output=True, cwd=tmp)
            with open(dst) as fh:
                tree = fh.read().strip()
            out[hashlib.sha256(text).hexdigest()] = {"source": source, "tree": tree}
            os.unlink(dst)
            print(source, len(tree), "chars")
    with open(os.path.join(REPO, "tests", "golden", "fastme_nj_spr.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
