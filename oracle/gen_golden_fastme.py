#!/usr/bin/env python3
"""FastME ``--nni --spr`` goldens: the trees of the reference README's tree pipeline (README.md:83-96 of the
reference) for the 20 test MSAs, so that the tests of that pipeline need no FastME binary.

Build container only; needs the built library (``format_phylip``) and the FastME binary the reference checkout
ships (``bin/bin_linux/fastme``), whose path is the argument.  Two sets of distances go through it: the reference's
own pf.ckpt distances (tests/golden/e2e_testdata.npz) and the distances the GPU wrote in round 2
(tests/golden/gpu_distances_r02.npz).  Each matrix is written with this build's ``format_phylip``, exactly as the
tests write it, and stored in ``tests/golden/fastme_nni_spr.json`` under the sha256 of that PHYLIP text:

    {"<sha256 of the PHYLIP bytes>": {"source": "<npz>:<key>", "tree": "<Newick text FastME wrote>"}, ...}

A test looks its tree up by the hash of the text it writes, so a change in ``format_phylip`` shows up as a missing
key, not as a tree of another matrix.

    python oracle/gen_golden_fastme.py PATH/TO/fastme
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
SOURCES = [("e2e_testdata.npz", "pf/{}"), ("gpu_distances_r02.npz", "{}")]


def main(fastme):
    from phyloformer_amd import fasta
    from phyloformer_amd.hostio import format_phylip
    from phyloformer_amd.phylip import vec_to_matrix
    msas = os.path.join(REPO, "data", "testdata", "msas")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for fname, key in SOURCES:
            gold = np.load(os.path.join(REPO, "tests", "golden", fname))
            for name in sorted(os.listdir(msas)):
                stem = name[:-3]
                _idx, ids = fasta.load_alignment(os.path.join(msas, name))
                n = len(ids)
                # what tests/test_treecmp.py feeds FastME: the float64 matrix's upper triangle through format_phylip
                dm = vec_to_matrix(gold[key.format(stem)], n).astype(np.float64)
                text = format_phylip(dm[np.triu_indices(n, 1)], ids)
                src, dst = os.path.join(tmp, "m.phy"), os.path.join(tmp, "t.nwk")
                with open(src, "wb") as fh:
                    fh.write(text)
                subprocess.run([fastme, "-i", src, "-o", dst, "--nni", "--spr"], check=True, capture_output=True, cwd=tmp)
                with open(dst) as fh:
                    tree = fh.read().strip()
                out[hashlib.sha256(text).hexdigest()] = {"source": f"{fname}:{key.format(stem)}", "tree": tree}
                os.unlink(dst)
                print(fname, stem, len(tree), "chars")
    with open(os.path.join(REPO, "tests", "golden", "fastme_nni_spr.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
