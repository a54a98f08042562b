#!/usr/bin/env python3
"""FastME ``-m N -n B`` goldens (neighbour joining, then balanced NNIs) for the 20 test MSAs: what ``--bme``
(phyloformer_amd/bme.py) is pinned against in tests/test_bme.py, so that the tests need no FastME binary.

Needs the built library (``format_phylip``) and a FastME 2.1.6 binary, whose path is the argument.  The reference's
own pf.ckpt distances (tests/golden/e2e_testdata.npz) are written with this build's ``format_phylip`` and the trees
stored in ``tests/golden/fastme_nj_bnni.json`` under the sha256 of that PHYLIP text, as ``fastme_nni_spr.json`` does:

    {"<sha256 of the PHYLIP bytes>": {"source": "<npz>:<key>", "tree": "<Newick text FastME wrote>"}, ...}

FastME keeps NJ's own branch lengths when it performs no swap, so pin topologies against these trees and balanced
lengths against ``fastme_nni_spr.json``.

    python tools/gen_golden_fastme_bnni.py PATH/TO/fastme
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


def main(fastme):
    from phyloformer_amd import fasta
    from phyloformer_amd.hostio import format_phylip
    from phyloformer_amd.phylip import vec_to_matrix
    msas = os.path.join(REPO, "data", "testdata", "msas")
    gold = np.load(os.path.join(REPO, "tests", "golden", "e2e_testdata.npz"))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(os.listdir(msas)):
            stem = name[:-3]
            _idx, ids = fasta.load_alignment(os.path.join(msas, name))
            n = len(ids)
            dm = vec_to_matrix(gold[f"pf/{stem}"], n).astype(np.float64)
            text = format_phylip(dm[np.triu_indices(n, 1)], ids)
            src, dst = os.path.join(tmp, "m.phy"), os.path.join(tmp, "t.nwk")
            with open(src, "wb") as fh:
                fh.write(text)
            subprocess.run([fastme, "-i", src, "-o", dst, "-m", "N", "-n", "B"], check=True, capture_output=True, cwd=tmp)
            with open(dst) as fh:
                tree = fh.read().strip()
            out[hashlib.sha256(text).hexdigest()] = {"source": f"e2e_testdata.npz:pf/{stem}", "tree": tree}
            os.unlink(dst)
            print(stem, len(tree), "chars")
    with open(os.path.join(REPO, "tests", "golden", "fastme_nj_bnni.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
