#!/usr/bin/env python3
"""FastME goldens from its default start tree, BIONJ, for the 20 test MSAs: what ``--bionj``
(phyloformer_amd/bionj.py) and the refinements started from it are pinned against in tests/test_bionj.py, so that the
tests need no FastME binary.

Needs the built library (``format_phylip``) and a FastME 2.1.6 binary, whose path is the argument.  Two sources of
distances - the reference's own pf.ckpt distances (tests/golden/e2e_testdata.npz) and the GPU distances of an earlier
run (tests/golden/gpu_distances_r02.npz) - are written with this build's ``format_phylip``, and three trees per matrix
stored in ``tests/golden/fastme_bionj.json`` under the sha256 of that PHYLIP text:

    {"<sha256 of the PHYLIP bytes>": {"source": "<npz>:<key>", "bionj": "<-m I>", "bnni": "<-m I -n B>",
                                      "spr": "<-m I -s>"}, ...}

FastME keeps its start tree's branch lengths when a search performs no move.

    python tools/gen_golden_fastme_bionj.py PATH/TO/fastme
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
RUNS = [("bionj", ["-m", "I"]), ("bnni", ["-m", "I", "-n", "B"]), ("spr", ["-m", "I", "-s"])]


def main(fastme):
    from phyloformer_amd import fasta
    from phyloformer_amd.hostio import format_phylip
    from phyloformer_amd.phylip import vec_to_matrix
    msas = os.path.join(REPO, "data", "testdata", "msas")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for npz, pattern in SOURCES:
            gold = np.load(os.path.join(REPO, "tests", "golden", npz))
            for name in sorted(os.listdir(msas)):
                stem = name[:-3]
                _idx, ids = fasta.load_alignment(os.path.join(msas, name))
                n = len(ids)
                dm = vec_to_matrix(gold[pattern.format(stem)], n).astype(np.float64)
                text = format_phylip(dm[np.triu_indices(n, 1)], ids)
                src, dst = os.path.join(tmp, "m.phy"), os.path.join(tmp, "t.nwk")
                with open(src, "wb") as fh:
                    fh.write(text)
                entry = {"source": f"{npz}:{pattern.format(stem)}"}
                for key, flags in RUNS:
                    subprocess.run([fastme, "-i", src, "-o", dst, *flags], check=True, capture_output=True, cwd=tmp)
                    with open(dst) as fh:
                        entry[key] = fh.read().strip()
                    os.unlink(dst)
                out[hashlib.sha256(text).hexdigest()] = entry
                print(npz, stem, len(entry["bionj"]), "chars")
    with open(os.path.join(REPO, "tests", "golden", "fastme_bionj.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
