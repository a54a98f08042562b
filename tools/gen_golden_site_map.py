#!/usr/bin/env python3
"""Generate ``tests/golden/site_map.npz``: the reference's own per-site head output for two shipped MSAs.

Runs the REFERENCE on the CPU the way ``oracle/gen_golden.py`` does (build container only: the reference is not part
of this repository) with a forward hook on ``pwFNN[0]`` (model.py:182), as the ``logits`` of ``taps_tiny.npz``.  Only
data is written: per stem the residue indices ``uint8 [N][L]``, the head logits ``float32 [P][L]`` and the reference's
distances ``float32 [P]`` (their site mean after softplus, model.py:185).

    python tools/gen_golden_site_map.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
STEMS = ("0_20_tips", "1_30_tips")


def main():
    from oracle.gen_golden import GOLD, _import_reference, _load_model, _onehot
    from phyloformer_amd.fasta import load_alignment
    torch, Phyloformer, _ref_load, _stub = _import_reference()
    model = _load_model(torch, Phyloformer, "pf")
    out = {}
    for stem in STEMS:
        idx, _ids = load_alignment(os.path.join(REPO, "data", "testdata", "msas", f"{stem}.fa"))
        got = {}
        hook = model.pwFNN[0].register_forward_hook(
            lambda mod, inp, res: got.__setitem__("logits", res[0, 0].numpy().astype(np.float32)))
        with torch.no_grad():
            dist = model(_onehot(torch, idx)).numpy().astype(np.float32)
        hook.remove()
        out[f"{stem}/idx"], out[f"{stem}/logits"], out[f"{stem}/dist"] = idx, got["logits"], dist
        print(stem, idx.shape, got["logits"].shape, dist.shape)
    path = os.path.join(GOLD, "site_map.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
