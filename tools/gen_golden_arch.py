#!/usr/bin/env python3
"""Generate ``tests/golden/arch_variants.npz``: the REFERENCE's outputs for architectures other than the shipped
(embed_dim 64, n_heads 4).  CPU only, build container only.

Like ``oracle/gen_golden.py`` it imports the reference (read-only, with an empty ``dendropy`` stub because
phyloformer/data.py imports it at module top) and writes data only.  For every architecture (E, NH, n_blocks) the
weights are ``phyloformer_amd.weights.random_weights(seed, ..., scale=2.0)`` - scale 2 spreads the distances over
~0.2-3.2, where a mixed-up head or channel shows (the default init gives nearly constant outputs) - loaded into the
reference's ``Phyloformer(n_blocks=, n_heads=, h_dim=)`` by reshaping to its conv shapes.  Stored per architecture:
the architecture, seed, scale, the sha256 of the float32 weight blob (tests regenerate the weights and check the hash
first, so a change of numpy's random stream fails loudly), and per alignment ``idx`` and the module's fp32 output.

    python tools/gen_golden_arch.py [--ref /path/to/reference]
"""
import argparse
import hashlib
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "arch_variants.npz")
ARCHS = [(32, 2, 2), (40, 5, 2), (64, 8, 2), (96, 4, 2), (128, 8, 3), (256, 4, 1)]     # (embed_dim, n_heads, n_blocks)
SCALE = 2.0


def alignments(k):
    """Per architecture: a simulated alignment, a gapped one with L < 32, one with N = 2, and 0_20_tips.fa."""
    from phyloformer_amd.fasta import load_alignment
    from phyloformer_amd.msa_sim import simulate_batch
    out = [simulate_batch(1, 12, 40, seed=500 + k)[0],
           simulate_batch(1, 7, 20, seed=600 + k, gaps=True)[0],
           simulate_batch(1, 2, 50, seed=700 + k)[0]]
    idx, _ids = load_alignment(os.path.join(REPO, "data", "testdata", "msas", "0_20_tips.fa"))
    out.append(np.ascontiguousarray(idx, dtype=np.uint8))
    return out


def weight_sha(w) -> str:
    return hashlib.sha256(w.blob().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("PF_REFERENCE", os.path.join(os.sep, "root", "reference")))
    args = ap.parse_args()
    stub = tempfile.mkdtemp(prefix="pf_stub_")
    os.makedirs(os.path.join(stub, "dendropy"))
    open(os.path.join(stub, "dendropy", "__init__.py"), "w").close()
    sys.path.insert(0, stub)
    sys.path.insert(0, args.ref)
    sys.path.insert(0, REPO)
    import torch
    from phyloformer.model import Phyloformer
    from phyloformer_amd.weights import random_weights

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {"archs": np.array(ARCHS, dtype=np.int32), "scale": np.float64(SCALE)}
    for k, (E, H, nb) in enumerate(ARCHS):
        seed = 1000 + k
        w = random_weights(seed, n_blocks=nb, n_heads=H, embed_dim=E, scale=SCALE)
        model = Phyloformer(n_blocks=nb, n_heads=H, h_dim=E)
        sd = model.state_dict()
        new = {}
        for key, ref_t in sd.items():
            if key in w.tensors:
                new[key] = torch.from_numpy(w.tensors[key].reshape(tuple(ref_t.shape)).copy())
            else:
                new[key] = ref_t            # buffers (seq2pair)
        missing = set(w.tensors) - set(new)
        assert not missing, missing
        model.load_state_dict(new)
        model.eval()
        out[f"a{k}/seed"] = np.int64(seed)
        out[f"a{k}/sha"] = np.array(weight_sha(w))
        for c, idx in enumerate(alignments(k)):
            x = torch.nn.functional.one_hot(torch.from_numpy(idx.astype(np.int64)), num_classes=22)
            x = x.permute(2, 1, 0)[None].float()                    # [1, 22, L, N] (infer_alns.py:112)
            with torch.no_grad():
                pred = model(x).reshape(-1).numpy().astype(np.float32)
            out[f"a{k}/idx{c}"] = idx
            out[f"a{k}/out{c}"] = pred
            print(f"E={E} H={H} nb={nb} case {c}: {idx.shape} -> {pred.min():.3f} .. {pred.max():.3f}", flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
