"""-m gpu: the generic float64 path (csrc/pf_generic.hip.h) - checkpoints of any embed_dim / n_heads, and the shipped
(64, 4) checkpoints forced onto it with option "generic".

Bounds: against the reference's fp32 outputs 1e-4 (the contract); against the float64 oracle 1e-9 + 6e-8 max|want|
(the result is narrowed to float once at the end: half an ulp of the largest distance), as tests/test_gpu_precise.py.
"""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import pf_oracle as O
from phyloformer_amd.msa_sim import simulate_batch
from phyloformer_amd.weights import random_weights

from test_arch_host import arch_weights, cases

pytestmark = pytest.mark.gpu
CKPTS = ("pf", "pf_base", "pf_indel", "pf_cherry", "pf_selreg")


def _f64(w, idx):
    return O.forward_batch(w.tensors, idx, n_blocks=w.n_blocks, n_heads=w.n_heads, dtype=np.float64)


def _bound(want):
    return 1e-9 + 6e-8 * float(np.abs(want).max())


def test_golden_architectures_against_the_reference(golden):
    """Every architecture of arch_variants.npz (E = 32 ... 256, n_heads 2 ... 8, E = 40 with padded channels) and
    every alignment (L < 32, N = 2, gaps, the reference's 0_20_tips.fa) against the reference's own fp32 outputs and
    the float64 oracle; only the generic kernels run."""
    from phyloformer_amd.engine import Engine
    g = golden("arch_variants.npz")
    worst_ref = 0.0
    for k in range(len(g["archs"])):
        w = arch_weights(g, k)
        with Engine(w, 0) as e:
            assert e.architecture == (w.n_blocks, w.n_heads, w.embed_dim)
            e.set_option("profile", 1)
            for idx, want in cases(g, k):
                got = e.forward(idx).astype(np.float64)
                err_ref = float(np.abs(got - want).max())
                assert err_ref <= 1e-4, (k, idx.shape, err_ref)
                worst_ref = max(worst_ref, err_ref)
                f64 = _f64(w, idx[None])[0]
                assert float(np.abs(got - f64).max()) <= _bound(f64), (k, idx.shape)
            assert e.profile_get("generic")[0] > 0 and e.profile_get("main")[0] == 0
            assert e.profile_get("precise")[0] == 0
    print(f"generic path vs reference: worst {worst_ref:.3e}")


@pytest.mark.parametrize("arch", [(40, 5, 2), (128, 8, 3)])
def test_edge_shapes_batches_and_emulated_shards(arch):
    """2 x 1, 3 x 2, ragged reduce axes (70 sites, 78 pairs: two chunks each), gaps, a batch of 3: the float64 bound,
    the same bits one alignment at a time and under a 1 MB workspace budget, and the emulated site shards within
    the float64 bound."""
    from phyloformer_amd.engine import Engine
    E, H, nb = arch
    w = random_weights(77, n_blocks=nb, n_heads=H, embed_dim=E, scale=2.0)
    shapes = [(2, 1, 1, False), (3, 2, 1, False), (5, 70, 1, False), (13, 9, 1, True), (4, 33, 3, True)]
    with Engine(w, 0) as e:
        for i, (n, l, b, gaps) in enumerate(shapes):
            idx = simulate_batch(b, n, l, seed=40 + i, gaps=gaps)
            got = e.forward(idx)
            want = _f64(w, idx)
            assert float(np.abs(got.astype(np.float64) - want).max()) <= _bound(want), (n, l, b)
            if b > 1:
                assert np.array_equal(np.stack([e.forward(x) for x in idx]), got)
                e.set_option("ws_limit_mb", 1)
                try:
                    assert np.array_equal(e.forward(idx), got)
                finally:
                    e.set_option("ws_limit_mb", 24576)
            sh = e.forward_shards_emulated(idx, 3).astype(np.float64)
            assert float(np.abs(sh - want).max()) <= _bound(want), (n, l, b)


def test_option_generic_on_the_shipped_checkpoints(weights, repo, golden):
    """"generic" = 1 on all five shipped checkpoints x the reference's 20 test MSAs: within 1e-4 of the reference's
    outputs, within float64 noise of the precise path, and only generic launches.  On a custom architecture the
    option cannot be switched off."""
    from phyloformer_amd.engine import Engine
    from phyloformer_amd.fasta import load_alignment
    gold = golden("e2e_testdata.npz")
    files = sorted(glob.glob(os.path.join(repo, "data", "testdata", "msas", "*.fa")))
    assert len(files) == 20
    alns = [(os.path.basename(f)[:-3], load_alignment(f)[0]) for f in files]
    for ck in CKPTS:
        with Engine(weights(ck), 0) as e:
            e.set_option("generic", 1)
            e.set_option("profile", 1)
            gen = {s: e.forward(idx) for s, idx in alns}
            assert e.profile_get("generic")[0] > 0 and e.profile_get("main")[0] == 0
            e.set_option("profile", 0)
            e.set_option("generic", 0)
            e.set_option("precise", 1)
            for s, idx in alns:
                ref = gold[f"{ck}/{s}"]
                assert float(np.abs(gen[s] - ref).max()) <= 1e-4, (ck, s)
                pre = e.forward(idx)
                assert float(np.abs(gen[s].astype(np.float64) - pre).max()) <= 1.2e-7 * max(1.0, float(np.abs(pre).max()))
    with Engine(random_weights(1, n_blocks=1, n_heads=2, embed_dim=32), 0) as e:
        e.set_option("generic", 1)
        e.set_option("precise", 0)              # accepted, no effect
        e.set_option("recheck_above", 0)
        with pytest.raises(ValueError, match="generic kernels only"):
            e.set_option("generic", 0)


def test_taps_of_a_custom_architecture():
    """debug_keep taps x1 ... x{n_blocks}: the residual stream after every block, narrowed to float with the true
    E = 40 channels, against the float64 oracle's."""
    from phyloformer_amd.engine import Engine
    E, H, nb = 40, 5, 2
    w = random_weights(5, n_blocks=nb, n_heads=H, embed_dim=E, scale=2.0)
    idx = simulate_batch(1, 6, 19, seed=3)[0]
    taps = {}
    O.forward(w.tensors, idx, n_blocks=nb, n_heads=H, dtype=np.float64, tap=lambda n, v: taps.__setitem__(n, v))
    with Engine(w, 0) as e:
        e.set_option("debug_keep", 1)
        e.forward(idx)
        for b in range(nb):
            got = e.debug_read(f"x{b + 1}").astype(np.float64)
            want = taps[f"block{b}.ffn"].reshape(-1)
            assert got.shape == want.shape
            assert float(np.abs(got - want).max()) <= 1e-9 + 1.2e-7 * float(np.abs(want).max()), b


def test_site_sharded_over_a_real_communicator():
    """pf_forward_sharded of a custom architecture over a single-rank RCCL communicator: n_blocks + 1 float64
    all-reduces, the bits of pf_forward; an empty site range joins the same collectives with zeros."""
    from phyloformer_amd.engine import Engine
    E, H, nb = 96, 4, 2
    w = random_weights(9, n_blocks=nb, n_heads=H, embed_dim=E, scale=2.0)
    idx = simulate_batch(3, 6, 41, seed=11)
    with Engine(w, 0) as e:
        want = e.forward(idx)
        e.set_option("force_rccl", 1)
        e.comm_init(e.unique_id(), 0, 1)
        e.profile_reset()
        got = e.forward_sharded(idx, 0, 41, 41)
        assert e.profile_get("collectives")[0] == nb + 1
        assert np.array_equal(got, want)
        e.profile_reset()
        zero = e.forward_sharded(np.zeros((3, 6, 0), np.uint8), 41, 41, 41)
        assert e.profile_get("collectives")[0] == nb + 1 and not zero.any()
        assert np.array_equal(e.forward(idx), want)


def test_cli_runs_a_custom_checkpoint(repo, tmp_path):
    """infer_alns.py on a Lightning .ckpt of a (128, 8, 3) model, --trees, three of the reference's test MSAs: the
    .phy distances match the float64 oracle to 1e-4 and the NJ trees are written."""
    torch = pytest.importorskip("torch")
    from phyloformer_amd.fasta import load_alignment
    from phyloformer_amd.phylip import pair_indices
    w = random_weights(3, n_blocks=3, n_heads=8, embed_dim=128, scale=2.0)
    sd = {"model." + k: torch.from_numpy(v.copy()) for k, v in w.tensors.items()}
    ckpt = tmp_path / "custom128.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": {}}, str(ckpt))
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    stems = ("0_20_tips", "1_30_tips", "2_40_tips")
    for s in stems:
        shutil.copy(os.path.join(repo, "data", "testdata", "msas", f"{s}.fa"), ind / f"{s}.fa")
    r = subprocess.run([sys.executable, os.path.join(repo, "infer_alns.py"), str(ckpt), str(ind), "-o", str(outd), "--trees"],
                       capture_output=True, text=True, cwd=repo, timeout=600)
    assert r.returncode == 0, r.stderr
    for s in stems:
        lines = open(outd / f"{s}.phy").read().splitlines()
        n = int(lines[0])
        dm = np.array([[float(v) for v in l.split(" ")[1:]] for l in lines[1:1 + n]])
        idx, _ids = load_alignment(os.path.join(repo, "data", "testdata", "msas", f"{s}.fa"))
        want = _f64(w, idx[None])[0]
        i, j = pair_indices(n)
        assert float(np.abs(dm[i, j] - want).max()) <= 1e-4, s
        assert os.path.exists(outd / f"{s}.nj.nwk")
