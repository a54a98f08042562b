"""The oracle on ``taxa.cut_taxa`` of two shipped alignments against the REFERENCE's own outputs for the same cuts
(``tests/golden/loo.npz``, written by ``tools/gen_golden_loo.py``): pins the row cut and the pair-index mapping
independently of this repository's oracle.  No GPU."""
import numpy as np
import pytest

from oracle import pf_oracle as O
from phyloformer_amd import taxa as T

# the bound tests/test_oracle.py applies to its end-to-end goldens (TOL_DIST there)
TOL_DIST = 2e-5
CASES = ("0_20_tips", "1_30_tips_12")


@pytest.fixture(scope="module")
def oracle_loo(golden, weights):
    """Per case: the oracle's distances of the whole alignment and of its cuts (computed once)."""
    g = golden("loo.npz")
    w = weights("pf").tensors
    out = {}
    for key in CASES:
        idx = g[f"{key}/idx"]
        cuts = T.cut_taxa(idx, T.leave_one_out_sets(idx.shape[0]))
        out[key] = (O.forward(w, idx), np.stack([O.forward(w, c) for c in cuts]))
    return out


@pytest.mark.parametrize("key", CASES)
def test_golden_is_what_it_says(golden, repo, key):
    import os
    from phyloformer_amd.fasta import load_alignment
    g = golden("loo.npz")
    stem, rows = ("0_20_tips", 20) if key == "0_20_tips" else ("1_30_tips", 12)
    idx, _ids = load_alignment(os.path.join(repo, "data", "testdata", "msas", f"{stem}.fa"))
    assert np.array_equal(g[f"{key}/idx"], idx[:rows]) and g[f"{key}/idx"].shape == (rows, 250)
    assert g[f"{key}/full"].shape == (rows * (rows - 1) // 2,) and g[f"{key}/loo"].shape == (rows, (rows - 1) * (rows - 2) // 2)
    if key == "0_20_tips":
        assert np.array_equal(g[f"{key}/full"], golden("e2e_testdata.npz")["pf/0_20_tips"])
    # the stored statistics (explicit loops in the generator) are the twin's of the stored distances
    infl, shift, ctx = T.loo_stats(g[f"{key}/full"], g[f"{key}/loo"])
    for got, name in ((infl, "influence"), (shift, "shift"), (ctx, "context")):
        assert g[f"{key}/{name}"].dtype == np.float64
        assert np.allclose(got, g[f"{key}/{name}"], rtol=2.0 ** -23, atol=1e-9), name
    # the effect is far above the error bounds: removing a taxon moves the others
    assert g[f"{key}/influence"].min() > 1e-3


@pytest.mark.parametrize("key", CASES)
def test_oracle_on_cut_taxa_matches_reference(golden, oracle_loo, key):
    g = golden("loo.npz")
    full, loo = oracle_loo[key]
    err_full = float(np.abs(full - g[f"{key}/full"]).max())
    err_loo = float(np.abs(loo - g[f"{key}/loo"]).max())
    print(f"{key}: oracle vs reference, whole {err_full:.3e}, cuts {err_loo:.3e}")
    assert err_full <= TOL_DIST and err_loo <= TOL_DIST
    # a cut is not a slice of the whole alignment's distances: the context matters (issue: 4 orders above the error)
    fmap = T._loo_map(loo.shape[0])
    assert np.abs(loo - full[fmap]).max() > 100 * TOL_DIST
    # a wrong row order or pair mapping would miss by the size of the distances themselves
    wrong = np.stack([loo[(t + 1) % len(loo)] for t in range(len(loo))])
    assert np.abs(wrong - g[f"{key}/loo"]).max() > 100 * TOL_DIST
