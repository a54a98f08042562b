"""Tree comparison (phyloformer_amd/treecmp.py) and the end-to-end tree check on the reference's
own distances."""
import os

import numpy as np
import pytest

from phyloformer_amd import fasta, treecmp
from phyloformer_amd.nj import neighbor_joining
from phyloformer_amd.phylip import vec_to_matrix

# FastME --nni --spr trees of the README pipeline, stored by the sha256 of the PHYLIP text they were built from
# (oracle/gen_golden_fastme.py, with the FastME binary of the reference checkout)
FASTME_GOLDEN = "fastme_nni_spr.json"


def test_newick_parser_and_splits():
    t = treecmp.parse_newick("((A:1,B:2)x:0.5,(C:1,'D d':1):0.25,E:3)[comment];")
    assert treecmp.leaf_names(t) == ["A", "B", "C", "D d", "E"]
    sp = treecmp.splits(t)
    internal = {k: v for k, v in sp.items() if 1 < len(k) < 4}
    # {A,B} | rest is stored as the side without the smallest leaf "A"
    assert internal == {frozenset(["C", "D d", "E"]): 0.5, frozenset(["C", "D d"]): 0.25}
    for bad in ("(A,B)", "((A,B);", "(A,B));", "(A,'B);"):
        with pytest.raises(ValueError):
            treecmp.parse_newick(bad)


def test_rf_known_values_and_rooting_invariance():
    a = treecmp.parse_newick("(((A,B),C),(D,E),F);")
    same_rooted_elsewhere = treecmp.parse_newick("((A,B),(C,((D,E),F)));")
    assert treecmp.robinson_foulds(a, same_rooted_elsewhere) == (0, 0.0)
    b = treecmp.parse_newick("(((A,C),B),(D,E),F);")          # one split differs: AB vs AC
    assert treecmp.robinson_foulds(a, b) == (2, 2 / 6)
    star = treecmp.parse_newick("(A,B,C,D,E,F);")
    assert treecmp.robinson_foulds(a, star) == (3, 1.0)
    with pytest.raises(ValueError):
        treecmp.robinson_foulds(a, treecmp.parse_newick("(A,B,(C,D));"))


def test_branch_score_and_root_edge_merging():
    a = treecmp.parse_newick("((A:1,B:1):1,(C:1,D:1):1);")     # bifurcating root: one unrooted edge of 2
    b = treecmp.parse_newick("((A:1,B:1):2,C:1,D:1);")
    assert treecmp.branch_score(a, b) == pytest.approx(0.0)
    c = treecmp.parse_newick("((A:1,B:1):2,C:1,D:4);")
    assert treecmp.branch_score(a, c) == pytest.approx(3.0)
    d = treecmp.parse_newick("((A:1,C:1):2,B:1,D:1);")         # different topology: both internal edges count
    assert treecmp.branch_score(a, d) == pytest.approx(np.sqrt(8.0))


def test_nj_recovers_true_trees_from_their_patristic_distances(repo):
    tdir = os.path.join(repo, "data/testdata/trees")
    for name in sorted(os.listdir(tdir))[::4]:
        true = treecmp.parse_newick(open(os.path.join(tdir, name)).read())
        names, dm = treecmp.patristic(true)
        est = treecmp.parse_newick(neighbor_joining(dm, names))
        assert treecmp.robinson_foulds(true, est)[0] == 0
        assert treecmp.branch_score(true, est) <= 1e-9


def test_nj_matches_fastme_nj_goldens(repo, golden):
    """`--trees` (infer_alns.py:62-64, 120-123) is `skbio.tree.nj` in the reference; scikit-bio is absent
    here, but the reference checkout ships FastME, whose `-m N` is the same neighbour joining.
    tests/golden/nj_fastme.json holds FastME's NJ trees of the reference's own pf.ckpt distances for the 20
    test MSAs (oracle/gen_golden_nj.py): this implementation must give the same topology (RF = 0) and the
    same branch lengths (FastME prints 8 decimals)."""
    import json
    with open(os.path.join(repo, "tests", "golden", "nj_fastme.json")) as fh:
        trees = json.load(fh)
    gold = golden("e2e_testdata.npz")
    assert len(trees) == 20
    for stem, nwk in trees.items():
        _idx, ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas", stem + ".fa"))
        # FastME read the "%.10f" PHYLIP text of the matrix
        dm = np.round(vec_to_matrix(gold[f"pf/{stem}"], len(ids)).astype(np.float64), 10)
        # FastME keeps negative branch lengths; skbio (and the CLI default) clamp them to zero
        mine = treecmp.parse_newick(neighbor_joining(dm, ids, clamp_negative=False))
        ref = treecmp.parse_newick(nwk)
        assert treecmp.robinson_foulds(ref, mine)[0] == 0, stem
        assert treecmp.branch_score(ref, mine) <= 1e-7, stem
        clamped = treecmp.parse_newick(neighbor_joining(dm, ids))
        assert treecmp.robinson_foulds(ref, clamped)[0] == 0, stem
        neg = sum(-v for v in treecmp.splits(ref).values() if v < 0)
        assert treecmp.branch_score(ref, clamped) <= neg + 1e-7, stem


def _tree_check(repo, golden, to_tree, source="e2e_testdata.npz", key="pf/{}"):
    gold = golden(source)
    rows = []
    for name in sorted(os.listdir(os.path.join(repo, "data/testdata/msas"))):
        stem = name[:-3]
        _idx, ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas", name))
        dm = vec_to_matrix(gold[key.format(stem)], len(ids)).astype(np.float64)
        true = treecmp.parse_newick(open(os.path.join(repo, "data/testdata/trees", stem + ".nwk")).read())
        est = treecmp.parse_newick(to_tree(dm, ids))
        rows.append(treecmp.robinson_foulds(true, est) + (treecmp.branch_score(true, est),))
    return np.mean(np.array(rows, dtype=np.float64), axis=0)


def test_end_to_end_tree_check_on_reference_distances(repo, golden):
    """pf.ckpt distances of the reference (goldens) -> NJ -> vs the true trees of data/testdata/trees.
    The values are the yard-stick for the GPU run (tests/test_cli_gpu.py)."""
    rf, nrf, kf = _tree_check(repo, golden, neighbor_joining)
    assert rf == pytest.approx(11.4) and nrf == pytest.approx(0.1857, abs=5e-4) and kf == pytest.approx(0.3964, abs=5e-4)


def test_end_to_end_tree_check_with_fastme(repo, golden):
    """README.md:83-96 of the reference: FastME --nni --spr on the predicted matrices.  The README's
    'average KF 0.333' comes from `phylocompare`, which is missing from the checkout, so that figure is
    unpinned; this pins the build's own comparison on the same pipeline instead (FastME's trees of exactly the
    PHYLIP text this build writes, tests/golden/fastme_nni_spr.json)."""
    rf, nrf, kf = _tree_check(repo, golden, _fastme_tree(repo))
    assert rf == pytest.approx(11.2) and nrf == pytest.approx(0.1837, abs=5e-4) and kf == pytest.approx(0.3935, abs=5e-4)


def _fastme_tree(repo):
    """dm, ids -> the tree FastME --nni --spr built from this build's PHYLIP text of dm (looked up by its sha256:
    a PHYLIP text FastME never saw is a KeyError, not another matrix's tree)."""
    import hashlib
    import json
    from phyloformer_amd.hostio import format_phylip
    with open(os.path.join(repo, "tests", "golden", FASTME_GOLDEN)) as fh:
        trees = json.load(fh)

    def tree(dm, ids):
        n = len(ids)
        text = format_phylip(dm[np.triu_indices(n, 1)], ids)
        return trees[hashlib.sha256(text).hexdigest()]["tree"]
    return tree


def test_gpu_distances_give_the_reference_distances_trees(repo, golden):
    """tests/golden/gpu_distances_r02.npz = what `infer_alns.py models/pf.ckpt data/testdata/msas` wrote on an
    MI355X (round 2, as printed in the .phy files).  They differ from the reference's distances by at most
    1.2e-5, and the trees built from them are the trees built from the reference's: same neighbour-joining
    topology and the same summary against the true trees - with the build's NJ, and with the README's
    FastME pipeline (tests/golden/fastme_nni_spr.json)."""
    gpu, ref = golden("gpu_distances_r02.npz"), golden("e2e_testdata.npz")
    for name in sorted(os.listdir(os.path.join(repo, "data/testdata/msas"))):
        stem = name[:-3]
        _idx, ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas", name))
        assert np.abs(gpu[stem] - ref[f"pf/{stem}"]).max() <= 2e-5
        a = treecmp.parse_newick(neighbor_joining(vec_to_matrix(gpu[stem], len(ids)).astype(np.float64), ids))
        b = treecmp.parse_newick(neighbor_joining(vec_to_matrix(ref[f"pf/{stem}"], len(ids)).astype(np.float64), ids))
        # (1_40_tips is barely resolved - RF 58 of 74 against its true tree - and has internal branches of
        # ~1e-7: such splits may flip)
        assert treecmp.robinson_foulds(a, b)[0] <= (4 if stem == "1_40_tips" else 0), stem
        assert treecmp.branch_score(a, b) <= 2e-5, stem
    rf, nrf, kf = _tree_check(repo, golden, neighbor_joining, "gpu_distances_r02.npz", "{}")
    assert rf == pytest.approx(11.4) and nrf == pytest.approx(0.1857, abs=5e-4) and kf == pytest.approx(0.3964, abs=5e-4)
    rf, nrf, kf = _tree_check(repo, golden, _fastme_tree(repo), "gpu_distances_r02.npz", "{}")
    assert rf == pytest.approx(11.2) and nrf == pytest.approx(0.1837, abs=5e-4) and kf == pytest.approx(0.3935, abs=5e-4)
