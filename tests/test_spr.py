"""``phyloformer_amd/bme.py::bme_spr`` - balanced SPR refinement of the NJ tree - pinned against FastME ``-m N -s`` on
the 20 test matrices and eight harder ones (tests/golden/fastme_nj_spr.json, tools/gen_golden_fastme_spr.py), and
checked by the independent path-count length and brute-force regrafting on the plain adjacency (``helpers/bme_check.py``,
``helpers/spr_check.py``).  No GPU, no native code besides the PHYLIP formatter that keys the goldens."""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import bme_check as bc
from helpers import spr_check as sc
from phyloformer_amd import bme, fasta, nj, treecmp

MOVES_ON_THE_20 = [0, 0, 1, 0, 0, 0, 6, 1, 0, 0, 0, 2, 0, 0, 3, 1, 0, 0, 2, 1]


def _site(tree, srow):
    e = srow if srow < tree.root else srow - tree.root
    return (e, int(tree.parent[e])) if srow < tree.root else (int(tree.parent[e]), e)


@pytest.mark.parametrize("start", ["nj", "caterpillar"])
@pytest.mark.parametrize("n", [4, 5, 6, 7, 9, 12])
def test_every_candidate_is_the_exact_change_of_the_path_count_length(n, start):
    d = bme.matrix_of_preds(bc.uniform_preds(n, 100 + n)[0], n)
    slots = bme.nj_start(d) if start == "nj" else bme.caterpillar_slots(n)
    tree = bme.Tree(slots, n)
    adj = bc.adjacency(slots, n)
    base = bc.pauplin_length(adj, d)
    cands = list(bme.spr_candidates(bme.PairTable(d, tree).t, tree))
    assert len(cands) == 4 * (n - 2) * (n - 3)
    assert len({(s, e) for _dl, s, e, _p in cands}) == len(cands)            # (S row, target edge) names a candidate
    seen, worst = set(), 0.0
    for dl, srow, edge, path in cands:
        s, a = _site(tree, srow)
        assert path[0] in adj[a] - {s} and edge in path[-2:] and len(path) >= 2
        moved = sc.regraft(adj, s, a, path[-2], path[-1])
        worst = max(worst, abs((bc.pauplin_length(moved, d) - base) - dl))
        seen.add(sc.internal_splits(moved, n))
        swapped = bme.Tree(slots, n)                                        # the same tree from the chain of swaps
        bme.spr_move(swapped, srow, path)
        out, _lengths = bme.joins_of_tree(swapped, np.zeros(2 * n - 3))
        assert frozenset(bc.splits_of(out, n)) == sc.internal_splits(moved, n), (srow, path)
    print("largest |dL - (L(moved) - L)|:", worst)
    assert worst <= 1e-12
    assert len(seen) == 2 * (n - 3) * (2 * n - 7)
    assert len(list(sc.spr_neighbours(adj, n))) == 4 * (n - 2) * (n - 3)
    assert {sc.internal_splits(t, n) for t in sc.spr_neighbours(adj, n)} == seen


@pytest.fixture(scope="module")
def cases(repo, golden):
    """The 28 matrices in file order, then helper order: ids, float64 matrix, the searches' results, FastME's tree."""
    from phyloformer_amd import build
    from phyloformer_amd.hostio import format_phylip
    build.build()
    gold = golden("e2e_testdata.npz")
    with open(os.path.join(repo, "tests", "golden", "fastme_nj_spr.json")) as fh:
        fastme = json.load(fh)
    inputs = []
    for name in sorted(os.listdir(os.path.join(repo, "data/testdata/msas"))):
        _idx, ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas", name))
        inputs.append((name[:-3], ids, gold[f"pf/{name[:-3]}"]))
    inputs += sc.harder_cases()
    out = {}
    for label, ids, vec in inputs:
        n = len(ids)
        dm = bme.matrix_of_preds(vec, n)
        key = hashlib.sha256(format_phylip(dm[np.triu_indices(n, 1)], ids)).hexdigest()
        start = bme.nj_start(dm)
        slots, lengths, steps, length, status = bme.bme_spr(dm, start)
        assert status == bme.OK
        text = nj.newick_of_joins(ids, *bme.table_to_joins(slots, lengths), clamp_negative=False)
        out[label] = dict(ids=ids, dm=dm, start=start, slots=slots, lengths=lengths, steps=steps, length=length,
                          tree=treecmp.parse_newick(text), fastme=treecmp.parse_newick(fastme[key]["tree"]))
    assert len(out) == 28 and len(fastme) == 28
    return out


def _index_tree(tree, ids):
    index = {name: i for i, name in enumerate(ids)}
    adj = {i: set() for i in range(len(ids))}
    nxt = [len(ids)]

    def visit(node):
        if node.is_leaf():
            return index[node.name]
        me = nxt[0]
        nxt[0] += 1
        adj[me] = set()
        for c in node.children:
            k = visit(c)
            adj[me].add(k)
            adj[k].add(me)
        return me
    visit(tree)
    return adj


def test_same_topology_as_fastme_nj_spr_on_all_28(cases):
    """FastME ``-m N -s``: RF 0 on 28 of 28.  Where FastME performed a move (we did, and the topology is the same) and
    its lengths are balanced lengths - recognised from its tree alone, as tests/test_bme.py does: the sum of its lengths
    against the path-count length of its topology within 1e-6 - all branch lengths agree within 3e-8."""
    rf = {label: treecmp.robinson_foulds(c["fastme"], c["tree"])[0] for label, c in cases.items()}
    assert all(v == 0 for v in rf.values()), rf
    steps = [c["steps"] for c in cases.values()]
    print("moves:", steps)
    assert steps[:20] == MOVES_ON_THE_20
    assert cases["1_40_tips"]["steps"] == 6 and cases["uniform_preds(40, 5)"]["steps"] >= 5
    worst, compared = 0.0, 0
    for label, c in cases.items():
        if c["steps"] == 0:
            continue
        mine, ref = treecmp.splits(c["tree"]), treecmp.splits(c["fastme"])
        assert set(mine) == set(ref)
        path_count = bc.pauplin_length(_index_tree(c["fastme"], c["ids"]), c["dm"])
        if abs(sum(ref.values()) - path_count) > 1e-6:
            continue
        diff = max(abs(mine[k] - ref[k]) for k in mine)
        worst, compared = max(worst, diff), compared + 1
        assert diff <= 3e-8, (label, diff)
    print("branch lengths compared on", compared, "trees; largest difference", worst)
    assert compared >= 10


def test_independent_check_of_length_lengths_and_local_optimality(cases):
    for label, c in cases.items():
        n = len(c["ids"])
        adj = bc.adjacency(c["slots"], n)
        pauplin = bc.pauplin_length(adj, c["dm"])
        assert c["length"] == pytest.approx(pauplin, rel=1e-9), label
        assert float(np.sum(c["lengths"])) == pytest.approx(pauplin, rel=1e-9), label
        assert pauplin <= bc.pauplin_length(bc.adjacency(c["start"], n), c["dm"]) + 1e-12, label
        if n > 30:
            continue
        seen = set()
        for other in sc.spr_neighbours(adj, n):
            key = sc.internal_splits(other, n)
            if key not in seen:
                seen.add(key)
                assert bc.pauplin_length(other, c["dm"]) >= pauplin - 1e-12, label
        assert len(seen) == 2 * (n - 3) * (2 * n - 7)


def test_spr_leaves_optima_that_bnni_is_stuck_in_and_neither_search_dominates(cases):
    c = cases["uniform_preds(40, 5)"]
    bnni = bme.bme_nni(c["dm"], c["start"])[3]
    print("uniform_preds(40, 5): BNNI", bnni, "SPR", c["length"])
    assert c["length"] < bnni - 0.1
    c = cases["1_40_tips"]
    bnni = bme.bme_nni(c["dm"], c["start"])[3]
    print("1_40_tips: BNNI", bnni, "SPR", c["length"])
    assert round(c["length"], 6) == 0.260904 and round(bnni, 6) == 0.260786


def test_the_same_topology_gives_the_same_bits_whichever_search_found_it(cases):
    """Every NNI neighbour is an SPR neighbour, so BNNI started from an SPR optimum makes no move - and returns that
    topology with ``Table``'s lengths: the bits ``bme_spr`` returned."""
    for label, c in cases.items():
        slots, lengths, steps, length, status = bme.bme_nni(c["dm"], c["slots"])
        assert steps == 0 and status == bme.OK, label
        assert (slots == c["slots"]).all() and lengths.tobytes() == c["lengths"].tobytes() and length == c["length"], label


def test_three_sequences_non_finite_input_and_invalid_starts():
    vec = np.array([0.3, 0.5, 0.4], dtype=np.float32)
    slots, lengths, steps, length, status = bme.bme_spr(bme.matrix_of_preds(vec, 3), [0, 1, 2], trace=(trace := []))
    assert (list(slots), steps, status) == ([0, 1, 2], 0, bme.OK) and trace == [(np.inf, -1, -1, ())]
    d = vec.astype(np.float64)
    assert lengths == pytest.approx([0.5 * (d[0] + d[1] - d[2]), 0.5 * (d[0] + d[2] - d[1]), 0.5 * (d[1] + d[2] - d[0])], abs=1e-15)
    assert length == pytest.approx(d.sum() / 2)
    bad = bc.uniform_preds(6, 1)[0]
    bad[4] = np.nan
    out = bme.bme_spr(bme.matrix_of_preds(bad, 6), bc.caterpillar_slots(6))
    assert out[4] == bme.NONFINITE and not out[0].any() and not out[1].any() and out[2:4] == (0, 0.0)
    ids = list("abcdef")
    assert bme.spr_newick_py(bad, ids) == nj.neighbor_joining(bme.matrix_of_preds(bad, 6), ids)
    assert bme.spr_newick_py(vec[:1], ["a", "b"]) == nj.neighbor_joining(bme.matrix_of_preds(vec[:1], 2), ["a", "b"])
    n = 9
    dm = bme.matrix_of_preds(bc.uniform_preds(n, 2)[0], n)
    for wrong in ([0, 1, 0, 1] + [0] * (2 * (n - 3) - 1), list(bc.caterpillar_slots(n))[:-1], [n] * (2 * (n - 3) + 3)):
        with pytest.raises(ValueError):
            bme.bme_spr(dm, wrong)
    text, steps = bme.spr_tree_py(bc.uniform_preds(n, 2)[0], [f"T{i}" for i in range(n)])
    assert text == bme.spr_newick_py(bc.uniform_preds(n, 2)[0], [f"T{i}" for i in range(n)]) and steps >= 0
