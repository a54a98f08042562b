"""``phyloformer_amd/bionj.py`` - BIONJ, FastME's default start tree - pinned against FastME ``-m I`` on two sources of
distances of the 20 test alignments (tests/golden/fastme_bionj.json, tools/gen_golden_fastme_bionj.py), its refinements
by ``bme.py`` against FastME ``-m I -n B`` and ``-m I -s``, and its three special cases - the window of the pick,
``v_ab = 0`` and the clamp of ``lambda`` - on constructed matrices.  No GPU, no native code besides the PHYLIP formatter
that keys the goldens."""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import bme_check as bc
from helpers.bionj_table import duplicated_rows
from helpers.nj_table import matrix_of
from phyloformer_amd import bionj, bme, fasta, nj, treecmp
from phyloformer_amd.phylip import vec_to_matrix

SOURCES = (("e2e_testdata.npz", "pf/{}"), ("gpu_distances_r02.npz", "{}"))


def _tree(ids, joins, final):
    return treecmp.parse_newick(nj.newick_of_joins(ids, joins, final, clamp_negative=False))


@pytest.fixture(scope="module")
def cases(repo, golden):
    """Per source of distances and test alignment: ids, the float64 matrix, FastME's three trees."""
    from phyloformer_amd import build
    from phyloformer_amd.hostio import format_phylip
    build.build()
    with open(os.path.join(repo, "tests", "golden", "fastme_bionj.json")) as fh:
        gold = json.load(fh)
    out = {}
    for npz, pattern in SOURCES:
        data = golden(npz)
        for name in sorted(os.listdir(os.path.join(repo, "data/testdata/msas"))):
            stem = name[:-3]
            _idx, ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas", name))
            n = len(ids)
            dm = vec_to_matrix(data[pattern.format(stem)], n).astype(np.float64)
            entry = gold[hashlib.sha256(format_phylip(dm[np.triu_indices(n, 1)], ids)).hexdigest()]
            out[(npz, stem)] = dict(ids=ids, dm=dm, **{k: treecmp.parse_newick(entry[k]) for k in ("bionj", "bnni", "spr")})
    assert len(out) == 40
    return out


def test_same_tree_as_fastme_bionj_on_all_40_and_nj_is_another(cases):
    """FastME ``-m I``: RF 0 and every branch length within 3e-8, unclamped, on 40 of 40 matrices (measured: 5.03e-9, the
    rounding of FastME's 8 decimals; a split that only one tree has counts with length 0 on the other side, so a
    zero-length branch FastME resolves otherwise is a star on both sides).  ``nj.nj_joins`` does not meet the pin: its
    topology differs on at least 10 of the 20 reference matrices (measured: 11)."""
    worst, nj_differs = 0.0, 0
    for (npz, stem), c in cases.items():
        mine = _tree(c["ids"], *bionj.bionj_joins(c["dm"]))
        sm, sr = treecmp.splits(mine), treecmp.splits(c["bionj"])
        diff = max(abs(sm.get(k, 0.0) - sr.get(k, 0.0)) for k in set(sm) | set(sr))
        worst = max(worst, diff)
        assert treecmp.robinson_foulds(mine, c["bionj"])[0] == 0, (npz, stem)
        assert diff <= 3e-8, (npz, stem, diff)
        if npz == SOURCES[0][0]:
            nj_differs += treecmp.robinson_foulds(_tree(c["ids"], *nj.nj_joins(c["dm"])), c["bionj"])[0] != 0
    print("largest branch-length difference to FastME -m I:", worst, "; NJ's topology differs on", nj_differs, "of 20")
    assert nj_differs >= 10


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


@pytest.mark.parametrize("search,key", [(bme.bme_nni, "bnni"), (bme.bme_spr, "spr")])
def test_refinements_from_the_bionj_start_against_fastme(cases, search, key):
    """``bme_nni`` / ``bme_spr`` from ``bionj_start`` against FastME ``-m I -n B`` / ``-m I -s`` on the reference's
    distances: RF 0 on at least 18 of 20 (measured: 18; the misses are 2_30_tips and 3_50_tips), and on every miss the
    balanced length of our tree, by the independent path-count formula, is not above that of FastME's topology."""
    same = 0
    for (npz, stem), c in cases.items():
        if npz != SOURCES[0][0]:
            continue
        n = len(c["ids"])
        slots, lengths, _steps, length, status = search(c["dm"], bionj.bionj_start(c["dm"]))
        assert status == bme.OK
        mine = _tree(c["ids"], *bme.table_to_joins(slots, lengths))
        if treecmp.robinson_foulds(mine, c[key])[0] == 0:
            same += 1
            continue
        ours = bc.pauplin_length(bc.adjacency(slots, n), c["dm"])
        theirs = bc.pauplin_length(_index_tree(c[key], c["ids"]), c["dm"])
        assert length == pytest.approx(ours, rel=1e-9)
        assert ours <= theirs, (stem, ours, theirs)
    print(key, ": RF 0 on", same, "of 20")
    assert same >= 18


def _first_join_matrix(close_to_first: bool) -> np.ndarray:
    """Five sequences of which 0 and 1 are joined first (d_01 = 0.1, q = -8.9 against -8.1 and -8.5 elsewhere) while
    one of the two is twice as far from the rest as the other: sum_k (v_1k - v_0k) = +-3 against 2 (m - 2) v_01 = 0.6."""
    near, far = (1.0, 2.0) if close_to_first else (2.0, 1.0)
    d = np.full((5, 5), 2.5)
    d[0, 1] = d[1, 0] = 0.1
    d[0, 2:] = d[2:, 0] = near
    d[1, 2:] = d[2:, 1] = far
    np.fill_diagonal(d, 0.0)
    return d


@pytest.mark.parametrize("close_to_first,want", [(True, 1.0), (False, 0.0)])
def test_lambda_clamps_at_zero_and_at_one(close_to_first, want):
    d = _first_join_matrix(close_to_first)
    trace = []
    joins, final = bionj.bionj_joins(d, trace)
    assert joins[0][:2] == (0, 1) and trace[0][0] == want and trace[0][1] == 0.1
    unclamped = 0.5 + (3.0 if close_to_first else -3.0) / (2 * 3 * 0.1)
    assert (unclamped > 1.0) if close_to_first else (unclamped < 0.0)
    assert bionj.weight(d[0].copy(), d[1].copy(), 0.1, 0, 1) == want
    # lambda = 1: the new cluster's distances are sequence 0's, shortened by its branch (lambda = 0: sequence 1's), so
    # the three other sequences, 2.5 apart and equally far from the cluster, end with equal branches of half of 2.5 ...
    keep = 0 if close_to_first else 1
    to_rest = d[keep, 2] - joins[0][2 + keep]
    # ... and the cluster's own last branch is what is left of its distance to them
    ends = [x for j in joins[1:] for x in j[2:]] + list(final[3:])
    assert sorted(ends)[-3:] == pytest.approx([1.25] * 3, abs=1e-12)
    assert sum(ends) == pytest.approx(3 * 1.25 + (to_rest - 1.25), abs=1e-12)
    bme.Tree([s for j in joins for s in j[:2]] + list(final[:3]), 5)            # a valid join table


def test_two_identical_sequences_have_variance_zero_and_lambda_one_half():
    """Sequences 1, 4 and 6 are identical, and 2 and 3: ``d_ab = v_ab = 0`` when two of them meet, ``lambda = 1/2``, both
    branch lengths 0, and the window holds more than one pair (their q differ by roundings at most).  (The other
    distances are random, not a tree's: the third copy need not be the cluster's next neighbour.)"""
    n = 9
    vec = duplicated_rows(n, 11)
    trace = []
    joins, final = bionj.bionj_joins(matrix_of(vec, n), trace)
    zero = [(j, t) for j, t in zip(joins, trace) if t[1] == 0.0]
    assert {j[:2] for j, _t in zero} >= {(2, 3), (1, 4)}
    for j, (lam, _vab, _window) in zero:
        assert lam == 0.5 and j[2] == 0.0 and j[3] == 0.0
    assert any(window > 1 for _j, (_lam, _vab, window) in zero)
    bme.Tree([s for j in joins for s in j[:2]] + list(final[:3]), n)


def _brute_pick(q):
    """The windowed rule, stated by loops: the exact minimum over y < x, then the first pair in the order (1,0), (2,0),
    (2,1), (3,0), ... within EPS of it."""
    m = len(q)
    qstar = min(q[x][y] for x in range(m) for y in range(x))
    for x in range(1, m):
        for y in range(x):
            if q[x][y] <= qstar + bionj.EPS:
                return y, x
    raise AssertionError("no pair")


def test_windowed_rule_against_its_brute_force_statement():
    """200 seeded matrices of 4 to 12 positions: values from a few levels, perturbed by 0, 1e-12, 1e-10, 0.9e-9, 1.1e-9
    and 1e-8 - inside and outside the window around the minimum - and all-equal ones."""
    rng = np.random.default_rng(26)
    several = 0
    for case in range(200):
        m = int(rng.integers(4, 13))
        if case % 10 == 0:
            q = np.full((m, m), float(rng.uniform(-5, 5)))
        else:
            levels = rng.uniform(-5, 5, size=3)
            q = rng.choice(levels, size=(m, m)) + rng.choice([0.0, 1e-12, 1e-10, 0.9e-9, 1.1e-9, 1e-8], size=(m, m))
        assert bionj.pick(q) == _brute_pick(q.tolist()), case
        xs, ys = np.tril_indices(m, -1)
        several += np.count_nonzero(q[xs, ys] <= q[xs, ys].min() + bionj.EPS) > 1
        # the first minimum alone would be another rule
    assert several >= 100
    # whole trees: all-equal distances join (0, 1) first - the first pair of the scan - and stay valid join tables
    for n in (4, 7, 12):
        d = np.full((n, n), 0.75)
        np.fill_diagonal(d, 0.0)
        joins, final = bionj.bionj_joins(d)
        assert joins[0][:2] == (0, 1)
        bme.Tree([s for j in joins for s in j[:2]] + list(final[:3]), n)


def test_table_takes_every_consumer_of_a_join_table():
    n = 10
    vec = np.random.default_rng(10).uniform(0.05, 2.0, size=n * (n - 1) // 2).astype(np.float32)
    dm = matrix_of(vec, n)
    joins, final = bionj.bionj_joins(dm)
    slots, lengths = bionj.bionj_table(dm)
    assert bme.table_to_joins(slots, lengths) == (joins, final)
    assert all(a < b for a, b, _la, _lb in joins) and list(final[:3]) == sorted(final[:3])
    assert len(set(nj.join_splits(joins, n))) == n - 3
    ids = [f"t{i}" for i in range(n)]
    assert bionj.bionj_newick_py(vec, ids) == nj.newick_of_joins(ids, joins, final)
    assert np.array_equal(bionj.bionj_start(dm), slots)
    # fewer than three sequences and non-finite distances: the NJ text
    assert bionj.bionj_newick_py(vec[:1], ids[:2]) == nj.neighbor_joining(matrix_of(vec[:1], 2), ids[:2])
    bad = vec.copy()
    bad[3] = np.nan
    assert bionj.bionj_newick_py(bad, ids) == nj.neighbor_joining(matrix_of(bad, n), ids)
    assert bionj.bionj_bme_newick_py(bad, ids) == bionj.bionj_spr_newick_py(bad, ids) == nj.neighbor_joining(matrix_of(bad, n), ids)
