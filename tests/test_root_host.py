"""Tree rooting without a GPU: the statement ``root.tree_root_py`` on tables worked out by hand, on clock trees (the MAD root is the true
root, the deviation is zero), against an evaluation of Tria's definition on the rooted text that knows nothing of ``D``, the midpoint
against ``treecmp.patristic``, the rooted text; the serial native twin (``pf_tree_root_host``, ``hostio.tree_root_host``) against the
statement bit for bit; the statuses, the refusals, ``root_scores``' identities, the sanitizer build of the twin as a stand-alone
program (``tests/native/pf_root_main.cpp``), and ``infer_alns.py --root`` through a stand-in engine whose device calls are the twins."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.root_inputs import CLOCK_SIZES, SIZES, clock_tree, kind_table, same, table_len, tables, uniform
from phyloformer_amd import bme
from phyloformer_amd import fit as F
from phyloformer_amd import hostio, nj, treecmp
from phyloformer_amd import root as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = [("statement", R.tree_root_batch_py), ("native", hostio.tree_root_host)]


def names(n):
    return [f"s{k}" for k in range(n)]


# ---- tables worked out by hand --------------------------------------------------------------------------------------------
# Every path between two leaves is 2 or 4 long, so every weight is 1/4 or 1/16 and every sum, product and quotient below is
# exact: the expected bits do not depend on an order.

@pytest.mark.parametrize("who,fn", BOTH)
def test_a_quartet_by_hand(who, fn):
    """((0, 1), (2, 3)): join (0, 1) -> node 4, then slots 0 (node 4), 2, 3; leaf branches 1, the inner branch 2.  D[0] = [0, 2, 4, 4],
    D[4] = [1, 1, 3, 3], D[5] = [3, 3, 1, 1].  Entry 0 (leaf 0): r1 = (0 - 2) / 4 + 2 (0 - 4) / 16 = -1, r0 = 1/4 + 2/16 = 3/8, lam = 1 / (3/4)
    = 4/3, clamped to L = 1: the root sits on node 4, t = [1, 1, 3, 3], four pairs of ((1 - 3) / 4)^2 = 1/4: ssq = 1.  Entry 2 (node 4):
    r1 = 2 (1 - 3) / 16 = -1/4 per leaf, S1 = -1/2, S0 = 4/16, lam = (1/2) / (1/2) = 1: t = [2, 2, 2, 2], ssq = 0.  The farthest pair is
    (0, 2) at 4, first in pair order; half = 2 lies on the branch above node 4, between D[4][0] = 1 and D[5][0] = 3: lam_mid = 1."""
    slots, lengths = np.array([0, 1, 0, 2, 3], dtype=np.int32), np.array([1.0, 1.0, 2.0, 1.0, 1.0])
    ssq, pos, mid, status = fn(slots, lengths)
    assert status == 0 and ssq.tolist() == [1.0, 1.0, 0.0, 1.0, 1.0] and pos.tolist() == [1.0] * 5 and mid.tolist() == [2.0, 1.0, 0.0, 2.0, 4.0]
    kids = R.kids_of(slots, 4)
    count, lo, order = R.leaf_order(kids, 4)
    d = R.path_lengths(*R.clamped_nodes(slots, lengths, 4), count, lo, 4)
    assert order.tolist() == [0, 1, 2, 3]
    assert d.tolist() == [[0, 2, 4, 4], [2, 0, 4, 4], [4, 4, 0, 2], [4, 4, 2, 0], [1, 1, 3, 3], [3, 3, 1, 1]]


@pytest.mark.parametrize("who,fn", BOTH)
def test_five_leaves_by_hand_with_a_negative_length(who, fn):
    """Join (0, 1) -> node 5; join (node 5, 2) -> node 6; the last three are node 6, 3, 4.  The branch above node 5 is -1/2 and counts as
    +0: leaves 0, 1, 2 hang 1 below node 6, the branch above node 6 is 2, leaves 3 and 4 are 1 long.  D[5] = D[6] = [1, 1, 1, 3, 3], D[7] =
    [3, 3, 3, 1, 1].  Leaf 0: r1 = 2 (0 - 2) / 4 + 2 (0 - 4) / 16 = -3/2, r0 = 5/8, lam = 6/5 clamped to 1; t = [1, 1, 1, 3, 3], six pairs of
    1/4: ssq = 3/2.  Node 5: S1 = 2 (2 (1 - 3) / 16) = -1/2, S0 = 2 (1/4 + 2/16) = 3/4, lam = 1/3 clamped to L = +0: ssq = 3/2 again.  Node 6:
    S1 = 3 (-1/4), S0 = 3/8, lam = 1: every tip at 2, ssq = 0.  Leaf 3: r1 = 3 (0 - 4) / 16 + (0 - 2) / 4 = -5/4, r0 = 7/16, lam = 10/7
    clamped to 1: ssq = 3/2.  The farthest pair is (0, 3) at 4; half = 2 is on the branch above node 6 (1 .. 3): lam_mid = 1."""
    slots, lengths = np.array([0, 1, 0, 2, 0, 3, 4], dtype=np.int32), np.array([1.0, 1.0, -0.5, 1.0, 2.0, 1.0, 1.0])
    ssq, pos, mid, status = fn(slots, lengths)
    assert status == 0 and ssq.tolist() == [1.5, 1.5, 1.5, 1.5, 0.0, 1.5, 1.5]
    assert pos.tolist() == [1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0] and not np.signbit(pos[2]) and mid.tolist() == [4.0, 1.0, 0.0, 3.0, 4.0]
    kids = R.kids_of(slots, 5)
    count, lo, order = R.leaf_order(kids, 5)
    parent, blen = R.clamped_nodes(slots, lengths, 5)
    d = R.path_lengths(parent, blen, count, lo, 5)
    assert order.tolist() == [0, 1, 2, 3, 4] and blen.tolist() == [1, 1, 1, 1, 1, 0, 2, 0] and not np.signbit(blen[5])
    assert d.tolist() == [[0, 2, 2, 4, 4], [2, 0, 2, 4, 4], [2, 2, 0, 4, 4], [4, 4, 4, 0, 2], [4, 4, 4, 2, 0], [1, 1, 1, 3, 3], [1, 1, 1, 3, 3],
                          [3, 3, 3, 1, 1]]
    text = R.rooted_newick(names(5), slots, lengths, 4, 1.0)
    assert text == "(((s0:1.0,s1:1.0):0.0,s2:1.0):1.0,(s3:1.0,s4:1.0):1.0);\n"
    assert R.rooted_newick(names(5), slots, lengths, 0, 0.25) == "(s0:0.25,(s1:1.0,(s2:1.0,(s3:1.0,s4:1.0):2.0):0.0):0.75);\n"


@pytest.mark.parametrize("n", SIZES)
def test_the_leaf_rows_are_the_patristic_distances_of_the_clamped_table(n):
    """Both add the same non-negative lengths of a path, in another order: a path has fewer than 2 N branches, a sum of them is off
    by 2 N x 2^-53 of its value at the most, two such sums by 4 N x 2^-53 (NJ tables measure 4.4e-16, a caterpillar of 31 3.6e-15)."""
    slots, lengths = tables(n, 60 + n, 1, 4)
    bound = 4 * n * 2.0 ** -53
    for s, l in zip(slots[0], lengths[0]):
        kids = R.kids_of(s, n)
        count, lo, _order = R.leaf_order(kids, n)
        d = R.path_lengths(*R.clamped_nodes(s, l, n), count, lo, n)
        want = F.patristic_py(s, np.where(l > 0, l, 0.0), n)
        for x in range(n):
            for y in range(x + 1, n):
                t = want[F.pair_index(x, y, n)]
                assert abs(d[x, lo[y]] - t) <= bound * t and abs(d[y, lo[x]] - t) <= bound * t


# ---- clock trees ------------------------------------------------------------------------------------------------------------

def clock_case(n):
    dm, left, right, (h_left, h_right, height) = clock_tree(n, 500 + n)
    slots, lengths = nj.table_of_joins(*nj.nj_joins(dm))
    return dm, slots, lengths, {tuple(left): height - h_left, tuple(right): height - h_right}


@pytest.mark.parametrize("n", CLOCK_SIZES)
def test_the_mad_and_midpoint_roots_of_a_clock_tree_are_its_root(n):
    """Node heights in multiples of 2^-10 and additive distances: the deviation of every pair is zero at the true root and nowhere
    else.  The bounds cover the order of the sums only."""
    _dm, slots, lengths, sides = clock_case(n)
    ssq, pos, mid, status = R.tree_root_py(slots, lengths, n)
    s = R.root_scores(slots, lengths, ssq, pos, mid, n)
    kids = R.kids_of(slots, n)
    count, lo, order = R.leaf_order(kids, n)
    v = int(kids[s.root_k])
    below = tuple(sorted(order[lo[v]:lo[v] + count[v]].tolist()))
    second = float(np.sort(np.sqrt(ssq / (n * (n - 1) // 2)))[1])
    print(f"N = {n}: mad = {s.mad:.3e}, second-best branch {second:.3e}, clock_cv = {s.clock_cv:.3e}, |pos - truth| = {abs(s.root_pos - sides.get(below, 9)):.3e}")
    assert status == 0 and below in sides and abs(s.root_pos - sides[below]) <= 1e-12 and s.mad <= 1e-12 and second > s.mad
    assert s.same_branch and abs(s.mid_pos - sides[below]) <= 1e-12 and s.clock_cv <= 1e-12 and s.mid_clock_cv <= 1e-12
    assert s.root_below == len(below) and 0 <= s.ambiguity < 1


# ---- an independent evaluation of Tria's definition -----------------------------------------------------------------------

def tria_ssq(text, ids):
    """The sum over the pairs of ``(2 d(b, ancestor) / d(b, c) - 1)^2`` of a rooted text: the ancestor of a pair by a walk over the parsed
    nodes, the distances by adding the text's lengths.  A pair at distance zero contributes nothing."""
    root = treecmp.parse_newick(text)
    up, stack = {}, [root]
    while stack:
        node = stack.pop()
        for c in node.children:
            up[id(c)] = (node, c.length or 0.0)
            stack.append(c)
            if c.is_leaf():
                up[c.name] = c
    paths = []
    for name in ids:
        node, dist, path = up[name], 0.0, {}
        while id(node) in up:
            path[id(node)] = dist
            node, step = up[id(node)]
            dist += step
        path[id(node)] = dist
        paths.append(path)
    total = 0.0
    for b in range(len(ids)):
        for c in range(b + 1, len(ids)):
            node, dist = up[ids[c]], 0.0
            while id(node) not in paths[b]:
                node, step = up[id(node)]
                dist += step
            d = paths[b][id(node)] + dist
            if d > 0.0:
                total += (2.0 * paths[b][id(node)] / d - 1.0) ** 2
    return total


@pytest.mark.parametrize("n", CLOCK_SIZES)
def test_the_scores_against_trias_definition_on_the_rooted_text(n):
    """Noisy tables: the clock distances times 1 + 0.3 U(0, 1), symmetrised, through NJ.  At the returned position the independent sum
    agrees with ``ssq`` to a relative 1e-9 (float64 sums of this length; the figures printed are 1e-14 or better); at ``pos +- L / 64``,
    clipped to the branch, it is not smaller."""
    dm = clock_case(n)[0]
    noise = 1.0 + 0.3 * np.random.default_rng(77 + n).uniform(size=dm.shape)
    noisy = dm * noise
    noisy = 0.5 * (noisy + noisy.T)
    slots, lengths = nj.table_of_joins(*nj.nj_joins(noisy))
    ssq, pos, _mid, status = hostio.tree_root_host(slots, lengths)
    assert status == 0
    _parent, blen = R.clamped_nodes(slots, lengths, n)
    kids = R.kids_of(slots, n)
    ids = names(n)
    picked = sorted(set(range(table_len(n)) if n <= 17 else [int(np.argmin(ssq)), 0, 1, n, table_len(n) - 1, table_len(n) - 2]))
    worst = 0.0
    for k in picked:
        length = float(blen[kids[k]])
        at = tria_ssq(R.rooted_newick(ids, slots, lengths, k, float(pos[k])), ids)
        worst = max(worst, abs(at - ssq[k]) / ssq[k])
        assert abs(at - ssq[k]) <= 1e-9 * ssq[k] and 0.0 <= pos[k] <= length
        for lam in (max(pos[k] - length / 64, 0.0), min(pos[k] + length / 64, length)):
            assert tria_ssq(R.rooted_newick(ids, slots, lengths, k, float(lam)), ids) >= ssq[k] * (1 - 1e-12)
    print(f"N = {n}: max relative |definition - ssq| over {len(picked)} branches = {worst:.3e}")


# ---- the midpoint, the rooted text -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_the_midpoint_against_the_patristic_distances_of_the_text(n):
    pred = uniform(n, 300 + n)[0]
    ids = names(n)
    for kind in ("nj", "bionj"):
        slots, lengths = kind_table(kind, pred)
        _ssq, _pos, mid, status = hostio.tree_root_host(slots, lengths)
        order, dm = treecmp.patristic(treecmp.parse_newick(hostio.newick_of_joins(slots, lengths, ids).decode()))
        where = [order.index(x) for x in ids]
        dm = dm[np.ix_(where, where)]
        far = max(((dm[b, c], -b, -c) for b in range(n) for c in range(b + 1, n)))
        _parent, blen = R.clamped_nodes(slots, lengths, n)
        assert status == 0 and (int(mid[2]), int(mid[3])) == (-far[1], -far[2]) and mid[4] == pytest.approx(far[0], rel=1e-12)
        assert 0.0 <= mid[1] <= blen[R.kids_of(slots, n)[int(mid[0])]]
        tips = R.tip_distances(slots, lengths, int(mid[0]), float(mid[1]), n)
        assert tips[int(mid[2])] == pytest.approx(0.5 * mid[4], rel=1e-12) and tips[int(mid[3])] == pytest.approx(0.5 * mid[4], rel=1e-12)
        assert tips.max() <= 0.5 * mid[4] * (1 + 1e-12)


@pytest.mark.parametrize("n", SIZES)
def test_the_rooted_text(n):
    pred = uniform(n, 400 + n)[0]
    ids = names(n)
    for kind in ("nj", "bme", "bionj"):
        slots, lengths = kind_table(kind, pred)
        ssq, pos, mid, _status = hostio.tree_root_host(slots, lengths)
        s = R.root_scores(slots, lengths, ssq, pos, mid, n)
        own = treecmp.parse_newick(hostio.newick_of_joins(slots, lengths, ids).decode())
        for method in R.METHODS:
            k, lam = R.root_choice(s, method)
            rooted = treecmp.parse_newick(R.rooted_newick(ids, slots, lengths, k, lam))
            assert treecmp.robinson_foulds(rooted, own) == (0, 0.0)
            (na, da), (nb, db) = treecmp.patristic(rooted), treecmp.patristic(own)
            back = [na.index(x) for x in nb]
            assert np.allclose(da[np.ix_(back, back)], db, rtol=1e-12, atol=0.0)
            length = max(float(lengths[k]), 0.0)
            assert len(rooted.children) == 2 and rooted.children[0].length == lam
            assert rooted.children[0].length + rooted.children[1].length == pytest.approx(length, rel=4e-16, abs=0.0)
            tips = R.tip_distances(slots, lengths, k, lam, n)
            text_tips = {leaf: d for leaf, d in zip(*_depths(rooted))}
            assert all(text_tips[ids[x]] == pytest.approx(tips[x], rel=1e-12, abs=1e-15) for x in range(n))


def _depths(root):
    out, stack = ([], []), [(root, 0.0)]
    while stack:
        node, d = stack.pop()
        if node.is_leaf():
            out[0].append(node.name)
            out[1].append(d)
        stack.extend((c, d + (c.length or 0.0)) for c in node.children)
    return out


# ---- the twin against the statement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_the_twin_equals_the_statement_bit_for_bit(n, b, m):
    slots, lengths = tables(n, 8000 + n, b, m)
    got, want = hostio.tree_root_host(slots, lengths), R.tree_root_batch_py(slots, lengths)
    assert [x.shape for x in got] == [(b, m, table_len(n)), (b, m, table_len(n)), (b, m, R.MID), (b, m)] and not got[3].any()
    assert all(x.tobytes() == y.tobytes() and x.dtype == y.dtype for x, y in zip(got, want))
    # the shapes without B and M
    assert same(hostio.tree_root_host(slots[0], lengths[0]), tuple(x[0] for x in got))
    assert same(hostio.tree_root_host(slots[0, 0], lengths[0, 0]), tuple(x[0, 0] for x in got))
    assert same(hostio.tree_root_host(slots[:, 0], lengths[:, 0]), tuple(x[:, 0] for x in got))


@pytest.mark.parametrize("who,fn", BOTH)
def test_duplicate_sequences_weigh_nothing(who, fn):
    """Leaves 0 and 1 at distance zero (both branches 0, one of them negative before the clamp), and a zero inner branch: ``W`` is 0 for
    the pair, nothing divides by zero, both sides agree."""
    n = 9
    slots, lengths = tables(n, 21, 1, 3)
    slots, lengths = slots[0, 2].copy(), lengths[0, 2].copy()          # the caterpillar: its first join is (0, 1)
    assert slots[:2].tolist() == [0, 1]
    lengths[0], lengths[1], lengths[5] = 0.0, -0.25, 0.0
    got = fn(slots, lengths)
    kids = R.kids_of(slots, n)
    count, lo, order = R.leaf_order(kids, n)
    w = R.weights(R.path_lengths(*R.clamped_nodes(slots, lengths, n), count, lo, n), order, n)
    assert w[lo[0], lo[1]] == 0.0 and w[lo[1], lo[0]] == 0.0 and np.count_nonzero(w == 0.0) == n + 2
    assert got[3] == 0 and np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and got[0].min() > 0
    assert same(got, R.tree_root_py(slots, lengths, n))
    # every length zero: every weight zero, every score and position zero, the midpoint on the first branch that separates 0 and 1
    zero = fn(slots, np.zeros(table_len(n)))
    assert zero[3] == 0 and not zero[0].any() and not zero[1].any() and zero[2].tolist() == [0.0, 0.0, 0.0, 1.0, 0.0]


# ---- statuses ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("who,fn", BOTH)
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_status_1_for_lengths_that_are_not_finite(who, fn, bad):
    n = 9
    slots, lengths = tables(n, 12, 2, 3)
    clean = fn(slots, lengths)
    lengths[1, 1, 4] = bad
    got = fn(slots, lengths)
    assert got[3].tolist() == [[0, 0, 0], [0, 1, 0]] and not any(x[1, 1].any() for x in got[:3])
    assert same(tuple(x[0] for x in got), tuple(x[0] for x in clean)) and same(tuple(x[1, 2] for x in got), tuple(x[1, 2] for x in clean))


def _malformed(n, what):
    slots = bme.caterpillar_slots(n).copy()
    if what == "a slot of N":
        slots[2] = n
    elif what == "a negative slot":
        slots[5] = -1
    elif what == "a slot joined after it left":
        slots[4] = slots[1]
    elif what == "a == b":
        slots[3] = slots[2]
    elif what == "a last slot that has left":
        slots[-1] = slots[1]
    elif what == "two equal last slots":
        slots[-1] = slots[-2]
    elif what == "a last slot outside":
        slots[-2] = 2 ** 31 - 1
    return slots


@pytest.mark.parametrize("who,fn", BOTH)
@pytest.mark.parametrize("what", ["a slot of N", "a negative slot", "a slot joined after it left", "a == b", "a last slot that has left",
                                  "two equal last slots", "a last slot outside"])
def test_status_2_for_a_table_that_is_no_join_table(who, fn, what):
    n = 8
    good = bme.caterpillar_slots(n)
    lengths = np.random.default_rng(5).uniform(0.1, 1.0, size=(1, 3, table_len(n)))
    assert F.table_status(good, n) == 0 and F.table_status(_malformed(n, what), n) == 2
    slots = np.stack([good, _malformed(n, what), good])[None]
    got = fn(slots, lengths)
    assert got[3].tolist() == [[0, 2, 0]] and not any(x[0, 1].any() for x in got[:3]) and got[0][0, 0].any()
    lengths[0, 1, 3] = np.nan                        # no table AND not finite: 2, the table is checked first
    lengths[0, 2, 3] = np.nan
    assert fn(slots, lengths)[3].tolist() == [[0, 2, 1]]


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_and_their_messages():
    s3, l3 = np.array([0, 1, 2], dtype=np.int32), np.ones(3)
    for fn in (hostio.tree_root_host, R.tree_root_batch_py):
        with pytest.raises(ValueError, match=r"tree root needs N >= 3 sequences \(got 2\)"):
            fn(np.zeros(1, dtype=np.int32), np.ones(1))
        with pytest.raises(ValueError, match=r"tree root needs B >= 1 sources \(got 0\)"):
            fn(np.zeros((0, 1, 3), dtype=np.int32), np.ones((0, 1, 3)))
        with pytest.raises(ValueError, match=r"tree root needs M >= 1 trees per source \(got 0\)"):
            fn(np.zeros((1, 0, 3), dtype=np.int32), np.ones((1, 0, 3)))
        with pytest.raises(ValueError, match="4 slots are the table of no number of sequences"):
            fn(np.zeros(4, dtype=np.int32), np.ones(4))
        with pytest.raises(ValueError, match="expected slots and lengths"):
            fn(np.zeros((2, 3), dtype=np.int32), np.ones((3, 3)))
    with pytest.raises(ValueError, match=r"tree root takes at most 8192 sequences \(got 8193\)"):
        R.refuse(1, 1, 8193)
    with pytest.raises(ValueError, match=r"tree root takes at most 8192 sequences \(got 8193\)"):
        hostio.tree_root_host(np.zeros(2 * 8193 - 3, dtype=np.int32), np.ones(2 * 8193 - 3))
    with pytest.raises(ValueError, match=r"tree root needs N >= 3 sequences \(got 2\)"):
        R.tree_root_py(s3, l3, 2)
    with pytest.raises(ValueError, match="--root takes one of mad, midpoint"):
        R.root_choice(R.no_scores(), "outgroup")
    # the library itself: PF_EINVAL (-1) for each of them and for a null buffer, nothing written
    lib = hostio._lib()
    out = (np.full(3, -7.0), np.full(3, -7.0), np.full(R.MID, -7.0), np.full(1, 9, dtype=np.uint8))
    ptrs = [a.ctypes.data for a in out]
    ins = [s3.ctypes.data, l3.ctypes.data]
    for b, m, n in ((1, 1, 2), (1, 1, 8193), (1, 1, 65537), (0, 1, 3), (1, 0, 3), (-1, 1, 3)):
        assert lib.pf_tree_root_host(*ins, b, m, n, *ptrs) == -1
    for hole in range(6):
        args = [*ins, *ptrs]
        args[hole] = None
        assert lib.pf_tree_root_host(*args[:2], 1, 1, 3, *args[2:]) == -1
    assert all((a == a.flat[0]).all() for a in out)
    # three leaves of length 1: the root a third ... no: lam = r1 / (2 r0) = 1, the last node; every pair at 2, all tips at 1
    assert lib.pf_tree_root_host(*ins, 1, 1, 3, *ptrs) == 0 and out[3][0] == 0
    assert out[0].tolist() == [0.0, 0.0, 0.0] and out[1].tolist() == [1.0, 1.0, 1.0] and out[2].tolist() == [0.0, 1.0, 0.0, 1.0, 2.0]


def test_the_bindings_name_the_three_entry_points():
    from phyloformer_amd import build, engine
    from phyloformer_amd.engine import CALL_TIME_SYMBOLS, SIGNATURES, Engine
    from phyloformer_amd.treekinds import NativeHost, PythonHost
    symbols = {"pf_tree_root", "pf_tree_root_device", "pf_tree_root_host"}
    assert symbols <= set(SIGNATURES) & CALL_TIME_SYMBOLS
    assert SIGNATURES["pf_tree_root"][1][1:] == SIGNATURES["pf_tree_root_device"][1][1:] == SIGNATURES["pf_tree_root_host"][1]
    assert callable(Engine.tree_root) and Engine.tree_root_device.__name__ == "tree_root_device"
    assert "tree_root_device" not in engine.PASS_THROUGHS                 # (attached beside the list, whose length is pinned)
    assert {"pf_root.hip.h", "pf_root_host.h"} <= set(build.HEADERS) and not {"pf_root.hip.h", "pf_root_host.h"} & set(build.KERNEL_FILES)
    with open(os.path.join(REPO, "include", "phyloformer_amd.h")) as fh:
        header = fh.read()
    assert all(f"int {name}(" in header for name in symbols)
    slots, lengths = tables(6, 8, 2, 2)
    assert same(NativeHost().tree_root(slots, lengths), PythonHost().tree_root(slots, lengths))
    e = Engine.__new__(Engine)
    e._lib, e._h = engine.load_library(), None
    with pytest.raises(ValueError):                                        # a NULL handle is refused, nothing dereferenced
        e.tree_root_device(0, 0, 1, 1, 3, 0, 0, 0, 0)
    with pytest.raises(TypeError):
        e.tree_root_device(0, 0, 1, 1, 3, 0, 0, 0)


# ---- root_scores --------------------------------------------------------------------------------------------------------------

def test_identities_of_the_derived_scores():
    n = 31
    pred = uniform(n, 55)[0]
    slots, lengths = kind_table("nj", pred)
    ssq, pos, mid, status = hostio.tree_root_host(slots, lengths)
    s = R.root_scores(slots, lengths, ssq, pos, mid, n)
    pairs = n * (n - 1) // 2
    mads = np.sqrt(ssq / pairs)
    assert status == 0 and s.root_k == int(np.argmin(ssq)) and s.mad == mads.min() and 0 < s.ambiguity <= 1
    assert s.ambiguity == s.mad / np.sort(mads)[1] and s.root_pos == pos[s.root_k] and s.root_length == max(lengths[s.root_k], 0.0)
    kids = R.kids_of(slots, n)
    count, lo, order = R.leaf_order(kids, n)
    assert s.root_below == count[kids[s.root_k]] and s.mid_below == count[kids[s.mid_k]] and s.same_branch == (s.root_k == s.mid_k)
    assert (s.mid_k, s.mid_pos, s.mid_i, s.mid_j, s.mid_diameter) == (int(mid[0]), mid[1], int(mid[2]), int(mid[3]), mid[4])
    # the tips: two leaves on either side of the root are as far apart as their tips add up to
    tips = R.tip_distances(slots, lengths, s.root_k, s.root_pos, n)
    tree = F.patristic_py(slots, np.where(lengths > 0, lengths, 0.0), n)
    v = int(kids[s.root_k])
    inside = set(order[lo[v]:lo[v] + count[v]].tolist())
    for x in range(n):
        for y in range(x + 1, n):
            if (x in inside) != (y in inside):
                assert tips[x] + tips[y] == pytest.approx(tree[F.pair_index(x, y, n)], rel=1e-12)
    assert s.clock_cv == pytest.approx(np.std(tips) / np.mean(tips), rel=1e-15) and s.clock_cv > 0
    # the line of the file and its way back
    line = R.root_line("nj", "mad", s, names(n))
    back = R.parse_root_tsv(R.root_tsv([("nj", "mad", s, names(n))]))["nj"]
    assert line.count("\t") == R.ROOT_HEAD.count("\t") == 14 and back["method"] == "mad" and back["mid_i"] == f"s{s.mid_i}"
    assert float(back["mad"]) == pytest.approx(s.mad, rel=1e-9) and int(back["root_below"]) == s.root_below
    assert int(back["same_branch"]) == int(s.same_branch)
    assert R.root_line("bme", "midpoint", R.no_scores()) == "bme\tmidpoint\tnan\tnan\t0\tnan\tnan\tnan\t-1\t-1\tnan\t0\tnan\tnan\tnan\n"


# ---- the twin under AddressSanitizer and UBSan, as a stand-alone program ----------------------------------------------------

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("root_native") / "pf_root_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_root_main.cpp"),
           "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


@pytest.mark.parametrize("n,b,m", [(3, 1, 1), (5, 3, 3), (31, 2, 3), (65, 3, 3)])
def test_twin_is_clean_under_asan_and_ubsan_and_equals_the_library(program, tmp_path, n, b, m):
    slots, lengths = tables(n, 900 + n, b, m)
    if n >= 5:                                 # tables that are none, and lengths that are not finite, among the fine ones
        slots[0, 0] = _malformed(n, "a last slot outside") if n > 5 else np.array([0, 1, 0, 2, 0, 3, 9], dtype=np.int32)
        slots[b - 1, m - 1] = _malformed(n, "a negative slot") if n > 5 else np.array([0, 1, -1, 2, 0, 3, 4], dtype=np.int32)
        lengths[1, 1, 2] = np.inf
    for name, a in (("slots", slots), ("lengths", lengths)):
        a.tofile(tmp_path / f"{name}.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([program, str(b), str(m), str(n), *(str(tmp_path / f"{x}.bin") for x in ("slots", "lengths")),
                          str(tmp_path / "res.bin")], capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert res.returncode == 0 and f"clean, B = {b}, M = {m}, N = {n}" in res.stdout, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    raw = (tmp_path / "res.bin").read_bytes()
    items, width = b * m, table_len(n)
    assert len(raw) == items * (2 * width + R.MID) * 8 + items
    got = (np.frombuffer(raw, np.float64, items * width).reshape(b, m, width),
           np.frombuffer(raw, np.float64, items * width, offset=items * width * 8).reshape(b, m, width),
           np.frombuffer(raw, np.float64, items * R.MID, offset=2 * items * width * 8).reshape(b, m, R.MID),
           np.frombuffer(raw, np.uint8, items, offset=items * (2 * width + R.MID) * 8).reshape(b, m))
    assert same(got, hostio.tree_root_host(slots, lengths))
    assert n < 5 or (got[3][0, 0] == 2 and got[3][b - 1, m - 1] == 2 and got[3][1, 1] == 1)


# ---- the CLI through a stand-in engine ------------------------------------------------------------------------------------

def _write_fasta(path, idx):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">s{k}\n{''.join(alpha[int(v)] for v in row)}\n")


@pytest.fixture(scope="module")
def root_alns():
    from phyloformer_amd.msa_sim import simulate_batch
    return {"six": simulate_batch(1, 6, 20, seed=401)[0], "nine": simulate_batch(1, 9, 20, seed=402)[0],
            "two": simulate_batch(1, 2, 20, seed=403)[0]}


@pytest.fixture(scope="module")
def root_dir(tmp_path_factory, root_alns):
    d = tmp_path_factory.mktemp("root_alns")
    for stem, a in root_alns.items():
        _write_fasta(d / f"{stem}.fa", a)
    return d


def _cli(args, tmp_path):
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_root_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=900)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


KIND_NAMES = ["nj", "bme", "bionj", "bionj.bme"]
PREFIXES = ["" if k == "nj" else k + "." for k in KIND_NAMES]


def check_root_files(files, stem, pred, ids, method):
    """The files of ``--root`` of ``stem`` hold ``root.root_scores`` of the written tables and every ``.rooted.nwk`` is the rooted text of
    the kind's table: RF 0 to the kind's own tree, a root of two children."""
    text = files[f"{stem}.root.tsv"].decode()
    assert text.startswith(R.ROOT_HEAD) and list(R.parse_root_tsv(text)) == KIND_NAMES
    for row, name, pre in zip(text.splitlines(keepends=True)[1:], KIND_NAMES, PREFIXES):
        slots, lengths = kind_table(name, pred)
        s = R.root_scores(slots, lengths, *hostio.tree_root_host(slots, lengths)[:3], len(ids))
        assert row == R.root_line(name, method, s, ids)
        assert files[f"{stem}.{pre}rooted.nwk"].decode() == R.rooted_newick(ids, slots, lengths, *R.root_choice(s, method))
        rooted, own = (treecmp.parse_newick(files[f"{stem}.{x}"].decode()) for x in (f"{pre}rooted.nwk", f"{name}.nwk"))
        assert treecmp.robinson_foulds(rooted, own) == (0, 0.0) and len(rooted.children) == 2


def test_cli_root_files_and_the_files_of_fit_ols_and_treedist_beside_them(root_dir, root_alns, tmp_path):
    from helpers.oracle_root_engine import make
    from phyloformer_amd.weights import load_weights
    others = ["-t", "--bme", "--bionj", "--fit", "--ols", "--treedist"]
    plain = _cli([str(root_dir), "-o", str(tmp_path / "plain"), *others], tmp_path)
    r = _cli([str(root_dir), "-o", str(tmp_path / "o"), *others, "--root", "mad", "--bench"], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, plain.stderr[-2000:] + r.stderr[-3000:]
    files, base = _files(tmp_path / "o"), _files(tmp_path / "plain")
    added = {f"{stem}.root.tsv" for stem in root_alns} | {f"{stem}.{pre}rooted.nwk" for stem in root_alns for pre in PREFIXES}
    assert set(files) == set(base) | added and not added & set(base) and {"six.fit.tsv", "six.ols.tsv", "six.treedist.tsv"} <= set(base)
    assert all(files[name] == base[name] for name in base)       # the files of --fit, --ols, --treedist and every other output keep their bytes
    eng = make(load_weights(os.path.join(REPO, "models", "pf_base.ckpt")), 0)
    preds = {stem: eng.forward(root_alns[stem]).astype(np.float32) for stem in ("six", "nine")}
    for stem, pred in preds.items():
        check_root_files(files, stem, pred, names(len(root_alns[stem])), "mad")
    # two sequences have no join table: the kind's own text, and nan
    assert files["two.root.tsv"].decode().splitlines()[1:] == [R.root_line(k, "mad", R.no_scores()).rstrip("\n") for k in KIND_NAMES]
    assert files["two.rooted.nwk"] == files["two.nj.nwk"] and files["two.bionj.bme.rooted.nwk"] == files["two.bionj.bme.nwk"]
    report = json.loads([line for line in r.stderr.splitlines() if line.startswith("{")][-1])
    assert report["root"] == 3 and report["root_s"] > 0 and report["fit"] == 3
    # the other method, through the Python I/O and one alignment per launch: its own texts, the same table but for the method
    q = _cli([str(root_dir), "-o", str(tmp_path / "p"), "-t", "--bme", "--bionj", "--root", "midpoint", "--python-io", "--batch", "1"], tmp_path)
    assert q.returncode == 0, q.stderr[-3000:]
    other = _files(tmp_path / "p")
    for stem, pred in preds.items():
        check_root_files(other, stem, pred, names(len(root_alns[stem])), "midpoint")
        assert other[f"{stem}.root.tsv"].decode().replace("\tmidpoint\t", "\tmad\t") == files[f"{stem}.root.tsv"].decode()
    native = _cli([str(root_dir), "-o", str(tmp_path / "n"), "-t", "--bme", "--bionj", "--root", "midpoint"], tmp_path)
    assert native.returncode == 0 and _files(tmp_path / "n") == other


def test_cli_refuses_root_without_trees_and_with_site_sharding(root_dir, tmp_path):
    r = _cli([str(root_dir), "-o", str(tmp_path / "o"), "--root", "mad"], tmp_path)
    assert r.returncode == 2 and "--root roots the trees of --trees: give -t as well" in r.stderr
    r = _cli([str(root_dir), "-o", str(tmp_path / "o"), "-t", "--root", "midpoint", "--shard", "sites"], tmp_path)
    assert r.returncode == 2
    assert "--root cannot be combined with --shard sites: the site-sharded runner writes NJ trees only" in r.stderr
    r = _cli([str(root_dir), "-o", str(tmp_path / "o"), "-t", "--root", "outgroup"], tmp_path)
    assert r.returncode == 2 and "invalid choice: 'outgroup'" in r.stderr
    assert not os.path.exists(tmp_path / "o") or not os.listdir(tmp_path / "o")
    from phyloformer_amd.scheduler import DirectoryRunner, SiteShardedRunner
    with pytest.raises(ValueError, match="--root cannot be combined with --shard sites"):
        SiteShardedRunner(None, None, 0, 1, str(tmp_path), trees=True, root="mad")
    with pytest.raises(ValueError, match="--root roots the trees of --trees: give -t as well"):
        DirectoryRunner(None, str(tmp_path), root="mad")
    with pytest.raises(ValueError, match=r"--root takes one of mad, midpoint \(got outgroup\)"):
        DirectoryRunner(None, str(tmp_path), trees=True, root="outgroup")


def test_runner_takes_both_routes_with_the_threshold_lowered(tmp_path, root_alns, monkeypatch):
    """With the thresholds of --bme, --bionj and the rooting at 3 sequences the two kinds' tables are made on the GPU thread and
    ``Engine.tree_root`` runs there, one call per launch for all of them; the NJ tree's stay the writer's.  The files are those of the
    host route; a launch whose distances are not finite gets ``nan`` files."""
    from helpers.oracle_root_engine import OracleRootEngine
    from phyloformer_amd import bionj as bionj_mod
    from phyloformer_amd.scheduler import DirectoryRunner
    from phyloformer_amd.weights import load_weights
    assert R.ROOT_DEVICE_MIN is None or R.ROOT_DEVICE_MIN in (20, 60, 200, 512, 1024, 2048, 4096, 8192)
    w = load_weights(os.path.join(REPO, "models", "pf_base.ckpt"))
    for stem in ("six", "nine"):
        _write_fasta(tmp_path / f"{stem}.fa", root_alns[stem])
    paths = [str(tmp_path / "six.fa"), str(tmp_path / "nine.fa")]
    outs = {}
    for name, minimum in (("host", None), ("device", 3)):
        monkeypatch.setattr(bme, "BME_DEVICE_MIN", minimum)
        monkeypatch.setattr(bionj_mod, "BIONJ_DEVICE_MIN", minimum)
        monkeypatch.setattr(R, "ROOT_DEVICE_MIN", minimum)
        OracleRootEngine.root_calls = 0
        out = tmp_path / name
        out.mkdir()
        stats = DirectoryRunner(OracleRootEngine(w, 0), str(out), trees=True, bme=True, bionj=True, root="mad").run(paths)
        assert stats["root"] == 2 and stats["root_s"] > 0
        assert OracleRootEngine.root_calls == (2 if minimum else 0)
        outs[name] = _files(out)
    assert outs["host"] == outs["device"] and {"nine.bionj.bme.rooted.nwk", "nine.rooted.nwk", "six.root.tsv"} <= set(outs["host"])

    class NanEngine(OracleRootEngine):
        def forward(self, idx):
            return np.full((len(idx), idx.shape[1] * (idx.shape[1] - 1) // 2), np.nan, dtype=np.float32)

    out = tmp_path / "nan"
    out.mkdir()
    DirectoryRunner(NanEngine(w, 0), str(out), trees=True, bme=True, bionj=True, root="midpoint", native_io=False).run(paths[:1])
    assert (out / "six.root.tsv").read_text().splitlines()[1:] == [R.root_line(k, "midpoint", R.no_scores()).rstrip("\n") for k in KIND_NAMES]
    assert "nan" in (out / "six.rooted.nwk").read_text() and (out / "six.bme.rooted.nwk").read_text() == (out / "six.bme.nwk").read_text()
