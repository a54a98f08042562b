"""Query placement on the host (no GPU): ``join_query`` and the pair-index algebra of ``place_stats`` against a naive
restatement, ``ls_place`` against the true position of a pruned leaf and against a brute-force grid, ``graft``, and
``infer_alns.py --place`` through an oracle engine."""
import os
import subprocess
import sys

import numpy as np
import pytest

from phyloformer_amd import place as PL
from phyloformer_amd import treecmp as TC
from phyloformer_amd.taxa import pair_index

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = os.path.join(REPO, "data", "testdata", "trees")


# ---- join_query, place_stats ---------------------------------------------------------------------------------------

def test_join_query_is_the_row_table():
    rng = np.random.default_rng(1)
    idx = rng.integers(0, 22, size=(3, 7, 11), dtype=np.uint8)
    for N, q in ((2, 0), (2, 4), (5, 1), (6, 0)):
        rows = list(range(N)) + [N + q]
        got = PL.join_query(idx, N, q)
        assert got.shape == (3, N + 1, 11) and got.flags.c_contiguous and np.array_equal(got, idx[:, rows])
        assert np.array_equal(PL.join_query(idx[1], N, q), idx[1][rows])
    for N, q in ((1, 0), (5, 2), (5, -1), (7, 0)):
        with pytest.raises(ValueError):
            PL.join_query(idx, N, q)


def _naive_stats(whole, base, sets, N, Q):
    """The definitions, one pair at a time."""
    M = N + Q
    place = np.zeros((Q, N), np.float32)
    disturb, shift, joint = np.zeros(Q), np.zeros(Q), np.zeros(Q)
    for q in range(Q):
        s2 = 0.0
        for i in range(N):
            place[q, i] = sets[q][pair_index(i, N, N + 1)]
            s2 += (float(whole[pair_index(i, N + q, M)]) - float(place[q, i])) ** 2
        joint[q] = np.sqrt(s2 / N)
        s1 = s2 = 0.0
        for i in range(N):
            for j in range(i + 1, N):
                d = float(sets[q][pair_index(i, j, N + 1)]) - float(base[pair_index(i, j, N)])
                s1 += d
                s2 += d * d
        P = N * (N - 1) // 2
        disturb[q], shift[q] = np.sqrt(s2 / P), s1 / P
    return place, disturb, shift, joint


def test_place_stats_equals_the_naive_restatement():
    rng = np.random.default_rng(2)
    seen = set()
    for _ in range(40):
        N, Q = int(rng.integers(2, 8)), int(rng.integers(1, 4))
        seen.add((N, Q))
        M = N + Q
        whole = rng.uniform(0.01, 2, size=M * (M - 1) // 2).astype(np.float32)
        base = rng.uniform(0.01, 2, size=N * (N - 1) // 2).astype(np.float32)
        sets = rng.uniform(0.01, 2, size=(Q, (N + 1) * N // 2)).astype(np.float32)
        got = PL.place_stats(whole, base, sets, N, Q)
        want = _naive_stats(whole, base, sets, N, Q)
        assert got[0].dtype == np.float32 and np.array_equal(got[0], want[0])
        for g, w in zip(got[1:], want[1:]):
            assert g.dtype == np.float32 and g.shape == (Q,) and np.allclose(g, w, rtol=1e-6, atol=1e-9)
        batched = PL.place_stats(np.stack([whole, whole]), np.stack([base, base]), np.stack([sets, sets]), N, Q)
        assert all(np.array_equal(b[1], g) for b, g in zip(batched, got))
    assert (2, 1) in seen or len(seen) > 10
    with pytest.raises(ValueError):
        PL.place_stats(np.zeros(10), np.zeros(3), np.zeros((2, 6)), 3, 1)


def test_a_query_that_changes_nothing_has_zero_statistics():
    """sets[q] restricted to the backbone equal to base, whole's query rows equal to place: disturb = shift = joint = 0."""
    N, Q = 4, 2
    M = N + Q
    rng = np.random.default_rng(3)
    whole = rng.uniform(0.1, 1, size=M * (M - 1) // 2).astype(np.float32)
    base = np.array([whole[pair_index(i, j, M)] for i in range(N) for j in range(i + 1, N)], np.float32)
    sets = np.zeros((Q, (N + 1) * N // 2), np.float32)
    for q in range(Q):
        rows = list(range(N)) + [N + q]
        for i in range(N + 1):
            for j in range(i + 1, N + 1):
                sets[q, pair_index(i, j, N + 1)] = whole[pair_index(rows[i], rows[j], M)]
    place, disturb, shift, joint = PL.place_stats(whole, base, sets, N, Q)
    assert not disturb.any() and not shift.any() and not joint.any()
    assert np.array_equal(place[1], [whole[pair_index(i, N + 1, M)] for i in range(N)])


# ---- ls_place ------------------------------------------------------------------------------------------------------

def _unrooted(root):
    """(adjacency {node id: {neighbour id: length}}, {leaf name: node id}) of the unrooted tree, by this test's own walk."""
    adj, leaf = {}, {}
    count = [0]

    def walk(n):
        me = count[0]
        count[0] += 1
        adj[me] = {}
        if n.is_leaf():
            leaf[n.name] = me
        for c in n.children:
            k = walk(c)
            adj[me][k] = adj[k][me] = float(c.length or 0.0)
        return me

    walk(root)
    if len(adj[0]) == 2:
        (a, la), (b, lb) = adj.pop(0).items()
        del adj[a][0], adj[b][0]
        adj[a][b] = adj[b][a] = la + lb
    return adj, leaf


def _leaves_behind(adj, leaf_ids, start, block):
    seen, todo, out = {start, block}, [start], set()
    while todo:
        a = todo.pop()
        if a in leaf_ids:
            out.add(leaf_ids[a])
        for c in adj[a]:
            if c not in seen:
                seen.add(c)
                todo.append(c)
    return out


@pytest.mark.parametrize("stem", ["0_20_tips", "1_30_tips"])
def test_ls_place_finds_every_pruned_leaf_again(stem):
    root = TC.parse_newick(open(os.path.join(TREES, f"{stem}.nwk")).read())
    names, dm = TC.patristic(root)
    adj, leaf = _unrooted(root)
    leaf_ids = {v: k for k, v in leaf.items()}
    for t, name in enumerate(names):
        rest = [n for n in names if n != name]
        bb = PL.Backbone(PL.prune_leaves(root, [name]), rest)
        assert len(bb.edges) == 2 * len(rest) - 3
        got = PL.ls_place(bb, np.delete(dm[t], t))
        (w, pend), = adj[leaf[name]].items()
        (p, lp), (q, lq) = [(k, v) for k, v in adj[w].items() if k != leaf[name]]
        side_p = _leaves_behind(adj, leaf_ids, p, w)
        side_q = set(rest) - side_p
        a, b = sorted(side_p), sorted(side_q)
        assert bb.edge_label(got.edge) == "|".join(min((len(a), a), (len(b), b))[1])
        u, v, ell = bb.edges[got.edge]
        v_side = {rest[i] for i in np.flatnonzero(bb.v_side[got.edge])}
        assert v_side in (side_p, side_q)
        want_x = lq if v_side == side_p else lp                    # x runs from u, the end on the other side
        assert abs(ell - (lp + lq)) <= 1e-9 and abs(got.x - want_x) <= 1e-9 and abs(got.pendant - pend) <= 1e-9
        assert got.residual <= 1e-9 and got.rss >= 0.0


def _random_tree(rng, n, trifurcating):
    subs = [f"t{k}" for k in range(n)]
    while len(subs) > (3 if trifurcating else 2):
        a, b = sorted(rng.choice(len(subs), size=2, replace=False))
        joined = f"({subs[a]}:{rng.uniform(0.02, 0.6):.6f},{subs[b]}:{rng.uniform(0.02, 0.6):.6f})"
        subs = [s for k, s in enumerate(subs) if k not in (a, b)] + [joined]
    return "(" + ",".join(f"{s}:{rng.uniform(0.02, 0.6):.6f}" for s in subs) + ");"


def _brute_cases():
    """20 seeded trees of 6..12 leaves, two or three queries each: the distances of a point of the tree (an existing leaf,
    pruned) with noise, the same pulled towards the tree so that the pendant length wants to be negative, and a point
    just "inside" the root node where the root has three edges."""
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(7, 14))
        root = TC.parse_newick(_random_tree(rng, n, trifurcating=seed % 2 == 0))
        names, dm = TC.patristic(root)
        t = int(rng.integers(0, n))
        rest = [x for x in names if x != names[t]]
        bb = PL.Backbone(PL.prune_leaves(root, [names[t]]), rest)
        d = np.delete(dm[t], t)
        yield seed, bb, np.abs(d + rng.normal(0, 0.05 if seed % 4 < 2 else 0.3, size=d.size))
        yield seed, bb, np.abs(d - rng.uniform(0.3, 0.8) + rng.normal(0, 0.05, size=d.size))
        if not bb.merged_root:
            # all distances a little short of the root node's: the pendant length clamps to 0, and where none of the
            # root's three branches holds more than half the leaves, walking down any of them only lengthens more
            # distances than it shortens - x = 0 on the root's first edge
            yield seed, bb, np.abs(bb.D[0] - 0.1 + rng.normal(0, 0.005, size=d.size))


def _edge_model(bb, k, x, y):
    u, v, ell = bb.edges[k]
    return np.where(bb.v_side[k], y + (ell - x) + bb.D[v], y + x + bb.D[u])


def test_ls_place_against_a_grid_on_every_edge():
    clamps = {"x=0": 0, "x=l": 0, "y=0": 0, "inside": 0}
    for seed, bb, d in _brute_cases():
        assert 6 <= len(bb.labels) <= 12
        fits = [PL.fit_edge(bb, k, d) for k in range(len(bb.edges))]
        grid_min = []
        for k, (x, y, r) in enumerate(fits):
            ell = bb.edges[k][2]
            assert 0.0 <= x <= ell and y >= 0.0
            assert abs(r - float(((d - _edge_model(bb, k, x, y)) ** 2).sum())) <= 1e-12
            xs = np.linspace(0.0, ell, 201)[:, None, None]
            ys = np.linspace(0.0, float(d.max()) + 0.5, 201)[None, :, None]
            u, v, _ = bb.edges[k]
            model = np.where(bb.v_side[k][None, None, :], ys + (ell - xs) + bb.D[v][None, None, :], ys + xs + bb.D[u][None, None, :])
            g = float(((d[None, None, :] - model) ** 2).sum(axis=-1).min())
            assert r <= g + 1e-12, (seed, k, r, g)
            grid_min.append(g)
        got = PL.ls_place(bb, d)
        rs = [f[2] for f in fits]
        assert got.edge == int(np.argmin(rs)) and got.rss == min(rs) and got.rss <= min(grid_min) + 1e-12
        assert (got.x, got.pendant) == fits[got.edge][:2] and got.residual == np.sqrt(got.rss / d.size)
        ell = bb.edges[got.edge][2]
        clamps["x=0" if got.x == 0.0 else "x=l" if got.x == ell else "inside"] += 1
        clamps["y=0"] += got.pendant == 0.0
    print(clamps)
    assert clamps["x=0"] >= 1 and clamps["x=l"] >= 1 and clamps["y=0"] >= 1 and clamps["inside"] >= 1


def test_ls_place_ties_go_to_the_first_edge_and_two_leaves_have_one_edge():
    bb = PL.Backbone("(a:0.5,b:0.5,(c:0.5,d:0.5):0.5);", ["a", "b", "c", "d"])
    assert [(u, v) for u, v, _l in bb.edges] == [(0, 1), (0, 2), (0, 3), (3, 4), (3, 5)]
    got = PL.ls_place(bb, np.array([0.7, 0.7, 1.2, 1.2]))          # the root node itself: x = 0 on all three of its edges
    assert got.edge == 0 and got.x == 0.0 and abs(got.pendant - 0.2) <= 1e-12 and got.residual <= 1e-12
    assert bb.edge_label(0) == "a" and bb.edge_label(2) == "a|b" and bb.edge_label(2, ["z", "b", "c", "d"]) == "b|z"
    two = PL.Backbone("(a:0.1,b:0.3);", ["a", "b"])
    assert two.edges == [(1, 2, 0.4)]
    got = PL.ls_place(two, np.array([0.3, 0.5]))
    assert abs(got.x - 0.1) <= 1e-12 and abs(got.pendant - 0.2) <= 1e-12 and got.residual <= 1e-12
    with pytest.raises(ValueError):
        PL.Backbone("(a:0.1,b:-0.3,c:1);", ["a", "b", "c"])
    with pytest.raises(ValueError):
        PL.Backbone("(a:0.1,b:0.3,c:1);", ["a", "b"])


# ---- graft ---------------------------------------------------------------------------------------------------------

def test_graft_orders_queries_on_an_edge_and_prunes_back_to_the_backbone():
    text = "((a:0.1,b:0.2):0.3,c:0.4,(d:0.5,e:0.6):0.7);"
    labels = ["a", "b", "c", "d", "e"]
    bb = PL.Backbone(text, labels)
    k = next(k for k in range(len(bb.edges)) if bb.edge_label(k) == "d|e")
    pls = [PL.Placement(k, 0.5, 0.11, 0.0, 0.0), PL.Placement(k, 0.2, 0.22, 0.0, 0.0), PL.Placement(k, 0.5, 0.33, 0.0, 0.0),
           PL.Placement(0, 0.0, 0.44, 0.0, 0.0)]
    out = PL.graft(bb, pls, ["q0", "q1", "q2", "q3"])
    assert out.endswith(";\n")
    tree = TC.parse_newick(out)
    names, dm = TC.patristic(tree)
    at = {n: i for i, n in enumerate(names)}
    assert sorted(names) == sorted(labels + ["q0", "q1", "q2", "q3"])
    # along the edge from the root: q1 at 0.2, then q0 and q2 at 0.5 (q0 first), then the node of d and e
    assert abs(dm[at["c"], at["q1"]] - (0.4 + 0.2 + 0.22)) <= 1e-12
    assert abs(dm[at["q1"], at["q0"]] - (0.22 + 0.3 + 0.11)) <= 1e-12
    assert abs(dm[at["q0"], at["q2"]] - (0.11 + 0.33)) <= 1e-12
    assert abs(dm[at["q2"], at["d"]] - (0.33 + 0.2 + 0.5)) <= 1e-12
    assert abs(dm[at["q3"], at["a"]] - (0.44 + 0.3 + 0.1)) <= 1e-12
    assert out.index("q1") > out.index("q0") and out.index("q2") < out.index("q0")   # nested from the far end inwards
    back = PL.prune_leaves(tree, ["q0", "q1", "q2", "q3"])
    assert TC.robinson_foulds(back, TC.parse_newick(text))[0] == 0 and TC.branch_score(back, TC.parse_newick(text)) <= 1e-12


@pytest.mark.parametrize("stem", ["0_20_tips", "1_30_tips"])
def test_graft_of_least_squares_placements_prunes_back(stem):
    """A rooted binary tree (its root edge is one edge of two written halves), three leaves placed again."""
    root = TC.parse_newick(open(os.path.join(TREES, f"{stem}.nwk")).read())
    names, dm = TC.patristic(root)
    queries = [names[1], names[7], names[8]]
    rest = [n for n in names if n not in queries]
    keep = [names.index(n) for n in rest]
    backbone = PL.prune_leaves(root, queries)
    bb = PL.Backbone(backbone, rest)
    pls = [PL.ls_place(bb, dm[names.index(q)][keep]) for q in queries]
    pls.append(PL.Placement(0, bb.edges[0][2], 0.25, 0.0, 0.0))     # the far end of the merged root edge
    pls.append(PL.Placement(0, 0.0, 0.5, 0.0, 0.0))                 # and its near end
    tree = TC.parse_newick(PL.graft(bb, pls, queries + ["far", "near"]))
    back = PL.prune_leaves(tree, queries + ["far", "near"])
    assert TC.robinson_foulds(back, backbone)[0] == 0 and TC.branch_score(back, backbone) <= 1e-12
    got_names, got = TC.patristic(tree)
    at = {n: i for i, n in enumerate(got_names)}
    for q, p in zip(queries, pls):                                  # every query sits where its placement says
        fit = bb.D[bb.edges[p.edge][0]] + p.x + p.pendant
        for i, n in enumerate(rest):
            if not bb.v_side[p.edge][i]:
                assert abs(got[at[q], at[n]] - fit[i]) <= 1e-9


# ---- the CLI through the oracle engine -------------------------------------------------------------------------------

def _write_fasta(path, idx, ids=None):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">{ids[k] if ids else f's{k}'}\n{''.join(alpha[int(v)] for v in row)}\n")


@pytest.fixture(scope="module")
def place_alns():
    from phyloformer_amd.msa_sim import simulate_batch
    a = simulate_batch(2, 7, 40, seed=171)
    return {"a0": a[0], "a1": a[1], "c0": simulate_batch(1, 4, 40, seed=172)[0]}


def _ids(stem, n):
    return ["dup", "dup"] + [f"s{k}" for k in range(2, n)] if stem == "a1" else [f"s{k}" for k in range(n)]


@pytest.fixture(scope="module")
def place_dir(tmp_path_factory, place_alns):
    d = tmp_path_factory.mktemp("place_alns")
    for stem, a in place_alns.items():
        _write_fasta(d / f"{stem}.fa", a, ids=_ids(stem, len(a)))
    return d


def _cli(args, tmp_path):
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_place_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=900)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def test_cli_place_files(place_dir, place_alns, tmp_path):
    from helpers.oracle_place_engine import make
    from phyloformer_amd.weights import load_weights
    Q = 2
    plain = _cli([str(place_dir), "-o", str(tmp_path / "plain"), "-t"], tmp_path)
    r = _cli([str(place_dir), "-o", str(tmp_path / "o"), "-t", "--place", str(Q)], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, plain.stderr[-2000:] + r.stderr[-3000:]
    files, base = _files(tmp_path / "o"), _files(tmp_path / "plain")
    assert set(files) == set(base) | {f"{s}.{ext}" for s in place_alns for ext in ("place.dist.tsv", "place.tsv", "placed.nwk")}
    for name, data in base.items():
        assert files[name] == data, name                         # <stem>.phy / <stem>.nj.nwk exactly as without the flag
    eng = make(load_weights(os.path.join(REPO, "models", "pf_base.ckpt")), 0)
    for stem, a in place_alns.items():
        M = a.shape[0]
        N = M - Q
        ids = _ids(stem, M)
        _dist, _base, place, disturb, shift, joint = eng.forward_place(a, Q)
        rows = [r.split("\t") for r in files[f"{stem}.place.dist.tsv"].decode().splitlines()]
        assert rows[0] == ["query"] + ids[:N] and len(rows) == Q + 1
        for q, row in enumerate(rows[1:]):
            assert row == [ids[N + q]] + [f"{float(v):.10f}" for v in place[q]]
        rows = [r.split("\t") for r in files[f"{stem}.place.tsv"].decode().splitlines()]
        assert rows[0] == ["index", "id", "nearest", "nearest_distance", "disturb", "shift", "joint", "edge", "x", "pendant",
                           "residual"] and len(rows) == Q + 1
        for q, row in enumerate(rows[1:]):
            near = int(np.argmin(place[q]))
            assert row[:4] == [str(N + q), ids[N + q], ids[near], f"{float(place[q][near]):.10f}"]
            assert row[4:7] == [f"{float(v[q]):.10f}" for v in (disturb, shift, joint)]
            if N == 2:
                assert row[7:] == ["NA"] * 4
            else:
                assert set(row[7].split("|")) < set(ids[:N]) and float(row[8]) >= 0 and float(row[9]) >= 0 and float(row[10]) >= 0
        assert disturb.min() > 0 and joint.min() > 0              # context dependence
        if len(set(ids)) == len(ids):
            grafted = TC.parse_newick(files[f"{stem}.placed.nwk"].decode())
            assert sorted(TC.leaf_names(grafted)) == sorted(ids)
            if N >= 3:
                back = PL.prune_leaves(grafted, ids[N:])
                nj = TC.parse_newick(eng_nj(_base, ids[:N]))
                assert TC.robinson_foulds(back, nj)[0] == 0 and TC.branch_score(back, nj) <= 1e-6
    # the same files through the Python I/O; without -t no tree columns and no grafted tree
    p = _cli([str(place_dir), "-o", str(tmp_path / "p"), "-t", "--place", str(Q), "--python-io"], tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _files(tmp_path / "p") == files
    n = _cli([str(place_dir), "-o", str(tmp_path / "n"), "--place", str(Q), "--batch", "1"], tmp_path)
    assert n.returncode == 0, n.stderr[-3000:]
    nf = _files(tmp_path / "n")
    assert set(nf) == {k for k in files if not k.endswith(".nwk")}
    for k, v in nf.items():
        if k.endswith(".place.tsv"):
            assert v.decode().splitlines() == ["\t".join(r.split("\t")[:7]) for r in files[k].decode().splitlines()]
        else:
            assert v == files[k], k


def eng_nj(vec, ids):
    from phyloformer_amd.nj import neighbor_joining
    from phyloformer_amd.phylip import vec_to_phylip
    return neighbor_joining(vec_to_phylip(vec, ids)[0].astype("float64"), ids)


def test_cli_place_short_file_is_an_error_naming_the_file(tmp_path, place_alns):
    d = tmp_path / "in"
    d.mkdir()
    _write_fasta(d / "b3.fa", place_alns["a0"][:3])
    for io in ([], ["--python-io"]):
        r = _cli([str(d), "-o", str(tmp_path / ("o" + "".join(io))), "--place", "2", *io], tmp_path)
        assert r.returncode != 0
        assert "b3.fa" in r.stderr and "n = 3" in r.stderr and "Q = 2" in r.stderr and "--place" in r.stderr, r.stderr[-2000:]
        assert not os.listdir(tmp_path / ("o" + "".join(io)))


def test_cli_place_refused_combinations_and_usage(place_dir, tmp_path):
    for extra, msg in ((["--bootstrap", "5"], "--place is not supported with --bootstrap"),
                       (["--windows", "16"], "--place is not supported with --windows"),
                       (["--site-profile"], "--place is not supported with --site-profile"),
                       (["--leave-one-out"], "--place is not supported with --leave-one-out"),
                       (["--compress-sites"], "--place is not supported with --compress-sites"),
                       (["--devices", "0,1", "--shard", "sites"], "--place is not supported with --shard sites"),
                       (["--shard", "sites"], "--place is not supported with --shard sites")):
        r = _cli([str(place_dir), "-o", str(tmp_path / "x"), "--place", "2", *extra], tmp_path)
        assert r.returncode == 2 and msg in r.stderr, r.stderr[-1000:]
        assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")
    r = _cli([str(place_dir), "-o", str(tmp_path / "x"), "--place", "-1"], tmp_path)
    assert r.returncode == 2 and "--place must be >= 0 (got -1)" in r.stderr, r.stderr[-1000:]
    assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")
