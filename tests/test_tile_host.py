"""Tiled inference on the host (no GPU): ``tile.plan`` against a naive restatement of the covering scheme, the native
``pf_tile_groups`` / ``pf_tile_bound`` against it, ``tile.combine`` against the definitions one pair at a time, and
``infer_alns.py --tile`` through an oracle engine."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from phyloformer_amd import tile as TL
from phyloformer_amd.taxa import pair_index

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the plan ----------------------------------------------------------------------------------------------------------

def test_plan_against_a_naive_restatement():
    """All N <= 60, 2 <= M < N: the groups partition the rows, sizes differ by at most one, every set has at most M rows,
    every pair is covered once across groups and G - 1 times within a group."""
    for N in range(3, 61):
        for M in range(2, N):
            p = TL.plan(N, M)
            G = -(-N // (M // 2))
            assert p.G == G >= 3 and p.S == G * (G - 1) // 2 and (p.N, p.M) == (N, M)
            groups = [list(range(g * N // G, (g + 1) * N // G)) for g in range(G)]
            assert sum(groups, []) == list(range(N))                                  # a partition, in order
            sizes = [len(g) for g in groups]
            assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1
            assert p.bounds.tolist() == [g[0] for g in groups] + [N]
            assert p.groups_of_rows().tolist() == [g for g, rows in enumerate(groups) for _ in rows]
            assert list(p.sets) == [(g, h) for g in range(G) for h in range(g + 1, G)]
            cover = np.zeros((N, N), np.int64)
            at = 0
            for k, (g, h) in enumerate(p.sets):
                rows = groups[g] + groups[h]
                assert p.set_rows(k).tolist() == rows and len(rows) <= M
                assert p.offset[k] == at
                at += len(rows) * (len(rows) - 1) // 2
                r = np.array(rows)
                cover[np.ix_(r, r)] += 1
            assert p.T == at == p.offset[-1]
            assert len({len(p.set_rows(k)) for k in range(p.S)}) <= 3                 # at most three set sizes
            grp = p.groups_of_rows()
            same = grp[:, None] == grp[None, :]
            off_diag = ~np.eye(N, dtype=bool)
            assert (cover[~same] == 1).all() and (cover[same & off_diag] == G - 1).all()


@pytest.mark.parametrize("N,M", [(5, 1), (5, 0), (5, -2), (5, 5), (4, 5), (2, 2), (0, 2)])
def test_plan_refusals(N, M):
    with pytest.raises(ValueError):
        TL.plan(N, M)
    with pytest.raises(ValueError):
        TL.groups(N, M)


def test_library_plan_agrees_with_twin():
    from phyloformer_amd import build, engine
    build.build()
    lib = engine.load_library()
    for N in range(3, 61):
        for M in range(2, N):
            p = TL.plan(N, M)
            assert lib.pf_tile_groups(N, M) == p.G, (N, M)
            assert [lib.pf_tile_bound(N, M, g) for g in range(p.G + 1)] == p.bounds.tolist(), (N, M)
            assert lib.pf_tile_bound(N, M, -1) == -1 and lib.pf_tile_bound(N, M, p.G + 1) == -1
    for N, M in [(2000, 100), (65536, 200), (2 ** 31 - 1, 200), (2 ** 31 - 1, 2), (201, 200)]:
        G = TL.groups(N, M)
        assert lib.pf_tile_groups(N, M) == G
        for g in (0, 1, G // 2, G - 1, G):
            assert lib.pf_tile_bound(N, M, g) == g * N // G, (N, M, g)
    for N, M in [(5, 1), (5, 0), (5, -2), (5, 5), (4, 5), (2, 2), (0, 2), (-3, 2)]:
        assert lib.pf_tile_groups(N, M) == -1 and lib.pf_tile_bound(N, M, 0) == -1, (N, M)


# ---- cut_sets, combine -------------------------------------------------------------------------------------------------

def test_cut_sets_are_the_rows_of_the_plan():
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 22, size=(2, 11, 9), dtype=np.uint8)
    p = TL.plan(11, 5)
    sets = TL.cut_sets(idx, 5)
    assert len(sets) == p.S
    for k, s in enumerate(sets):
        assert s.flags.c_contiguous and s.dtype == np.uint8 and np.array_equal(s, idx[:, p.set_rows(k)])
        assert np.array_equal(TL.cut_sets(idx[1], 5)[k], idx[1][p.set_rows(k)])
    with pytest.raises(ValueError):
        TL.cut_sets(idx, 11)


def _naive_combine(sets, N, M):
    """The definitions, one pair and one set at a time; ``sets[k]`` float32 [P_m]."""
    p = TL.plan(N, M)
    grp = p.groups_of_rows()
    out = np.zeros(N * (N - 1) // 2, np.float32)
    spread = np.zeros_like(out)
    for i in range(N):
        for j in range(i + 1, N):
            vals = []
            for k in range(p.S):                                   # lexicographic (g, h): for a within-group pair this
                rows = p.set_rows(k).tolist()                      # IS ascending order of the partner group
                if i in rows and j in rows:
                    vals.append(sets[k][pair_index(rows.index(i), rows.index(j), len(rows))])
            if grp[i] != grp[j]:
                assert len(vals) == 1
                out[pair_index(i, j, N)] = vals[0]
                continue
            assert len(vals) == p.G - 1
            s = np.float64(0.0)
            for v in vals:
                s = s + np.float64(v)
            mean = s / np.float64(p.G - 1)
            ss = np.float64(0.0)
            for v in vals:
                d = np.float64(v) - mean
                ss = ss + d * d
            out[pair_index(i, j, N)] = np.float32(mean)
            spread[pair_index(i, j, N)] = np.float32(np.sqrt(ss / np.float64(p.G - 2)))
    return out, spread


@pytest.mark.parametrize("N,M", [(10, 6), (13, 8), (7, 4), (9, 2), (9, 3), (23, 5)])
def test_combine_on_random_values(N, M):
    """Cross-group entries are copies, within-group entries the ordered double mean, spread is 0 across groups."""
    rng = np.random.default_rng(N * 100 + M)
    p = TL.plan(N, M)
    sets = [rng.uniform(0.01, 3.0, size=(2, len(p.set_rows(k)) * (len(p.set_rows(k)) - 1) // 2)).astype(np.float32) for k in range(p.S)]
    out, spread = TL.combine(sets, N, M)
    assert out.shape == spread.shape == (2, N * (N - 1) // 2) and out.dtype == spread.dtype == np.float32
    flat = TL.assemble(sets)
    assert flat.shape == (2, p.T)
    again = TL.combine(flat, N, M)
    assert np.array_equal(out.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(spread.view(np.uint32), again[1].view(np.uint32))
    grp = p.groups_of_rows()
    cross = np.array([grp[i] != grp[j] for i in range(N) for j in range(i + 1, N)])
    for b in range(2):
        want = _naive_combine([s[b] for s in sets], N, M)
        assert np.array_equal(out[b].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(spread[b].view(np.uint32), want[1].view(np.uint32))
        one = TL.combine([s[b] for s in sets], N, M)                 # no batch axis
        assert np.array_equal(one[0].view(np.uint32), out[b].view(np.uint32))
    assert (spread[:, cross] == 0).all() and np.signbit(spread[:, cross]).sum() == 0
    if (~cross).any():
        assert (spread[:, ~cross] > 0).all()
    with pytest.raises(ValueError):
        TL.combine(flat[:, :-1], N, M)


def test_combine_of_equal_contexts_is_the_value_with_zero_spread():
    """When every context gives a pair the same value, the mean is that value and the spread 0."""
    N, M = 12, 6
    p = TL.plan(N, M)
    rng = np.random.default_rng(5)
    full = rng.uniform(0.1, 2.0, size=N * (N - 1) // 2).astype(np.float32)
    sets = []
    for k in range(p.S):
        rows = p.set_rows(k)
        sets.append(np.array([full[pair_index(rows[a], rows[b], N)] for a in range(len(rows)) for b in range(a + 1, len(rows))], np.float32))
    out, spread = TL.combine(sets, N, M)
    # G - 1 = 3 equal addends: 3 v / 3 is exact in double for a float v
    assert np.array_equal(out, full) and (spread == 0).all()


# ---- the CLI through the oracle engine ---------------------------------------------------------------------------------

def _write_fasta(path, idx, ids=None):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">{ids[k] if ids else f's{k}'}\n{''.join(alpha[int(v)] for v in row)}\n")


@pytest.fixture(scope="module")
def tile_alns():
    from phyloformer_amd.msa_sim import simulate_batch
    return {"big7": simulate_batch(1, 7, 24, seed=191)[0], "small3": simulate_batch(1, 3, 24, seed=192)[0]}


@pytest.fixture(scope="module")
def tile_dir(tmp_path_factory, tile_alns):
    d = tmp_path_factory.mktemp("tile_alns")
    for stem, a in tile_alns.items():
        _write_fasta(d / f"{stem}.fa", a)
    return d


def _cli(args, tmp_path):
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_tile_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=900)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def test_cli_tile_files(tile_dir, tile_alns, tmp_path):
    from helpers.oracle_tile_engine import make
    from phyloformer_amd.nj import neighbor_joining
    from phyloformer_amd.phylip import vec_to_phylip
    from phyloformer_amd.weights import load_weights
    M = 4
    plain = _cli([str(tile_dir), "-o", str(tmp_path / "plain"), "-t"], tmp_path)
    r = _cli([str(tile_dir), "-o", str(tmp_path / "o"), "-t", "--tile", str(M)], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, plain.stderr[-2000:] + r.stderr[-3000:]
    files, base = _files(tmp_path / "o"), _files(tmp_path / "plain")
    assert set(files) == set(base) | {"big7.spread.phy", "big7.tile.tsv"}
    # the file with N <= M runs exactly as without the flag
    assert files["small3.phy"] == base["small3.phy"] and files["small3.nj.nwk"] == base["small3.nj.nwk"]
    # the large file: the four outputs are those of combine on the oracle's forwards of the host-cut sets
    eng = make(load_weights(os.path.join(REPO, "models", "pf_base.ckpt")), 0)
    a = tile_alns["big7"]
    ids = [f"s{k}" for k in range(7)]
    sets = [eng.forward(s).astype(np.float32) for s in TL.cut_sets(a, M)]
    out, spread = TL.combine(sets, 7, M)
    got = eng.forward_tiled(a, M)
    assert np.array_equal(got[0], out) and np.array_equal(got[1], spread)
    assert files["big7.phy"].decode() == vec_to_phylip(out, ids)[1]
    assert files["big7.phy"] != base["big7.phy"]                            # context dependence: tiled is not untiled
    assert files["big7.spread.phy"].decode() == vec_to_phylip(spread, ids)[1]
    assert files["big7.nj.nwk"].decode() == neighbor_joining(vec_to_phylip(out, ids)[0].astype("float64"), ids)
    p = TL.plan(7, M)                                                        # G = 4 groups of 1, 2, 2, 2 rows
    assert p.G == 4 and np.diff(p.bounds).tolist() == [1, 2, 2, 2]
    rows = [line.split("\t") for line in files["big7.tile.tsv"].decode().splitlines()]
    assert rows[0] == ["index", "id", "group"]
    assert rows[1:] == [[str(k), ids[k], str(g)] for k, g in enumerate([0, 1, 1, 2, 2, 3, 3])]
    within = [pair_index(1, 2, 7), pair_index(3, 4, 7), pair_index(5, 6, 7)]
    assert (spread[within] > 0).all() and np.count_nonzero(spread) == 3
    # the same files through the Python I/O, and one alignment per launch; without -t no trees
    q = _cli([str(tile_dir), "-o", str(tmp_path / "p"), "-t", "--tile", str(M), "--python-io"], tmp_path)
    assert q.returncode == 0, q.stderr[-3000:]
    assert _files(tmp_path / "p") == files
    n = _cli([str(tile_dir), "-o", str(tmp_path / "n"), "--tile", str(M), "--batch", "1"], tmp_path)
    assert n.returncode == 0, n.stderr[-3000:]
    assert _files(tmp_path / "n") == {k: v for k, v in files.items() if not k.endswith(".nwk")}
    # a context that holds both files: exactly the run without the flag
    w = _cli([str(tile_dir), "-o", str(tmp_path / "w"), "-t", "--tile", "7"], tmp_path)
    assert w.returncode == 0 and _files(tmp_path / "w") == base, w.stderr[-3000:]


def test_cli_cap_stays_without_the_flag_and_is_lifted_with_it(tmp_path):
    """A 201-sequence file: the reference's ValueError without --tile (and with a context that does not lift it for
    another file's sake), tiled with --tile 200."""
    from phyloformer_amd.msa_sim import simulate_batch
    d = tmp_path / "in"
    d.mkdir()
    _write_fasta(d / "wide.fa", simulate_batch(1, 201, 4, seed=193)[0])
    msg = "n_seqs must be smaller or equal to 200 (or pre-compute a larger global_seq2pair)"
    for k, io in enumerate(([], ["--python-io"])):
        r = _cli([str(d), "-o", str(tmp_path / f"o{k}"), *io], tmp_path)
        assert r.returncode != 0 and "ValueError" in r.stderr and msg in r.stderr, r.stderr[-2000:]
        assert not os.listdir(tmp_path / f"o{k}")
    from phyloformer_amd import analyses, scheduler
    assert str(scheduler.too_many_seqs(201)) == msg and scheduler.too_many_seqs(200) is None
    t = analyses.Tile(200)
    assert scheduler.too_many_seqs(201, [t]) is None and scheduler.too_many_seqs(200, [t]) is None
    assert scheduler.over_seq_cap(np.array([3, 200, 201, 500]), [analyses.Tile(300)]).tolist() == [False, False, True, False]
    assert isinstance(scheduler.too_many_seqs(1, [t]), RuntimeError)


def test_cli_tile_refused_combinations_and_usage(tile_dir, tmp_path):
    for extra, msg in ((["--bootstrap", "5"], "--tile is not supported with --bootstrap"),
                       (["--windows", "16"], "--tile is not supported with --windows"),
                       (["--site-profile"], "--tile is not supported with --site-profile"),
                       (["--leave-one-out"], "--tile is not supported with --leave-one-out"),
                       (["--compress-sites"], "--tile is not supported with --compress-sites"),
                       (["--place", "1"], "--tile is not supported with --place"),
                       (["--devices", "0,1", "--shard", "sites"], "--tile is not supported with --shard sites"),
                       (["--shard", "sites"], "--tile is not supported with --shard sites")):
        r = _cli([str(tile_dir), "-o", str(tmp_path / "x"), "--tile", "4", *extra], tmp_path)
        assert r.returncode == 2 and msg in r.stderr, r.stderr[-1000:]
        assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")
    for bad in ("-1", "1", "201"):
        r = _cli([str(tile_dir), "-o", str(tmp_path / "x"), "--tile", bad], tmp_path)
        assert r.returncode == 2 and f"--tile must be 0 (off) or a context of 2 to 200 sequences (got {bad})" in r.stderr, r.stderr[-1000:]
        assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")


def test_tile_is_the_last_mode():
    from phyloformer_amd import analyses
    assert analyses.MODES[-1] is analyses.Tile and analyses.Tile.flag == "--tile"
    assert [o for o, _ in analyses.Tile.refuses] == [m.flag for m in analyses.MODES[:-1]] + [analyses.SHARD_SITES]


# ---- ABI ---------------------------------------------------------------------------------------------------------------

def test_header_declares_the_tile_entry_points():
    h = open(os.path.join(REPO, "include", "phyloformer_amd.h")).read()
    names = ("pf_forward_tiled", "pf_tile_combine_device", "pf_tile_groups", "pf_tile_bound")
    for name in names:
        assert re.search(rf"^int {name}\(", h, re.M), name
    assert int(re.search(r"#define PF_ABI_VERSION (\d+)", h).group(1)) == 5
    from phyloformer_amd import build, engine
    assert {"pf_tile.hip.h", "pf_tile_host.h"} <= set(build.HEADERS)
    assert not {"pf_tile.hip.h", "pf_tile_host.h"} & set(build.KERNEL_FILES)         # the kernel hash does not move
    assert set(names) <= set(engine.SIGNATURES) and engine.ABI_VERSION == 5
    build.build()
    lib = engine.load_library()
    assert all(hasattr(lib, n) for n in names) and lib.pf_abi_version() == 5
