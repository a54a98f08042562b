"""Delta scores without a GPU: the statement ``delta.delta_py`` on closed forms, the serial native twin
(``pf_delta_host``, ``hostio.delta_host``) against it bit for bit, the invariants of the integers, the refusals, the
sanitizer build of the twin as a stand-alone program (``tests/native/pf_delta_main.cpp``), and ``infer_alns.py --delta``
through a stand-in engine whose ``delta`` is the native twin."""
import ctypes as C
import os
import shutil
import subprocess
import sys
from math import comb

import numpy as np
import pytest

from helpers.delta_inputs import check_delta_files, mixed, pairs_of, relabel, small_integers, tree_distances, uniform
from phyloformer_amd import delta as D
from phyloformer_amd import hostio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
BOTH = [("statement", lambda p, n, k=20: D.delta_py(p, n, k)), ("native", lambda p, n, k=20: hostio.delta_host(p, n, k))]


def same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) and np.asarray(x).dtype == np.asarray(y).dtype for x, y in zip(a, b))


# ---- closed forms --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("who,fn", BOTH)
def test_one_quartet_two_thirds(who, fn):
    """d01 = d23 = 1, d02 = d13 = 2, d03 = d12 = 4: the sums are 2, 4, 8, delta = 2/3, q = rint(2^31 / 3), bin 13 of 20."""
    pred = np.array([1, 2, 4, 4, 2, 1], dtype=np.float32)       # pairs 01 02 03 12 13 23
    pair_sum, hist, flag = fn(pred, 4)
    q = int(np.rint(np.float64(2 ** 31) / np.float64(3)))
    assert q == 715827883 and pair_sum.tolist() == [q] * 6 and flag == 0
    assert hist.tolist() == [int(b == 13) for b in range(20)]
    s = D.delta_scores(pair_sum, hist, 4)
    assert s.quartets == 1 and s.overall == q / 2 ** 30 and s.taxon.tolist() == [q / 2 ** 30] * 4 and s.pair.tolist() == [q / 2 ** 30] * 6


@pytest.mark.parametrize("who,fn", BOTH)
@pytest.mark.parametrize("value", [0.0, 0.75])
def test_all_equal_distances_are_zeros(who, fn, value):
    n = 9
    pair_sum, hist, flag = fn(np.full(pairs_of(n), value, dtype=np.float32), n)
    assert not pair_sum.any() and flag == 0 and hist.tolist() == [comb(n, 4)] + [0] * 19


@pytest.mark.parametrize("who,fn", BOTH)
def test_a_tree_with_integer_branch_lengths_is_exactly_tree_like(who, fn):
    n = 12
    pred = tree_distances(n, 5)
    assert len(set(pred.tolist())) > 10
    pair_sum, hist, flag = fn(pred, n)
    assert not pair_sum.any() and flag == 0 and hist[0] == comb(n, 4) == hist.sum()


def test_a_sequence_off_the_tree_has_the_largest_delta():
    """A 13th sequence whose distances to the 12 others are perturbed off the tree: its per-taxon delta is the largest."""
    n = 13
    pred = tree_distances(n, 6)
    index = {(i, j): k for k, (i, j) in enumerate((i, j) for i in range(n) for j in range(i + 1, n))}
    rng = np.random.default_rng(7)
    for i in range(n - 1):
        pred[index[i, n - 1]] += np.float32(rng.integers(1, 12))
    got = hostio.delta_host(pred)
    assert same(got, D.delta_py(pred, n))
    s = D.delta_scores(got[0], got[1], n)
    assert int(np.argmax(s.taxon)) == n - 1 and s.taxon[n - 1] > 1.5 * np.delete(s.taxon, n - 1).max()
    # the quartets without it are still exactly tree-like: the other sequences' means come from its quartets alone
    assert got[1][0] >= comb(n - 1, 4)


# ---- the native twin against the statement ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 5, 7, 16, 33])
def test_native_equals_statement_on_random_matrices(n):
    for bins in (20, 1, 64) if n <= 16 else (20,):
        pred = uniform(n, 1000 + n)[0]
        assert same(hostio.delta_host(pred, bins=bins), D.delta_py(pred, n, bins))


@pytest.mark.parametrize("n,top", [(6, 2), (11, 3), (16, 4)])
def test_native_equals_statement_on_matrices_with_ties(n, top):
    pred = small_integers(n, 77 + n, top=top)[0]
    got = hostio.delta_host(pred, n)
    assert same(got, D.delta_py(pred, n))
    assert got[1][0] > 0 and got[1][-1] > 0           # zero denominators or equal larger sums, and delta = 1


def test_nonfinite_sources_among_clean_ones_and_batches():
    n = 8
    preds = uniform(n, 5, 3)
    preds[0, 4], preds[2, 11] = np.nan, -np.inf
    preds = np.concatenate([preds[:1], uniform(n, 6), preds[2:]])[[1, 0, 2]]      # clean, NaN, infinity
    pair_sum, hist, flag = hostio.delta_host(preds)
    assert flag.tolist() == [0, 1, 1] and pair_sum.dtype == np.int64 and hist.dtype == np.int64 and flag.dtype == np.uint8
    assert not pair_sum[1:].any() and not hist[1:].any()
    for b in range(3):
        one = hostio.delta_host(preds[b])
        assert same(one, (pair_sum[b], hist[b], flag[b]))
        assert same(one, D.delta_py(preds[b], n))
    mix = mixed(n, 12, 5)
    whole = hostio.delta_host(mix)
    assert whole[2].tolist() == [0, 0, 1, 0, 0]
    for b in range(5):
        assert same(hostio.delta_host(mix[b:b + 1]), tuple(x[b:b + 1] for x in whole))


# ---- invariants ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,bins", [(4, 20), (9, 7), (21, 64)])
def test_invariants_of_the_integers(n, bins):
    pred = uniform(n, 300 + n)[0]
    pair_sum, hist, flag = hostio.delta_host(pred, bins=bins)
    assert flag == 0 and int(hist.sum()) == comb(n, 4) and (pair_sum >= 0).all()
    i, j = np.triu_indices(n, k=1)
    taxon = np.zeros(n, dtype=np.int64)
    np.add.at(taxon, i, pair_sum)
    np.add.at(taxon, j, pair_sum)
    total = int(pair_sum.sum())
    assert not (taxon % 3).any() and total % 6 == 0
    assert int((taxon // 3).sum()) == 4 * (total // 6)
    s = D.delta_scores(pair_sum, hist, n)
    assert s.quartets == comb(n, 4) and 0 <= s.overall <= 1
    assert np.isclose(s.taxon.mean(), s.overall, rtol=1e-12) and np.isclose(s.pair.mean(), s.overall, rtol=1e-12)


def test_relabelling_permutes_the_pair_sums_and_keeps_the_histogram():
    n = 10
    pred = uniform(n, 41)[0]
    perm = np.random.default_rng(42).permutation(n).tolist()
    moved, where = relabel(pred, perm)
    a, b = hostio.delta_host(pred), hostio.delta_host(moved)
    assert np.array_equal(a[1], b[1]) and np.array_equal(b[0], a[0][where]) and not np.array_equal(a[0], b[0])


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_of_the_host_entry_points():
    p6 = np.ones(6, dtype=np.float32)
    for fn in (lambda p, **k: hostio.delta_host(p, **k), lambda p, **k: D.delta_py(p, D.n_of_pairs(len(p)), **k)):
        with pytest.raises(ValueError, match=r"delta scores take 4 <= N <= 2048 sequences \(got 3\)"):
            fn(np.ones(3, dtype=np.float32))
        with pytest.raises(ValueError, match=r"delta scores take 1 <= K <= 64 bins \(got 0\)"):
            fn(p6, bins=0)
        with pytest.raises(ValueError, match=r"delta scores take 1 <= K <= 64 bins \(got 65\)"):
            fn(p6, bins=65)
    with pytest.raises(ValueError, match=r"4 <= N <= 2048 sequences \(got 2049\)"):
        hostio.delta_host(np.ones((1, 2049 * 2048 // 2), dtype=np.float32))
    with pytest.raises(ValueError, match="bad dimensions B=0 N=4"):
        hostio.delta_host(np.ones((0, 6), dtype=np.float32))
    with pytest.raises(ValueError, match="expected 10 distances for 5 sequences, got 6"):
        hostio.delta_host(p6, 5)
    # the library itself: PF_EINVAL (-1) for each of them and for a null buffer, nothing written
    lib = hostio._lib()
    out, hist, flag = np.full(6, -7, dtype=np.int64), np.full(20, -7, dtype=np.int64), np.full(1, 9, dtype=np.uint8)
    ptrs = (out.ctypes.data, hist.ctypes.data, flag.ctypes.data)
    for b, n, k in ((1, 3, 20), (1, 2049, 20), (0, 4, 20), (1, 4, 0), (1, 4, 65)):
        assert lib.pf_delta_host(p6.ctypes.data, b, n, k, *ptrs) == -1
    for hole in range(4):
        args = [p6.ctypes.data, *ptrs]
        args[hole] = None
        assert lib.pf_delta_host(args[0], 1, 4, 20, *args[1:]) == -1
    assert (out == -7).all() and (hist == -7).all() and flag[0] == 9
    assert lib.pf_delta_host(p6.ctypes.data, 1, 4, 20, *ptrs) == 0 and not out.any() and hist[0] == 1 and flag[0] == 0


def test_the_bindings_name_the_three_entry_points():
    from phyloformer_amd.engine import CALL_TIME_SYMBOLS, SIGNATURES, Engine
    assert {"pf_delta", "pf_delta_device", "pf_delta_host"} <= set(SIGNATURES) & CALL_TIME_SYMBOLS
    assert SIGNATURES["pf_delta"][1][1:] == SIGNATURES["pf_delta_device"][1][1:] == SIGNATURES["pf_delta_host"][1]
    assert callable(Engine.delta) and callable(Engine.delta_device)
    with open(os.path.join(REPO, "include", "phyloformer_amd.h")) as fh:
        header = fh.read()
    for name in ("pf_delta(", "pf_delta_device(", "pf_delta_host("):
        assert f"int {name}" in header


# ---- the twin under AddressSanitizer and UBSan, as a stand-alone program ----------------------------------------------

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("delta_native") / "pf_delta_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_delta_main.cpp"),
           "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


@needs_gxx
@pytest.mark.parametrize("n,b,bins", [(4, 1, 1), (5, 3, 20), (17, 3, 64), (40, 2, 20)])
def test_twin_is_clean_under_asan_and_ubsan_and_equals_the_library(program, tmp_path, n, b, bins):
    preds = mixed(n, 900 + n, b)
    preds.tofile(tmp_path / "preds.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([program, str(b), str(n), str(bins), str(tmp_path / "preds.bin"), str(tmp_path / "res.bin")],
                         capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert res.returncode == 0 and f"clean, B = {b}, N = {n}, K = {bins}" in res.stdout, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    raw = (tmp_path / "res.bin").read_bytes()
    p = pairs_of(n)
    assert len(raw) == b * p * 8 + b * bins * 8 + b
    got = (np.frombuffer(raw, np.int64, b * p).reshape(b, p), np.frombuffer(raw, np.int64, b * bins, offset=b * p * 8).reshape(b, bins),
           np.frombuffer(raw, np.uint8, b, offset=(b * p + b * bins) * 8))
    assert same(got, hostio.delta_host(preds, bins=bins))
    assert got[2].tolist() == ([0, 1, 0] if b == 3 else [0] * b)


# ---- the CLI through a stand-in engine ----------------------------------------------------------------------------------

def _write_fasta(path, idx):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">s{k}\n{''.join(alpha[int(v)] for v in row)}\n")


@pytest.fixture(scope="module")
def delta_alns():
    from phyloformer_amd.msa_sim import simulate_batch
    return {"six": simulate_batch(1, 6, 20, seed=301)[0], "seven": simulate_batch(1, 7, 20, seed=302)[0],
            "three": simulate_batch(1, 3, 20, seed=303)[0]}


@pytest.fixture(scope="module")
def delta_dir(tmp_path_factory, delta_alns):
    d = tmp_path_factory.mktemp("delta_alns")
    for stem, a in delta_alns.items():
        _write_fasta(d / f"{stem}.fa", a)
    return d


def _cli(args, tmp_path):
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_delta_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=900)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def test_cli_delta_files(delta_dir, delta_alns, tmp_path):
    from helpers.oracle_delta_engine import make
    from phyloformer_amd.weights import load_weights
    plain = _cli([str(delta_dir), "-o", str(tmp_path / "plain"), "-t"], tmp_path)
    r = _cli([str(delta_dir), "-o", str(tmp_path / "o"), "-t", "--delta", "--bench"], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, plain.stderr[-2000:] + r.stderr[-3000:]
    files, base = _files(tmp_path / "o"), _files(tmp_path / "plain")
    added = {f"{stem}.delta.{kind}" for stem in delta_alns for kind in ("tsv", "phy", "hist.tsv")}
    assert set(files) == set(base) | added and not added & set(base)
    assert all(files[name] == base[name] for name in base)                 # .phy and .nj.nwk keep their bytes
    assert {n for n in base if n.endswith(".nj.nwk")} == {f"{stem}.nj.nwk" for stem in delta_alns}
    eng = make(load_weights(os.path.join(REPO, "models", "pf_base.ckpt")), 0)
    for stem in ("six", "seven"):
        a = delta_alns[stem]
        s = check_delta_files(files, stem, eng.forward(a).astype(np.float32), [f"s{k}" for k in range(len(a))])
        assert s.overall > 0
    # three sequences have no quartet: the files, with nan and 0 quartets
    text = files["three.delta.tsv"].decode().splitlines()
    assert text[0] == "# overall_delta=nan\tquartets=0" and text[2:] == [f"{k}\ts{k}\tnan\tnan" for k in range(3)]
    assert files["three.delta.phy"].decode().splitlines()[1].split()[1:] == ["0.0000000000", "nan", "nan"]
    assert D.parse_hist_tsv(files["three.delta.hist.tsv"].decode()).tolist() == [0] * 20
    assert all(r.split("\t")[4] == "nan" for r in files["three.delta.hist.tsv"].decode().splitlines()[1:])
    import json
    report = json.loads([line for line in r.stderr.splitlines() if line.startswith("{")][-1])
    assert report["delta"] == 3 and report["delta_s"] > 0
    # without -t, through the Python I/O and one alignment per launch: the same files but the trees
    q = _cli([str(delta_dir), "-o", str(tmp_path / "p"), "--delta", "--python-io", "--batch", "1"], tmp_path)
    assert q.returncode == 0, q.stderr[-3000:]
    assert _files(tmp_path / "p") == {k: v for k, v in files.items() if not k.endswith(".nwk")}


def test_cli_refuses_delta_with_site_sharding(delta_dir, tmp_path):
    r = _cli([str(delta_dir), "-o", str(tmp_path / "o"), "--delta", "--shard", "sites"], tmp_path)
    assert r.returncode == 2
    assert "--delta cannot be combined with --shard sites: the site-sharded runner writes distances and NJ trees only" in r.stderr
    assert not os.path.exists(tmp_path / "o") or not os.listdir(tmp_path / "o")
    from phyloformer_amd.scheduler import SiteShardedRunner
    with pytest.raises(ValueError, match="--delta cannot be combined with --shard sites"):
        SiteShardedRunner(None, None, 0, 1, str(tmp_path), delta=True)


def test_nonfinite_distances_get_nan_files(tmp_path):
    """The writer's side of a flagged file, without a run: ``no_scores`` through the three writers."""
    s = D.no_scores(5)
    assert s.quartets == 5 and np.isnan(s.taxon).all() and np.isnan(s.pair).all() and np.isnan(s.overall)
    text = D.delta_tsv([f"s{k}" for k in range(5)], s).splitlines()
    assert text[0] == "# overall_delta=nan\tquartets=5" and text[2] == "0\ts0\tnan\tnan"
    assert D.hist_tsv(np.zeros(20, dtype=np.int64)).splitlines()[1] == "0\t0.0000\t0.0500\t0\tnan"


def test_runner_writes_nan_files_for_a_flagged_file(tmp_path, delta_alns):
    """A launch whose engine hands over distances that are not finite: the flag comes back from ``delta`` and the three
    files hold ``nan`` and the number of quartets."""
    from phyloformer_amd.scheduler import DirectoryRunner

    class NanEngine:
        def forward(self, idx):
            return np.full((len(idx), pairs_of(idx.shape[1])), np.nan, dtype=np.float32)

        def delta(self, preds, bins=20):
            return hostio.delta_host(preds, bins=bins)

    _write_fasta(tmp_path / "six.fa", delta_alns["six"])
    out = tmp_path / "out"
    out.mkdir()
    stats = DirectoryRunner(NanEngine(), str(out), native_io=False, delta=True).run([str(tmp_path / "six.fa")])
    assert stats["delta"] == 1 and stats["delta_s"] > 0
    text = (out / "six.delta.tsv").read_text().splitlines()
    assert text[0] == "# overall_delta=nan\tquartets=15" and text[2:] == [f"{k}\ts{k}\tnan\tnan" for k in range(6)]
    assert D.parse_hist_tsv((out / "six.delta.hist.tsv").read_text()).tolist() == [0] * 20
    assert (out / "six.delta.phy").read_text().splitlines()[1].split()[1:] == ["0.0000000000"] + ["nan"] * 5
