"""Tree fit without a GPU: the statement ``fit.tree_fit_py`` on tables worked out by hand, the serial native twin
(``pf_tree_fit_host``, ``hostio.tree_fit_host``) against it bit for bit, an independent route through the Newick text, additive
distances, the statuses, the refusals, ``fit_scores``' identities, the sanitizer build of the twin as a stand-alone program
(``tests/native/pf_fit_main.cpp``), and ``infer_alns.py --fit`` through a stand-in engine whose device calls are the twins."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers.delta_inputs import tree_distances
from helpers.fit_inputs import balanced_slots, check_fit_files, pairs_of, same, table_len, trees, uniform
from phyloformer_amd import bme
from phyloformer_amd import fit as F
from phyloformer_amd import hostio, treecmp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
BOTH = [("statement", lambda p, s, l: F.tree_fit_batch_py(p, s, l)), ("native", lambda p, s, l: hostio.tree_fit_host(p, s, l))]


# ---- tables worked out by hand --------------------------------------------------------------------------------------

# five leaves: join (0, 1) at 1 and 2 -> node 5; join (0, 2) at 0.5 (node 5's branch) and -0.25 (leaf 2's, negative) -> node
# 6; the last three are slots 0 (node 6), 3, 4 at 1.5, 3 and 4.  Every figure below is a dyadic fraction: exact in any order.
HAND_SLOTS = np.array([0, 1, 0, 2, 0, 3, 4], dtype=np.int32)
HAND_LENGTHS = np.array([1.0, 2.0, 0.5, -0.25, 1.5, 3.0, 4.0])
#                     01    02   03   04   12    13   14   23    24    34
HAND_TREE = np.array([3.0, 1.25, 6.0, 7.0, 2.25, 7.0, 8.0, 4.25, 5.25, 7.0])
# the distances: the tree's but d01 = 3.5 (e = 0.5), d04 = 8 (e = 1), d13 = 6 (e = -1)
HAND_PRED = np.array([3.5, 1.25, 6.0, 8.0, 2.25, 6.0, 8.0, 4.25, 5.25, 7.0], dtype=np.float32)
HAND_ROWS = np.array([
    # ss    fm                          st     stt       sdt       worst
    [1.25, 0.25 / 12.25 + 1.0 / 64.0, 17.25, 95.5625, 104.0625, 1.0],      # 0: partners 1 (e 0.5, d 3.5) and 4 (e 1, d 8)
    [1.25, 0.25 / 12.25 + 1.0 / 36.0, 20.25, 127.0625, 121.5625, 1.0],     # 1: partners 0 (e 0.5) and 3 (e -1, d 6)
    [0.0, 0.0, 13.0, 52.25, 52.25, 0.0],                                   # 2: no residual
    [1.0, 1.0 / 36.0, 24.25, 152.0625, 145.0625, 1.0],                     # 3: partner 1
    [1.0, 1.0 / 64.0, 27.25, 189.5625, 196.5625, 1.0]])                    # 4: partner 0
HAND_WORST_J = [4, 3, 0, 1, 0]             # row 2: every |e| is 0, the smallest partner


@pytest.mark.parametrize("who,fn", BOTH)
def test_five_leaves_by_hand_with_a_negative_branch(who, fn):
    tree, rows, worst_j, status = fn(HAND_PRED, HAND_SLOTS, HAND_LENGTHS)
    assert status == 0 and tree.tolist() == HAND_TREE.tolist()
    assert same((rows,), (HAND_ROWS,)) and worst_j.tolist() == HAND_WORST_J
    parent, blen = F.nodes_of(HAND_SLOTS, HAND_LENGTHS, 5)
    assert parent.tolist() == [5, 5, 6, 7, 7, 6, 7, 7] and blen.tolist() == [1.0, 2.0, -0.25, 3.0, 4.0, 0.5, 1.5, 0.0]
    s = F.fit_scores(HAND_PRED, rows, worst_j, 5)
    assert s.ss == 2.25 and s.rmse == np.sqrt(0.225) and s.worst == (0, 4, 1.0)
    assert s.fm == (HAND_ROWS[0, 1] + HAND_ROWS[1, 1] + 0.0 + HAND_ROWS[3, 1] + HAND_ROWS[4, 1]) * 0.5
    assert s.taxon_rms.tolist() == [np.sqrt(1.25 / 4), np.sqrt(1.25 / 4), 0.0, 0.5, 0.5]


@pytest.mark.parametrize("who,fn", BOTH)
def test_three_sequences_have_no_join(who, fn):
    """T = 3: the three leaves under node 3, at 1, 2 and -0.5."""
    pred = np.array([3.0, 1.0, 1.5], dtype=np.float32)
    tree, rows, worst_j, status = fn(pred, np.array([0, 1, 2], dtype=np.int32), np.array([1.0, 2.0, -0.5]))
    assert status == 0 and tree.tolist() == [3.0, 0.5, 1.5]
    assert rows.tolist() == [[0.25, 0.25, 3.5, 9.25, 9.5, 0.5], [0.0, 0.0, 4.5, 11.25, 11.25, 0.0], [0.25, 0.25, 2.0, 2.5, 2.75, 0.5]]
    assert worst_j.tolist() == [2, 0, 0]
    # the slots in another order: the same tree
    again = fn(pred, np.array([2, 0, 1], dtype=np.int32), np.array([-0.5, 1.0, 2.0]))
    assert same(again, (tree, rows, worst_j, status))


# ---- the native twin against the statement ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 4, 5, 31, 64, 65, 130])
def test_native_equals_statement_bit_for_bit(n):
    """NJ and BIONJ tables of random distances and a caterpillar with random lengths, B = 3 sources of M = 3 trees; B = 1 and M
    = 1 are their slices, which must come out the same."""
    preds, slots, lengths = trees(n, 2000 + n, 3, 3)
    got = hostio.tree_fit_host(preds, slots, lengths)
    assert got[0].dtype == np.float64 and got[1].shape == (3, 3, n, 6) and got[2].dtype == np.int32 and got[3].dtype == np.uint8
    assert not got[3].any()
    for b in range(3 if n <= 65 else 1):
        for m in range(3):
            assert same(tuple(x[b, m] for x in got), F.tree_fit_py(preds[b], slots[b, m], lengths[b, m], n)), (b, m)
    assert same(hostio.tree_fit_host(preds[:1], slots[:1, :1], lengths[:1, :1]), tuple(x[:1, :1] for x in got))      # B = 1, M = 1
    assert same(hostio.tree_fit_host(preds[1:2], slots[1:2], lengths[1:2]), tuple(x[1:2] for x in got))              # B = 1, M = 3
    assert same(hostio.tree_fit_host(preds, slots[:, 2], lengths[:, 2]), tuple(x[:, 2] for x in got))                # B = 3, M = 1
    assert same(hostio.tree_fit_host(preds[2], slots[2, 1], lengths[2, 1]), tuple(x[2, 1] for x in got))
    without = hostio.tree_fit_host(preds, slots, lengths, patristic=False)
    assert without[0] is None and same(without[1:], got[1:])


@pytest.mark.parametrize("n", [5, 31, 130])
def test_an_independent_route_through_the_newick_text(n):
    """``newick_of_joins`` writes every length with ``repr``; ``treecmp.patristic`` sums child by child, in another order.  A
    distance is a sum of at most 260 terms, so the two differ by a few hundred float64 roundings: a relative 1e-12."""
    preds, slots, lengths = trees(n, 3000 + n, 1, 3)
    ids = [f"s{k}" for k in range(n)]
    got = hostio.tree_fit_host(preds, slots, lengths)[0]
    for m in range(3):
        root = treecmp.parse_newick(hostio.newick_of_joins_py(slots[0, m], lengths[0, m], ids, clamp_negative=False))
        names, dm = treecmp.patristic(root)
        order = [names.index(x) for x in ids]
        want = dm[np.ix_(order, order)][np.triu_indices(n, k=1)]
        worst = (np.abs(got[0, m] - want) / np.abs(want)).max()
        print(f"n={n} tree {m}: largest relative difference {worst:.3e}")
        assert worst <= 1e-12


def test_additive_distances_are_fitted_exactly():
    """The path lengths of a tree with integer branches in [1, 9] through NJ: the tree reproduces them.  Measured: the
    largest residual is 0.0 at all three sizes (NJ's lengths are halves of small integers here, every sum exact), explained
    is 1.0, and the correlation 1.0, 1.0 and 0.9999999999999999 (its own sums of products round)."""
    for n, seed in ((12, 5), (33, 6), (70, 7)):
        pred = tree_distances(n, seed)
        slots, lengths, flag = hostio.nj_joins_host(pred[None])
        tree, rows, worst_j, status = hostio.tree_fit_host(pred, slots[0], lengths[0])
        s = F.fit_scores(pred, rows, worst_j, n)
        print(f"additive n={n}: largest residual {rows[:, F.WORST].max()!r}, explained {s.explained!r}, correlation {s.correlation!r}")
        # float64 NJ on integers below 2^10: a residual is at most a few roundings of sums below 2^11
        assert status == 0 and rows[:, F.WORST].max() <= 1e-9
        assert round(s.explained, 12) == 1.0 and s.correlation == pytest.approx(1.0, abs=1e-12)


# ---- the statuses ---------------------------------------------------------------------------------------------------------

def _zeros(out):
    return not any(np.asarray(x).any() for x in out[:3])


@pytest.mark.parametrize("who,fn", BOTH)
def test_status_1_for_a_nan_distance_or_an_infinite_length(who, fn):
    n = 9
    preds, slots, lengths = trees(n, 41, 1, 3)
    clean = fn(preds, slots, lengths)
    bad = preds.copy()
    bad[0, 11] = np.nan
    out = fn(bad, slots, lengths)
    assert out[3].tolist() == [[1, 1, 1]] and _zeros(out)
    for value in (np.inf, -np.inf, np.nan):
        longer = lengths.copy()
        longer[0, 1, table_len(n) - 1] = value
        out = fn(preds, slots, longer)
        assert out[3].tolist() == [[0, 1, 0]] and _zeros(tuple(x[0, 1] for x in out))
        assert same(tuple(x[0, ::2] for x in out), tuple(x[0, ::2] for x in clean))
    bad[0, 11] = np.inf
    assert fn(bad, slots, lengths)[3].tolist() == [[1, 1, 1]]


def _malformed(n, case):
    slots = bme.caterpillar_slots(n).copy()
    if case == "a slot of N":
        slots[2] = n
    elif case == "a negative slot":
        slots[5] = -1
    elif case == "a slot joined after it left":
        slots[4] = slots[1]                     # join 0's b has left
    elif case == "a == b":
        slots[3] = slots[2]
    elif case == "a last slot that has left":
        slots[-1] = slots[1]
    elif case == "two equal last slots":
        slots[-1] = slots[-2]
    elif case == "a last slot outside":
        slots[-2] = 2 ** 31 - 1
    return slots


@pytest.mark.parametrize("who,fn", BOTH)
@pytest.mark.parametrize("case", ["a slot of N", "a negative slot", "a slot joined after it left", "a == b", "a last slot that has left",
                                  "two equal last slots", "a last slot outside"])
def test_status_2_for_a_table_that_is_no_join_table(who, fn, case):
    n = 8
    preds = uniform(n, 3)
    good = bme.caterpillar_slots(n)
    assert F.table_status(good, n) == 0 and F.table_status(_malformed(n, case), n) == 2
    slots = np.stack([good, _malformed(n, case), good])[None]
    lengths = np.random.default_rng(4).uniform(0.1, 1.0, size=slots.shape)
    lengths[0, 2] = lengths[0, 0]
    lengths[0, 1, 0] = np.nan                   # no table AND not finite: 2, the table is checked first
    out = fn(preds, slots, lengths)
    assert out[3].tolist() == [[0, 2, 0]] and _zeros(tuple(x[0, 1] for x in out))
    assert same(tuple(x[0, 0] for x in out), tuple(x[0, 2] for x in out)) and out[1][0, 0].any()


# ---- refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_and_their_messages():
    p3, s3, l3 = np.ones(3, dtype=np.float32), np.array([0, 1, 2], dtype=np.int32), np.ones(3)
    for fn in (hostio.tree_fit_host, F.tree_fit_batch_py):
        with pytest.raises(ValueError, match=r"tree fit needs N >= 3 sequences \(got 2\)"):
            fn(np.ones(1, dtype=np.float32), np.zeros(1, dtype=np.int32), np.zeros(1))
        with pytest.raises(ValueError, match=r"tree fit needs B >= 1 sources \(got 0\)"):
            fn(np.ones((0, 3), dtype=np.float32), np.zeros((0, 1, 3), dtype=np.int32), np.zeros((0, 1, 3)))
        with pytest.raises(ValueError, match=r"tree fit needs M >= 1 trees per source \(got 0\)"):
            fn(np.ones((1, 3), dtype=np.float32), np.zeros((1, 0, 3), dtype=np.int32), np.zeros((1, 0, 3)))
        with pytest.raises(ValueError, match="3 distances and 5 slots are not those of one number of sequences"):
            fn(p3, np.zeros(5, dtype=np.int32), np.zeros(5))
        with pytest.raises(ValueError, match="expected distances"):
            fn(p3, s3, np.ones(4))
    with pytest.raises(ValueError, match=r"tree fit takes at most 8192 sequences \(got 8193\)"):
        F.refuse(1, 1, 8193)
    with pytest.raises(ValueError, match=r"tree fit needs N >= 3 sequences \(got 2\)"):
        F.tree_fit_py(p3, s3, l3, 2)
    # the library itself: PF_EINVAL (-1) for each of them and for a null buffer other than patristic, nothing written
    lib = hostio._lib()
    out = (np.full(3, -7.0), np.full((3, 6), -7.0), np.full(3, -7, dtype=np.int32), np.full(1, 9, dtype=np.uint8))
    ptrs = [a.ctypes.data for a in out]
    ins = [p3.ctypes.data, s3.ctypes.data, l3.ctypes.data]
    for b, m, n in ((1, 1, 2), (1, 1, 8193), (1, 1, 65537), (0, 1, 3), (1, 0, 3), (-1, 1, 3)):
        assert lib.pf_tree_fit_host(*ins, b, m, n, *ptrs) == -1
    for hole in (0, 1, 2, 4, 5, 6):
        args = [*ins, *ptrs]
        args[hole] = None
        assert lib.pf_tree_fit_host(*args[:3], 1, 1, 3, *args[3:]) == -1
    assert all((a == a.flat[0]).all() for a in out)
    assert lib.pf_tree_fit_host(*ins, 1, 1, 3, None, *ptrs[1:]) == 0 and out[3][0] == 0 and (out[0] == -7).all()
    assert out[1][:, 2].tolist() == [4.0, 4.0, 4.0]


def test_the_bindings_name_the_three_entry_points():
    from phyloformer_amd.engine import CALL_TIME_SYMBOLS, SIGNATURES, Engine
    from phyloformer_amd.treekinds import NativeHost, PythonHost
    names = {"pf_tree_fit", "pf_tree_fit_device", "pf_tree_fit_host"}
    assert names <= set(SIGNATURES) & CALL_TIME_SYMBOLS
    assert SIGNATURES["pf_tree_fit"][1][1:] == SIGNATURES["pf_tree_fit_device"][1][1:] == SIGNATURES["pf_tree_fit_host"][1]
    assert callable(Engine.tree_fit) and callable(Engine.tree_fit_device)
    with open(os.path.join(REPO, "include", "phyloformer_amd.h")) as fh:
        header = fh.read()
    assert all(f"int {name}(" in header for name in names)
    preds, slots, lengths = trees(6, 8, 2, 2)
    assert same(NativeHost().tree_fit(preds, slots, lengths), PythonHost().tree_fit(preds, slots, lengths))
    assert PythonHost().tree_fit(preds, slots, lengths, patristic=False)[0] is None


# ---- fit_scores -------------------------------------------------------------------------------------------------------------

def test_identities_of_the_derived_scores():
    n = 31
    preds, slots, lengths = trees(n, 77, 1, 1)
    tree, rows, worst_j, status = hostio.tree_fit_host(preds[0], slots[0, 0], lengths[0, 0])
    s = F.fit_scores(preds[0], rows, worst_j, n)
    # the half sum is exact: twice the score is the sum over the rows in their order
    total = 0.0
    for x in rows[:, F.SS].tolist():
        total = total + x
    assert s.ss * 2.0 == total and F.half_sum(rows[:, F.FM]) == s.fm
    e = preds[0].astype(np.float64) - tree
    assert s.ss == pytest.approx(float(e @ e), rel=1e-13) and s.rmse == pytest.approx(np.sqrt(np.mean(e * e)), rel=1e-13)
    d = preds[0].astype(np.float64)
    assert s.explained == pytest.approx(1 - float(e @ e) / float(((d - d.mean()) ** 2).sum()), rel=1e-12)
    assert s.correlation == pytest.approx(np.corrcoef(d, tree)[0, 1], abs=1e-12)
    i, j, worst = s.worst
    p = F.pair_index(i, j, n)
    assert i < j and worst == np.abs(e).max() == abs(e[p]) and int(np.argmax(np.abs(e))) == p
    assert s.taxon_rms == pytest.approx(np.sqrt(rows[:, F.SS] / (n - 1)))
    # a tree against its own distances (rounded to float32 and lifted again): residual 0 beyond float32, correlation 1
    own = tree.astype(np.float32)
    t2, rows2, worst2, _ = hostio.tree_fit_host(own, slots[0, 0], lengths[0, 0])
    s2 = F.fit_scores(own, rows2, worst2, n)
    assert s2.correlation == pytest.approx(1.0, abs=1e-12) and round(s2.explained, 12) == 1.0
    # constant distances: no variance to explain
    flat = np.full(pairs_of(n), 0.5, dtype=np.float32)
    _, rows3, worst3, _ = hostio.tree_fit_host(flat, slots[0, 0], lengths[0, 0])
    s3 = F.fit_scores(flat, rows3, worst3, n)
    assert np.isnan(s3.explained) and np.isnan(s3.correlation) and s3.rmse > 0
    # distances of zero and below carry no Fitch-Margoliash term
    zero = preds[0].copy()
    zero[:5] = 0.0
    zero[5] = -1.0
    _, rows4, _, st4 = hostio.tree_fit_host(zero, slots[0, 0], lengths[0, 0])
    assert st4 == 0 and np.isfinite(rows4).all()
    assert same((rows4,), (F.tree_fit_py(zero, slots[0, 0], lengths[0, 0], n)[1],))


def test_a_balanced_table_is_a_join_table_and_shallow():
    for n in (3, 4, 7, 8, 9, 130):
        slots = balanced_slots(n)
        assert len(slots) == table_len(n) and F.table_status(slots, n) == 0
    parent, _ = F.nodes_of(balanced_slots(130), np.ones(table_len(130)), 130)

    def depth(x):
        return 0 if parent[x] == x else 1 + depth(parent[x])
    deep = F.nodes_of(bme.caterpillar_slots(130), np.ones(table_len(130)), 130)[0]

    def depth_cat(x):
        return 0 if deep[x] == x else 1 + depth_cat(deep[x])
    assert max(depth(x) for x in range(130)) <= 9 and max(depth_cat(x) for x in range(130)) >= 127


# ---- the twin under AddressSanitizer and UBSan, as a stand-alone program ------------------------------------------------

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fit_native") / "pf_fit_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_fit_main.cpp"),
           "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


@needs_gxx
@pytest.mark.parametrize("n,b,m,keep", [(3, 1, 1, 1), (5, 3, 3, 1), (31, 2, 3, 0), (65, 3, 3, 1)])
def test_twin_is_clean_under_asan_and_ubsan_and_equals_the_library(program, tmp_path, n, b, m, keep):
    preds, slots, lengths = trees(n, 900 + n, b, m)
    if n >= 5:                                 # tables that are none, and lengths that are not finite, among the fine ones
        slots[0, 0] = _malformed(n, "a last slot outside")
        slots[b - 1, m - 1] = _malformed(n, "a negative slot")
        lengths[b - 1, 0, 1] = np.inf
    for name, a in (("preds", preds), ("slots", slots), ("lengths", lengths)):
        a.tofile(tmp_path / f"{name}.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([program, str(b), str(m), str(n), str(keep), *(str(tmp_path / f"{x}.bin") for x in ("preds", "slots", "lengths")),
                          str(tmp_path / "res.bin")], capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert res.returncode == 0 and f"clean, B = {b}, M = {m}, N = {n}, keep = {keep}" in res.stdout, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    raw = (tmp_path / "res.bin").read_bytes()
    p, items = pairs_of(n), b * m
    sizes = [items * p * 8 * keep, items * n * 6 * 8, items * n * 4, items]
    assert len(raw) == sum(sizes)
    at = np.cumsum([0] + sizes)
    got = (np.frombuffer(raw, np.float64, items * p * keep, offset=int(at[0])).reshape(b, m, p) if keep else None,
           np.frombuffer(raw, np.float64, items * n * 6, offset=int(at[1])).reshape(b, m, n, 6),
           np.frombuffer(raw, np.int32, items * n, offset=int(at[2])).reshape(b, m, n),
           np.frombuffer(raw, np.uint8, items, offset=int(at[3])).reshape(b, m))
    assert same(got, hostio.tree_fit_host(preds, slots, lengths, patristic=bool(keep)))
    assert n < 5 or (got[3][0, 0] == 2 and got[3][b - 1, m - 1] == 2)


# ---- the CLI through a stand-in engine ------------------------------------------------------------------------------------

def _write_fasta(path, idx):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">s{k}\n{''.join(alpha[int(v)] for v in row)}\n")


@pytest.fixture(scope="module")
def fit_alns():
    from phyloformer_amd.msa_sim import simulate_batch
    return {"six": simulate_batch(1, 6, 20, seed=401)[0], "nine": simulate_batch(1, 9, 20, seed=402)[0],
            "two": simulate_batch(1, 2, 20, seed=403)[0]}


@pytest.fixture(scope="module")
def fit_dir(tmp_path_factory, fit_alns):
    d = tmp_path_factory.mktemp("fit_alns")
    for stem, a in fit_alns.items():
        _write_fasta(d / f"{stem}.fa", a)
    return d


def _cli(args, tmp_path):
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_fit_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=900)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


KIND_NAMES = ["nj", "bme", "bionj", "bionj.bme"]


def test_cli_fit_files(fit_dir, fit_alns, tmp_path):
    from helpers.oracle_fit_engine import make
    from phyloformer_amd.weights import load_weights
    plain = _cli([str(fit_dir), "-o", str(tmp_path / "plain"), "-t", "--bme", "--bionj"], tmp_path)
    r = _cli([str(fit_dir), "-o", str(tmp_path / "o"), "-t", "--bme", "--bionj", "--fit", "--bench"], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, plain.stderr[-2000:] + r.stderr[-3000:]
    files, base = _files(tmp_path / "o"), _files(tmp_path / "plain")
    prefixes = ["" if k == "nj" else k + "." for k in KIND_NAMES]
    added = ({f"{stem}.fit.tsv" for stem in fit_alns} |
             {f"{stem}.{pre}{end}" for stem in fit_alns for pre in prefixes for end in ("fit.taxa.tsv", "patristic.phy")})
    assert set(files) == set(base) | added and not added & set(base)
    assert all(files[name] == base[name] for name in base)                 # every other output keeps its bytes
    eng = make(load_weights(os.path.join(REPO, "models", "pf_base.ckpt")), 0)
    for stem in ("six", "nine"):
        a = fit_alns[stem]
        lines = check_fit_files(files, stem, eng.forward(a).astype(np.float32), [f"s{k}" for k in range(len(a))], KIND_NAMES)
        assert all(v[0] >= 0 and v[1] <= 1 for v in lines.values())
    # two sequences have no join table: the files, with nan
    text = files["two.fit.tsv"].decode().splitlines()
    assert text[1:] == [f"{k}\tnan\tnan\tnan\tnan\t0\t0\tnan" for k in KIND_NAMES]
    assert files["two.bme.fit.taxa.tsv"].decode().splitlines()[1:] == ["0\ts0\tnan\tnan", "1\ts1\tnan\tnan"]
    assert files["two.patristic.phy"].decode().splitlines()[1].split()[1:] == ["0.0000000000", "nan"]
    report = json.loads([line for line in r.stderr.splitlines() if line.startswith("{")][-1])
    assert report["fit"] == 3 and report["fit_s"] > 0
    # through the Python I/O and one alignment per launch: the same files
    q = _cli([str(fit_dir), "-o", str(tmp_path / "p"), "-t", "--bme", "--bionj", "--fit", "--python-io", "--batch", "1"], tmp_path)
    assert q.returncode == 0, q.stderr[-3000:]
    assert _files(tmp_path / "p") == files


def test_cli_refuses_fit_without_trees_and_with_site_sharding(fit_dir, tmp_path):
    r = _cli([str(fit_dir), "-o", str(tmp_path / "o"), "--fit"], tmp_path)
    assert r.returncode == 2 and "--fit measures the trees of --trees: give -t as well" in r.stderr
    r = _cli([str(fit_dir), "-o", str(tmp_path / "o"), "-t", "--fit", "--shard", "sites"], tmp_path)
    assert r.returncode == 2
    assert "--fit cannot be combined with --shard sites: the site-sharded runner writes NJ trees only" in r.stderr
    assert not os.path.exists(tmp_path / "o") or not os.listdir(tmp_path / "o")
    from phyloformer_amd.scheduler import DirectoryRunner, SiteShardedRunner
    with pytest.raises(ValueError, match="--fit cannot be combined with --shard sites"):
        SiteShardedRunner(None, None, 0, 1, str(tmp_path), trees=True, fit=True)
    with pytest.raises(ValueError, match="--fit measures the trees of --trees: give -t as well"):
        DirectoryRunner(None, str(tmp_path), fit=True)


def test_runner_fits_on_the_gpu_thread_where_the_tables_are_made_there(tmp_path, fit_alns, monkeypatch):
    """With the thresholds of --bme, --bionj and the fit at 3 sequences the two kinds' tables are made on the GPU thread and ``Engine.tree_fit``
    runs there, one call per launch for all of them; the NJ tree's fit stays the writer's.  The files are those of the host
    path; a launch whose distances are not finite gets ``nan`` files."""
    from helpers.oracle_fit_engine import OracleFitEngine
    from phyloformer_amd import bionj as bionj_mod
    from phyloformer_amd.scheduler import DirectoryRunner
    from phyloformer_amd.weights import load_weights
    w = load_weights(os.path.join(REPO, "models", "pf_base.ckpt"))
    for stem in ("six", "nine"):
        _write_fasta(tmp_path / f"{stem}.fa", fit_alns[stem])
    paths = [str(tmp_path / "six.fa"), str(tmp_path / "nine.fa")]
    outs = {}
    for name, minimum in (("host", None), ("device", 3)):
        monkeypatch.setattr(bme, "BME_DEVICE_MIN", minimum)
        monkeypatch.setattr(bionj_mod, "BIONJ_DEVICE_MIN", minimum)
        monkeypatch.setattr(F, "FIT_DEVICE_MIN", minimum)
        OracleFitEngine.calls = 0
        out = tmp_path / name
        out.mkdir()
        stats = DirectoryRunner(OracleFitEngine(w, 0), str(out), trees=True, bme=True, bionj=True, fit=True).run(paths)
        assert stats["fit"] == 2 and stats["fit_s"] > 0 and OracleFitEngine.calls == (2 if minimum else 0)
        outs[name] = _files(out)
    assert outs["host"] == outs["device"] and "nine.bionj.bme.patristic.phy" in outs["host"]

    class NanEngine(OracleFitEngine):
        def forward(self, idx):
            return np.full((len(idx), pairs_of(idx.shape[1])), np.nan, dtype=np.float32)

    out = tmp_path / "nan"
    out.mkdir()
    DirectoryRunner(NanEngine(w, 0), str(out), trees=True, bme=True, bionj=True, fit=True, native_io=False).run(paths[:1])
    assert (out / "six.fit.tsv").read_text().splitlines()[1:] == [f"{k}\tnan\tnan\tnan\tnan\t0\t0\tnan" for k in KIND_NAMES]
    assert (out / "six.bionj.patristic.phy").read_text().splitlines()[1].split()[1:] == ["0.0000000000"] + ["nan"] * 5


def test_runner_fits_the_tiled_tree_on_the_gpu_thread(tmp_path, fit_alns, monkeypatch):
    """Under ``--tile`` the NJ tree of a file beyond the context is the mode's, from the device's table (``analyses.
    NJ_DEVICE_MIN``): its fit runs on the GPU thread on that table and gives the files of the host path."""
    from helpers.oracle_fit_engine import OracleFitEngine
    from helpers.oracle_tile_engine import OracleTileEngine
    from phyloformer_amd import analyses
    from phyloformer_amd.scheduler import DirectoryRunner
    from phyloformer_amd.weights import load_weights

    class Both(OracleFitEngine, OracleTileEngine):
        pass

    w = load_weights(os.path.join(REPO, "models", "pf_base.ckpt"))
    _write_fasta(tmp_path / "nine.fa", fit_alns["nine"])
    outs = {}
    for name, minimum in (("host", None), ("device", 3)):
        monkeypatch.setattr(analyses, "NJ_DEVICE_MIN", minimum)
        monkeypatch.setattr(F, "FIT_DEVICE_MIN", minimum)
        Both.calls = 0
        out = tmp_path / name
        out.mkdir()
        stats = DirectoryRunner(Both(w, 0), str(out), trees=True, fit=True, modes=[analyses.Tile(4)]).run([str(tmp_path / "nine.fa")])
        assert stats["fit"] == 1 and stats["tiled"] == 1 and Both.calls == (1 if minimum else 0)
        outs[name] = _files(out)
    assert outs["host"] == outs["device"] and {"nine.fit.tsv", "nine.fit.taxa.tsv", "nine.patristic.phy", "nine.nj.nwk"} <= set(outs["host"])
    pred = Both(w, 0).forward_tiled(fit_alns["nine"], 4)[0].astype(np.float32)
    check_fit_files(outs["device"], "nine", pred, [f"s{k}" for k in range(9)], ["nj"])
