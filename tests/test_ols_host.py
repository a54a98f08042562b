"""Least-squares branch lengths without a GPU: the statement ``ols.tree_ols_py`` on tables worked out by hand, against
``numpy.linalg.lstsq`` of the path matrix, through the normal equations by way of ``tree_fit``, on additive distances; the serial
native twin (``pf_tree_ols_host``, ``hostio.tree_ols_host``) against it bit for bit; the statuses, the refusals, ``ols_scores``'
identities, the sanitizer build of the twin as a stand-alone program (``tests/native/pf_ols_main.cpp``), and ``infer_alns.py
--ols`` through a stand-in engine whose device calls are the twins."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.fit_inputs import same
from helpers.ols_inputs import SIZES, check_ols_files, four_tables, kind_table, path_matrix, table_len, tables, uniform
from phyloformer_amd import bme
from phyloformer_amd import fit as F
from phyloformer_amd import ols as O
from phyloformer_amd import hostio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = [("statement", O.tree_ols_batch_py), ("native", hostio.tree_ols_host)]
# |statement - lstsq| over NJ, BIONJ, caterpillar and balanced tables of 3, 4, 5, 31, 64, 65 and 130 sequences, distances uniform
# in (0.05, 3): the maximum measured is 1.5e-13 (130 sequences, caterpillar; the residuals over a branch sum to 2.7e-15 a pair at the
# most); that is below 1e-11, so the bound is 1e-9 - a hundred times lstsq's own error under another BLAS.  A wrong gamma or a swapped pair of subtrees shows at 1e-2 or more.
LSTSQ_BOUND = 1e-9


# ---- tables worked out by hand --------------------------------------------------------------------------------------------
# Every distance is a dyadic fraction (the five leaves': a multiple of 3, so that the averages over 3 and 6 pairs are too):
# every sum, product and quotient is exact and the expected bits do not depend on an order.

@pytest.mark.parametrize("who,fn", BOTH)
def test_three_sequences_by_hand(who, fn):
    """l_i = (d_ij + d_ik - d_jk) / 2, in the order of the table's last three slots."""
    d01, d02, d12 = 1.5, 2.25, 2.75
    got, status = fn(np.array([d01, d02, d12], dtype=np.float32), np.array([2, 0, 1], dtype=np.int32))
    assert status == 0 and got.tolist() == [0.5 * (d02 + d12 - d01), 0.5 * (d01 + d02 - d12), 0.5 * (d01 + d12 - d02)] == [1.75, 0.5, 1.0]


@pytest.mark.parametrize("who,fn", BOTH)
def test_a_quartet_by_hand(who, fn):
    """((0, 1), (2, 3)): join (0, 1), then slots 0 (the join), 2, 3.  gamma = 1/2 on the inner branch."""
    #                 01   02   03   12   13   23
    pred = np.array([2.0, 5.0, 6.5, 5.5, 7.0, 3.5], dtype=np.float32)
    got, status = fn(pred, np.array([0, 1, 0, 2, 3], dtype=np.int32))
    inner = 0.5 * (0.5 * (5.0 + 7.0) + 0.5 * (5.5 + 6.5) - (2.0 + 3.5))
    assert status == 0 and got.tolist() == [0.5 * (2.0 + (5.0 + 6.5) / 2 - (5.5 + 7.0) / 2), 0.5 * (2.0 + (5.5 + 7.0) / 2 - (5.0 + 6.5) / 2),
                                            inner, 0.5 * ((5.0 + 5.5) / 2 + 3.5 - (6.5 + 7.0) / 2), 0.5 * ((6.5 + 7.0) / 2 + 3.5 - (5.0 + 5.5) / 2)]
    assert got.tolist() == [0.75, 1.25, 3.25, 1.0, 2.5]


#                      01   02    03    04    12    13    14   23    24   34
HAND_PRED = np.array([6.0, 9.0, 15.0, 18.0, 12.0, 18.0, 15.0, 9.0, 12.0, 6.0], dtype=np.float32)


@pytest.mark.parametrize("who,fn", BOTH)
def test_five_leaves_by_hand(who, fn):
    """Join (0, 1) -> node 5; join (node 5, 2) -> node 6; the last three are node 6, 3, 4.  Entry 2 is the branch above node 5 (A = {0},
    B = {1}, C = {2}, D = {3, 4}: gamma = (1 + 2) / (2 x 3)), entry 4 the one above node 6 (A = {0, 1}, B = {2}, C = {3}, D = {4}:
    gamma = (1 + 2) / (3 x 2)); the others end in leaves.  A second table on the same distances has a negative length."""
    got, status = fn(HAND_PRED, np.array([0, 1, 0, 2, 0, 3, 4], dtype=np.int32))
    leaf0 = 0.5 * ((6.0 + (9.0 + 15.0 + 18.0) / 3) - (12.0 + 18.0 + 15.0) / 3)
    above5 = 0.5 * ((0.5 * (9.0 + (18.0 + 15.0) / 2) + 0.5 * (12.0 + (15.0 + 18.0) / 2)) - (6.0 + (9.0 + 12.0) / 2))
    leaf2 = 0.5 * (((9.0 + 12.0) / 2 + (9.0 + 12.0) / 2) - (15.0 + 18.0 + 18.0 + 15.0) / 4)
    above6 = 0.5 * ((0.5 * ((15.0 + 18.0) / 2 + 12.0) + 0.5 * (9.0 + (18.0 + 15.0) / 2)) - ((9.0 + 12.0) / 2 + 6.0))
    leaf3 = 0.5 * (((15.0 + 18.0 + 9.0) / 3 + 6.0) - (18.0 + 15.0 + 12.0) / 3)
    assert status == 0 and got.tolist() == [leaf0, 3.5, above5, leaf2, above6, leaf3, 3.5] == [2.5, 3.5, 5.25, 2.25, 5.25, 2.5, 3.5]
    got, status = fn(HAND_PRED, np.array([3, 1, 4, 3, 0, 2, 4], dtype=np.int32))
    assert status == 0 and got.tolist() == [8.5, 9.5, 7.5, -6.0, 5.5, 3.5, 3.0]
    kids = O.kids_of([3, 1, 4, 3, 0, 2, 4], 5)
    count, lo, order = O.leaf_order(kids, 5)
    assert kids.tolist() == [3, 1, 4, 5, 0, 2, 6] and count.tolist() == [1, 1, 1, 1, 1, 2, 3, 5]
    assert lo.tolist() == [0, 4, 1, 3, 2, 3, 2, 0] and order.tolist() == [0, 2, 4, 3, 1]


# ---- against lstsq, the normal equations, optimality, additive distances -------------------------------------------------

_cases = {}


def case(n):
    """One source of ``n`` sequences, its four tables and the statement's lengths on each, computed once."""
    if n not in _cases:
        pred, slots = four_tables(n, 4200 + n)
        _cases[n] = pred, slots, {name: O.tree_ols_py(pred, s, n) for name, s in slots.items()}
    return _cases[n]


@pytest.mark.parametrize("n", SIZES)
def test_the_statement_against_lstsq_of_the_path_matrix(n):
    pred, slots, made = case(n)
    for name, s in slots.items():
        got, status = made[name]
        want = np.linalg.lstsq(path_matrix(s, n), pred.astype(np.float64), rcond=None)[0]
        worst = float(np.abs(got - want).max())
        print(f"N = {n}, {name}: max |statement - lstsq| = {worst:.3e}")
        assert status == 0 and worst <= LSTSQ_BOUND


@pytest.mark.parametrize("n", SIZES)
def test_the_normal_equations_through_tree_fit(n):
    """An independent route: with T the path lengths ``tree_fit`` gives the OLS table, the residuals d - T of the pairs that a
    branch separates sum to zero, branch by branch - within the bound times the number of those pairs."""
    pred, slots, made = case(n)
    for name, s in slots.items():
        tree, _rows, _worst_j, status = hostio.tree_fit_host(pred, s, made[name][0])
        assert status == 0
        over = path_matrix(s, n)
        sums, counts = over.T @ (pred.astype(np.float64) - tree), over.sum(axis=0)
        print(f"N = {n}, {name}: max |sum of residuals over a branch| / pairs = {float(np.abs(sums / counts).max()):.3e}")
        assert (np.abs(sums) <= LSTSQ_BOUND * counts).all()


@pytest.mark.parametrize("n", [4, 5, 31, 65, 130])
def test_no_table_of_the_engines_fits_better_than_its_ols_lengths(n):
    pred = uniform(n, 300 + n)[0]
    for name in ("nj", "bionj", "bme", "bionj.bme"):
        slots, lengths = kind_table(name, pred)
        best, status = hostio.tree_ols_host(pred, slots)
        _tree, rows, worst_j, st = hostio.tree_fit_host(pred, np.stack([slots, slots]), np.stack([lengths, best]), patristic=False)
        s = O.ols_scores(pred, lengths, best, rows, worst_j, n)
        assert status == 0 and not st.any() and 0 < s.rmse_ols <= s.rmse and s.explained_ols >= s.explained


@pytest.mark.parametrize("who,fn", BOTH)
@pytest.mark.parametrize("n", SIZES)
def test_additive_distances_give_their_lengths_back(who, fn, n):
    """Lengths that are multiples of 2^-10 in [-8 x 2^-10, 1]: a path of at most 130 of them is exact in float32, so the distances
    are the tree's.  A sum of at most 4,225 terms of at most 130 each is off by 4,225 x 130 x 2^-53 at the very most, about 1e-10
    relative to 16 per term - 1e-9 -, and three such sums meet in a length: 1e-8.  The smallest wrong answer is 2^-11."""
    rng = np.random.default_rng(90 + n)
    _pred, slots, _made = case(n)
    for name, s in slots.items():
        lengths = rng.integers(-8, 1025, size=table_len(n)) / 1024.0
        tree = F.patristic_py(s, lengths, n)
        assert (tree.astype(np.float32).astype(np.float64) == tree).all()
        got, status = fn(tree.astype(np.float32), s)
        assert status == 0 and float(np.abs(got - lengths).max()) <= 1e-8, name


# ---- the twin against the statement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_the_twin_equals_the_statement_bit_for_bit(n, b, m):
    preds, slots = tables(n, 8000 + n, b, m)
    got, want = hostio.tree_ols_host(preds, slots), O.tree_ols_batch_py(preds, slots)
    assert got[0].shape == (b, m, table_len(n)) and got[1].shape == (b, m) and not got[1].any()
    assert all(x.tobytes() == y.tobytes() and x.dtype == y.dtype for x, y in zip(got, want))
    # the shapes without B and M
    assert same(hostio.tree_ols_host(preds[0], slots[0]), tuple(x[0] for x in got))
    assert same(hostio.tree_ols_host(preds[0], slots[0, 0]), tuple(x[0, 0] for x in got))
    assert same(hostio.tree_ols_host(preds, slots[:, 0]), tuple(x[:, 0] for x in got))


def test_a_caterpillar_and_a_balanced_table_of_130():
    pred, slots, made = case(130)
    for name in ("caterpillar", "balanced"):
        assert same(hostio.tree_ols_host(pred, slots[name]), made[name])


# ---- statuses ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("who,fn", BOTH)
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_status_1_for_distances_that_are_not_finite(who, fn, bad):
    n = 9
    preds, slots = tables(n, 12, 2, 3)
    clean = fn(preds, slots)
    preds[1, 17] = bad
    got = fn(preds, slots)
    assert got[1].tolist() == [[0, 0, 0], [1, 1, 1]] and not got[0][1].any()
    assert same(tuple(x[0] for x in got), tuple(x[0] for x in clean)) and got[0][0].any()


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
    preds = uniform(n, 3)
    good = bme.caterpillar_slots(n)
    assert F.table_status(good, n) == 0 and F.table_status(_malformed(n, what), n) == 2
    slots = np.stack([good, _malformed(n, what), good])[None]
    got = fn(preds, slots)
    assert got[1].tolist() == [[0, 2, 0]] and not got[0][0, 1].any() and got[0][0, 0].any()
    assert same((got[0][0, 0],), (got[0][0, 2],))
    preds[0, 3] = np.nan                        # no table AND not finite: 2, the table is checked first
    assert fn(preds, slots)[1].tolist() == [[1, 2, 1]]


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_and_their_messages():
    p3, s3 = np.ones(3, dtype=np.float32), np.array([0, 1, 2], dtype=np.int32)
    for fn in (hostio.tree_ols_host, O.tree_ols_batch_py):
        with pytest.raises(ValueError, match=r"tree OLS needs N >= 3 sequences \(got 2\)"):
            fn(np.ones(1, dtype=np.float32), np.zeros(1, dtype=np.int32))
        with pytest.raises(ValueError, match=r"tree OLS needs B >= 1 sources \(got 0\)"):
            fn(np.ones((0, 3), dtype=np.float32), np.zeros((0, 1, 3), dtype=np.int32))
        with pytest.raises(ValueError, match=r"tree OLS needs M >= 1 trees per source \(got 0\)"):
            fn(np.ones((1, 3), dtype=np.float32), np.zeros((1, 0, 3), dtype=np.int32))
        with pytest.raises(ValueError, match="3 distances and 5 slots are not those of one number of sequences"):
            fn(p3, np.zeros(5, dtype=np.int32))
        with pytest.raises(ValueError, match="expected distances"):
            fn(np.ones((2, 3), dtype=np.float32), np.zeros((3, 1, 3), dtype=np.int32))
    with pytest.raises(ValueError, match=r"tree OLS takes at most 8192 sequences \(got 8193\)"):
        O.refuse(1, 1, 8193)
    with pytest.raises(ValueError, match=r"tree OLS needs N >= 3 sequences \(got 2\)"):
        O.tree_ols_py(p3, s3, 2)
    # the library itself: PF_EINVAL (-1) for each of them and for a null buffer, nothing written
    lib = hostio._lib()
    out = (np.full(3, -7.0), np.full(1, 9, dtype=np.uint8))
    ptrs = [a.ctypes.data for a in out]
    ins = [p3.ctypes.data, s3.ctypes.data]
    for b, m, n in ((1, 1, 2), (1, 1, 8193), (1, 1, 65537), (0, 1, 3), (1, 0, 3), (-1, 1, 3)):
        assert lib.pf_tree_ols_host(*ins, b, m, n, *ptrs) == -1
    for hole in range(4):
        args = [*ins, *ptrs]
        args[hole] = None
        assert lib.pf_tree_ols_host(*args[:2], 1, 1, 3, *args[2:]) == -1
    assert all((a == a.flat[0]).all() for a in out)
    assert lib.pf_tree_ols_host(*ins, 1, 1, 3, *ptrs) == 0 and out[1][0] == 0 and out[0].tolist() == [0.5, 0.5, 0.5]


def test_the_bindings_name_the_three_entry_points():
    from phyloformer_amd import build, engine
    from phyloformer_amd.engine import CALL_TIME_SYMBOLS, SIGNATURES, Engine
    from phyloformer_amd.treekinds import NativeHost, PythonHost
    names = {"pf_tree_ols", "pf_tree_ols_device", "pf_tree_ols_host"}
    assert names <= set(SIGNATURES) & CALL_TIME_SYMBOLS
    assert SIGNATURES["pf_tree_ols"][1][1:] == SIGNATURES["pf_tree_ols_device"][1][1:] == SIGNATURES["pf_tree_ols_host"][1]
    assert callable(Engine.tree_ols) and Engine.tree_ols_device.__name__ == "tree_ols_device"
    assert "tree_ols_device" not in engine.PASS_THROUGHS                 # (attached beside the list, whose length is pinned)
    assert {"pf_ols.hip.h", "pf_ols_host.h"} <= set(build.HEADERS) and not {"pf_ols.hip.h", "pf_ols_host.h"} & set(build.KERNEL_FILES)
    with open(os.path.join(REPO, "include", "phyloformer_amd.h")) as fh:
        header = fh.read()
    assert all(f"int {name}(" in header for name in names)
    preds, slots = tables(6, 8, 2, 2)
    assert same(NativeHost().tree_ols(preds, slots), PythonHost().tree_ols(preds, slots))
    e = Engine.__new__(Engine)
    e._lib, e._h = engine.load_library(), None
    with pytest.raises(ValueError):                                        # a NULL handle is refused, nothing dereferenced
        e.tree_ols_device(0, 0, 1, 1, 3, 0, 0)
    with pytest.raises(TypeError):
        e.tree_ols_device(0, 0, 1, 1, 3, 0)


# ---- ols_scores -----------------------------------------------------------------------------------------------------------------

def test_identities_of_the_derived_scores():
    n = 31
    pred = uniform(n, 55)[0]
    slots, lengths = kind_table("nj", pred)
    best, status = hostio.tree_ols_host(pred, slots)
    both = np.stack([lengths, best])
    tree, rows, worst_j, st = hostio.tree_fit_host(pred, np.stack([slots, slots]), both)
    s = O.ols_scores(pred, lengths, best, rows, worst_j, n)
    assert status == 0 and not st.any()
    assert s.length == pytest.approx(lengths.sum(), rel=1e-13) and s.length_ols == pytest.approx(best.sum(), rel=1e-13)
    assert s.length == O.tree_length(lengths) and s.negative == int((lengths < 0).sum()) and s.negative_ols == int((best < 0).sum())
    assert s.most_negative_ols == min(0.0, best.min()) and s.max_change == np.abs(best - lengths).max() > 0
    for k, (rmse, explained) in enumerate(((s.rmse, s.explained), (s.rmse_ols, s.explained_ols))):
        fit = F.fit_scores(pred, rows[k], worst_j[k], n)
        e = pred.astype(np.float64) - tree[k]
        assert (rmse, explained) == (fit.rmse, fit.explained) and rmse == pytest.approx(np.sqrt(np.mean(e * e)), rel=1e-12)
    assert s.rmse_ols <= s.rmse
    # the OLS lengths of the OLS table are the same: the lengths are no input
    assert O.ols_scores(pred, best, best, rows[[1, 1]], worst_j[[1, 1]], n).max_change == 0.0
    # the line of the file and its way back
    line = O.ols_line("nj", s)
    back = O.parse_ols_tsv(O.ols_tsv([("nj", s)]))["nj"]
    assert line.count("\t") == O.OLS_HEAD.count("\t") == 10 and back.negative == s.negative and back.rmse_ols == pytest.approx(s.rmse_ols, rel=1e-9)
    assert O.ols_line("bme", O.no_scores()) == "bme\tnan\tnan\tnan\tnan\tnan\tnan\t0\t0\tnan\tnan\n"


# ---- the twin under AddressSanitizer and UBSan, as a stand-alone program ----------------------------------------------------

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ols_native") / "pf_ols_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_ols_main.cpp"),
           "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


@pytest.mark.parametrize("n,b,m", [(3, 1, 1), (5, 3, 3), (31, 2, 3), (65, 3, 3)])
def test_twin_is_clean_under_asan_and_ubsan_and_equals_the_library(program, tmp_path, n, b, m):
    preds, slots = tables(n, 900 + n, b, m)
    if n >= 5:                                 # tables that are none, and distances that are not finite, among the fine ones
        slots[0, 0] = _malformed(n, "a last slot outside") if n > 5 else np.array([0, 1, 0, 2, 0, 3, 9], dtype=np.int32)
        slots[b - 1, m - 1] = _malformed(n, "a negative slot") if n > 5 else np.array([0, 1, -1, 2, 0, 3, 4], dtype=np.int32)
        preds[1, 2] = np.inf
    for name, a in (("preds", preds), ("slots", slots)):
        a.tofile(tmp_path / f"{name}.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([program, str(b), str(m), str(n), *(str(tmp_path / f"{x}.bin") for x in ("preds", "slots")),
                          str(tmp_path / "res.bin")], capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert res.returncode == 0 and f"clean, B = {b}, M = {m}, N = {n}" in res.stdout, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    raw = (tmp_path / "res.bin").read_bytes()
    items, width = b * m, table_len(n)
    assert len(raw) == items * width * 8 + items
    got = (np.frombuffer(raw, np.float64, items * width).reshape(b, m, width),
           np.frombuffer(raw, np.uint8, items, offset=items * width * 8).reshape(b, m))
    assert same(got, hostio.tree_ols_host(preds, slots))
    assert n < 5 or (got[1][0, 0] == 2 and got[1][b - 1, m - 1] == 2 and (got[1][1] >= 1).all())


# ---- the CLI through a stand-in engine ------------------------------------------------------------------------------------

def _write_fasta(path, idx):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">s{k}\n{''.join(alpha[int(v)] for v in row)}\n")


@pytest.fixture(scope="module")
def ols_alns():
    from phyloformer_amd.msa_sim import simulate_batch
    return {"six": simulate_batch(1, 6, 20, seed=401)[0], "nine": simulate_batch(1, 9, 20, seed=402)[0],
            "two": simulate_batch(1, 2, 20, seed=403)[0]}


@pytest.fixture(scope="module")
def ols_dir(tmp_path_factory, ols_alns):
    d = tmp_path_factory.mktemp("ols_alns")
    for stem, a in ols_alns.items():
        _write_fasta(d / f"{stem}.fa", a)
    return d


def _cli(args, tmp_path):
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_ols_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=900)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


KIND_NAMES = ["nj", "bme", "bionj", "bionj.bme"]


def test_cli_ols_files_and_the_files_of_fit_beside_them(ols_dir, ols_alns, tmp_path):
    from helpers.oracle_ols_engine import make
    from phyloformer_amd import treecmp
    from phyloformer_amd.weights import load_weights
    fit = _cli([str(ols_dir), "-o", str(tmp_path / "fit"), "-t", "--bme", "--bionj", "--fit"], tmp_path)
    r = _cli([str(ols_dir), "-o", str(tmp_path / "o"), "-t", "--bme", "--bionj", "--fit", "--ols", "--bench"], tmp_path)
    assert fit.returncode == 0 and r.returncode == 0, fit.stderr[-2000:] + r.stderr[-3000:]
    files, base = _files(tmp_path / "o"), _files(tmp_path / "fit")
    prefixes = ["" if k == "nj" else k + "." for k in KIND_NAMES]
    added = {f"{stem}.ols.tsv" for stem in ols_alns} | {f"{stem}.{pre}ols.nwk" for stem in ols_alns for pre in prefixes}
    assert set(files) == set(base) | added and not added & set(base) and "six.fit.tsv" in base
    assert all(files[name] == base[name] for name in base)       # the files of --fit and every other output keep their bytes
    eng = make(load_weights(os.path.join(REPO, "models", "pf_base.ckpt")), 0)
    for stem in ("six", "nine"):
        a = ols_alns[stem]
        lines = check_ols_files(files, stem, eng.forward(a).astype(np.float32), [f"s{k}" for k in range(len(a))], KIND_NAMES)
        assert all(0 < s.rmse_ols <= s.rmse for s in lines.values())
        for k, pre in zip(KIND_NAMES, prefixes):
            best, own = (treecmp.parse_newick(files[f"{stem}.{name}"].decode()) for name in (f"{pre}ols.nwk", f"{k}.nwk"))
            assert treecmp.robinson_foulds(best, own)[0] == 0
    # two sequences have no join table: the kind's own text, and nan
    assert files["two.ols.tsv"].decode().splitlines()[1:] == [O.ols_line(k, O.no_scores()).rstrip("\n") for k in KIND_NAMES]
    assert files["two.ols.nwk"] == files["two.nj.nwk"] and files["two.bionj.bme.ols.nwk"] == files["two.bionj.bme.nwk"]
    report = json.loads([line for line in r.stderr.splitlines() if line.startswith("{")][-1])
    assert report["ols"] == 3 and report["ols_s"] > 0 and report["fit"] == 3
    # through the Python I/O and one alignment per launch: the same files
    q = _cli([str(ols_dir), "-o", str(tmp_path / "p"), "-t", "--bme", "--bionj", "--fit", "--ols", "--python-io", "--batch", "1"], tmp_path)
    assert q.returncode == 0, q.stderr[-3000:]
    assert _files(tmp_path / "p") == files


def test_cli_refuses_ols_without_trees_and_with_site_sharding(ols_dir, tmp_path):
    r = _cli([str(ols_dir), "-o", str(tmp_path / "o"), "--ols"], tmp_path)
    assert r.returncode == 2 and "--ols re-estimates the branch lengths of the trees of --trees: give -t as well" in r.stderr
    r = _cli([str(ols_dir), "-o", str(tmp_path / "o"), "-t", "--ols", "--shard", "sites"], tmp_path)
    assert r.returncode == 2
    assert "--ols cannot be combined with --shard sites: the site-sharded runner writes NJ trees only" in r.stderr
    assert not os.path.exists(tmp_path / "o") or not os.listdir(tmp_path / "o")
    from phyloformer_amd.scheduler import DirectoryRunner, SiteShardedRunner
    with pytest.raises(ValueError, match="--ols cannot be combined with --shard sites"):
        SiteShardedRunner(None, None, 0, 1, str(tmp_path), trees=True, ols=True)
    with pytest.raises(ValueError, match="--ols re-estimates the branch lengths of the trees of --trees: give -t as well"):
        DirectoryRunner(None, str(tmp_path), ols=True)


def test_runner_takes_both_routes_with_the_threshold_lowered(tmp_path, ols_alns, monkeypatch):
    """With the thresholds of --bme, --bionj and the OLS lengths at 3 sequences the two kinds' tables are made on the GPU thread and
    ``Engine.tree_ols`` runs there, one call per launch for all of them, followed by one ``Engine.tree_fit``; the NJ tree's stay the
    writer's.  The files are those of the host route; a launch whose distances are not finite gets ``nan`` files."""
    from helpers.oracle_ols_engine import OracleOlsEngine
    from phyloformer_amd import bionj as bionj_mod
    from phyloformer_amd.scheduler import DirectoryRunner
    from phyloformer_amd.weights import load_weights
    assert O.OLS_DEVICE_MIN is None or O.OLS_DEVICE_MIN in (20, 60, 200, 512, 1024, 2048, 4096)
    w = load_weights(os.path.join(REPO, "models", "pf_base.ckpt"))
    for stem in ("six", "nine"):
        _write_fasta(tmp_path / f"{stem}.fa", ols_alns[stem])
    paths = [str(tmp_path / "six.fa"), str(tmp_path / "nine.fa")]
    outs = {}
    for name, minimum in (("host", None), ("device", 3)):
        monkeypatch.setattr(bme, "BME_DEVICE_MIN", minimum)
        monkeypatch.setattr(bionj_mod, "BIONJ_DEVICE_MIN", minimum)
        monkeypatch.setattr(O, "OLS_DEVICE_MIN", minimum)
        monkeypatch.setattr(F, "FIT_DEVICE_MIN", None)
        OracleOlsEngine.ols_calls = OracleOlsEngine.calls = 0
        out = tmp_path / name
        out.mkdir()
        stats = DirectoryRunner(OracleOlsEngine(w, 0), str(out), trees=True, bme=True, bionj=True, ols=True).run(paths)
        assert stats["ols"] == 2 and stats["ols_s"] > 0
        assert OracleOlsEngine.ols_calls == OracleOlsEngine.calls == (2 if minimum else 0)
        outs[name] = _files(out)
    assert outs["host"] == outs["device"] and {"nine.bionj.bme.ols.nwk", "nine.ols.nwk", "six.ols.tsv"} <= set(outs["host"])

    class NanEngine(OracleOlsEngine):
        def forward(self, idx):
            return np.full((len(idx), idx.shape[1] * (idx.shape[1] - 1) // 2), np.nan, dtype=np.float32)

    out = tmp_path / "nan"
    out.mkdir()
    DirectoryRunner(NanEngine(w, 0), str(out), trees=True, bme=True, bionj=True, ols=True, native_io=False).run(paths[:1])
    assert (out / "six.ols.tsv").read_text().splitlines()[1:] == [O.ols_line(k, O.no_scores()).rstrip("\n") for k in KIND_NAMES]
    assert "nan" in (out / "six.ols.nwk").read_text() and (out / "six.bme.ols.nwk").read_text() == (out / "six.bme.nwk").read_text()
