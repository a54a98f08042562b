"""AddressSanitizer + UBSan build of the device neighbour joining's bodies as a stand-alone program
(``tests/native/pf_nj_main.cpp``, its own ``main``; nothing is loaded into Python): ``csrc/pf_nj_host.h``, which the
kernels of ``csrc/pf_nj.hip.h`` share with the CPU, run thread by thread and workgroup by workgroup on exactly-sized heap
arrays.  The join table is compared bit for bit with ``nj.nj_joins`` on the same float32-derived matrix.  The formatter
``pf_nj_format_joins_n`` is compared byte for byte with ``nj.newick_of_joins``.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers.nj_table import assert_table, matrix_of, table_of, tie_cases
from phyloformer_amd import nj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nj_native") / "pf_nj_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_nj_main.cpp"),
           "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(program, tmp_path, preds: np.ndarray, n: int, threads: int, groups: int):
    b = preds.shape[0]
    t = 2 * (n - 3) + 3
    np.ascontiguousarray(preds, dtype=np.float32).tofile(tmp_path / "preds.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([program, str(b), str(n), str(threads), str(groups), str(tmp_path / "preds.bin"), str(tmp_path / "res.bin")],
                         capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert res.returncode == 0 and f"clean, N = {n}, joins = {n - 3}" in res.stdout, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    raw = (tmp_path / "res.bin").read_bytes()
    assert len(raw) == b * t * 12 + b
    slots = np.frombuffer(raw, np.int32, b * t).reshape(b, t)
    lengths = np.frombuffer(raw, np.float64, b * t, offset=b * t * 4).reshape(b, t)
    flag = np.frombuffer(raw, np.uint8, b, offset=b * t * 12)
    return slots, lengths, flag


# (N, threads, groups): no join; the under-8 path; eight accumulators with and without a tail as m shrinks; the
# recursive split (129, 137) on the way down; 200.  threads = 3: more rows and columns than threads; 256: the kernels'
# own workgroup size; groups > 1: more than one workgroup in the minimum of Q.
CASES = [(3, 3, 2), (4, 256, 4), (5, 3, 1), (9, 3, 4), (17, 256, 5), (17, 3, 3), (129, 256, 7), (137, 3, 256), (200, 256, 16)]


@needs_gxx
@pytest.mark.parametrize("n,threads,groups", CASES)
def test_bodies_are_clean_under_asan_and_ubsan_and_equal_nj_joins(program, tmp_path, n, threads, groups):
    preds = np.random.default_rng(n * 100 + threads).uniform(0.01, 3.0, size=(2, n * (n - 1) // 2)).astype(np.float32)
    slots, lengths, flag = run(program, tmp_path, preds, n, threads, groups)
    assert not flag.any()
    for b in range(2):
        assert_table(slots[b], lengths[b], preds[b], n)


@needs_gxx
def test_ties_go_to_the_first_minimum_in_row_major_order(program, tmp_path):
    """All-equal distances: every Q ties at every join.  Duplicated sequences: zero distances, ties among them."""
    n = 23
    preds = tie_cases(n)
    for threads, groups in ((3, 5), (256, 2)):
        slots, lengths, flag = run(program, tmp_path, preds, n, threads, groups)
        assert not flag.any()
        for b in range(3):
            assert_table(slots[b], lengths[b], preds[b], n)


@needs_gxx
def test_a_matrix_of_the_test_data(program, tmp_path):
    vec = np.load(os.path.join(REPO, "tests", "golden", "e2e_testdata.npz"))["pf/3_50_tips"]
    slots, lengths, flag = run(program, tmp_path, vec[None, :], 50, 256, 8)
    assert not flag.any()
    assert_table(slots[0], lengths[0], vec, 50)


@needs_gxx
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_sets_that_sources_flag_only(program, tmp_path, bad):
    n = 9
    preds = np.random.default_rng(9).uniform(0.01, 3.0, size=(3, n * (n - 1) // 2)).astype(np.float32)
    preds[1, 17] = bad
    slots, lengths, flag = run(program, tmp_path, preds, n, 3, 2)
    assert flag.tolist() == [0, 1, 0]
    for b in (0, 2):
        assert_table(slots[b], lengths[b], preds[b], n)


@pytest.mark.parametrize("clamp", [True, False])
def test_formatter_equals_newick_of_joins(clamp):
    from phyloformer_amd import hostio
    n = 12
    vec = np.random.default_rng(12).uniform(0.01, 3.0, size=n * (n - 1) // 2).astype(np.float32)
    vec[5] = 2.9                                     # some negative branch lengths for the clamp
    slots, lengths = table_of(vec, n)
    ids = ["a", "b b", "", "a", "tax:on", "é", "x" * 40, "a", "7", "(", "nul\0in", "last"]
    got = hostio.newick_of_joins(slots, lengths, ids, clamp_negative=clamp)
    joins, final = nj.nj_joins(matrix_of(vec, n))
    assert got == nj.newick_of_joins(ids, joins, final, clamp).encode("utf8")
    assert got == hostio.newick_of_joins_py(slots, lengths, ids, clamp_negative=clamp).encode("utf8")
    if clamp:
        assert got == hostio.nj_newick(vec, ids)
    # three sequences: no join, the trifurcation alone
    s3, l3 = table_of(vec[:3], 3)
    assert hostio.newick_of_joins(s3, l3, ids[:3]) == hostio.nj_newick(vec[:3], ids[:3])


def test_formatter_refuses_a_bad_table():
    from phyloformer_amd import hostio
    slots, lengths = table_of(np.linspace(0.1, 1.0, 10, dtype=np.float32), 5)
    with pytest.raises(ValueError):
        hostio.newick_of_joins(slots[:-1], lengths[:-1], list("abcde"))
    bad = slots.copy()
    bad[2] = 5
    with pytest.raises(ValueError):
        hostio.newick_of_joins(bad, lengths, list("abcde"))
