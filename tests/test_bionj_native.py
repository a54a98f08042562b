"""AddressSanitizer + UBSan build of the device BIONJ's bodies as a stand-alone program
(``tests/native/pf_bionj_main.cpp``, its own ``main``; nothing is loaded into Python): ``csrc/pf_bionj_host.h``, which the
kernels of ``csrc/pf_bionj.hip.h`` share with the CPU, run thread by thread and workgroup by workgroup on exactly-sized
heap arrays.  The join table is compared bit for bit with ``bionj.bionj_joins`` on the same float32-derived matrix.
Then, through the loaded library (built without sanitizers): ``pf_bionj_joins_host``, ``pf_bionj_newick_n``, the
refusals, the ABI.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers.bionj_table import assert_table, duplicated_rows, table_of, uniform
from helpers.nj_table import tie_cases
from phyloformer_amd import bionj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bionj_native") / "pf_bionj_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_bionj_main.cpp"),
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


# (N, threads, groups): no join; the under-8 path of both sums; eight accumulators with and without a tail as m
# shrinks; the recursive split (129, 137) on the way down; 200.  threads = 3: more rows and columns than threads; 256:
# the kernels' own workgroup size; groups from 1 to 256: the workgroups of both minima.
CASES = [(3, 3, 2), (4, 256, 4), (5, 3, 1), (9, 3, 4), (17, 256, 5), (17, 3, 3), (129, 256, 7), (137, 3, 256), (200, 256, 16)]


@needs_gxx
@pytest.mark.parametrize("n,threads,groups", CASES)
def test_bodies_are_clean_under_asan_and_ubsan_and_equal_bionj_joins(program, tmp_path, n, threads, groups):
    preds = uniform(n, n * 100 + threads, 2)
    slots, lengths, flag = run(program, tmp_path, preds, n, threads, groups)
    assert not flag.any()
    for b in range(2):
        assert_table(slots[b], lengths[b], preds[b], n)


@needs_gxx
def test_all_equal_distances_duplicated_sequences_and_negative_zeros(program, tmp_path):
    """All-equal distances: every q ties at every join, the whole triangle is inside the window.  Duplicated sequences:
    zero distances, v_ab = 0, q equal up to rounding.  Negative zeros enter as +0."""
    n = 23
    preds = np.concatenate([tie_cases(n), duplicated_rows(n, 7)[None, :]])
    assert any(v == 0.0 and w > 1 for _lam, v, w in _trace(preds[3], n))
    for threads, groups in ((3, 5), (256, 2), (256, 256)):
        slots, lengths, flag = run(program, tmp_path, preds, n, threads, groups)
        assert not flag.any()
        for b in range(4):
            assert_table(slots[b], lengths[b], preds[b], n)


def _trace(vec, n):
    from helpers.nj_table import matrix_of
    trace = []
    bionj.bionj_joins(matrix_of(vec, n), trace)
    return trace


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
    preds = uniform(n, 9, 3)
    preds[1, 17] = bad
    slots, lengths, flag = run(program, tmp_path, preds, n, 3, 2)
    assert flag.tolist() == [0, 1, 0]
    for b in (0, 2):
        assert_table(slots[b], lengths[b], preds[b], n)


# ---- through the loaded library ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from phyloformer_amd import build
    from phyloformer_amd.engine import load_library
    build.build()
    return load_library()


def test_abi_stays_5_and_the_symbols_are_there(lib):
    assert lib.pf_abi_version() == 5
    for name in ("pf_bionj_joins", "pf_bionj_joins_device", "pf_bionj_joins_host", "pf_bionj_newick_n"):
        assert hasattr(lib, name), name


@pytest.mark.parametrize("n", [3, 4, 17, 65, 137])
def test_host_entry_point_equals_bionj_py(lib, n):
    from phyloformer_amd import hostio
    preds = np.concatenate([uniform(n, n, 2), duplicated_rows(max(n, 8), n)[None, :n * (n - 1) // 2]])
    preds[1, 0] = np.inf
    slots, lengths, flag = hostio.bionj_joins_host(preds)
    assert flag.tolist() == [False, True, False]
    assert not slots[1].any() and not lengths[1].any()
    for b in (0, 2):
        assert_table(slots[b], lengths[b], preds[b], n)


@pytest.mark.parametrize("clamp", [True, False])
def test_newick_equals_bionj_newick_py(lib, clamp):
    from phyloformer_amd import hostio
    n = 12
    vec = uniform(n, 12)[0]
    vec[5] = 2.9                                     # some negative branch lengths for the clamp
    ids = ["a", "b b", "", "a", "tax:on", "é", "x" * 40, "a", "7", "(", "nul\0in", "last"]
    text = hostio.bionj_newick(vec, ids, clamp_negative=clamp)
    assert text == bionj.bionj_newick_py(vec, ids, clamp).encode("utf8")
    assert text == hostio.newick_of_joins(*table_of(vec, n), ids, clamp_negative=clamp)
    assert text != hostio.nj_newick(vec, ids, clamp_negative=clamp)
    for search, py in (("bme", bionj.bionj_bme_newick_py), ("spr", bionj.bionj_spr_newick_py)):
        assert hostio.bionj_refined_newick(search, vec, ids, clamp) == py(vec, ids, clamp).encode("utf8")
    # fewer than three sequences and non-finite distances: the NJ text
    for m in (1, 2):
        assert hostio.bionj_newick(vec[:m * (m - 1) // 2], ids[:m]) == hostio.nj_newick(vec[:m * (m - 1) // 2], ids[:m])
    assert hostio.bionj_newick(vec[:3], ids[:3]) == bionj.bionj_newick_py(vec[:3], ids[:3]).encode("utf8")
    bad = vec.copy()
    bad[7] = np.inf
    assert hostio.bionj_newick(bad, ids) == hostio.nj_newick(bad, ids) == bionj.bionj_newick_py(bad, ids).encode("utf8")
    assert hostio.bionj_refined_newick("bme", bad, ids) == hostio.nj_newick(bad, ids) == bionj.bionj_bme_newick_py(bad, ids).encode("utf8")
    # the sizing protocol: the length without a buffer, nothing written into one that is too small
    import ctypes as C
    enc = [s.encode("utf8") for s in ids]
    arr = (C.c_char_p * n)(*enc)
    lens = np.array([len(e) for e in enc], dtype=np.int64)
    assert lib.pf_bionj_newick_n(vec.ctypes.data, n, arr, lens.ctypes.data, int(clamp), None, 0) == len(text)
    small = C.create_string_buffer(b"\x7f" * 8, 8)
    assert lib.pf_bionj_newick_n(vec.ctypes.data, n, arr, lens.ctypes.data, int(clamp), small, 8) == len(text)
    assert small.raw == b"\x7f" * 8


def test_refusals(lib):
    from phyloformer_amd import hostio
    n = 6
    preds = uniform(n, 6)
    out_s, out_l, flag = np.zeros(9, np.int32), np.zeros(9, np.float64), np.zeros(1, np.uint8)

    def call(p, b, m, s=out_s.ctypes.data, l=out_l.ctypes.data, f=flag.ctypes.data):
        return lib.pf_bionj_joins_host(p, b, m, s, l, f)
    assert call(preds.ctypes.data, 1, n) == 0
    assert call(preds.ctypes.data, 1, 2) == -1           # N < 3
    assert call(preds.ctypes.data, 0, n) == -1           # B < 1
    assert call(None, 1, n) == -1
    assert call(preds.ctypes.data, 1, n, s=None) == -1 and call(preds.ctypes.data, 1, n, l=None) == -1
    assert call(preds.ctypes.data, 1, n, f=None) == -1
    with pytest.raises(ValueError):
        hostio.bionj_joins_host(preds[:, :-1])
    with pytest.raises(ValueError):
        hostio.bionj_joins_host(preds[:, :1])
