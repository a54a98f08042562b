"""AddressSanitizer + UBSan build of the balanced-NNI kernels' bodies as a stand-alone program
(``tests/native/pf_bme_main.cpp``, its own ``main``; nothing is loaded into Python): ``csrc/pf_bme_host.h``, which the
kernels of ``csrc/pf_bme.hip.h`` share with the CPU, run thread by thread and workgroup by workgroup on exactly-sized heap
arrays.  The refined join table, steps and tree length are compared bit for bit with ``bme.py``.  Then the same through
the loaded library (built without sanitizers): ``pf_bme_nni_host``, ``pf_bme_newick_n``, the refusals, the ABI.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import bme_check as bc
from helpers.nj_table import tie_cases
from phyloformer_amd import bme, nj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bme_native") / "pf_bme_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_bme_main.cpp"),
           "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(program, tmp_path, preds, starts, n, threads, epg, expect=0, resumes=None):
    b, t = preds.shape[0], 2 * (n - 3) + 3
    np.ascontiguousarray(preds, dtype=np.float32).tofile(tmp_path / "preds.bin")
    np.ascontiguousarray(starts, dtype=np.int32).tofile(tmp_path / "start.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([program, str(b), str(n), str(threads), str(epg), str(tmp_path / "preds.bin"), str(tmp_path / "start.bin"),
                          str(tmp_path / "res.bin")], capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert res.returncode == expect, tail
    if expect:
        return None
    assert f"clean, N = {n}, edges = {2 * n - 3}" in res.stdout, tail
    if resumes is not None:
        assert int(res.stdout.rsplit("resumes = ", 1)[1]) >= resumes, tail
    raw = (tmp_path / "res.bin").read_bytes()
    assert len(raw) == b * t * 12 + b * 13
    at = 0
    slots = np.frombuffer(raw, np.int32, b * t, at).reshape(b, t); at += b * t * 4
    lengths = np.frombuffer(raw, np.float64, b * t, at).reshape(b, t); at += b * t * 8
    steps = np.frombuffer(raw, np.int32, b, at); at += b * 4
    length = np.frombuffer(raw, np.float64, b, at); at += b * 8
    status = np.frombuffer(raw, np.uint8, b, at)
    return slots, lengths, steps, length, status


def reference(vec, start, n):
    """``bme.py`` on one source, with the check that its choices are unambiguous: at every performed step the best
    ``delta`` is at least 1e-9 below the second best, and at every table the best ``delta`` is at least 1e-9 away from
    the threshold - so the native code, whose table is updated incrementally between two from-scratch builds and
    differs from ``bme.py``'s in the last bits, must take the same moves."""
    trace = []
    out = bme.bme_nni(bme.matrix_of_preds(vec, n), start, trace=trace)
    for delta, _c, _k, second in trace[:-1]:
        assert second - delta >= 1e-9, (n, delta, second)
    for delta, _c, _k, _second in trace:
        assert abs(delta - bme.THRESHOLD) >= 1e-9, (n, delta)
    return out


def assert_equal(got, b, want):
    slots, lengths, steps, length, status = got
    w_slots, w_lengths, w_steps, w_length, w_status = want
    assert status[b] == w_status and steps[b] == w_steps
    assert np.array_equal(slots[b], w_slots)
    assert np.array_equal(np.ascontiguousarray(lengths[b]).view(np.uint64), w_lengths.view(np.uint64))
    assert np.float64(length[b]).view(np.uint64) == np.float64(w_length).view(np.uint64)


def newick(slots, lengths, n):
    return nj.newick_of_joins([f"t{i}" for i in range(n)], *bme.table_to_joins(slots, lengths))


# (N, threads, edges per workgroup): no internal edge; one; two; the under-8 sums; eight accumulators; beyond one wave of
# edges and a tail; the recursive split of the sums (137 > 128).  threads = 3: more elements than threads everywhere;
# 256 / 32: the kernels' own geometry.
NJ_CASES = [(3, 3, 1), (4, 256, 32), (5, 3, 2), (9, 3, 4), (17, 256, 32), (65, 3, 5), (137, 256, 32)]
# seeds of random_tree_distances at which reference()'s assertions hold (a seed that stops holding fails there)
BAD_CASES = [(4, 256, 32, (2, 5)), (5, 3, 2, (2, 3)), (9, 3, 4, (1, 2)), (17, 256, 32, (1, 2)), (65, 3, 5, (1, 2)), (65, 256, 32, (1, 2))]


@needs_gxx
@pytest.mark.parametrize("n,threads,epg", NJ_CASES)
def test_bodies_from_nj_starts_equal_bme_py_bit_for_bit(program, tmp_path, n, threads, epg):
    preds = bc.uniform_preds(n, n * 100 + threads, 2)
    starts = np.stack([bme.nj_start(bme.matrix_of_preds(p, n)) for p in preds])
    got = run(program, tmp_path, preds, starts, n, threads, epg)
    for b in range(2):
        want = reference(preds[b], starts[b], n)
        assert_equal(got, b, want)
        assert newick(got[0][b], got[1][b], n) == newick(want[0], want[1], n)
    if n >= 65:
        assert got[2].min() >= 1


@needs_gxx
@pytest.mark.parametrize("n,threads,epg,seeds", BAD_CASES)
def test_bodies_from_bad_starts_equal_bme_py_bit_for_bit(program, tmp_path, n, threads, epg, seeds):
    """The caterpillar in index order on the path lengths of a random tree: up to hundreds of swaps, several rounds,
    and from-scratch rebuilds on the way."""
    preds = np.stack([bc.random_tree_distances(n, s) for s in seeds])
    starts = np.stack([bc.caterpillar_slots(n)] * 2)
    got = run(program, tmp_path, preds, starts, n, threads, epg)
    for b in range(2):
        want = reference(preds[b], starts[b], n)
        assert_equal(got, b, want)
        assert newick(got[0][b], got[1][b], n) == newick(want[0], want[1], n)
    assert got[2].min() >= 1
    if n == 65:
        assert got[2].min() > 32                                      # more than one round


@needs_gxx
def test_ties_zero_distances_and_negative_zeros(program, tmp_path):
    """All-equal distances: every delta is 0, nothing moves.  Duplicated sequences: zero distances and deltas of exactly
    0 among them - not taken.  Negative zeros enter as +0."""
    n = 23
    preds = tie_cases(n)
    starts = np.stack([bme.nj_start(bme.matrix_of_preds(p, n)) for p in preds])
    for threads, epg in ((3, 5), (256, 32)):
        got = run(program, tmp_path, preds, starts, n, threads, epg)
        for b in range(3):
            want = bme.bme_nni(bme.matrix_of_preds(preds[b], n), starts[b])
            assert_equal(got, b, want)
        assert got[2][0] == 0 and got[2][2] == 0


@needs_gxx
def test_a_from_scratch_table_resumes_the_search(program, tmp_path):
    """``bme_check.star_tie_preds``: the updated table comes to rest, the from-scratch table of the same tree offers a
    move, the search goes on - twice.  Every delta is rounding noise here, so ``bme.py`` (a from-scratch table at
    every step) may walk elsewhere: the geometries are compared with each other, and the result with the independent
    length."""
    n = 40
    vec = bc.star_tie_preds(n, 2)
    start = bc.caterpillar_slots(n)
    a = run(program, tmp_path, vec[None, :], start[None, :], n, 3, 5, resumes=1)
    b = run(program, tmp_path, vec[None, :], start[None, :], n, 256, 32, resumes=1)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert a[4][0] == bme.OK and a[2][0] >= 2
    pauplin = bc.pauplin_length(bc.adjacency(a[0][0], n), bme.matrix_of_preds(vec, n))
    assert a[3][0] == pytest.approx(pauplin, rel=1e-9)


@needs_gxx
def test_a_matrix_of_the_test_data(program, tmp_path):
    vec = np.load(os.path.join(REPO, "tests", "golden", "e2e_testdata.npz"))["pf/1_40_tips"]
    start = bme.nj_start(bme.matrix_of_preds(vec, 40))
    got = run(program, tmp_path, vec[None, :], start[None, :], 40, 256, 32)
    want = bme.bme_nni(bme.matrix_of_preds(vec, 40), start)
    assert want[2] == 9
    assert_equal(got, 0, want)


@needs_gxx
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_sets_that_sources_status_only(program, tmp_path, bad):
    n = 9
    preds = bc.uniform_preds(n, 9, 3)
    preds[1, 17] = bad
    starts = np.stack([bc.caterpillar_slots(n)] * 3)
    got = run(program, tmp_path, preds, starts, n, 3, 2)
    assert got[4].tolist() == [0, 1, 0]
    assert not got[0][1].any() and not got[1][1].any() and got[2][1] == 0 and got[3][1] == 0.0
    for b in (0, 2):
        assert_equal(got, b, bme.bme_nni(bme.matrix_of_preds(preds[b], n), starts[b]))


@needs_gxx
def test_an_invalid_start_table_is_refused(program, tmp_path):
    n = 6
    preds = bc.uniform_preds(n, 6, 1)
    start = bc.caterpillar_slots(n).copy()
    start[3] = 1                                       # slot 1 was consumed by join 0
    run(program, tmp_path, preds, start[None, :], n, 3, 2, expect=3)


# ---- through the loaded library ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from phyloformer_amd import build
    from phyloformer_amd.engine import load_library
    build.build()
    return load_library()


def test_abi_stays_5_and_the_symbols_are_there(lib):
    assert lib.pf_abi_version() == 5
    for name in ("pf_bme_nni", "pf_bme_nni_device", "pf_bme_nni_host", "pf_bme_newick_n"):
        assert hasattr(lib, name), name


@pytest.mark.parametrize("n", [3, 4, 17, 65])
def test_host_entry_point_equals_bme_py(lib, n):
    from phyloformer_amd import hostio
    preds = np.concatenate([bc.uniform_preds(n, n * 100 + 256 if n >= 17 else n * 100 + 3, 1), bc.random_tree_distances(n, 1 if n > 5 else 2)[None, :]])
    starts = np.stack([bme.nj_start(bme.matrix_of_preds(preds[0], n)), bc.caterpillar_slots(n)])
    got = hostio.bme_nni_host(preds, starts)
    for b in range(2):
        assert_equal(got, b, reference(preds[b], starts[b], n))


@pytest.mark.parametrize("clamp", [True, False])
def test_newick_equals_bme_newick_py(lib, clamp):
    from phyloformer_amd import hostio
    n = 17
    vec = bc.uniform_preds(n, 1956, 1)[0]                            # 6 moves from the NJ tree
    ids = ["a", "b b", "", "a", "tax:on", "é", "x" * 40, "a", "7", "(", "nul\0in", "last", "m", "n", "o", "p", "q"]
    reference(vec, bme.nj_start(bme.matrix_of_preds(vec, n)), n)
    text, steps = hostio.bme_newick(vec, ids, clamp_negative=clamp, with_steps=True)
    assert steps == 6 and text == bme.bme_newick_py(vec, ids, clamp).encode("utf8")
    assert text != hostio.nj_newick(vec, ids, clamp_negative=clamp)
    # fewer than three sequences and non-finite distances: the NJ text
    for m in (1, 2):
        assert hostio.bme_newick(vec[:m * (m - 1) // 2], ids[:m]) == hostio.nj_newick(vec[:m * (m - 1) // 2], ids[:m])
    assert hostio.bme_newick(vec[:3], ids[:3]) == bme.bme_newick_py(vec[:3], ids[:3]).encode("utf8")
    bad = vec.copy()
    bad[7] = np.inf
    assert hostio.bme_newick(bad, ids) == hostio.nj_newick(bad, ids) == bme.bme_newick_py(bad, ids).encode("utf8")
    # the sizing protocol: the length without a buffer, nothing written into one that is too small
    import ctypes as C
    enc = [s.encode("utf8") for s in ids]
    arr = (C.c_char_p * n)(*enc)
    lens = np.array([len(e) for e in enc], dtype=np.int64)
    assert lib.pf_bme_newick_n(vec.ctypes.data, n, arr, lens.ctypes.data, int(clamp), None, 0) == len(text)
    small = C.create_string_buffer(b"\x7f" * 8, 8)
    assert lib.pf_bme_newick_n(vec.ctypes.data, n, arr, lens.ctypes.data, int(clamp), small, 8) == len(text)
    assert small.raw == b"\x7f" * 8


def test_refusals(lib):
    from phyloformer_amd import hostio
    n = 6
    preds = bc.uniform_preds(n, 6, 1)
    good = bc.caterpillar_slots(n)[None, :]
    out_s, out_l = np.zeros(9, np.int32), np.zeros(9, np.float64)
    steps, length, status = np.zeros(1, np.int32), np.zeros(1), np.zeros(1, np.uint8)

    def call(p, st, b, m):
        return lib.pf_bme_nni_host(p, st, b, m, out_s.ctypes.data, out_l.ctypes.data, steps.ctypes.data, length.ctypes.data,
                                   status.ctypes.data)
    assert call(preds.ctypes.data, good.ctypes.data, 1, n) == 0
    assert call(preds.ctypes.data, good.ctypes.data, 1, 2) == -1           # N < 3
    assert call(preds.ctypes.data, good.ctypes.data, 0, n) == -1           # B < 1
    assert call(None, good.ctypes.data, 1, n) == -1 and call(preds.ctypes.data, None, 1, n) == -1
    for k, v in ((0, n), (0, -1), (3, 1), (8, 0)):                          # outside [0, N); consumed slot; repeated slot
        bad = good.copy()
        bad[0, k] = v
        assert call(preds.ctypes.data, bad.ctypes.data, 1, n) == -1, (k, v)
        with pytest.raises(ValueError):
            hostio.bme_nni_host(preds, bad)
