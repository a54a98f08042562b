"""AddressSanitizer + UBSan build of the balanced-SPR kernels' bodies as a stand-alone program
(``tests/native/pf_spr_main.cpp``, its own ``main``; nothing is loaded into Python): the SPR part of
``csrc/pf_bme_host.h``, which the kernels of ``csrc/pf_bme.hip.h`` share with the CPU, run thread by thread and workgroup
by workgroup on exactly-sized heap arrays.  Every step forms its table from scratch, so everything is compared with
``bme.bme_spr`` for equality - there is no near-tie caveat: slots, steps, status, and lengths and tree length as uint64;
the depth table the bodies build equals ``Tree.depths()`` (and the host's ``build_depth`` at every step, which the
program checks itself), the pair table equals ``bme.PairTable`` bit for bit from the tiled bodies and from the
one-thread-per-entry body.  Then the same through the loaded library (built without sanitizers): ``pf_bme_spr_host``,
``pf_bme_spr_newick_n``, the refusals, the ABI.  No GPU."""
import functools
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
    exe = str(tmp_path_factory.mktemp("spr_native") / "pf_spr_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_spr_main.cpp"),
           "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(program, tmp_path, preds, starts, n, threads, epg, tiled, cap=-1, expect=0):
    """The program's results, and the first depth and pair table of source 0."""
    b, t = preds.shape[0], 2 * (n - 3) + 3
    np.ascontiguousarray(preds, dtype=np.float32).tofile(tmp_path / "preds.bin")
    np.ascontiguousarray(starts, dtype=np.int32).tofile(tmp_path / "start.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    files = [str(tmp_path / f) for f in ("preds.bin", "start.bin", "res.bin", "depth.bin", "pairs.bin")]
    for f in files[2:]:
        if os.path.exists(f):
            os.unlink(f)
    res = subprocess.run([program, str(b), str(n), str(threads), str(epg), str(cap), str(int(tiled)), *files],
                         capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert res.returncode == expect, tail
    if expect:
        return None
    assert f"clean, N = {n}, rows = {4 * n - 6}" in res.stdout, tail
    raw = (tmp_path / "res.bin").read_bytes()
    assert len(raw) == b * t * 12 + b * 13
    at = 0
    slots = np.frombuffer(raw, np.int32, b * t, at).reshape(b, t); at += b * t * 4
    lengths = np.frombuffer(raw, np.float64, b * t, at).reshape(b, t); at += b * t * 8
    steps = np.frombuffer(raw, np.int32, b, at); at += b * 4
    length = np.frombuffer(raw, np.float64, b, at); at += b * 8
    status = np.frombuffer(raw, np.uint8, b, at)
    tables = None
    if os.path.exists(files[3]):
        tables = (np.fromfile(files[3], np.int16).reshape(4 * n - 6, 2 * n - 2), np.fromfile(files[4], np.float64).reshape(4 * n - 6, 4 * n - 6))
    return (slots, lengths, steps, length, status), tables


@functools.lru_cache(maxsize=None)
def _reference(vec_bytes, start_bytes, n):
    vec, start = np.frombuffer(vec_bytes, np.float32), np.frombuffer(start_bytes, np.int32)
    return bme.bme_spr(bme.matrix_of_preds(vec, n), start)


def reference(vec, start, n):
    """``bme.bme_spr`` of one source, computed once per input."""
    return _reference(np.ascontiguousarray(vec, np.float32).tobytes(), np.ascontiguousarray(start, np.int32).tobytes(), n)


def assert_equal(got, b, want):
    slots, lengths, steps, length, status = got
    w_slots, w_lengths, w_steps, w_length, w_status = want
    assert status[b] == w_status and steps[b] == w_steps
    assert np.array_equal(slots[b], w_slots)
    assert np.array_equal(np.ascontiguousarray(lengths[b]).view(np.uint64), w_lengths.view(np.uint64))
    assert np.float64(length[b]).view(np.uint64) == np.float64(w_length).view(np.uint64)


def assert_tables(tables, vec, start, n):
    tree = bme.Tree(start, n)
    want = bme.PairTable(bme.matrix_of_preds(vec, n), tree)
    assert np.array_equal(tables[0], tree.depths())
    assert np.array_equal(tables[1].view(np.uint64), want.t.view(np.uint64))
    return tables[1]


def nj_inputs(n, seed):
    """Two sources of ``n`` sequences and their NJ tables.  137: noisy path lengths of random trees, a few moves from
    their NJ trees, so that ``bme.py`` stays quick where the sums split (137 > 128)."""
    if n < 137:
        preds = bc.uniform_preds(n, seed, 2)
    else:
        preds = np.stack([(bc.random_tree_distances(n, s) * np.random.default_rng(s).uniform(0.85, 1.15, n * (n - 1) // 2)).astype(np.float32)
                          for s in (seed, seed + 1)])
    return preds, np.stack([bme.nj_start(bme.matrix_of_preds(p, n)) for p in preds])


# (N, threads, target edges per workgroup): threads = 3: more elements than threads everywhere; 256 / 256: the kernels' own
# geometry.  3: no candidate; 4: the first ones; 5, 6: the under-8 sums; 9, 17: eight accumulators; 65: several tiles and
# a ragged one; 137: the recursive split of the sums and more than one workgroup of target edges at epg = 64.
NJ_CASES = [(3, 3, 1), (4, 256, 256), (5, 3, 2), (6, 256, 256), (9, 3, 4), (17, 256, 256), (65, 3, 5), (137, 256, 64)]
BAD_CASES = [(4, 256, 256), (5, 3, 2), (6, 3, 1), (9, 3, 4), (17, 256, 256), (65, 256, 256)]


@needs_gxx
@pytest.mark.parametrize("n,threads,epg", NJ_CASES)
def test_bodies_from_nj_starts_equal_bme_py_bit_for_bit(program, tmp_path, n, threads, epg):
    preds, starts = nj_inputs(n, n * 100 + threads)
    got, tables = run(program, tmp_path, preds, starts, n, threads, epg, tiled=True)
    for b in range(2):
        assert_equal(got, b, reference(preds[b], starts[b], n))
    tiled = assert_tables(tables, preds[0], starts[0], n)
    if n in (9, 65, 137):                                            # the other body of the pair table: the same bits
        again, tables = run(program, tmp_path, preds, starts, n, threads, epg, tiled=False)
        assert np.array_equal(assert_tables(tables, preds[0], starts[0], n).view(np.uint64), tiled.view(np.uint64))
        for x, y in zip(got, again):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    if n >= 65:
        assert got[2].min() >= 1
    print(n, "steps", got[2])


@needs_gxx
@pytest.mark.parametrize("n,threads,epg", BAD_CASES)
def test_bodies_from_caterpillar_starts_equal_bme_py_bit_for_bit(program, tmp_path, n, threads, epg):
    """The caterpillar in index order on the path lengths of a random tree: long paths, many moves, at 65 more than one
    round of 32 steps."""
    preds = np.stack([bc.random_tree_distances(n, s) for s in (1, 2)])
    starts = np.stack([bc.caterpillar_slots(n)] * 2)
    got, tables = run(program, tmp_path, preds, starts, n, threads, epg, tiled=n != 9)
    for b in range(2):
        assert_equal(got, b, reference(preds[b], starts[b], n))
    assert_tables(tables, preds[0], starts[0], n)
    if n >= 9:
        assert got[2].min() >= 1
    if n == 65:
        assert got[2].max() > 32                                      # more than one round
    print(n, "steps", got[2])


@needs_gxx
def test_ties_zero_distances_and_negative_zeros(program, tmp_path):
    """All-equal distances: every candidate is 0, nothing moves - and from the caterpillar, where roundings make some of
    them negative, the order of the key decides among equals.  Duplicated sequences: zero distances.  Negative zeros
    enter as +0."""
    n = 23
    preds = tie_cases(n)
    for starts in (np.stack([bme.nj_start(bme.matrix_of_preds(p, n)) for p in preds]), np.stack([bc.caterpillar_slots(n)] * len(preds))):
        for threads, epg in ((3, 5), (256, 256)):
            got, _tables = run(program, tmp_path, preds, starts, n, threads, epg, tiled=True)
            for b in range(len(preds)):
                assert_equal(got, b, reference(preds[b], starts[b], n))


@needs_gxx
def test_the_matrix_with_a_candidate_of_exactly_zero(program, tmp_path):
    """``1_40_tips``: six moves, and the final table holds a candidate whose change is exactly 0.0."""
    vec = np.load(os.path.join(REPO, "tests", "golden", "e2e_testdata.npz"))["pf/1_40_tips"]
    dm = bme.matrix_of_preds(vec, 40)
    start = bme.nj_start(dm)
    trace = []
    want = bme.bme_spr(dm, start, trace=trace)
    assert want[2] == 6 and len(trace) == 7
    final = bme.Tree(want[0], 40)
    assert any(c[0] == 0.0 for c in bme.spr_candidates(bme.PairTable(dm, final).t.tolist(), final))
    got, _tables = run(program, tmp_path, vec[None, :], start[None, :], 40, 256, 256, tiled=True)
    assert_equal(got, 0, want)


@needs_gxx
def test_a_lowered_cap(program, tmp_path):
    n = 17
    preds = bc.uniform_preds(n, 1956, 1)
    start = bc.caterpillar_slots(n)[None, :]
    free, _t = run(program, tmp_path, preds, start, n, 3, 4, tiled=True)
    assert free[2][0] >= 3 and free[4][0] == bme.OK
    got, _t = run(program, tmp_path, preds, start, n, 3, 4, tiled=True, cap=2)
    assert got[2][0] == 2 and got[4][0] == bme.CAPPED


@needs_gxx
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_sets_that_sources_status_only(program, tmp_path, bad):
    n = 9
    preds = bc.uniform_preds(n, 9, 3)
    preds[1, 17] = bad
    starts = np.stack([bc.caterpillar_slots(n)] * 3)
    got, _tables = run(program, tmp_path, preds, starts, n, 3, 2, tiled=True)
    assert got[4].tolist() == [0, 1, 0]
    assert not got[0][1].any() and not got[1][1].any() and got[2][1] == 0 and got[3][1] == 0.0
    for b in (0, 2):
        assert_equal(got, b, reference(preds[b], starts[b], n))


@needs_gxx
def test_an_invalid_start_table_is_refused(program, tmp_path):
    n = 6
    preds = bc.uniform_preds(n, 6, 1)
    start = bc.caterpillar_slots(n).copy()
    start[3] = 1                                       # slot 1 was consumed by join 0
    run(program, tmp_path, preds, start[None, :], n, 3, 2, tiled=True, expect=3)


# ---- through the loaded library ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from phyloformer_amd import build
    from phyloformer_amd.engine import load_library
    build.build()
    return load_library()


def test_abi_stays_5_and_the_symbols_are_there(lib):
    from phyloformer_amd import engine
    assert lib.pf_abi_version() == 5
    for name in ("pf_bme_spr", "pf_bme_spr_device", "pf_bme_spr_host", "pf_bme_spr_newick_n"):
        assert hasattr(lib, name) and name in engine.SIGNATURES and name in engine.CALL_TIME_SYMBOLS, name
    for name in ("pf_bme_nni", "pf_bme_nni_device", "pf_bme_nni_host", "pf_bme_newick_n"):
        assert hasattr(lib, name), name


@pytest.mark.parametrize("n", [3, 4, 17, 65])
def test_host_entry_point_equals_bme_py(lib, n):
    from phyloformer_amd import hostio
    preds = np.concatenate([nj_inputs(n, n * 100 + (256 if n in (4, 17) else 3))[0][:1], bc.random_tree_distances(n, 1)[None, :]])
    starts = np.stack([bme.nj_start(bme.matrix_of_preds(preds[0], n)), bc.caterpillar_slots(n)])
    got = hostio.bme_spr_host(preds, starts)
    for b in range(2):
        assert_equal(got, b, reference(preds[b], starts[b], n))


@pytest.mark.parametrize("clamp", [True, False])
def test_newick_equals_spr_newick_py(lib, clamp):
    from phyloformer_amd import hostio
    n = 17
    vec = bc.uniform_preds(n, 1956, 1)[0]
    ids = ["a", "b b", "", "a", "tax:on", "é", "x" * 40, "a", "7", "(", "nul\0in", "last", "m", "n", "o", "p", "q"]
    text, steps = hostio.spr_newick(vec, ids, clamp_negative=clamp, with_steps=True)
    assert steps == bme.spr_tree_py(vec, ids, clamp)[1] >= 1 and text == bme.spr_newick_py(vec, ids, clamp).encode("utf8")
    assert text != hostio.nj_newick(vec, ids, clamp_negative=clamp)
    # fewer than three sequences and non-finite distances: the NJ text
    for m in (1, 2):
        assert hostio.spr_newick(vec[:m * (m - 1) // 2], ids[:m]) == hostio.nj_newick(vec[:m * (m - 1) // 2], ids[:m])
    assert hostio.spr_newick(vec[:3], ids[:3]) == bme.spr_newick_py(vec[:3], ids[:3]).encode("utf8")
    bad = vec.copy()
    bad[7] = np.inf
    assert hostio.spr_newick(bad, ids) == hostio.nj_newick(bad, ids) == bme.spr_newick_py(bad, ids).encode("utf8")
    # the sizing protocol: the length without a buffer, nothing written into one that is too small
    import ctypes as C
    enc = [s.encode("utf8") for s in ids]
    arr = (C.c_char_p * n)(*enc)
    lens = np.array([len(e) for e in enc], dtype=np.int64)
    assert lib.pf_bme_spr_newick_n(vec.ctypes.data, n, arr, lens.ctypes.data, int(clamp), None, 0) == len(text)
    small = C.create_string_buffer(b"\x7f" * 8, 8)
    assert lib.pf_bme_spr_newick_n(vec.ctypes.data, n, arr, lens.ctypes.data, int(clamp), small, 8) == len(text)
    assert small.raw == b"\x7f" * 8


def test_refusals(lib):
    from phyloformer_amd import hostio
    n = 6
    preds = bc.uniform_preds(n, 6, 1)
    good = bc.caterpillar_slots(n)[None, :]
    out_s, out_l = np.zeros(9, np.int32), np.zeros(9, np.float64)
    steps, length, status = np.zeros(1, np.int32), np.zeros(1), np.zeros(1, np.uint8)

    def call(p, st, b, m):
        return lib.pf_bme_spr_host(p, st, b, m, out_s.ctypes.data, out_l.ctypes.data, steps.ctypes.data, length.ctypes.data,
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
            hostio.bme_spr_host(preds, bad)
