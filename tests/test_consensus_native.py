"""The bodies of the consensus kernels (``csrc/pf_consensus_host.h``) as a stand-alone program
(``tests/native/pf_consensus_main.cpp``, its own ``main``; nothing is loaded into Python) under
``g++ -fsanitize=address,undefined``: the kernels' geometry - workgroups of 1, 3 and 256 threads, the counting in a
scrambled order - with every array at its exact size, against ``consensus.join_consensus``; hash tables of capacities the
library never uses (barely enough slots: probe chains that wrap around the end; too few: the error status, no loop and no
access out of bounds); and tables that are none, which must be flagged without one access out of bounds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import support_inputs as si
from phyloformer_amd import consensus, supports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("consensus_native") / "pf_consensus_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_consensus_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(program, tmp_path, reps, lengths, flag, n, threads, percent=50, cap=0):
    r, s = len(reps), n - 3
    np.ascontiguousarray(reps, dtype=np.int32).tofile(tmp_path / "tables.bin")
    np.ascontiguousarray(lengths, dtype=np.float64).tofile(tmp_path / "lengths.bin")
    np.ascontiguousarray(flag, dtype=np.uint8).tofile(tmp_path / "flags.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([program, str(n), str(r), str(threads), str(percent), str(cap),
                          *(str(tmp_path / f) for f in ("tables.bin", "lengths.bin", "flags.bin", "out.bin"))],
                         capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert res.returncode == 0 and "clean" in res.stdout, tail
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == 4 + 12 * s + 4 * n + 8 * s + 8 * n + 1
    ints = np.frombuffer(raw, np.int32, 1 + 3 * s + n, 0)
    at = 4 * (1 + 3 * s + n)
    return consensus.Consensus(int(ints[0]), ints[1:1 + s].tolist(), ints[1 + s:1 + 2 * s].tolist(), ints[1 + 2 * s:1 + 3 * s].tolist(),
                               raw[at:at + 8 * s], ints[1 + 3 * s:].tolist(), raw[at + 8 * s:at + 8 * (s + n)], raw[-1])


def same(got, want):
    """The program's results against the statement's: integers equal, doubles bit for bit."""
    return (got[:4] == want[:4] and got[5] == want[5] and got[7] == want[7] and
            got[4] == np.asarray(want[4], dtype=np.float64).tobytes() and got[6] == np.asarray(want[6], dtype=np.float64).tobytes())


def distinct_splits(reps, flag, n):
    return len({s for tab, f in zip(reps, flag) if not f for s in supports.table_splits(tab, n)})


@pytest.mark.parametrize("n", [4, 5, 9, 64, 65, 137])
def test_kernel_geometry_equals_the_statement(program, tmp_path, n):
    _ref, reps, flag = si.sources(n, 5)
    lengths = np.random.default_rng(n).standard_normal(reps.shape)
    for b in range(2):
        for percent in (50, 70):
            want = consensus.join_consensus(reps[b], n, lengths[b], flag[b], percent)
            for threads in (1, 3, 256):
                assert same(run(program, tmp_path, reps[b], lengths[b], flag[b], n, threads, percent), want), (n, b, percent, threads)


@pytest.mark.parametrize("n", [9, 65, 137])
def test_capacities_the_library_never_uses(program, tmp_path, n):
    """The least power of two that holds the distinct splits: a table (nearly) full, whose probe chains wrap around its
    end - the statement's results.  Half of it: some split finds no slot - status 2 and zeros, after at most ``cap``
    probes each."""
    _ref, reps, flag = si.sources(n, 6)
    lengths = np.random.default_rng(n).standard_normal(reps.shape)
    for b in range(2):
        d = distinct_splits(reps[b], flag[b], n)
        cap = 1 << (d - 1).bit_length()
        assert cap // 2 < d <= cap < 2 * (n - 3) * 6
        want = consensus.join_consensus(reps[b], n, lengths[b], flag[b])
        assert same(run(program, tmp_path, reps[b], lengths[b], flag[b], n, 256, cap=cap), want), (n, b, d, cap)
        got = run(program, tmp_path, reps[b], lengths[b], flag[b], n, 256, cap=cap // 2)
        assert got.status == 2 and got.n_splits == 0, (n, b, d, cap)
        assert not any(got.count) and not any(got.size) and not any(got.parent) and not any(got.leaf_parent)
        assert not any(got.split_length) and not any(got.leaf_length)


def test_tables_that_are_none_are_flagged_without_an_access_out_of_bounds(program, tmp_path):
    n = 65
    _ref, reps, flag = si.sources(n, 5)
    lengths = np.random.default_rng(1).standard_normal(reps.shape)
    t = 2 * (n - 3) + 3
    for k, v in ((7, n), (0, -1), (30, 1 << 30), (t - 1, n), (11, -(1 << 31))):
        q = reps[0].copy()
        q[3, k] = v
        got = run(program, tmp_path, q, lengths[0], flag[0], n, 256)
        assert got.status == 1 and got.n_splits == 0 and not any(got.count) and not any(got.leaf_parent), (k, v)
        assert not any(got.split_length) and not any(got.leaf_length), (k, v)
    dead = reps[0].copy()
    dead[0, 2 * 10] = dead[0, 1]                                # join 10 names the slot that join 0 joined away
    assert run(program, tmp_path, dead, lengths[0], flag[0], n, 256).status == 1
