"""The bodies of the tree-distance kernels (``csrc/pf_treedist_host.h``) as a stand-alone program
(``tests/native/pf_treedist_main.cpp``, its own ``main``; nothing is loaded into Python) under
``g++ -fsanitize=address,undefined``: the kernels' geometry - workgroups of 1, 3 and 256 threads, the hashing and the pairs
in a scrambled order - with every array at its exact size, against ``treedist.join_distances_py``; hash tables of capacities
the library never uses (barely enough slots: probe chains that wrap around the end; too few: status 2, no loop and no access
out of bounds); and tables that are none, which must be flagged without one access out of bounds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import treedist_inputs as ti
from phyloformer_amd import supports, treedist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("treedist_native") / "pf_treedist_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_treedist_main.cpp"),
           "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(program, tmp_path, slots, lengths, flag, n, threads, cap=0):
    k = len(slots)
    np.ascontiguousarray(slots, dtype=np.int32).tofile(tmp_path / "tables.bin")
    np.ascontiguousarray(lengths, dtype=np.float64).tofile(tmp_path / "lengths.bin")
    np.ascontiguousarray(flag, dtype=np.uint8).tofile(tmp_path / "flags.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([program, str(n), str(k), str(threads), str(cap),
                          *(str(tmp_path / f) for f in ("tables.bin", "lengths.bin", "flags.bin", "out.bin"))],
                         capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert res.returncode == 0 and "clean" in res.stdout, tail
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == 20 * k * k + 1
    return (np.frombuffer(raw, np.int32, k * k, 0).reshape(k, k), np.frombuffer(raw, np.float64, k * k, 4 * k * k).reshape(k, k),
            np.frombuffer(raw, np.float64, k * k, 12 * k * k).reshape(k, k), np.uint8(raw[-1]))


def statement(slots, lengths, flag, n):
    w = treedist.join_distances_py(slots, lengths, flag, n)
    return w.shared, w.kf, w.wrf, np.uint8(w.status)


def inputs(n, k):
    slots, lengths = ti.mixed(n, k)
    slots = slots.copy()
    flag = np.zeros(k, dtype=bool)
    if k > 3:
        flag[2] = True
        slots[2] = np.iinfo(np.int32).min                       # (never read)
    return slots, lengths, flag


@pytest.mark.parametrize("n", [4, 5, 9, 64, 65, 67, 130])
def test_kernel_geometry_equals_the_statement(program, tmp_path, n):
    for k in (1, 2, 7):
        slots, lengths, flag = inputs(n, k)
        want = statement(slots, lengths, flag, n)
        for threads in (1, 3, 256):
            assert ti.same(run(program, tmp_path, slots, lengths, flag, n, threads), want), (n, k, threads)


@pytest.mark.parametrize("n", [9, 65, 130])
def test_capacities_the_library_never_uses(program, tmp_path, n):
    """The least power of two that holds the distinct splits: a table (nearly) full, whose probe chains wrap around its
    end - the statement's results.  Half of it: some split finds no slot - status 2 and zeros, after at most ``cap`` probes
    each."""
    slots, lengths, flag = inputs(n, 7)
    d = len({s for tab, f in zip(slots, flag) if not f for s in supports.table_splits(tab, n)})
    cap = 1 << (d - 1).bit_length()
    assert cap // 2 < d <= cap < 2 * (n - 3) * 7
    assert ti.same(run(program, tmp_path, slots, lengths, flag, n, 256, cap=cap), statement(slots, lengths, flag, n)), (n, d, cap)
    got = run(program, tmp_path, slots, lengths, flag, n, 256, cap=cap // 2)
    assert got[3] == 2 and not got[0].any() and not got[1].any() and not got[2].any()


def test_tables_that_are_none_are_flagged_without_an_access_out_of_bounds(program, tmp_path):
    n = 65
    slots, lengths, flag = inputs(n, 5)
    t = 2 * (n - 3) + 3
    for k, v in ((7, n), (0, -1), (30, 1 << 30), (t - 1, n), (11, -(1 << 31))):
        q = slots.copy()
        q[3, k] = v
        got = run(program, tmp_path, q, lengths, flag, n, 256)
        assert got[3] == 1 and not got[0].any() and not got[1].any() and not got[2].any(), (k, v)
    dead = slots.copy()
    dead[0, 2 * 10] = dead[0, 1]                                # join 10 names the slot that join 0 joined away
    assert run(program, tmp_path, dead, lengths, flag, n, 256)[3] == 1
