"""The bodies of the split-support kernels (``csrc/pf_support_host.h``) as a stand-alone program
(``tests/native/pf_support_main.cpp``, its own ``main``; nothing is loaded into Python) under
``g++ -fsanitize=address,undefined``: the kernels' geometry - workgroups of 1, 3 and 256 threads, chunks of replicates -
with every array at its exact size, against ``supports.split_supports``; and tables that are none, which must be flagged
without one access out of bounds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import support_inputs as si
from phyloformer_amd import supports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("support_native") / "pf_support_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_support_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(program, tmp_path, ref, reps, flag, n, threads, rc):
    r, s = len(reps), n - 3
    np.ascontiguousarray(np.concatenate([np.asarray(ref, np.int32)[None, :], np.asarray(reps, np.int32)])).tofile(tmp_path / "tables.bin")
    np.ascontiguousarray(flag, dtype=np.uint8).tofile(tmp_path / "flags.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([program, str(n), str(r), str(threads), str(rc), *(str(tmp_path / f) for f in ("tables.bin", "flags.bin", "out.bin"))],
                         capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert res.returncode == 0 and "clean" in res.stdout, tail
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == s * 16 + 1
    return (np.frombuffer(raw, np.int32, s, 0).tolist(), np.frombuffer(raw, np.int64, s, 4 * s).tolist(),
            np.frombuffer(raw, np.int32, s, 12 * s).tolist(), raw[-1])


@pytest.mark.parametrize("n", [4, 5, 9, 64, 65, 137])
def test_kernel_geometry_equals_the_statement(program, tmp_path, n):
    ref, reps, flag = si.sources(n, 5)
    for b in range(2):
        want = supports.split_supports(ref[b], reps[b], n, flag[b])
        for threads, rc in ((1, 5), (3, 2), (256, 5), (256, 1)):
            got = run(program, tmp_path, ref[b], reps[b], flag[b], n, threads, rc)
            assert got == (*want, 0), (n, b, threads, rc)


def test_tables_that_are_none_are_flagged_without_an_access_out_of_bounds(program, tmp_path):
    n = 65
    ref, reps, flag = si.sources(n, 5)
    t = 2 * (n - 3) + 3
    for where, k, v in (("ref", 7, n), ("ref", 0, -1), ("ref", 30, 1 << 30), ("rep", 40, -1), ("rep", t - 1, n), ("rep", 11, -(1 << 31))):
        r, q = ref[0].copy(), reps[0].copy()
        if where == "ref":
            r[k] = v
        else:
            q[3, k] = v
        for rc in (5, 2):                                       # (the flag of an earlier chunk's tree holds in the later ones)
            count, transfer, depth, status = run(program, tmp_path, r, q, flag[0], n, 256, rc)
            assert status == 1 and not any(count) and not any(transfer) and not any(depth), (where, k, v, rc)
    dead = ref[0].copy()
    dead[2 * 10] = dead[1]                                      # join 10 names the slot that join 0 joined away
    assert run(program, tmp_path, dead, reps[0], flag[0], n, 256, 5)[3] == 1
