"""The bodies of the transfer-count kernels (``csrc/pf_support_host.h``: the matching that keeps its key and
``k_sup_moves``) as a stand-alone program (``tests/native/pf_transfers_main.cpp``, its own ``main``; nothing is loaded
into Python) under ``g++ -fsanitize=address,undefined``: the kernels' geometry - workgroups of 1, 3 and 256 threads, chunks
of 1 and 2 replicates - with every array at its exact size, against ``supports.transfer_taxa``; and tables that are none,
which must be flagged without one access out of bounds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import support_inputs as si
from helpers import transfer_inputs as ti

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("transfers_native") / "pf_transfers_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_transfers_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(program, tmp_path, ref, reps, flag, n, threads, rc, cutoff, branch=True):
    """``ti.NAMES``' results as lists (``branch_moves`` None without ``branch``)."""
    r, s = len(reps), n - 3
    np.ascontiguousarray(np.concatenate([np.asarray(ref, np.int32)[None, :], np.asarray(reps, np.int32)])).tofile(tmp_path / "tables.bin")
    np.ascontiguousarray(flag, dtype=np.uint8).tofile(tmp_path / "flags.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([program, str(n), str(r), str(threads), str(rc), str(cutoff), str(int(branch)),
                          *(str(tmp_path / f) for f in ("tables.bin", "flags.bin", "out.bin"))],
                         capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert res.returncode == 0 and "clean" in res.stdout, tail
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == s * 24 + n * 8 + (s * n * 4 if branch else 0) + 1
    at, out = 0, {}
    for name, dtype, count in (("count", np.int32, s), ("transfer", np.int64, s), ("depth", np.int32, s), ("moves", np.int64, n),
                               ("used", np.int32, s), ("capped", np.int32, s), ("branch_moves", np.int32, s * n if branch else 0)):
        out[name] = np.frombuffer(raw, dtype, count, at).tolist()
        at += count * np.dtype(dtype).itemsize
    out["branch_moves"] = [out["branch_moves"][t * n:(t + 1) * n] for t in range(s)] if branch else None
    out["status"] = raw[-1]
    return out


@pytest.mark.parametrize("n", [4, 5, 9, 64, 65, 137])
def test_kernel_geometry_equals_the_statement(program, tmp_path, n):
    ref, reps, flag = si.sources(n, 5)
    for b in range(2):
        for cutoff in ti.CUTOFFS:
            want = dict(ti.statement(n, 5, b, cutoff), status=0)
            for threads, rc, branch in ((1, 5, True), (3, 2, True), (256, 5, False), (256, 1, True)):
                got = run(program, tmp_path, ref[b], reps[b], flag[b], n, threads, rc, cutoff, branch)
                assert got == (want if branch else dict(want, branch_moves=None)), (n, b, cutoff, threads, rc)


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
        for rc in (5, 2, 1):                                    # (the flag of an earlier chunk's tree holds in the later ones)
            got = run(program, tmp_path, r, q, flag[0], n, 256, rc, 100)
            assert got.pop("status") == 1
            assert not any(np.asarray(v).any() for v in got.values()), (where, k, v, rc)
    dead = ref[0].copy()
    dead[2 * 10] = dead[1]                                      # join 10 names the slot that join 0 joined away
    assert run(program, tmp_path, dead, reps[0], flag[0], n, 256, 5, 30)["status"] == 1
