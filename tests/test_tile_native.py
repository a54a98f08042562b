"""AddressSanitizer + UBSan build of the tiling host code as a stand-alone program (``tests/native/pf_tile_main.cpp``,
its own ``main``; nothing is loaded into Python): ``csrc/pf_tile_host.h``'s plan and the body of ``k_tile_combine``,
which the kernel shares with the CPU, run thread by thread on exactly-sized heap arrays.  The program's results are
compared bit for bit with ``tile.combine``.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from phyloformer_amd import tile as TL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_native") / "pf_tile_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_tile_main.cpp"),
           "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


# (N, M, threads): three set sizes; two; M = 2 and 3 (groups of one row: no within-group pair); a last group that is a
# single row; more rows than threads in a group and in a row (threads = 3), and the kernel's 256
CASES = [(10, 6, 256), (13, 8, 3), (9, 2, 256), (9, 3, 2), (7, 4, 1), (23, 5, 4), (41, 40, 3), (64, 9, 256)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("N,M,threads", CASES)
def test_combine_body_is_clean_under_asan_and_ubsan_and_equals_the_twin(program, tmp_path, N, M, threads):
    B = 2
    p = TL.plan(N, M)
    flat = np.random.default_rng(N * 1000 + M).uniform(0.01, 3.0, size=(B, p.T)).astype(np.float32)
    flat.tofile(tmp_path / "sets.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([program, str(B), str(N), str(M), str(threads), str(tmp_path / "sets.bin"), str(tmp_path / "res.bin")],
                         capture_output=True, text=True, env=env, timeout=300)
    tail = (run.stdout + run.stderr)[-4000:]
    assert run.returncode == 0 and f"clean, G = {p.G}, S = {p.S}, T = {p.T}" in run.stdout, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    res = np.fromfile(tmp_path / "res.bin", np.float32).reshape(2, B, N * (N - 1) // 2)
    want = TL.combine(flat, N, M)
    assert np.array_equal(res[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(res[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("N,M", [(5, 5), (4, 6), (5, 1)])
def test_program_refuses_what_the_plan_refuses(program, tmp_path, N, M):
    (tmp_path / "sets.bin").write_bytes(b"")
    run = subprocess.run([program, "1", str(N), str(M), "4", str(tmp_path / "sets.bin"), str(tmp_path / "res.bin")],
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and not (tmp_path / "res.bin").exists(), run.stderr[-2000:]
