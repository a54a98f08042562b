"""The row layout of option ``stats_dedup`` walked on the CPU (``tests/native/pf_row_stats_layout_main.cpp``, a
stand-alone program with its own ``main``, built with AddressSanitizer + UBSan; nothing is loaded into Python).
``csrc/pf_layout.h`` holds what k_row_stats needs of a pair row: its parts in the original tiling (flat or by rows) with
their tiles, first sites and partial slots, and its compact tiles.  The program prints them for every P <= 6, L <= 100
(and every K <= 100); a plain Python model, written from the tilings' definitions, must give the same lines.  No GPU."""
import os
import shutil
import subprocess

import pytest

from helpers.row_stats_model import ctile_lines, kmax, part_lines

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("row_stats_layout") / "pf_row_stats_layout_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_row_stats_layout_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    tail = (res.stdout + res.stderr)[-4000:]
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    return res


@needs_gxx
def test_the_program_finds_every_token_once_and_no_slot_twice(output):
    assert output.returncode == 0 and "pf_row_stats_layout_main: clean" in output.stdout, (output.stdout + output.stderr)[-4000:]


@needs_gxx
def test_row_parts_and_slots_are_the_models(output):
    got = [ln for ln in output.stdout.splitlines() if ln.startswith("part ")]
    want = [ln for P in range(1, 7) for L in range(1, 101)
            for flat in ((0, 1) if L >= 32 and L % 32 else (0,)) for ln in part_lines(flat, P, L)]
    assert got == want


@needs_gxx
def test_compact_tiles_of_a_row_are_the_models(output):
    got = [ln for ln in output.stdout.splitlines() if ln.startswith("ctile ")]
    assert got == [ln for K in range(1, 101) for ln in ctile_lines(K)]


@needs_gxx
def test_kmax_is_what_the_header_says(output):
    assert f"kmax {kmax()}" in output.stdout.splitlines() and kmax() >= 425
