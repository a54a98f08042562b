"""The compact tiling of option ``main_dedup`` walked on the CPU (``tests/native/pf_main_dedup_layout_main.cpp``, a
stand-alone program with its own ``main``, built with AddressSanitizer + UBSan; nothing is loaded into Python).
``csrc/pf_layout.h`` holds the tile -> (row, first compacted token) mapping for host and device alike: for small
``(P, K)`` every compacted token is covered exactly once, no tile spans more than two rows and only an alignment's last
tile is ragged; the routing rule is monotone in the number of distinct columns.  No GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_compact_tiles_cover_every_token_once(tmp_path):
    exe = str(tmp_path / "pf_main_dedup_layout_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_main_dedup_layout_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    tail = (res.stdout + res.stderr)[-4000:]
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert res.returncode == 0 and "pf_main_dedup_layout_main: clean" in res.stdout, tail
