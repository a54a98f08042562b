"""AddressSanitizer + UBSan build of the site-weight host code, fuzzed: ``csrc/pf_weights_host.h`` - pattern
compression (``pf_compress_sites``), bootstrap counts (``pf_boot_counts``), the padding rule (``pf_padded_sites``) and the
weight check that stands between a caller's weights and the device.  Plain C++: compiled with ``g++
-fsanitize=address,undefined -fno-sanitize-recover`` through ``tests/native/pf_weights_shim.cpp`` and driven with
hypothesis from a child process that has libasan preloaded (``tests/native/fuzz_weights.py``), against
``phyloformer_amd/weights_sites.py``.  No GPU."""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    out = subprocess.run(["gcc", f"-print-file-name={name}"], capture_output=True, text=True).stdout.strip()
    return out if os.path.isabs(out) and os.path.exists(out) else None


@pytest.mark.skipif(shutil.which("g++") is None or _tool("libasan.so") is None, reason="g++ / libasan not available")
def test_site_weight_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    lib = str(tmp_path / "libpf_weights_asan.so")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
           os.path.join(REPO, "tests", "native", "pf_weights_shim.cpp"), "-o", lib]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, LD_PRELOAD=_tool("libasan.so"), ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", PYTHONPATH=REPO)
    run = subprocess.run([sys.executable, os.path.join(REPO, "tests", "native", "fuzz_weights.py"), lib, "300"], env=env,
                         capture_output=True, text=True, timeout=900)
    tail = (run.stdout + run.stderr)[-4000:]
    assert run.returncode == 0 and "fuzz_weights: clean" in run.stdout, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
