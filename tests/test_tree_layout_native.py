"""AddressSanitizer + UBSan build of the device layouts of the three tree searches as a stand-alone program
(``tests/native/pf_layout_main.cpp``, its own ``main``; nothing is loaded into Python).  Neighbour joining, balanced NNI
and balanced SPR each list their arrays once (``csrc/pf_nj_host.h``, ``csrc/pf_bme_host.h``); the bytes per source, the
spans of the device workspace and the host allocations all come from that list.  The program checks alignment,
disjointness and bounds of what the list carves; this side pins the bytes per source, which decide which ``N`` a given
``ws_limit_mb`` refuses and how a batch is chunked.  No GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

# Bytes of one source's state, from the formulas the layouts had before they were lists (``pfnj::state_bytes``,
# ``pfbme::Layout``, ``pfbme::SprLayout`` of the commit that added balanced SPR, compiled and run).
SIZES = (3, 4, 9, 65, 137, 300)
BYTES = {
    "nj": (4216, 4288, 4888, 38936, 156440, 728896),
    "bnni": (584, 1048, 5024, 240944, 1060384, 5060568),
    "spr": (976, 2032, 12832, 762384, 3430528, 16528912),
}


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layout_native") / "pf_layout_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_layout_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    return res


@needs_gxx
def test_every_array_is_aligned_disjoint_and_inside_the_workspace(output):
    """N in {3, 4, 9, 65, 137, 300}, B in {1, 3}, all three states; for B = 1 the measured bytes are the carved extent."""
    assert output.returncode == 0 and "pf_layout_main: clean" in output.stdout, (output.stdout + output.stderr)[-4000:]


@needs_gxx
@pytest.mark.parametrize("state", sorted(BYTES))
def test_bytes_per_source_are_those_of_the_former_formulas(output, state):
    got = {}
    for line in output.stdout.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[0] == state:
            got[int(parts[1])] = int(parts[2])
    assert got == dict(zip(SIZES, BYTES[state]))
