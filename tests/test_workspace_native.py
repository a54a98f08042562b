"""AddressSanitizer + UBSan build of the default kernels' workspace list as a stand-alone program
(``tests/native/pf_workspace_main.cpp``, its own ``main``; nothing is loaded into Python).  The workspace of a run - x,
qrow, qcol, srow, mrow, part, ctx, mfrag, spart, outpart, rq and one span of ints cut into srep | ulist | ucount | plan -
is listed once (``csrc/pf_host_prep.h``: ``workspace_arrays``) and measured and carved by the visitors of
``csrc/pf_spans.h``.  The program keeps the offset chain the list replaced and checks, for every shape, that every offset
and the total are byte-equal to it, that each array is 256-aligned, inside the total and disjoint from the others, that
the trash area behind x, qrow and qcol lies inside their spans, and - on real memory of the span's exact size - the cut
of the int span.  No GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

# B in {1, 2, 3, 17} x N in {2, 3, 20, 200} x Lloc in {0, 1, 31, 32, 33, 500, 4096} x colstats_fine in {-1, 0, 1}
# x tile_force in {-1, 0, 1}
SHAPES = 4 * 4 * 7 * 3 * 3


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("workspace_native") / "pf_workspace_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_workspace_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    return res


@needs_gxx
def test_every_workspace_array_is_where_the_former_chain_put_it(output):
    assert output.returncode == 0 and "pf_workspace_main: clean" in output.stdout, (output.stdout + output.stderr)[-4000:]


@needs_gxx
def test_every_shape_ran_and_measures_what_the_former_chain_did(output):
    """Lines are ``ws <B> <N> <Lloc> <fine> <tile_force> <total> <former>``."""
    rows = [line.split() for line in output.stdout.splitlines() if line.split()[:1] == ["ws"]]
    assert len(rows) == SHAPES and len({tuple(r[1:6]) for r in rows}) == SHAPES
    assert all(int(r[6]) == int(r[7]) > 0 and int(r[6]) % 256 == 0 for r in rows)
