"""AddressSanitizer + UBSan build of the staging lists as a stand-alone program (``tests/native/pf_staging_main.cpp``,
its own ``main``; nothing is loaded into Python).  What a host entry point carves from one grow-only device buffer - the
staging of ``pf_nj_joins``, ``pf_join_supports``, ``pf_join_transfers`` and ``pf_join_consensus``, the two tables of the
tiling plan, the float spans of leave-one-out and placement, the attention operator's workspace - is listed once and
driven by the visitors of ``csrc/pf_spans.h``.  The program checks, for every list and shape, that each array is aligned
for its type, lies inside the measured total and is disjoint from the others, that only the arrays a variant does
without are empty, and that the total is the former offset chain's plus alignment padding only.  The four calls' lists
also carry a pattern per array through the upload and download visitors (``memcpy`` as the copy) between exactly sized
caller's arrays of the documented shapes and an exactly sized staging: a count that disagrees with the public header is
a red-zone hit.  No GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

# cases per list: N in {3, 4, 9, 65} x B in {1, 3} (x R in {1, 3}); supports, transfers and consensus start at N = 4;
# transfers without and with branch_moves, consensus without and with lengths; three tiling plans
CASES = {"nj": 8, "loo": 8, "supports": 12, "transfers": 24, "consensus": 24, "place": 16, "mha": 16, "tiled": 3}
# arrays per list
ARRAYS = {"nj": 4, "loo": 4, "supports": 7, "transfers": 11, "consensus": 11, "place": 6, "mha": 4, "tiled": 2}
TRIPS = ("nj", "supports", "transfers", "consensus")


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("staging_native") / "pf_staging_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_staging_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:]
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    return res


@needs_gxx
def test_every_staging_array_is_aligned_disjoint_and_inside_its_total(output):
    assert output.returncode == 0 and "pf_staging_main: clean" in output.stdout, (output.stdout + output.stderr)[-4000:]


@needs_gxx
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_shape_ran_and_grew_by_padding_only(output, name):
    """Lines are ``<list> <N> <B or M> <R> <total> <former>``: 8 bytes per array at most (256 for the attention operator)."""
    arrays = ARRAYS[name]
    rows = [line.split() for line in output.stdout.splitlines() if line.split()[:1] == [name]]
    assert len(rows) == CASES[name]
    for _, _n, _b, _r, total, former in rows:
        assert 0 <= int(total) - int(former) <= arrays * (256 if name == "mha" else 8)


@needs_gxx
@pytest.mark.parametrize("name", TRIPS)
def test_every_call_made_its_round_trip_at_every_shape(output, name):
    """Lines are ``trip <list> <N> <B> <R> <arrays> <bytes the caller holds>``: one per case of the list, every array named."""
    rows = [line.split() for line in output.stdout.splitlines() if line.split()[:2] == ["trip", name]]
    assert len(rows) == CASES[name]
    assert all(int(row[5]) == ARRAYS[name] and int(row[6]) > 0 for row in rows)
