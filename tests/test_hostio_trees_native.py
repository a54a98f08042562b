"""AddressSanitizer + UBSan build of the tree half of ``csrc/pf_hostio.cpp`` as a stand-alone program
(``tests/native/pf_hostio_trees_main.cpp``, its own ``main``, compiled together with ``pf_hostio.cpp``; nothing is loaded
into Python).  The program checks the frame of every text entry point itself - capacities 0, need - 1 and need on
exactly sized buffers, every refusal - and the table round trip ``pf_nj_joins_host_n`` -> ``pf_nj_format_joins_n``
against ``pf_nj_newick_n``.  What it prints is compared here with the pure-Python twins: byte for byte the texts of the
three (start, search) combinations, integer for integer the joint supports / transfers implementation.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import bme_check as bc
from helpers import support_inputs as si
from helpers.nj_table import matrix_of
from phyloformer_amd import bionj, bme, bootstrap, nj, supports

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostio_trees_native") / "pf_hostio_trees_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "native", "pf_hostio_trees_main.cpp"),
           os.path.join(REPO, "phyloformer_amd", "csrc", "pf_hostio.cpp"), "-pthread", "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(program, *args) -> bytes:
    res = subprocess.run([program, *map(str, args)], capture_output=True, env=ENV, timeout=600)
    tail = (res.stdout + res.stderr)[-4000:].decode("utf8", "replace")
    assert res.returncode == 0 and res.stdout.endswith(b"pf_hostio_trees_main: clean\n"), tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail and "MISS" not in tail, tail
    return res.stdout


def ids_of(n: int):
    """The ids of the program's ``ids()``: an empty one, a NUL byte, multi-byte UTF-8, then plain ones."""
    return ["", "a\0b", "é日"][:n] + [f"t{i}" for i in range(3, n)]


def distances(n: int) -> np.ndarray:
    """Uniform distances (negative branch lengths, many moves) while the twins are quick; a noisy tree above."""
    if n < 10:
        return bc.uniform_preds(n, 7 * n)[0]
    base = bc.random_tree_distances(n, 5)
    return (base * np.random.default_rng(n).uniform(0.8, 1.2, size=base.shape)).astype(np.float32)


def texts_of(out: bytes) -> dict:
    """``== name steps bytes\\n`` and the text, one after the other."""
    got, at = {}, 0
    while not out.startswith(b"pf_hostio_trees_main", at):
        head = re.match(rb"== (\w+) (\d+) (\d+)\n", out[at:])
        assert head, out[at:at + 80]
        size = int(head.group(3))
        at += head.end()
        got[head.group(1).decode()] = (int(head.group(2)), out[at:at + size])
        at += size
    return got


# 3: no join, the trifurcation alone; 4: one join, nothing to move for SPR; 9; 65: a second word of the split sets
@needs_gxx
@pytest.mark.parametrize("clamp", [1, 0])
@pytest.mark.parametrize("n", [3, 4, 9, 65])
def test_texts_equal_the_python_twins_and_the_frame_holds(program, tmp_path, n, clamp):
    vec, ids = distances(n), ids_of(n)
    vec.tofile(tmp_path / "preds.bin")
    got = texts_of(run(program, "text", n, clamp, tmp_path / "preds.bin"))
    want_nj = nj.newick_of_joins(ids, *nj.nj_joins(matrix_of(vec, n)), bool(clamp)).encode("utf8")
    assert got["nj"] == (0, want_nj)
    assert got["joins"] == (0, want_nj)                                                    # (NJ, no search, through the table)
    assert got["bionj"] == (0, bionj.bionj_newick_py(vec, ids, bool(clamp)).encode("utf8"))   # (BIONJ, no search)
    for name, twin in (("bme", bme.bme_tree_py), ("spr", bme.spr_tree_py)):                # (NJ, NNI) and (NJ, SPR)
        text, steps = twin(vec, ids, bool(clamp))                                           # (bme_newick_py / spr_newick_py: the text)
        assert got[name] == (steps, text.encode("utf8")), name
    assert got["support"] == (0, bootstrap.support_newick_py(vec, np.stack([vec, vec]), ids, bool(clamp)).encode("utf8"))
    if n == 65:
        assert got["spr"][0] > 0                                                           # (a search that moved)


# B = 2 sources of R = 3 replicates that reach every branch of the definition (helpers.support_inputs.sources)
@needs_gxx
@pytest.mark.parametrize("n", [5, 65])
def test_supports_and_transfers_share_one_implementation(program, tmp_path, n):
    cutoff = 30
    ref, reps, flag = si.sources(n, 3)
    reps = reps.copy()
    reps[1, 2] = reps[0, 0]               # (the flagged replicate's table of zeros: the run without flags reads it)
    with open(tmp_path / "tables.bin", "wb") as fh:
        fh.write(ref.astype(np.int32).tobytes() + reps.astype(np.int32).tobytes() + flag.astype(np.uint8).tobytes())
    got = {}
    for line in run(program, "supports", 2, 3, n, cutoff, tmp_path / "tables.bin").decode().splitlines()[:-1]:
        name, values = line.split(":")
        key, flags, branch = name.split()
        got[key, int(flags), int(branch)] = [int(v) for v in values.split()]
    s = n - 3
    for flags in (0, 1):
        fl = [flag[b] if flags else None for b in range(2)]
        assert got["supports.status", flags, 0] == [0, 0]
        for b in range(2):
            want = supports.transfer_taxa(ref[b], reps[b], n, fl[b], cutoff)
            assert (want["count"], want["transfer"], want["depth"]) == supports.split_supports(ref[b], reps[b], n, fl[b])
            for key in ("count", "transfer", "depth"):
                assert got["supports." + key, flags, 0][b * s:(b + 1) * s] == want[key], (key, flags, b)
            for branch in (0, 1):
                assert got["transfers.moves", flags, branch][b * n:(b + 1) * n] == want["moves"], (flags, branch, b)
                for key in ("used", "capped"):
                    assert got["transfers." + key, flags, branch][b * s:(b + 1) * s] == want[key], (key, flags, branch, b)
            rows = got["transfers.branch_moves", flags, 1][b * s * n:(b + 1) * s * n]
            assert [rows[t * n:(t + 1) * n] for t in range(s)] == want["branch_moves"], (flags, b)
