"""The tap checker of tests/test_gpu_taps.py, tested on the CPU: would it fail for a subtly wrong kernel?

The stand-in device is the float32 oracle: its x taps, ``devmath``'s srow / mrow / ctx on its activations narrowed to
float32, its distances.  It must pass with the bounds the GPU test asserts.  Then six faults of the kind a ragged tile tail,
a mis-masked lane or a wrong batch offset produces are planted one at a time, at 12 x 40 and 9 x 65 (the alignments of
``simulate_batch(2, n, l, seed=43)``): each must fail, and the first kernel-local finding must name the planted buffer and
block.  For the smallest of them the distances move by less than 1e-5: the end-to-end 1e-4 cannot see it.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import devmath
from helpers import tap_check
from oracle import pf_oracle as O
from phyloformer_amd.msa_sim import simulate_batch
from test_gpu_taps import BOUNDS

SHAPES = [(12, 40), (9, 65)]
NB = 6
_CASES = {}


def case(weights, n, l):
    """(idx, float64 oracle taps per alignment, the stand-in's taps, its distances): built once per shape, read-only."""
    if (n, l) not in _CASES:
        w = weights("pf").tensors
        idx = simulate_batch(2, n, l, seed=43)
        P = n * (n - 1) // 2
        taps = {f"x{k}": np.empty((2, P, l, 64), np.float32) for k in range(NB + 1)}
        taps.update({f"srow{k}": np.empty((2, P, 72), np.float32) for k in range(NB)})
        taps.update({f"mrow{k}": np.empty((2, P, 4, 64), np.float32) for k in range(NB)})
        taps.update({f"ctx{k}": np.empty((2, l, 64), np.float32) for k in range(NB)})
        dist = np.empty((2, P), np.float32)
        for b in range(2):
            act = {}
            dist[b] = O.forward(w, idx[b], dtype=np.float32, tap=lambda name, a: act.__setitem__(name, np.array(a)))
            taps["x0"][b] = act["embed"]
            for k in range(NB):
                srow = devmath.expected_srow(w, k, act["embed"] if k == 0 else act[f"block{k - 1}.ffn"])[0]
                taps[f"srow{k}"][b] = srow
                taps[f"mrow{k}"][b] = devmath.expected_mrow(w, k, srow, l)[:, :4]
                taps[f"ctx{k}"][b] = devmath.expected_ctx(w, k, act[f"block{k}.row"])[0]
                taps[f"x{k + 1}"][b] = act[f"block{k}.ffn"]
        for a in list(taps.values()) + [dist, idx]:
            a.setflags(write=False)
        _CASES[n, l] = (idx, [tap_check.oracle_taps(w, a) for a in idx], taps, dist)
    return _CASES[n, l]


def blocks_from(w, x, start, l):
    """Blocks start .. 5 and the head in float64, by devmath's restatement of the device's algebra."""
    for k in range(start, NB):
        srow = devmath.expected_srow(w, k, x)[0]
        x_row = devmath.expected_x_row(w, k, x, devmath.expected_mrow(w, k, srow, l))
        x = devmath.expected_block_out(w, k, x_row, devmath.expected_ctx(w, k, x_row)[0])
    return devmath.expected_distances(w, x)


@pytest.mark.parametrize("n,l", SHAPES)
def test_the_kernel_local_formulas_are_the_oracles(weights, n, l):
    """With the float64 oracle's own taps standing in for the device, every kernel-local expectation agrees with them
    to rounding: the checker's chain of formulas is the oracle's forward, not a second model of it."""
    w = weights("pf").tensors
    idx = simulate_batch(1, n, l, seed=43)
    orc = tap_check.oracle_taps(w, idx[0])
    taps = {"x0": orc["embed"]}     # (float64, so that block 0 too starts from the oracle's bits; x0's own finding is not the point)
    for k in range(NB):
        x_in = orc["embed"] if k == 0 else orc[f"block{k - 1}.ffn"]
        taps[f"srow{k}"] = devmath.expected_srow(w, k, x_in)[0]
        taps[f"mrow{k}"] = devmath.expected_mrow(w, k, taps[f"srow{k}"], l)[:, :4]
        taps[f"ctx{k}"] = devmath.expected_ctx(w, k, orc[f"block{k}.row"])[0]
        taps[f"x{k + 1}"] = orc[f"block{k}.ffn"]
    tight = {"chain": dict.fromkeys(tap_check.KINDS, 1e-12), "kernel-local": dict.fromkeys(tap_check.KINDS + ("dist",), 1e-12)}
    rep = tap_check.check_taps(w, idx, taps, orc["dist"][None], tight, oracle=[orc], must_pass=False)
    assert [f.kind for f in rep.failures] in ([], ["x0"]), rep.message()
    print(f"float64 stand-in {n}x{l}: worst kernel-local error {max(v for k, v in rep.errors.items() if k[0] == 'kernel-local'):.1e}")
    assert np.abs(blocks_from(w, orc["block2.ffn"], 3, l) - orc["dist"]).max() <= 1e-12 * np.abs(orc["dist"]).max()


@pytest.mark.parametrize("n,l", SHAPES)
def test_the_float32_stand_in_passes_the_gpu_tests_bounds(weights, n, l):
    idx, orc, taps, dist = case(weights, n, l)
    rep = tap_check.check_taps(weights("pf").tensors, idx, taps, dist, BOUNDS, oracle=orc)
    assert not rep.failures
    assert set(rep.errors) == {(c, k) for c in ("chain", "kernel-local") for k in tap_check.KINDS} | {("kernel-local", "dist")}
    for key, err in sorted(rep.errors.items()):
        print(f"float32 stand-in {n}x{l} {key[0]} {key[1]}: {err:.2e}")


def last_site_scaled(t, n, l):
    t["x3"][:, :, l - 1] *= np.float32(1.01)


def last_site_from_its_neighbour(t, n, l):
    t["x3"][:, :, l - 1] = t["x3"][:, :, l - 2]


def srow_without_the_last_site(t, n, l, w=None):
    pair = 5
    t["srow2"][0, pair] = devmath.expected_srow(w, 2, t["x2"][0, pair:pair + 1, :l - 1])[0][0]


def ctx_of_the_last_site_from_site_0(t, n, l):
    t["ctx4"][:, l - 1] = t["ctx4"][:, 0]


def mrow_of_two_pairs_exchanged(t, n, l):
    t["mrow1"][0, [3, 4]] = t["mrow1"][0, [4, 3]]


def batch_rows_shifted_by_one_pair(t, n, l):
    t["x5"][1] = np.roll(t["x5"][1], 1, axis=0)


FAULTS = [(last_site_scaled, "x3", 2), (last_site_from_its_neighbour, "x3", 2), (srow_without_the_last_site, "srow2", 2),
          (ctx_of_the_last_site_from_site_0, "ctx4", 4), (mrow_of_two_pairs_exchanged, "mrow1", 1),
          (batch_rows_shifted_by_one_pair, "x5", 4)]


@pytest.mark.parametrize("n,l", SHAPES)
@pytest.mark.parametrize("fault,buffer,block", FAULTS, ids=[f[0].__name__ for f in FAULTS])
def test_a_planted_fault_fails_and_is_named(weights, n, l, fault, buffer, block):
    w = weights("pf").tensors
    idx, orc, taps, dist = case(weights, n, l)
    t = {name: a.copy() for name, a in taps.items()}
    if fault is srow_without_the_last_site:
        fault(t, n, l, w)
    else:
        fault(t, n, l)
    changed = [name for name in t if not np.array_equal(t[name], taps[name])]
    assert changed == [buffer]
    with pytest.raises(AssertionError) as exc:
        tap_check.check_taps(w, idx, t, dist, BOUNDS, oracle=orc)
    rep = tap_check.check_taps(w, idx, t, dist, BOUNDS, oracle=orc, must_pass=False)
    first = rep.local_failures()[0]
    assert (first.buffer, first.block) == (buffer, block), rep.message()
    assert any(f.comparison == "chain" and f.buffer == buffer for f in rep.failures), rep.message()
    text = str(exc.value)
    assert text.splitlines()[1].startswith(f"kernel-local: {buffer} (block {block},"), text
    if buffer == "x3":          # the worst element is a last-site token, and the report says what that means for the tiles
        assert f"site {l - 1}," in str(first) and "in its row's last tile" in str(first), first
        assert "in the last site chunk" + (" (1 sites)" if l == 65 else " (8 sites)") in str(first), first
    if buffer == "ctx4":
        assert f"site {l - 1}," in str(first) and "the site lies in the last site chunk" in str(first), first
    if buffer == "x5":
        assert first.aln == 1 and all(f.aln == 1 for f in rep.failures), rep.message()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_gpu_cases_reach_the_edges_their_table_names(tmp_path):
    """The host's own plans (csrc/pf_host_prep.h through tests/native/pf_host_prep_shim.cpp) for the shapes of
    tests/test_gpu_taps.py: the tiling each case is listed with, its pair groups and runs - so that a change of those
    heuristics cannot quietly move a case off the edge it is there for - and the checker's copy of the tiling rule."""
    import test_gpu_taps as T
    lib_path = str(tmp_path / "libpf_host_prep_shim.so")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared",
                          os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "pf_host_prep_shim.cpp"), "-o", lib_path],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    shim = C.CDLL(lib_path)

    def tile_plan(P, L, force=-1):
        out = [C.c_int() for _ in range(3)]
        shim.t_tile_plan(P, L, force, *[C.byref(v) for v in out])
        return tuple(v.value for v in out)             # flat, tiles, slots per alignment

    def col_plan(B, P, L, fine=-1):
        out = [C.c_int() for _ in range(4)]
        shim.t_colstats_plan(B, P, L, fine, *[C.byref(v) for v in out])
        return tuple(v.value for v in out)             # G, sub, S, fine

    for P in (1, 3, 21, 36, 66, 78):
        for L in list(range(1, 131)) + [159, 160, 161, 200, 500]:
            for force in (-1, 0, 1):
                assert tap_check.flat_tiling(P, L, force) == bool(tile_plan(P, L, force)[0]), (P, L, force)
    shapes = {name: build().shape for name, (_ck, build, _flat) in T.CASES.items()}
    for name, (B, N, L) in shapes.items():
        assert bool(tile_plan(N * (N - 1) // 2, L)[0]) == T.CASES[name][2], name
    assert shapes["3x31"][2] < 32 and tile_plan(3, 31) == (0, 3, 3)                       # one ragged tile per row
    assert tile_plan(10, 64)[:2] == (0, 20) and tile_plan(15, 63)[:2] == (0, 30)          # whole tiles; ragged row tiles
    assert tile_plan(36, 65) == (1, 74, 110) and 36 * 65 % 32                             # flat, the last tile short
    assert col_plan(1, 36, 65) == (1, 8, 5, 1)                                            # one group, runs of 8, by runs
    assert tile_plan(21, 33)[:2] == (1, 22) and (21 * 33) % 32 == 21                      # alignments at 693, 1386
    assert tile_plan(21, 33, 0)[0] == 0 and tile_plan(36, 65, 0)[0] == 0                  # PF_ROW_TILES forces rows
    assert col_plan(2, 1, 45)[0] == 1 and shapes["2x45_b2"][1] == 2                       # a single pair
    assert col_plan(2, 66, 40)[:3] == (2, 8, 5) and 33 % 8 == 1                           # groups of 33, short last run
    assert col_plan(2, 66, 40, 0)[3] == 0 and col_plan(2, 66, 40, 1)[3] == 1              # by groups / by runs, forced
    assert col_plan(1, 78, 100)[:2] == (2, 8) and 78 // 2 == 39                           # two groups of 39
    assert tile_plan(28, 200)[0] == 1 and (200 + 31) // 32 == 7                           # 7 tiles per row, flat


def test_the_distances_do_not_see_a_last_site_that_is_one_percent_off(weights):
    """x3's last site scaled by 1.01 in every pair of 12 x 40, blocks 3-5 and the head run from there in float64: no
    distance moves by 1e-5, a tenth of what tests/test_gpu_parity.py::_check allows - while the token itself is 5e-3 of
    its buffer, fifty times the 1e-4 cap (the first fault above)."""
    n, l = 12, 40
    w = weights("pf").tensors
    idx, orc, taps, dist = case(weights, n, l)
    x3 = orc[0]["block2.ffn"].copy()
    clean = blocks_from(w, x3, 3, l)
    assert np.abs(clean - orc[0]["dist"]).max() <= 1e-12 * np.abs(clean).max()
    x3[:, l - 1] *= 1.01
    moved = float(np.abs(blocks_from(w, x3, 3, l) - clean).max())
    print(f"12x40, last site of x3 scaled by 1.01: largest change of a distance {moved:.2e}")
    assert 0 < moved < 1e-5
