"""-m gpu: every buffer of the default kernels, per token, at the edges of their tilings.

``debug_keep`` 1 leaves x0, srow{k}, mrow{k}, ctx{k} and x{k+1} of a whole batch behind; ``helpers/tap_check.py`` compares
each of them with the float64 oracle (chain) and with what float64 makes of the device's own upstream taps (kernel-local),
as the largest error of a buffer over its largest entry.  The end-to-end distances are a mean over sites: one token in a
ragged tile tail that is 1 % wrong moves them by 3e-6 and below (tests/test_tap_check_host.py) - here it is 5e-3 of its buffer, fifty
times the chain cap and a thousand times the kernel-local bound.

Shapes (pf_host_prep.h, tile_plan_core and colstats_plan_core decide what a shape reaches; none above 10,000 tokens, so
that the float64 oracle and the checker take a second or two):

  3x31            L < 32: one ragged tile per row, row tiling
  5x64, batch 2   whole tiles; k_embed's 64-site block exactly full
  6x63            row tiling with a ragged last tile (waste 1.6 % < the straddle's cost)
  9x65            flat tiling, tiles over two rows; the third site chunk holds one site; 36 pairs in runs of 8, walked by
                  runs (a lone alignment); also with the row tiling forced
  7x33, batch 3   flat tiling; alignments 1 and 2 start at tokens 693 and 1386, no tile multiples; the batch's last tile
                  is short; also with the row tiling forced
  2x45, batch 2   one pair: the column statistics sum over a single pair
  12x40, batch 2  66 pairs: two pair groups of 33, runs of 8 with a short last run; also colstats_fine 0 and 1
  13x100 gapped   pf_indel, 78 pairs in two groups of 39; gaps and X
  8x200           the benchmark's row length (7 tiles, flat), 28 pairs
  6x70 dedup      1, 33 and 70 distinct columns in one batch, options at their defaults: the split and the fused route of
                  main_dedup against the oracle, not only against each other

Left to the bit-identity and golden tests: runs of 32 and 64 pairs (500 or more pairs at several hundred sites: minutes in
the float64 oracle), and the schedule - ``debug_keep`` runs a batch as one chunk on one stream and runs the full last FFN
beside the folded head, so these tests pin the kernels' arithmetic, and tests/test_gpu_parity.py / test_gpu_main_dedup.py tie
the two-stream, chunked and routed schedules to it bit for bit.
"""
import os

import numpy as np
import pytest

import test_gpu_parity as parity
from helpers import tap_check
from helpers.dedup_model import alignment
from phyloformer_amd.msa_sim import simulate_batch

pytestmark = pytest.mark.gpu
NB = 6

# Shares of a buffer's largest expected entry.  chain: the caps of test_tiny_taps_localise_every_kernel, not to be widened.
# (measured worst over the cases below: srow 2.0e-5, mrow 2.2e-5, ctx 4.3e-5, x 6.2e-5, all four in the 6x70 batch of
# uniformly random residues; on simulated alignments srow 5.0e-6, mrow 3.6e-6, ctx 1.9e-5, x 1.2e-5.)
# kernel-local: four times the worst value measured on MI355X against the float64 expectations over all cases below
# (beside each bound, with the case), never above the chain cap; the same rule for the head - the distances recomputed
# from the device's x6 against the device's distances, head_fold 1 and 0.  The float32 oracle standing in for the device
# sits at 1.0e-6 (x) and below (tests/test_tap_check_host.py).
BOUNDS = {
    "chain": dict(tap_check.CHAIN_CAPS),
    "kernel-local": {
        "srow": 1.7e-6,     # 4 x 4.18e-7 (6x70 dedup; simulated: 2.56e-7 at 9x65)
        "mrow": 9.0e-7,     # 4 x 2.23e-7 (12x40 batch 2)
        "ctx": 5.1e-6,      # 4 x 1.27e-6 (2x45 batch 2: a single pair; otherwise 6.8e-7, 6x70 dedup)
        "x": 3.7e-6,        # 4 x 9.12e-7 (6x70 dedup; 9.08e-7 at 12x40 batch 2)
        "dist": 1.6e-6,     # 4 x 4.00e-7 (7x33 batch 3, head_fold 1; head_fold 0: 1.97e-7 at 2x45 batch 2)
    },
}


def _gapped_with_x():
    idx = simulate_batch(1, 13, 100, seed=58, gaps=True)
    idx[0, ::4, 9::17] = 20                                  # X, besides the simulated gaps
    assert (idx == 21).any() and (idx == 20).any()
    return idx


def _dedup_batch():
    return np.stack([alignment(6, 70, 1, "front"), alignment(6, 70, 33, "between"), alignment(6, 70, 70, "front")])


# name -> (checkpoint, alignment builder, is the shape's own tiling flat?)
CASES = {
    "3x31": ("pf", lambda: simulate_batch(1, 3, 31, seed=51), False),
    "5x64_b2": ("pf", lambda: simulate_batch(2, 5, 64, seed=52), False),
    "6x63": ("pf", lambda: simulate_batch(1, 6, 63, seed=53), False),
    "9x65": ("pf", lambda: simulate_batch(1, 9, 65, seed=43), True),
    "7x33_b3": ("pf", lambda: simulate_batch(3, 7, 33, seed=41), True),
    "2x45_b2": ("pf", lambda: simulate_batch(2, 2, 45, seed=44), True),
    "12x40_b2": ("pf", lambda: simulate_batch(2, 12, 40, seed=43), True),
    "13x100_gapped": ("pf_indel", _gapped_with_x, True),
    "8x200": ("pf", lambda: simulate_batch(1, 8, 200, seed=57), True),
    "6x70_dedup": ("pf", _dedup_batch, True),
}
RUNS = [(name, None) for name in CASES] + [("9x65", "row_tiles"), ("7x33_b3", "row_tiles"), ("12x40_b2", "fine0"), ("12x40_b2", "fine1")]

_INPUTS, _ERRORS = {}, {}


def inputs(weights, name):
    """(idx, the float64 oracle's taps per alignment) of a case: computed once, shared by its variants, left unchanged."""
    if name not in _INPUTS:
        ck, build, _flat = CASES[name]
        idx = build()
        idx.setflags(write=False)
        B, N, L = idx.shape
        assert B * (N * (N - 1) // 2) * L <= 10_000
        _INPUTS[name] = (idx, [tap_check.oracle_taps(weights(ck).tensors, a) for a in idx])
    return _INPUTS[name]


def record(run, rep):
    """The measured errors, printed and added to tests/test_gpu_parity.py's error table (parity_errors.json): one row per
    run - its worst kernel-local error, every figure under "detail" - and a row of the worst over the runs so far."""
    _ERRORS[run] = {f"{c} {k}": v for (c, k), v in sorted(rep.errors.items())}
    print(f"taps {run}: " + ", ".join(f"{n} {v:.2e}" for n, v in _ERRORS[run].items()))
    worst = {}
    for row in _ERRORS.values():
        for n, v in row.items():
            worst[n] = max(worst.get(n, 0.0), v)

    def entry(row):
        return {"max_abs_err": max(v for n, v in row.items() if n.startswith("kernel-local")), "max_abs_ref": None, "detail": row}
    parity._ERRORS[f"taps {run}: relative error per buffer kind"] = entry(_ERRORS[run])
    parity._ERRORS["taps, worst over the runs: relative error per buffer kind"] = entry(worst)
    parity._dump()


def read_taps(e, nb=NB):
    names = [f"x{k}" for k in range(nb + 1)] + [f"{b}{k}" for b in ("srow", "mrow", "ctx") for k in range(nb)]
    return {name: e.debug_read(name) for name in names}


def run_and_check(e, w, idx, orc, flat, run, nb=NB, bounds=BOUNDS):
    """Both head forms under debug_keep 1: the folded head's distances and every tap, then the full head's distances
    against its own last x.  nb, bounds: the checkpoint's block count and the bounds to hold it to
    (tests/test_gpu_ckpt_family.py brings its own)."""
    e.set_option("debug_keep", 1)
    try:
        e.set_option("head_fold", 1)
        dist = e.forward(idx)
        rep = tap_check.check_taps(w, idx, read_taps(e, nb), dist, bounds, flat=flat, oracle=orc, n_blocks=nb, must_pass=False)
        e.set_option("head_fold", 0)
        dist0 = e.forward(idx)
        rep0 = tap_check.check_taps(w, idx, {f"x{nb}": e.debug_read(f"x{nb}")}, dist0, bounds, flat=flat, n_blocks=nb,
                                    head_only=True, must_pass=False)
    finally:
        e.set_option("head_fold", 1)
        e.set_option("debug_keep", 0)
    rep.errors["kernel-local", "dist (head_fold 0)"] = rep0.errors["kernel-local", "dist"]
    record(run, rep)
    assert not rep.failures, rep.message()
    assert not rep0.failures, "head_fold 0: " + rep0.message()
    assert np.isfinite(dist).all() and np.isfinite(dist0).all()
    return dist, rep


@pytest.mark.parametrize("name,variant", RUNS, ids=[n if v is None else f"{n}-{v}" for n, v in RUNS])
def test_every_buffer_against_float64(engines, weights, name, variant):
    ck, _build, flat = CASES[name]
    idx, orc = inputs(weights, name)
    w = weights(ck).tensors
    run = name if variant is None else f"{name} {variant}"
    if variant == "row_tiles":
        # (the tiling is read once, when the engine is made: as test_flat_tiling_against_row_tiling forces it)
        from phyloformer_amd.engine import Engine
        assert flat and tap_check.flat_tiling(idx.shape[1] * (idx.shape[1] - 1) // 2, idx.shape[2])
        os.environ["PF_ROW_TILES"] = "1"
        try:
            with Engine(weights(ck), 0) as e:
                e.set_option("precise", 0)
                run_and_check(e, w, idx, orc, False, run)
        finally:
            os.environ.pop("PF_ROW_TILES", None)
        return
    e = engines(ck, precise=0)
    assert tap_check.flat_tiling(idx.shape[1] * (idx.shape[1] - 1) // 2, idx.shape[2]) == flat
    if variant in ("fine0", "fine1"):
        e.set_option("colstats_fine", int(variant[-1]))
    try:
        run_and_check(e, w, idx, orc, flat, run)
    finally:
        e.set_option("colstats_fine", -1)
