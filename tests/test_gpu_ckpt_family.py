"""-m gpu: the default kernels on (64, 4) checkpoints other than the five shipped ones.

The family is ``helpers/ckpt_family.py``'s: three checkpoints of another recipe (``random_weights``), ``pf`` with the
v / out_proj pair of its row or column attentions rescaled by 2^k - an exact invariance of the model, so the oracle and its
conditioning do not move and a change of the error is the kernels' own -, a ladder of members just inside and just outside
each quantity of the fp16 operand guard (pf_lib.hip::check_f16_ranges, f16_range_ok), and exact zeros.
tests/test_ckpt_family_host.py proves on the CPU what the members claim.

Every member makes its own engine with ``precise`` 0, so the small edge shapes of tests/test_gpu_taps.py stay on the default
kernels whenever the guard allows.  Per member and shape:

  * the library's verdict and figures (``f16_ranges`` debug read) against ``ckpt_family.f16_bounds``;
  * the guard says yes: the default kernels ran (profile: ``main`` > 0, ``precise`` 0); the distances are finite, within
    max(1e-4, 2 x |f32 oracle - f64 oracle|) of the fp32 oracle and the same bits one alignment at a time; every buffer
    under ``debug_keep`` 1 through ``tap_check.check_taps`` with the member's own tensors - the chain caps unchanged, the
    kernel-local bounds of test_gpu_taps.BOUNDS unchanged for the foreign checkpoints, |k| <= 3 and the zeros, and
    ``bounds_for`` (MEASURED below) for the others;
  * the guard says no: ``main`` stays 0 for ``precise`` -1 and 0, the result is within 1e-9 + 6e-8 max|want| of the float64
    oracle, and a checkpoint with an inf or a NaN gives non-finite distances exactly where the oracle does.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_taps as taps
from helpers import ckpt_family as F
from helpers import tap_check
from helpers.profiled import Profiled
from oracle import pf_oracle as O

pytestmark = pytest.mark.gpu

# member -> the worst kernel-local error measured on MI355X over the member's shapes, per buffer kind and for the distances
# (both head forms), as a share of the buffer's largest expected entry (DESIGN.md section 5 has the table).  The bound is
# section 5's rule with the member added to the cases: four times the worst measured over test_gpu_taps' cases and the
# member's own, never above the chain cap.
MEASURED = {
    "pf-row+6": dict(srow=2.55e-07, mrow=2.31e-07, ctx=3.94e-07, x=9.06e-07, dist=2.28e-07),        # worst of 6x63, 9x65, 12x40_b2
    "pf-row+6-blk0": dict(srow=2.68e-07, mrow=2.23e-07, ctx=3.30e-07, x=9.08e-07, dist=3.07e-07),
    "pf-row+6-blk5": dict(srow=2.68e-07, mrow=2.08e-07, ctx=3.30e-07, x=9.04e-07, dist=2.96e-07),
    "pf-row-4": dict(srow=2.11e-06, mrow=2.37e-07, ctx=2.93e-07, x=1.01e-06, dist=2.54e-07),        # S_kv: Wv' at 2^-4
    "pf-col+6": dict(srow=2.53e-07, mrow=2.34e-07, ctx=3.34e-07, x=8.79e-07, dist=2.82e-07),        # worst of 6x63, 9x65, 12x40_b2
    "pf-col+6-blk0": dict(srow=2.90e-07, mrow=2.68e-07, ctx=3.34e-07, x=8.74e-07, dist=2.43e-07),
    "pf-col+6-blk5": dict(srow=2.68e-07, mrow=2.23e-07, ctx=3.30e-07, x=9.08e-07, dist=2.75e-07),
    "pf-col-4": dict(srow=2.88e-07, mrow=2.08e-07, ctx=3.11e-07, x=3.61e-06, dist=2.23e-07),        # x: q' ctx / 16 at 2^-4
    "pf-row-6-blk0": dict(srow=2.68e-07, mrow=2.23e-07, ctx=3.30e-07, x=9.08e-07, dist=3.07e-07),
    "pf-row+10": dict(srow=2.44e-07, mrow=2.08e-07, ctx=3.94e-07, x=9.06e-07, dist=2.92e-07),
    "pf-col+9": dict(srow=1.86e-07, mrow=1.34e-07, ctx=9.20e-07, x=1.64e-06, dist=7.22e-08),        # 2x45_b2; x: Wo at 2^-9
    "pf-row+14": dict(srow=2.44e-07, mrow=2.08e-07, ctx=3.94e-07, x=9.06e-07, dist=2.92e-07),
    "pf-row+15": dict(srow=2.44e-07, mrow=2.08e-07, ctx=3.94e-07, x=9.06e-07, dist=2.92e-07),
    "pf-hidden-x128": dict(srow=2.69e-07, mrow=2.31e-07, ctx=3.30e-07, x=2.99e-06, dist=2.45e-07),  # x: W2 over 128
    "pf-mbase-x12": dict(srow=2.48e-07, mrow=2.08e-07, ctx=3.30e-07, x=7.99e-07, dist=2.77e-07),
    # distances of 1e-8: softplus far down its left tail, where x . w + b of entries near 3e4 is rounded to 2e-3
    "pf-rowbias-3e4": dict(srow=3.98e-07, mrow=3.33e-07, ctx=5.93e-07, x=6.22e-07, dist=3.12e-06),
    "pf-colbias-3e4": dict(srow=3.76e-07, mrow=2.49e-07, ctx=5.34e-07, x=6.22e-07, dist=5.08e-06),
}


def bounds_for(member):
    if member.bounds == "shipped" or all(r != "default" for r in member.shapes.values()):
        return taps.BOUNDS
    local = {}
    for kind, shipped in taps.BOUNDS["kernel-local"].items():
        local[kind] = min(max(shipped, 4.0 * MEASURED[member.name][kind]), tap_check.CHAIN_CAPS.get(kind, np.inf))
    return {"chain": dict(tap_check.CHAIN_CAPS), "kernel-local": local}


_WEIGHTS, _IDX, _ORACLE = {}, {}, {}


def member_weights(weights, m):
    if m.name not in _WEIGHTS:
        _WEIGHTS[m.name] = m.make(weights(m.base) if m.base else None)
    return _WEIGHTS[m.name]


def shape(name):
    if name not in _IDX:
        _IDX[name] = F.shapes()[name]()
        _IDX[name].setflags(write=False)
        B, N, L = _IDX[name].shape
        assert B * (N * (N - 1) // 2) * L <= 10_000
    return _IDX[name]


def oracle(weights, m, sname, taps_too):
    """(float64 distances, float32 distances, the float64 taps per alignment or None): computed once per checkpoint and
    shape, left unchanged.  An exact member shares its base's (tests/test_ckpt_family_host.py: the same bits)."""
    key = (m.base if m.exact else m.name, sname)
    if key not in _ORACLE or (taps_too and _ORACLE[key][2] is None):
        w = (weights(m.base) if m.exact else member_weights(weights, m))
        idx = shape(sname)
        with np.errstate(all="ignore"):
            d32 = O.forward_batch(w.tensors, idx, dtype=np.float32, n_blocks=w.n_blocks)
            if taps_too:
                orc = [tap_check.oracle_taps(w.tensors, a, w.n_blocks) for a in idx]
                d64 = np.stack([o["dist"] for o in orc])
            else:
                orc, d64 = None, O.forward_batch(w.tensors, idx, dtype=np.float64, n_blocks=w.n_blocks)
        _ORACLE[key] = (d64, d32, orc)
    return _ORACLE[key]


FIGURES = ("vmax_col", "hidden", "mbase64", "wmax", "bias", "wo_l1")


def library_ranges(e):
    """[ok, vmax_col, hidden, mbase * 64, wmax, bias, wo_l1] of the handle; a library without the added figures: the two."""
    out = np.full(1 + len(FIGURES), np.nan, np.float32)
    n = e._lib.pf_debug_read(e._h, b"f16_ranges", out.ctypes.data_as(C.c_void_p), out.size)
    assert n in (2, out.size), n
    return out[:n]


def verdict_problems(m, mw, P, route, got):
    """The library's figures against f16_bounds: the same verdict for the checkpoint, the same numbers to 1e-5."""
    b = F.f16_bounds(mw.tensors)
    problems = []
    want_ok = F.predicted_ok(b, 0)                          # the checkpoint's part of the verdict (P enters per forward)
    if bool(got[0]) != want_ok:
        problems.append(f"f16_ranges says ok = {bool(got[0])}, f16_bounds says {want_ok}: {b}")
    if len(got) != 1 + len(FIGURES):
        problems.append("the f16_ranges debug read returns no hidden / mbase / wmax / bias / wo_l1 figures")
    elif b["finite"] and all(np.isfinite(b[name]) for name in FIGURES):
        for name, lib in zip(FIGURES, got[1:]):
            if not abs(float(lib) - b[name]) <= 1e-5 * b[name]:
                problems.append(f"{name}: library {float(lib):.7g}, f16_bounds {b[name]:.7g}")
    assert F.predicted_ok(b, P) == (route == "default"), (m.name, b)
    return problems


def run_default(e, m, mw, idx, sname, weights):
    d64, d32, orc = oracle(weights, m, sname, True)
    B, N, L = idx.shape
    P = N * (N - 1) // 2
    with Profiled(e):
        got = e.forward(idx)
        assert e.profile_get("main")[0] > 0 and e.profile_get("precise")[0] == 0, "the guard sent the forward to float64"
    tol = max(1e-4, 2.0 * float(np.abs(d32.astype(np.float64) - d64).max()))
    err = float(np.abs(got.astype(np.float64) - d32).max()) if np.isfinite(got).all() else np.inf
    print(f"ckpt family {m.name}@{sname}: |got - f32 oracle| {err:.3e} (allowed {tol:.3e}), largest distance {np.abs(d64).max():.3g}")
    run = f"ckpt family {m.name}@{sname}"
    tap_failure = None
    try:
        taps.run_and_check(e, mw.tensors, idx, orc, tap_check.flat_tiling(P, L), run, mw.n_blocks, bounds_for(m))
    except AssertionError as exc:                             # (the end-to-end rule is judged first, the buffers named after it)
        tap_failure = exc
    assert np.isfinite(got).all(), "non-finite distances from the default kernels"
    assert err <= tol, (err, tol)
    if tap_failure is not None:
        raise tap_failure
    if B > 1:
        assert np.array_equal(np.stack([e.forward(a) for a in idx]), got)


def run_float64(e, m, mw, idx, sname, weights, problems):
    d64, _d32, _ = oracle(weights, m, sname, False)
    for opt in (-1, 0):
        e.set_option("precise", opt)
        with Profiled(e):
            got = e.forward(idx).astype(np.float64)
            n_main, n_precise = e.profile_get("main")[0], e.profile_get("precise")[0]
        if n_main != 0 or n_precise == 0:
            problems.append(f"precise {opt}: the default kernels ran (main {n_main}, precise {n_precise})")
        fin = np.isfinite(d64)
        if not np.array_equal(np.isfinite(got), fin):
            problems.append(f"precise {opt}: {int((~np.isfinite(got)).sum())} non-finite distances of {got.size}, "
                            f"the float64 oracle has {int((~fin).sum())}")
        elif fin.any():
            err, scale = float(np.abs(got[fin] - d64[fin]).max()), float(np.abs(d64[fin]).max())
            print(f"ckpt family {m.name}@{sname} precise {opt}: |got - f64 oracle| {err:.3e}, largest distance {scale:.3g}")
            if not err <= 1e-9 + 6e-8 * scale:
                problems.append(f"precise {opt}: {err:.3e} from the float64 oracle (largest distance {scale:.3g})")


@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_member(weights, case):
    from phyloformer_amd.engine import Engine
    m, sname = case
    mw = member_weights(weights, m)
    idx = shape(sname)
    N = idx.shape[1]
    route = m.shapes[sname]
    with Engine(mw, 0) as e:
        e.set_option("precise", 0)
        problems = verdict_problems(m, mw, N * (N - 1) // 2, route, library_ranges(e))
        if route == "default":
            assert not problems, "\n".join(problems)
            run_default(e, m, mw, idx, sname, weights)
        else:
            run_float64(e, m, mw, idx, sname, weights, problems)
            assert not problems, "\n".join(problems)
