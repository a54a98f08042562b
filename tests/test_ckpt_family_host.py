"""The checkpoint family of tests/test_gpu_ckpt_family.py, checked on the CPU: does it prove what it claims?

  * every rescaled member gives the float64 and the float32 oracle's distances of its base bit for bit, on every shape the
    GPU test runs it on (so the GPU test may share the base's oracle, and a changed error is the kernels' own);
  * every member meant for the default kernels is an input they are judged on: a finite fp32 oracle, the largest distance
    below 8 (the range re-check stays out), |f32 oracle - f64 oracle| <= 2.5e-5 (the contract's 1e-4 floor judges the
    kernel, not the reference);
  * ``f16_bounds`` predicts the route each member is listed with, at least the member's margin away from F16_LIMIT (1.5;
    the few members the family keeps nearer say why in helpers/ckpt_family.py), and reproduces the figures pf_lib.hip
    quotes for the shipped checkpoints: 61 / 196 / 30;
  * the tap checker fails, naming the right buffer first, when one operand of a k = -6 member loses its lo limb.
"""
import numpy as np
import pytest

import devmath
from helpers import ckpt_family as F
from helpers import tap_check
from oracle import pf_oracle as O
from test_gpu_ckpt_family import bounds_for

CKPTS = ("pf", "pf_base", "pf_indel", "pf_cherry", "pf_selreg")
_ORACLE, _IDX = {}, {}


def shape(name):
    if name not in _IDX:
        _IDX[name] = F.shapes()[name]()
        _IDX[name].setflags(write=False)
    return _IDX[name]


def both_oracles(key, w, sname):
    """(float64, float32) distances, once per checkpoint and shape."""
    if (key, sname) not in _ORACLE:
        with np.errstate(all="ignore"):
            _ORACLE[key, sname] = tuple(O.forward_batch(w.tensors, shape(sname), dtype=dt, n_blocks=w.n_blocks)
                                        for dt in (np.float64, np.float32))
    return _ORACLE[key, sname]


EXACT = [c for c in F.CASES if c[0].exact]
DEFAULT = [c for c in F.CASES if c[0].shapes[c[1]] == "default" and not c[0].exact]


@pytest.mark.parametrize("case", EXACT, ids=F.case_id)
def test_a_rescaled_member_is_an_exact_invariance(weights, case):
    m, sname = case
    base = weights(m.base)
    mw = m.make(base)
    changed = [k for k in base.tensors if not np.array_equal(base.tensors[k], mw.tensors[k])]
    assert changed and all(k.endswith(("v_proj.weight", "v_proj.bias", "out_proj.weight")) for k in changed)
    want = both_oracles(m.base, base, sname)
    for dt, ref in zip((np.float64, np.float32), want):
        got = O.forward_batch(mw.tensors, shape(sname), dtype=dt)
        assert got.dtype == ref.dtype and np.array_equal(got, ref), (m.name, sname, dt)


def _caps(d64, d32):
    assert np.isfinite(d32).all() and np.isfinite(d64).all()
    assert float(np.abs(d64).max()) < 8.0
    assert float(np.abs(d32.astype(np.float64) - d64).max()) <= 2.5e-5


@pytest.mark.parametrize("ck,sname", sorted({(c[0].base, c[1]) for c in EXACT if c[0].shapes[c[1]] == "default"}))
def test_the_bases_are_inputs_the_default_kernels_are_judged_on(weights, ck, sname):
    _caps(*both_oracles(ck, weights(ck), sname))


@pytest.mark.parametrize("case", DEFAULT, ids=F.case_id)
def test_a_member_for_the_default_kernels_is_an_input_they_are_judged_on(weights, case):
    m, sname = case
    mw = m.make(weights(m.base) if m.base else None)
    d64, d32 = both_oracles(m.name, mw, sname)
    print(f"{m.name}@{sname}: largest distance {np.abs(d64).max():.3g}, f32 vs f64 oracle {np.abs(d32 - d64).max():.2e}")
    _caps(d64, d32)


@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_the_predicted_route_keeps_its_margin(weights, case):
    m, sname = case
    mw = m.make(weights(m.base) if m.base else None)
    N = shape(sname).shape[1]
    P = N * (N - 1) // 2
    b = F.f16_bounds(mw.tensors)
    assert F.predicted_ok(b, P) == (m.shapes[sname] == "default"), b
    assert b["finite"] != m.nonfinite
    assert 1.15 <= m.min_margin <= 1.5 and (m.min_margin == 1.5 or m.ladder)
    assert F.margin(b, P) >= m.min_margin, (F.margin(b, P), b)
    # "just" inside or outside: within a factor of 3
    if m.ladder and m.min_margin == 1.5:
        assert F.margin(b, P) < 3.0, (F.margin(b, P), b)


def test_every_guarded_quantity_has_a_member_on_each_side():
    sides = {(m.ladder, route) for m in F.MEMBERS for route in m.shapes.values() if m.ladder and m.min_margin == 1.5}
    assert sides == {(q, r) for q in ("hidden", "mbase", "wmax", "vmax_col", "wo_l1") for r in ("default", "float64")} | {("bias", "default")}
    # the biases' outer members are the +-7e4 the finding names (1.17 past the limit)
    assert {m.name for m in F.MEMBERS if m.ladder == "bias" and "float64" in m.shapes.values()} == {"pf-rowbias+7e4", "pf-colbias-7e4"}
    assert sum(m.nonfinite for m in F.MEMBERS) == 4


def test_f16_bounds_reproduces_the_shipped_checkpoints_figures(weights):
    """pf_lib.hip: "The five shipped checkpoints sit at 61 / 196 / 30 (P = 19,900 gives 37,600)"."""
    b = [F.f16_bounds(weights(ck).tensors) for ck in CKPTS]
    hidden, mbase, vmax = (max(x[k] for x in b) for k in ("hidden", "mbase64", "vmax_col"))
    print(f"shipped: hidden {hidden:.2f}, M_base {mbase / 64:.2f}, column |v| {vmax:.2f}, wmax {max(x['wmax'] for x in b):.2f}")
    assert 61.0 <= hidden < 62.0 and 195.5 <= mbase / 64.0 < 196.5 and 30.0 <= vmax < 30.5
    assert 37_500 <= 19_900 * vmax / 16.0 <= 37_700
    assert all(x["finite"] and F.predicted_ok(x, 19_900) for x in b)


def test_f16_bounds_sees_what_std_max_does_not(weights):
    t = {k: v.copy() for k, v in weights("pf").tensors.items()}
    t["attention_blocks.1.col_attention.out_proj.bias"][9] = np.nan
    b = F.f16_bounds(t)
    assert not b["finite"] and np.isnan(b["bias"]) and not F.predicted_ok(b, 1)


# ---- a planted fault: one operand of a k = -6 member without its lo limb -----------------------------------------------

def _stand_in(w, idx, nb=6):
    """The float32 oracle in the device's place (tests/test_tap_check_host.py::case), for any checkpoint."""
    B, N, L = idx.shape
    P = N * (N - 1) // 2
    t = {f"x{k}": np.empty((B, P, L, 64), np.float32) for k in range(nb + 1)}
    t.update({f"srow{k}": np.empty((B, P, 72), np.float32) for k in range(nb)})
    t.update({f"mrow{k}": np.empty((B, P, 4, 64), np.float32) for k in range(nb)})
    t.update({f"ctx{k}": np.empty((B, L, 64), np.float32) for k in range(nb)})
    dist = np.empty((B, P), np.float32)
    for b in range(B):
        act = {}
        dist[b] = O.forward(w, idx[b], dtype=np.float32, tap=lambda name, a: act.__setitem__(name, np.array(a)))
        t["x0"][b] = act["embed"]
        for k in range(nb):
            srow = devmath.expected_srow(w, k, act["embed"] if k == 0 else act[f"block{k - 1}.ffn"])[0]
            t[f"srow{k}"][b] = srow
            t[f"mrow{k}"][b] = devmath.expected_mrow(w, k, srow, L)[:, :4]
            t[f"ctx{k}"][b] = devmath.expected_ctx(w, k, act[f"block{k}.row"])[0]
            t[f"x{k + 1}"][b] = act[f"block{k}.ffn"]
    return t, dist


def _hi_limb_only(w, name, gamma):
    """The tensors with the folded matrix ``w[name] * gamma`` rounded to its fp16 hi limb (the lo limb dropped)."""
    t = dict(w)
    folded = t[name].astype(np.float64) * gamma.astype(np.float64)[None, :]
    t[name] = (folded.astype(np.float16).astype(np.float64) / gamma.astype(np.float64)[None, :])
    return t


@pytest.mark.parametrize("name,kind,block,buffer", [("pf-row-6-blk0", "row", 0, "srow0"), ("pf-col-6", "col", 3, "ctx3")])
def test_a_dropped_lo_limb_fails_on_a_k_minus_6_member_and_is_named(weights, name, kind, block, buffer):
    """The folded v projection of one block (row: read by the k_main in front for srow; column: by k_colstats for ctx)
    as its fp16 hi limb alone - 11 significant bits where the two limbs carry 22.  Everything else is the float32
    oracle's.  The member's own bounds (test_gpu_ckpt_family.bounds_for) must fail it, the planted buffer first."""
    m = next(x for x in F.MEMBERS if x.name == name)
    w = m.make(weights(m.base)).tensors
    idx = shape("12x40_b2")
    orc = [tap_check.oracle_taps(w, a) for a in idx]
    t, dist = _stand_in(w, idx)
    rep = tap_check.check_taps(w, idx, t, dist, bounds_for(m), oracle=orc, must_pass=False)
    assert not rep.failures, rep.message()
    p = f"attention_blocks.{block}."
    wf = _hi_limb_only(w, p + f"{kind}_attention.v_proj.weight", w[p + f"{kind}_norm.weight"])
    L = idx.shape[2]
    for b in range(idx.shape[0]):
        if kind == "row":
            t[buffer][b] = devmath.expected_srow(wf, block, t[f"x{block}"][b])[0]
        else:
            x_row = devmath.expected_x_row(w, block, t[f"x{block}"][b], t[f"mrow{block}"][b])
            t[buffer][b] = devmath.expected_ctx(wf, block, x_row)[0]
    rep = tap_check.check_taps(w, idx, t, dist, bounds_for(m), oracle=orc, must_pass=False)
    assert rep.local_failures(), "the dropped limb passed"
    first = rep.local_failures()[0]
    print(f"{name}: {first}")
    assert (first.buffer, first.block) == (buffer, block), rep.message()
    with pytest.raises(AssertionError):
        tap_check.check_taps(w, idx, t, dist, bounds_for(m), oracle=orc)
