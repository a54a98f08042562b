"""A deterministic family of (embed_dim, n_heads) = (64, 4) checkpoints beyond the five shipped ones, and a float64
statement of the guard that decides whether a checkpoint may use the default kernels' fp16 operands.

  rescaled(base, kind, k, blocks)   v_proj (weight and bias) of the row or column attention times 2^k, the same attention's
                                    out_proj.weight times 2^-k.  Linear attention is linear in v, and a power of two moves
                                    no mantissa: the float64 and the float32 oracle return the bits of the base checkpoint
                                    (tests/test_ckpt_family_host.py asserts it), so any change of the device's error under
                                    it is the kernels' own.
  foreign(seed, scale, n_blocks)    ``random_weights`` at the default architecture: another recipe altogether.
  mutated(base, edits)              named single-tensor edits: the guard ladder and the zero cases.
  f16_bounds(tensors)               the guard's quantities as pf_lib.hip documents them above ``F16Ranges``, from
                                    ``devmath._fold`` (LayerNorm gamma / beta folded into the projections), in float64.
"""
import numpy as np

import devmath
from phyloformer_amd.weights import ModelWeights, random_weights

F16_LIMIT = 60000.0                      # pf_lib.hip: 65504 with a margin for the rounding of the bounds
LO_HIDDEN, LO_VMAX_COL, LO_WO_L1 = 8192.0, 16384.0, 512.0    # the low side: what multiplies a subnormal lo limb's 2^-25
ALPHA = np.sqrt(0.5 * np.log2(np.e))     # the hidden layer is carried as alpha * h (W1', b1' times alpha; W2 / alpha / 2)
COLAPPLY_A_SCALE = 16.0                  # the column out_proj carries 2^4, q' (x) ctx 2^-4
ROWMIX_A_MAX = 64.0                      # k_rowfin's a_scale at most


def n_blocks_of(tensors):
    n = 0
    while f"attention_blocks.{n}.ffn.0.weight" in tensors:
        n += 1
    return n


def _copy(base):
    return {k: np.array(v, np.float32) for k, v in base.tensors.items()}


def rescaled(base, kind, k, blocks=None):
    """kind: "row" or "col"; blocks: the blocks to rescale (None: all).  The power of two is applied in float32."""
    assert kind in ("row", "col")
    t = _copy(base)
    f = np.float32(2.0) ** np.float32(k)
    assert np.isfinite(f) and f > 0 and np.float32(1) / f * f == 1
    for b in (range(base.n_blocks) if blocks is None else blocks):
        p = f"attention_blocks.{b}.{kind}_attention."
        t[p + "v_proj.weight"] = t[p + "v_proj.weight"] * f
        t[p + "v_proj.bias"] = t[p + "v_proj.bias"] * f
        t[p + "out_proj.weight"] = t[p + "out_proj.weight"] / f
    return ModelWeights(base.n_blocks, base.n_heads, base.embed_dim, t)


def foreign(seed, scale, n_blocks):
    return random_weights(seed, n_blocks=n_blocks, n_heads=4, embed_dim=64, scale=scale)


def mutated(base, edits):
    """edits: [(tensor name, op, argument)], op one of
         "scale"  the whole tensor times the argument,
         "scale_row"  argument = (row, factor): one row of a matrix,
         "set"    argument = (flat index, value): one entry,
         "zero"   the whole tensor zero (argument None), or argument = a flat index: that entry zero."""
    t = _copy(base)
    for name, op, arg in edits:
        a = t[name]
        if op == "scale":
            t[name] = (a * np.float32(arg)).astype(np.float32)
        elif op == "scale_row":
            a[arg[0]] = (a[arg[0]] * np.float32(arg[1])).astype(np.float32)
        elif op == "set":
            a.reshape(-1)[arg[0]] = np.float32(arg[1])
        elif op == "zero":
            if arg is None:
                a[...] = 0
            else:
                a.reshape(-1)[arg] = 0
        else:
            raise ValueError(op)
    return ModelWeights(base.n_blocks, base.n_heads, base.embed_dim, t)


def f16_bounds(tensors):
    """{hidden, mbase64, vmax_col, wmax, bias, wo_l1, finite}: what must stay below F16_LIMIT for the fp16 operands
    (vmax_col per shape: P * vmax_col / 16), and on the low side hidden, vmax_col and wo_l1 - the largest sum of
    |entries| of an out_proj row - below LO_HIDDEN, LO_VMAX_COL and LO_WO_L1.  LayerNorm without affine gives |x~| <= sqrt(63), ||x~||_2 <= 8, hence for a folded
    projection W', b':  |W' x~ + b'| <= ||W' row||_2 * 8 + |b'|.  np.max keeps a NaN, so a NaN shows in the figures."""
    w = {k: np.asarray(v, np.float64) for k, v in tensors.items()}
    out = dict(hidden=0.0, mbase64=0.0, vmax_col=0.0, wmax=0.0, bias=0.0, wo_l1=0.0)

    def up(key, v):
        out[key] = float(np.max([out[key], np.max(np.abs(v))]))

    with np.errstate(all="ignore"):
        for b in range(n_blocks_of(w)):
            p = f"attention_blocks.{b}."
            for kind in ("row", "col"):
                f = devmath._fold(w, p, kind)
                Wv, bv = f["v"]
                vmax = np.sqrt((Wv * Wv).sum(1)) * 8.0 + np.abs(bv)                  # [64 = (head, dim)]
                Wo = w[p + f"{kind}_attention.out_proj.weight"]
                up("wmax", Wv)
                up("bias", w[p + f"{kind}_attention.out_proj.bias"])
                up("wo_l1", np.abs(Wo).sum(1))                                       # what multiplies the error of v
                if kind == "row":
                    up("wmax", Wo)
                    up("wmax", f["q"][0])
                    up("wmax", f["k"][0])
                    # M_base[h][c] = sum_d Wo[c][16 h + d] * ctx[16 h + d], ctx a k'-weighted mean of v
                    up("mbase64", ROWMIX_A_MAX * (np.abs(Wo).reshape(64, 4, 16) * vmax.reshape(1, 4, 16)).sum(2))
                else:
                    up("wmax", Wo * COLAPPLY_A_SCALE)
                    up("vmax_col", vmax)
            g, beta = w[p + "ffn_norm.weight"], w[p + "ffn_norm.bias"]
            W1 = w[p + "ffn.0.weight"]
            W1f, b1f = ALPHA * W1 * g[None, :], ALPHA * (w[p + "ffn.0.bias"] + W1 @ beta)
            up("hidden", 2.0 * (np.sqrt((W1f * W1f).sum(1)) * 8.0 + np.abs(b1f)))       # gelu_scaled returns at most 2 |x|
            up("wmax", W1f)
            up("wmax", w[p + "ffn.3.weight"] / ALPHA * 0.5)
    out["finite"] = bool(all(np.isfinite(v).all() for v in w.values()))
    return out


def _shares(bounds, P):
    """Every guarded figure over its limit."""
    return [bounds["hidden"] / LO_HIDDEN, bounds["mbase64"] / F16_LIMIT, bounds["wmax"] / F16_LIMIT, bounds["bias"] / F16_LIMIT,
            P * bounds["vmax_col"] / COLAPPLY_A_SCALE / F16_LIMIT, bounds["vmax_col"] / LO_VMAX_COL, bounds["wo_l1"] / LO_WO_L1]


def predicted_ok(bounds, P):
    """The verdict the library must reach for alignments of P pairs: True = the default kernels may run."""
    return bool(bounds["finite"] and all(np.isfinite(v) and v < 1.0 for v in _shares(bounds, P)))


def margin(bounds, P):
    """How far the verdict is from flipping, as a factor on the figure nearest to (inside) or furthest past (outside) its
    limit.  inf for a non-finite checkpoint."""
    shares = _shares(bounds, P)
    if not bounds["finite"] or not all(np.isfinite(v) for v in shares):
        return float("inf")
    return 1.0 / max(max(shares), 1e-300) if max(shares) < 1.0 else max(shares)


# ---- the members the tests run (tests/test_ckpt_family_host.py proves what each claims, tests/test_gpu_ckpt_family.py runs them)

def shapes():
    """name -> builder of uint8[B, N, L]: edge shapes of tests/test_gpu_taps.py (each at most 10,000 tokens)."""
    from phyloformer_amd.msa_sim import simulate_batch
    import test_gpu_taps
    return {
        "6x63": lambda: simulate_batch(1, 6, 63, seed=53),           # row tiling, ragged tile
        "9x65": lambda: simulate_batch(1, 9, 65, seed=43),           # flat tiling, tiles over two rows
        "12x40_b2": lambda: simulate_batch(2, 12, 40, seed=43),      # two pair groups, short last run; P = 66
        "2x45_b2": lambda: simulate_batch(2, 2, 45, seed=44),        # P = 1
        "18x40": lambda: simulate_batch(1, 18, 40, seed=45),         # P = 153: where the column |v| decides by shape
        "13x100_gapped": test_gpu_taps._gapped_with_x,               # pf_indel, gaps and X
    }


class Member:
    """name; base: the shipped checkpoint it is made from (None: foreign); make(base weights) -> ModelWeights;
    shapes: {shape name: "default" | "float64"}, the kernels the guard must choose (precise = 0);
    exact: an exact invariance of base (the oracle's bits do not move); bounds: "shipped" = test_gpu_taps.BOUNDS unchanged,
    "measured" = the member's own row in MEASURED of tests/test_gpu_ckpt_family.py; ladder: the guarded quantity the
    member stands just inside or just outside of; min_margin: how far f16_bounds must keep the verdict from F16_LIMIT;
    nonfinite: the checkpoint holds an inf or a NaN."""
    def __init__(self, name, base, make, shapes, *, exact=False, bounds="shipped", ladder=None, min_margin=1.5, nonfinite=False):
        self.name, self.base, self.make, self.shapes = name, base, make, dict(shapes)
        self.exact, self.bounds, self.ladder, self.min_margin, self.nonfinite = exact, bounds, ladder, min_margin, nonfinite


def _members():
    out = []
    three = ("6x63", "9x65", "12x40_b2")
    on = lambda names, route="default": {n: route for n in names}
    for seed, scale, nb in ((1, 1.0, 6), (2, 2.0, 6), (3, 2.0, 2)):
        out.append(Member(f"foreign-s{seed}-x{scale:g}-b{nb}", None, (lambda _b, a=(seed, scale, nb): foreign(*a)), on(three)))

    def resc(kind, k, blocks=None, base="pf", shapes=None, **kw):
        tag = "" if blocks is None else "-blk" + "".join(str(b) for b in blocks)
        kw.setdefault("bounds", "shipped" if abs(k) <= 3 else "measured")
        out.append(Member(f"{base}-{kind}{k:+d}{tag}", base, (lambda b: rescaled(b, kind, k, blocks)),
                          shapes or on(["12x40_b2"]), exact=True, **kw))
    f64 = lambda names: on(names, "float64")
    for kind in ("row", "col"):
        for k in (-3, 3):
            resc(kind, k)
        resc(kind, 6, shapes=on(three))
        resc(kind, 6, blocks=[0])
        resc(kind, 6, blocks=[5])
        # the low side, out_proj row sums (512): 2^-4 leaves 307 / 303 (1.67 inside), 2^-6 1228 / 1214 (2.4 outside) - measured
        # before that limit existed: column 2^-6 6.3e-5 from the fp32 oracle and past the chain caps at 9x65 and 12x40
        resc(kind, -4, ladder="wo_l1")
        resc(kind, -6, shapes=f64(three), ladder="wo_l1")
        resc(kind, -6, blocks=[5], shapes=f64(["12x40_b2"]))
    resc("row", -6, blocks=[0])                               # block 0's row out_proj is small: 291, inside
    resc("col", -6, blocks=[0], shapes=f64(["12x40_b2"]))     # 800
    resc("row", -12, shapes=f64(["12x40_b2"]))                # (2.4e-4 from the fp32 oracle on the default kernels)
    resc("row", 10)
    resc("col", -12, shapes=f64(["12x40_b2"]))
    # the column |v|: 2^9 gives 9,665 - inside its own limit of 16,384 (1.69) and inside by shape at P = 1, outside by shape
    # at P = 153 (153 * 9,665 / 16 = 92,400: 1.54 past); 2^11 gives 38,670 (2.36 past 16,384 at any shape).  2^10, 19,330,
    # is outside at 12x40 by shape (79,700: 1.33) and at P = 1 by the limit (1.18) - nearer than 1.5, the figure of an
    # exact power of two times a bound that is 1e-7 from the library's
    resc("col", 9, shapes={"18x40": "float64", "2x45_b2": "default"}, ladder="vmax_col")
    resc("col", 11, shapes=f64(["12x40_b2", "2x45_b2"]), ladder="vmax_col")
    resc("col", 10, shapes=f64(["12x40_b2", "2x45_b2"]), ladder="vmax_col", min_margin=1.15)
    resc("col", -6, base="pf_indel", shapes=f64(["13x100_gapped"]))
    resc("col", 3, base="pf_indel", shapes=on(["13x100_gapped"]))
    # wmax, row v_proj: max |Wv'| = 1.277, so 2^15 gives 41,850 (1.43 inside) and 2^16 83,700 (1.39 outside) - two
    # neighbouring powers of two cannot both stand 1.5 away; 2^14 (2.87 inside) and 2^17 (2.79 outside) do
    resc("row", 14, ladder="wmax")
    resc("row", 17, shapes=f64(["12x40_b2"]), ladder="wmax")
    resc("row", 15, ladder="wmax", min_margin=1.3)
    resc("row", 16, shapes=f64(["12x40_b2"]), ladder="wmax", min_margin=1.3)

    p = "attention_blocks.2."

    def mut(name, edits, route, base="pf", **kw):
        out.append(Member(name, base, (lambda b: mutated(b, edits)), on(["12x40_b2"], route), **kw))
    # hidden: block 2's W1 times s, W2 over s (tests/test_gpu_precise.py's edit): 2 alpha |W1' x~ + b1'| <= 4,150 / 12,980
    # against the low side's 8,192 (at s = 900, 29,200 - inside the fp16 range - k_main's x was 2.6e-5 off, seven times
    # the shipped bound)
    for s, route in ((128.0, "default"), (400.0, "float64")):
        mut(f"pf-hidden-x{s:g}", [(p + "ffn.0.weight", "scale", s), (p + "ffn.3.weight", "scale", 1.0 / s)], route,
            ladder="hidden", bounds="measured")
    # row-mix base: ONE output channel (row 0) of block 2's row out_proj times 12 / 32 - 35,800 / 95,500.  (The whole
    # matrix times 4 drives the distances to 14.6, past the 8 the default kernels are judged up to.)
    for f, route in ((12.0, "default"), (32.0, "float64")):
        mut(f"pf-mbase-x{f:g}", [(p + "row_attention.out_proj.weight", "scale_row", (0, f))], route, ladder="mbase", bounds="measured")
    # out_proj biases, one channel: -3e4 inside (+3e4 gives distances of 25: past 8), +-7e4 outside (7e4 / 6e4 = 1.17; the
    # figure is the entry itself)
    mut("pf-rowbias-3e4", [(p + "row_attention.out_proj.bias", "set", (5, -3e4))], "default", ladder="bias", bounds="measured")
    mut("pf-colbias-3e4", [(p + "col_attention.out_proj.bias", "set", (5, -3e4))], "default", ladder="bias", bounds="measured")
    mut("pf-rowbias+7e4", [(p + "row_attention.out_proj.bias", "set", (5, 7e4))], "float64", ladder="bias", min_margin=1.15)
    mut("pf-colbias-7e4", [(p + "col_attention.out_proj.bias", "set", (5, -7e4))], "float64", ladder="bias", min_margin=1.15)
    mut("pf-rowbias-inf", [(p + "row_attention.out_proj.bias", "set", (3, np.inf))], "float64", nonfinite=True)
    mut("pf-colbias-nan", [(p + "col_attention.out_proj.bias", "set", (3, np.nan))], "float64", nonfinite=True)
    mut("pf-colwv-inf", [(p + "col_attention.v_proj.weight", "set", (100, np.inf))], "float64", nonfinite=True)
    mut("pf-w2-nan", [(p + "ffn.3.weight", "set", (100, np.nan))], "float64", nonfinite=True)
    # zeros
    for kind in ("row", "col"):
        mut(f"pf-zero-{kind}-v", [(p + f"{kind}_attention.v_proj.weight", "zero", None), (p + f"{kind}_attention.v_proj.bias", "zero", None)], "default")
    mut("pf-zero-w2", [(p + "ffn.3.weight", "zero", None)], "default")
    mut("pf-zero-head", [("pwFNN.0.weight", "zero", None)], "default")
    mut("pf-zero-ffn-norm-channel", [(p + "ffn_norm.weight", "zero", 7)], "default")
    assert len({m.name for m in out}) == len(out)
    return out


MEMBERS = _members()
CASES = [(m, s) for m in MEMBERS for s in m.shapes]


def case_id(case):
    return f"{case[0].name}@{case[1]}"
