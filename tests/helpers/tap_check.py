"""Every buffer the default forward leaves behind under ``debug_keep`` 1, per token, against float64.

``check_taps`` runs two comparisons per alignment and per block k, everything in float64:

  * chain: every tap against the float64 oracle's own forward - ``embed`` and ``block{k}.ffn`` for the x taps, ``devmath``'s
    expected_srow / expected_mrow / expected_ctx fed with the oracle's activations for the others.  The error of the blocks
    in front adds up in it; its bounds are the project's per-buffer caps (CHAIN_CAPS).
  * kernel-local: every tap against what float64 makes of the DEVICE's own upstream taps - srow{k} from the device's x{k},
    mrow{k} from its srow{k}, ctx{k} from x{k} with the device's mrow{k} applied, x{k+1} from that and the device's ctx{k},
    the distances from the device's last x.  A kernel is judged on its own arithmetic; a wrong token shows at full size in
    the one buffer it was written to.

The measure of both is the largest absolute error of a buffer (one alignment's) over its largest expected entry; srow's
two parts, S_kv and S_q | S_k, each over their own.  x0 is a
gather and one fp32 addition: bit-exact.  A failure names comparison, buffer, block, alignment, pair, site and channel of
the worst element, and how k_main's tiles and k_colstats' site chunks meet that token.
"""
import numpy as np

import devmath
from oracle import pf_oracle as O

KINDS = ("srow", "mrow", "ctx", "x")
# the bounds of tests/test_gpu_parity.py::test_tiny_taps_localise_every_kernel, shares of the largest reference entry
CHAIN_CAPS = {"srow": 1e-4, "mrow": 1e-4, "ctx": 3e-4, "x": 1e-4}
KERNEL = {"srow": "k_embed, or the k_main in front + k_rowsum", "mrow": "k_rowfin", "ctx": "k_colstats + k_colfin",
          "x": "k_main", "dist": "k_main's head + k_outsum", "x0": "k_embed"}


def flat_tiling(P, L, force=-1):
    """pf_host_prep.h, tile_plan_core: does k_main cut P x L tokens into tiles of 32 consecutive tokens (flat) or give
    every row its own tiles?  force: 0 = PF_ROW_TILES, 1 = PF_FLAT_TILES, -1 = from the shape.  (Only the wording of a
    failure depends on this copy of the rule.)"""
    ntiles = (L + 31) // 32
    waste, straddle = (ntiles * 32 - L) / (ntiles * 32), 0.10 * 32.0 / max(L, 1)
    flat = L >= 32 and waste > straddle and force != 0
    if force == 1 and L >= 32 and L % 32:
        flat = True
    return bool(flat)


def token_class(p, l, P, L, flat):
    """Where token (pair p, site l) stands in k_main's tiling and k_colstats' chunks of 32 sites, in words."""
    out = []
    if flat:
        t = (p * L + l) // 32
        lo, hi = 32 * t, min(32 * t + 32, P * L) - 1
        if t == (p * L + L - 1) // 32:
            out.append("in its row's last tile")
        if lo // L != hi // L:
            out.append("in a tile that covers two rows")
        if hi - lo + 1 < 32:
            out.append("in the alignment's short last tile")
    elif l >= 32 * ((L + 31) // 32 - 1):
        out.append("in its row's last tile" + (" (ragged)" if L % 32 else ""))
    if l >= 32 * ((L + 31) // 32 - 1):
        out.append("in the last site chunk" + (f" ({L - 32 * ((L - 1) // 32)} sites)" if L % 32 else ""))
    return ", ".join(out) if out else "in the interior of its row (no tile or chunk edge)"


def oracle_taps(w, idx, n_blocks=6):
    """The float64 oracle's activations of one alignment uint8[N, L]: embed, block{k}.row, block{k}.ffn, dist."""
    keep = {}

    def tap(name, a):
        if name == "embed" or name == "dist" or name.endswith(".row") or name.endswith(".ffn"):
            keep[name] = np.array(a, np.float64)
    O.forward(w, idx, dtype=np.float64, tap=tap, n_blocks=n_blocks)
    return keep


def embed_fp32(w, idx):
    """x0 as the device forms it: the float32 table's rows of both sequences of a pair, one fp32 addition."""
    e = O.embedding_table(w, np.dtype(np.float32))[idx]
    pi, pj = O.pair_index(idx.shape[0])
    return e[pi] + e[pj]


class Finding:
    def __init__(self, comparison, kind, buffer, block, aln, err, bound, where):
        self.comparison, self.kind, self.buffer, self.block, self.aln = comparison, kind, buffer, block, aln
        self.err, self.bound, self.where = err, bound, where

    def __str__(self):
        kernel = KERNEL[self.kind]
        if self.kind == "srow":
            kernel = "k_embed" if self.block == 0 else f"block {self.block - 1}'s k_main + k_rowsum"
        return (f"{self.comparison}: {self.buffer} (block {self.block}, {kernel}) of alignment {self.aln}: "
                f"error {self.err:.3e} of the largest entry, bound {self.bound:.3e}; worst at {self.where}")


class Report:
    """errors[(comparison, kind)]: the worst measure over alignments and blocks; buffers[(comparison, buffer, aln)]: each
    buffer's; failures: what crossed its bound, in the order the forward writes the buffers."""
    def __init__(self):
        self.errors, self.buffers, self.failures = {}, {}, []

    def local_failures(self):
        return [f for f in self.failures if f.comparison == "kernel-local"]

    def message(self):
        head = f"{len(self.failures)} buffer(s) over their bounds; the first kernel-local one is where to look:\n"
        return head + "\n".join(str(f) for f in self.local_failures() + [f for f in self.failures if f.comparison == "chain"])


def _where(kind, flatidx, shape, P, L, flat, got, want):
    pos = np.unravel_index(int(flatidx), shape)
    vals = f": got {got.reshape(-1)[flatidx]:.9g}, want {want.reshape(-1)[flatidx]:.9g}"
    if kind in ("x", "x0"):
        p, l, c = (int(v) for v in pos)
        return f"pair {p}, site {l}, channel {c}{vals}; the token lies {token_class(p, l, P, L, flat)}"
    if kind == "ctx":
        l, c = (int(v) for v in pos)
        chunk = "in the last site chunk" if l >= 32 * ((L + 31) // 32 - 1) else "not in the last site chunk"
        return f"site {l}, channel {c} (head {c // 16}){vals}; the site lies {chunk}"
    if kind == "srow":
        p, c = (int(v) for v in pos)
        part = f"S_kv head {c // 16} dim {c % 16}" if c < 64 else f"S_q head {c - 64}" if c < 68 else f"S_k head {c - 68}"
        return f"pair {p}, entry {c} ({part}){vals}"
    if kind == "mrow":
        p, h, c = (int(v) for v in pos)
        return f"pair {p}, head {h}, channel {c}{vals}"
    return f"pair {int(pos[0])}{vals}"


def check_taps(w, idx, taps, dist, bounds, *, flat=None, oracle=None, n_blocks=6, head_only=False, must_pass=True):
    """w: the checkpoint's tensors; idx uint8[B, N, L]; taps: name -> the tap of the whole batch (``Engine.debug_read``);
    dist [B, P]; bounds: {"chain": {srow, mrow, ctx, x}, "kernel-local": {srow, mrow, ctx, x, dist}}.  flat: the tiling the
    run used (None: the shape's own, pf_host_prep.h); oracle: ``oracle_taps`` per alignment, if the caller keeps them;
    head_only: only the distances against the device's last x.  Returns the Report; raises AssertionError with its message
    when a buffer crossed its bound, unless must_pass is False."""
    idx = np.asarray(idx)
    B, N, L = idx.shape
    P = N * (N - 1) // 2
    flat = flat_tiling(P, L) if flat is None else bool(flat)
    rep = Report()
    t = {n: np.asarray(a) for n, a in taps.items()}
    x = {k: t[f"x{k}"].reshape(B, P, L, 64) for k in (range(n_blocks + 1) if not head_only else [n_blocks])}
    dist = np.asarray(dist, np.float64).reshape(B, P)

    def judge(comparison, kind, buffer, block, b, got, want):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, (buffer, got.shape, want.shape)
        diff = np.abs(got - want)
        diff[~np.isfinite(diff)] = np.inf                        # a NaN is the worst element, not an ignored one
        # srow holds two quantities of unrelated size, S_kv and S_q | S_k: each is measured against its own largest entry
        # (a checkpoint with a small v_proj would otherwise hide any error of S_kv behind S_q)
        parts = (np.s_[:, :64], np.s_[:, 64:]) if kind == "srow" else (np.s_[...],)
        rel = np.zeros_like(diff)
        for part in parts:
            scale = float(np.abs(want[part]).max())
            # (a buffer that is exactly zero - a zeroed v_proj - has no largest entry to measure against: any difference fails)
            with np.errstate(invalid="ignore", divide="ignore"):
                rel[part] = diff[part] / scale if scale > 0 else np.where(diff[part] == 0, 0.0, np.inf)
        worst = int(rel.argmax())
        err = float(rel.reshape(-1)[worst])
        rep.buffers[comparison, buffer, b] = err
        rep.errors[comparison, kind] = max(rep.errors.get((comparison, kind), 0.0), err)
        bound = bounds[comparison][kind]
        if not err <= bound:
            rep.failures.append(Finding(comparison, kind, buffer, block, b, err, bound,
                                        _where(kind, worst, want.shape, P, L, flat, got, want)))

    for b in range(B):
        if not head_only:
            orc = oracle[b] if oracle is not None else oracle_taps(w, idx[b], n_blocks)
            want0 = embed_fp32(w, idx[b])
            rep.buffers["chain", "x0", b] = float(np.abs(x[0][b].astype(np.float64) - want0).max())
            if not np.array_equal(x[0][b], want0):
                bad = int((x[0][b] != want0).reshape(-1).argmax())
                rep.failures.append(Finding("kernel-local", "x0", "x0", 0, b, rep.buffers["chain", "x0", b], 0.0,
                                            _where("x0", bad, want0.shape, P, L, flat, x[0][b], want0)))
        for k in range(0 if not head_only else n_blocks, n_blocks):
            srow = t[f"srow{k}"].reshape(B, P, 72)[b]
            mrow = t[f"mrow{k}"].reshape(B, P, 4, 64)[b]
            ctx = t[f"ctx{k}"].reshape(B, L, 64)[b]
            # chain: the oracle's activations in, the oracle's (or devmath's) buffers out
            o_in = orc["embed"] if k == 0 else orc[f"block{k - 1}.ffn"]
            o_srow = devmath.expected_srow(w, k, o_in)[0]
            # kernel-local: the device's own upstream taps in
            x_in = x[k][b].astype(np.float64)
            x_row = devmath.expected_x_row(w, k, x_in, mrow)
            for comparison, wants in (
                    ("kernel-local", (devmath.expected_srow(w, k, x_in)[0], devmath.expected_mrow(w, k, srow.astype(np.float64), L)[:, :4],
                                      devmath.expected_ctx(w, k, x_row)[0], devmath.expected_block_out(w, k, x_row, ctx))),
                    ("chain", (o_srow, devmath.expected_mrow(w, k, o_srow, L)[:, :4],
                               devmath.expected_ctx(w, k, orc[f"block{k}.row"])[0], orc[f"block{k}.ffn"]))):
                judge(comparison, "srow", f"srow{k}", k, b, srow, wants[0])
                judge(comparison, "mrow", f"mrow{k}", k, b, mrow, wants[1])
                judge(comparison, "ctx", f"ctx{k}", k, b, ctx, wants[2])
                judge(comparison, "x", f"x{k + 1}", k, b, x[k + 1][b], wants[3])
        judge("kernel-local", "dist", "distances", n_blocks - 1, b, dist[b], devmath.expected_distances(w, x[n_blocks][b]))
    # the order the forward writes: alignment by alignment is the reader's order, block by block the kernels'
    order = {"x0": -1, "srow": 0, "mrow": 1, "ctx": 2, "x": 3, "dist": 4}
    rep.failures.sort(key=lambda f: (f.block, order[f.kind], f.aln))
    if rep.failures and must_pass:
        raise AssertionError(rep.message())
    return rep
