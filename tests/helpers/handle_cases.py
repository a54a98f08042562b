"""The calls that share a handle's grow-only device buffers, at a small shape, a larger one and the small one again
(``tests/test_gpu_handle_buffers.py``): every host entry point whose staging or workspace is carved from one of them."""
import numpy as np

# (B, N, L, R, (tiled N, tiled M)) of the three visits: the buffers grow at the second and are reused, too large, at the third
VISITS = ((1, 4, 8, 2, (9, 4)), (2, 9, 40, 5, (5, 2)), (1, 4, 8, 2, (9, 4)))
NAMES = ("forward", "forward_weighted", "forward_site_profile", "forward_leave_one_out", "forward_place", "forward_tiled",
         "nj_joins", "bionj_joins", "bme_nni", "bme_spr", "join_supports", "join_transfers", "join_consensus")


def random_tables(rng, shape, n: int) -> np.ndarray:
    """``int32 shape + [T]``: valid join tables of random joins (no distances behind them)."""
    out = np.zeros(tuple(shape) + (2 * (n - 3) + 3,), dtype=np.int32)
    for row in out.reshape(-1, out.shape[-1]):
        alive = list(range(n))
        for t in range(n - 3):
            i, j = sorted(rng.choice(len(alive), size=2, replace=False).tolist())
            row[2 * t], row[2 * t + 1] = alive[i], alive[j]
            alive.pop(j)
        row[2 * (n - 3):] = alive
    return out


def calls(visit: int):
    """``{name: f(engine) -> tuple of arrays}`` of visit 0, 1 or 2; the inputs depend on the visit's shape alone."""
    B, N, L, R, (TN, TM) = VISITS[visit]
    rng = np.random.default_rng(1000 * N + L)
    idx = rng.integers(0, 20, size=(B, N, L), dtype=np.uint8)
    w = rng.integers(0, 4, size=(B, L)).astype(np.float32)
    w[:, 0] = 1.0
    big = rng.integers(0, 20, size=(B, TN, L), dtype=np.uint8)
    preds = rng.uniform(0.01, 3.0, size=(B, N * (N - 1) // 2)).astype(np.float32)
    start = random_tables(rng, (B,), N)
    ref, rep = random_tables(rng, (B,), N), random_tables(rng, (B, R), N)
    rep_lengths = rng.uniform(0.01, 1.0, size=rep.shape)
    tup = lambda x: x if isinstance(x, tuple) else (x,)
    return {
        "forward": lambda e: tup(e.forward(idx)),
        "forward_weighted": lambda e: tup(e.forward_weighted(idx, w)),
        "forward_site_profile": lambda e: tup(e.forward_site_profile(idx)),
        "forward_leave_one_out": lambda e: tup(e.forward_leave_one_out(idx, keep_loo=True)),
        "forward_place": lambda e: tup(e.forward_place(idx, 1, keep_sets=True)),
        "forward_tiled": lambda e: tup(e.forward_tiled(big, TM)),
        "nj_joins": lambda e: tup(e.nj_joins(preds)),
        "bionj_joins": lambda e: tup(e.bionj_joins(preds)),
        "bme_nni": lambda e: tup(e.bme_nni(preds, start)),
        "bme_spr": lambda e: tup(e.bme_spr(preds, start)),
        "join_supports": lambda e: tup(e.join_supports(ref, rep)),
        "join_transfers": lambda e: tup(e.join_transfers(ref, rep, branch_moves=True)),
        "join_consensus": lambda e: tup(e.join_consensus(rep, rep_lengths)),
    }


def same_bytes(got, want) -> bool:
    return len(got) == len(want) and all(
        g.shape == w.shape and g.dtype == w.dtype and np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes()
        for g, w in zip(map(np.asarray, got), map(np.asarray, want)))
