"""-m gpu: the last block's FFN output projection folded into the softplus head (k_main<MODE_LAST_FOLD>, option
"head_fold", default 1) against the full last FFN (head_fold = 0, k_main<MODE_LAST>): the same distances up to fp32
rounding, inside the golden bounds, with the result-bit invariances of the unfolded kernel (batch, tiling, entry point)."""
import os

import numpy as np
import pytest

from phyloformer_amd.msa_sim import simulate_batch

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the golden bound of tests/test_gpu_parity.py
FOLD_REL = 5e-7     # folded vs unfolded, relative to the largest distance


@pytest.fixture(scope="module")
def pair(weights):
    """(folded, unfolded) engines per checkpoint, both on the default (split-fp16) kernels for every shape."""
    from phyloformer_amd.engine import Engine
    cache = {}

    def get(ck):
        if ck not in cache:
            es = []
            for fold in (1, 0):
                e = Engine(weights(ck), 0)
                e.set_option("precise", 0)
                e.set_option("head_fold", fold)
                es.append(e)
            cache[ck] = tuple(es)
        return cache[ck]
    yield get
    for es in cache.values():
        for e in es:
            e.close()


def _cases(golden, repo):
    c = golden("configs.npz")
    out = [("configs[1] 20x200 x3", "pf", c["c2_idx"], c["c2_dist"]),
           ("configs[2] 60x500", "pf", c["c3_idx"], c["c3_dist"])]
    path = os.path.join(repo, "tests/golden/configs_big.npz")
    if os.path.exists(path):
        b = np.load(path)
        out += [("configs[3] 60x2000", "pf", b["c4_idx"], b["c4_dist"]),
                ("configs[4] 200x500 gapped", "pf_indel", b["c5_idx"], b["c5_dist"])]
    m = golden("configs_more.npz")
    out.append(("60x500 gapped", "pf_indel", m["c3g_idx"], m["c3g_dist"]))
    return out


def test_folded_head_equals_full_ffn_within_goldens(pair, golden, repo):
    for name, ck, idx, want in _cases(golden, repo):
        ef, eu = pair(ck)
        got_f, got_u = ef.forward(idx), eu.forward(idx)
        rel = float(np.abs(got_f - got_u).max() / np.abs(got_u).max())
        err_f, err_u = float(np.abs(got_f - want).max()), float(np.abs(got_u - want).max())
        print(f"head_fold {name} ({ck}): folded vs full {rel:.2e} relative; vs golden {err_f:.3e} folded, "
              f"{err_u:.3e} full")
        assert rel <= FOLD_REL, (name, rel)
        assert err_f <= TOL and err_u <= TOL, (name, err_f, err_u)


def test_folded_head_batch_invariant(pair, golden):
    ef, _ = pair("pf")
    a = golden("configs.npz")["c2_idx"]
    batch3 = ef.forward(a)
    single = np.stack([ef.forward(x) for x in a])
    assert np.array_equal(batch3, single)
    b16 = ef.forward(np.concatenate([a] * 6)[:16])
    for k in range(16):
        assert np.array_equal(b16[k], batch3[k % 3]), k


def test_folded_head_flat_vs_row_tiling(weights, golden):
    from phyloformer_amd.engine import Engine
    cases = [simulate_batch(3, 7, 33, seed=41), simulate_batch(1, 14, 97, seed=45, gaps=True),
             golden("configs.npz")["c2_idx"]]
    for idx in cases:
        out = {}
        for row_tiles in (0, 1):
            os.environ["PF_ROW_TILES" if row_tiles else "PF_FLAT_TILES"] = "1"
            try:
                with Engine(weights("pf"), 0) as e:
                    e.set_option("precise", 0)
                    e.set_option("head_fold", 1)
                    out[row_tiles] = e.forward(idx)
                    assert np.array_equal(np.stack([e.forward(x) for x in idx]), out[row_tiles])
            finally:
                os.environ.pop("PF_ROW_TILES", None)
                os.environ.pop("PF_FLAT_TILES", None)
        err = np.abs(out[0] - out[1]).max()
        assert err <= 2e-5 * max(1.0, float(np.abs(out[1]).max())), (idx.shape, err)


def test_debug_keep_taps_x6_and_keeps_the_folded_distances(weights, golden):
    """The folded head never forms x6: with debug_keep the full last FFN runs as well, for the tap only.  The
    distances stay the folded ones, and the tap is the full FFN's x6, as with head_fold = 0."""
    from phyloformer_amd.engine import Engine
    a = golden("configs.npz")["c2_idx"]
    B, n, L = a.shape
    x6, dist = {}, {}
    for fold in (0, 1):
        with Engine(weights("pf"), 0) as e:
            e.set_option("precise", 0)
            e.set_option("head_fold", fold)
            plain = e.forward(a)
            e.set_option("debug_keep", 1)
            dist[fold] = e.forward(a)
            x6[fold] = e.debug_read("x6")
            assert np.array_equal(dist[fold], plain), fold
    assert x6[1].size == B * (n * (n - 1) // 2) * L * 64 and np.isfinite(x6[1]).all()
    assert np.array_equal(x6[0], x6[1])
    assert np.abs(dist[1] - dist[0]).max() <= FOLD_REL * np.abs(dist[0]).max()


def test_folded_head_same_bits_on_every_entry_point(pair, golden):
    ef, _ = pair("pf")
    a = golden("configs.npz")["c2_idx"]
    B, n, L = a.shape
    want = ef.forward(a)
    d_idx, d_out = ef.malloc(a.nbytes), ef.malloc(B * (n * (n - 1) // 2) * 4)
    try:
        ef.h2d(d_idx, np.ascontiguousarray(a))
        ef.forward_device(d_idx, B, n, L, d_out)
        dev = np.empty_like(want)
        ef.d2h(dev, d_out)
    finally:
        ef.free(d_idx)
        ef.free(d_out)
    assert np.array_equal(dev, want)
    assert np.array_equal(ef.forward_sharded(a, 0, L, L), want)
    assert np.array_equal(ef.forward_shards_emulated(a, 1), want)
