"""-m gpu: arguments through the binding's computed prototypes (phyloformer_amd/cabi.py) at the smallest shapes at which a
mis-typed one still shows - a generated pass-through against its host form, a ``uint64_t`` seed beyond 2^63 (and beyond
32 bits: a narrower type gives other sites), an ``int32_t`` between pointers with ``int64_t`` results, and a plain 0 that
has to arrive as NULL."""
import numpy as np
import pytest

from phyloformer_amd import bootstrap
from phyloformer_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(weights):
    with Engine(weights("pf"), 0) as e:
        yield e


def device_call(e, call, inputs, outputs):
    """``call(*device addresses)`` with ``inputs`` uploaded and ``outputs`` filled with 0x77 bytes first; the outputs."""
    bufs = [e.malloc(max(a.nbytes, 1)) for a in (*inputs, *outputs)]
    try:
        for host, dev in zip(inputs, bufs):
            e.h2d(dev, host)
        for host, dev in zip(outputs, bufs[len(inputs):]):
            e.h2d(dev, np.full(host.nbytes, 0x77, np.uint8))
        call(*bufs)
        for host, dev in zip(outputs, bufs[len(inputs):]):
            e.d2h(host, dev)
        e.synchronize()
    finally:
        for p in bufs:
            e.free(p)
    return outputs


def test_forward_device_is_forward_bit_for_bit(eng):
    B, N, L = 2, 3, 5
    idx = np.random.default_rng(1).integers(0, 22, (B, N, L)).astype(np.uint8)
    out, = device_call(eng, lambda d_idx, d_out: eng.forward_device(d_idx, B, N, L, d_out), [idx],
                       [np.empty((B, N * (N - 1) // 2), np.float32)])
    assert out.tobytes() == eng.forward(idx).tobytes()


def test_resample_sites_device_takes_any_seed_as_uint64(eng):
    B, N, L, R = 1, 2, 7, 3
    idx = np.random.default_rng(2).integers(0, 22, (B, N, L)).astype(np.uint8)
    got = {}
    for seed in (-1, 2 ** 64 - 1, 2 ** 63):
        got[seed], = device_call(eng, lambda d_src, d_dst: eng.resample_sites_device(d_src, B, N, L, 0, R, seed, d_dst), [idx],
                                 [np.empty((B, R, N, L), np.uint8)])
        sites = bootstrap.resample_sites(L, R, seed & 0xFFFFFFFFFFFFFFFF)                  # [R][L]
        assert np.array_equal(got[seed], np.moveaxis(idx[..., sites], -2, -3)), seed
    assert np.array_equal(got[-1], got[2 ** 64 - 1])
    # the seeds' low 32 bits alone give other sites: the three comparisons above do tell a 32-bit seed
    assert not np.array_equal(bootstrap.resample_sites(L, R, 2 ** 63), bootstrap.resample_sites(L, R, 0))
    assert not np.array_equal(bootstrap.resample_sites(L, R, 2 ** 64 - 1), bootstrap.resample_sites(L, R, 2 ** 32 - 1))


def test_delta_device_is_delta(eng):
    B, N, bins = 1, 4, 20
    preds = np.random.default_rng(3).uniform(0.1, 2.0, (B, N * (N - 1) // 2)).astype(np.float32)
    got = device_call(eng, lambda d_preds, *d_out: eng.delta_device(d_preds, B, N, bins, *d_out), [preds],
                      [np.empty((B, preds.shape[1]), np.int64), np.empty((B, bins), np.int64), np.empty(B, np.uint8)])
    want = eng.delta(preds, bins)
    assert all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))
    assert got[1].sum() == 1 and not got[2].any()                                        # one quartet, a finite source


def test_tree_fit_device_without_patristic_gets_a_null(eng):
    B, M, N = 1, 1, 3
    preds = np.random.default_rng(4).uniform(0.1, 2.0, (B, 3)).astype(np.float32)
    slots, lengths, nonfinite = eng.nj_joins(preds)
    assert slots.shape == (B, 3) and not nonfinite.any()
    rows, worst_j, status = device_call(
        eng, lambda d_preds, d_slots, d_lengths, *d_out: eng.tree_fit_device(d_preds, d_slots, d_lengths, B, M, N, 0, *d_out),
        [preds, slots, lengths], [np.empty((B, N, 6), np.float64), np.empty((B, N), np.int32), np.empty(B, np.uint8)])
    none, want_rows, want_worst, want_status = eng.tree_fit(preds, slots, lengths, patristic=False)
    assert none is None and status.tolist() == [0]
    assert rows.tobytes() == want_rows.tobytes() and np.array_equal(worst_j, want_worst) and np.array_equal(status, want_status)
