"""-m gpu: k_main's per-token work once per distinct column (option ``main_dedup``).

An alignment on the split route runs row apply, column apply and the feed-forward over its compacted tokens (first
sites only), then the row statistics - after the last block the head's site sums - over every site in place.  No sum
changes its order, so everything here is ``np.array_equal`` on the float bits: ``main_dedup`` 0 (every alignment fused),
1 (routed per alignment) and 2 (every alignment split, even one without a repeat) against each other.

Alignments are built from a pool of columns (``helpers/dedup_model.py``).  Shapes: (4, 33), (6, 70) and (8, 200) flat
tiling, (5, 64) row tiling.
Distinct counts 1, 31, 32, 33, L - 1 and L (below 32 the compact tiling has one ragged tile per row, from 32 on tiles of
32 consecutive compacted tokens that may cover two rows), with the repeats in front of the other columns' first
occurrences ("front": the last site is a first occurrence), behind all of them ("behind") or scattered between them
("between": the last site is a first occurrence as well).  One batch per shape mixes them all: with option 1 it holds
both routes, whatever the threshold (one distinct column: split; no repeat: fused).
"""
import numpy as np
import pytest

from helpers.dedup_model import PLACEMENTS, alignment

pytestmark = pytest.mark.gpu
SHAPES = [(4, 33), (6, 70), (8, 200), (5, 64)]


def counts(l):
    return sorted({1, 31, 32, 33, l - 1, l} & set(range(1, l + 1)))


_BATCHES = {}


def batch(n, l):
    """Every distinct count in every placement (where a placement differs), built once per shape and left unchanged."""
    if (n, l) not in _BATCHES:
        alns = [alignment(n, l, k, p) for k in counts(l) for p in (PLACEMENTS if 1 < k < l else PLACEMENTS[:1])]
        idx = np.stack(alns)
        idx.setflags(write=False)
        _BATCHES[n, l] = idx
    return _BATCHES[n, l]


@pytest.fixture()
def eng(engines):
    e = engines("pf", precise=0)
    yield e
    for key, value in (("main_dedup", 1), ("debug_keep", 0), ("head_fold", 1), ("two_streams", 1)):
        e.set_option(key, value)


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def per_option(e, call):
    out = {}
    for mode in (0, 1, 2):
        e.set_option("main_dedup", mode)
        out[mode] = call()
    e.set_option("main_dedup", 1)
    return out


@pytest.mark.parametrize("n,l", SHAPES)
@pytest.mark.parametrize("head_fold", [1, 0])
@pytest.mark.parametrize("two_streams", [1, 0])
def test_distances_keep_their_bits_on_every_route(eng, n, l, head_fold, two_streams):
    idx = batch(n, l)
    _, ucount = eng.site_classes(idx)
    assert ucount.min() == 1 and ucount.max() == l          # option 1: both routes in this batch
    eng.set_option("head_fold", head_fold)
    eng.set_option("two_streams", two_streams)
    out = per_option(eng, lambda: eng.forward(idx))
    assert np.isfinite(out[0]).all()
    assert same(out[1], out[0]) and same(out[2], out[0])


@pytest.mark.parametrize("n,l", SHAPES)
@pytest.mark.parametrize("mode", [1, 2])
def test_an_alignment_keeps_its_bits_alone_and_at_another_place(eng, n, l, mode):
    idx = batch(n, l)
    eng.set_option("main_dedup", 0)
    want = eng.forward(idx)
    eng.set_option("main_dedup", mode)
    back = eng.forward(np.ascontiguousarray(idx[::-1]))
    assert same(back[::-1], want)
    for b in range(0, len(idx), 3):
        assert same(eng.forward(idx[b]), want[b]), b
        assert same(eng.forward(np.stack([idx[-1], idx[b]]))[1], want[b]), b


@pytest.mark.parametrize("n,l", SHAPES)
@pytest.mark.parametrize("head_fold", [1, 0])
def test_taps_keep_their_bits_on_every_route(eng, weights, n, l, head_fold):
    nb = weights("pf").n_blocks
    idx = batch(n, l)
    names = [f"x{k}" for k in range(nb + 1)] + [f"srow{k}" for k in range(nb)] + [f"ctx{k}" for k in range(nb)]
    eng.set_option("head_fold", head_fold)
    eng.set_option("debug_keep", 1)

    def taps():
        d = eng.forward(idx)
        return [d] + [eng.debug_read(name) for name in names]
    out = per_option(eng, taps)
    for i, name in enumerate(["distances"] + names):
        assert out[0][i].size, name
        assert same(out[1][i], out[0][i]), (name, 1)
        assert same(out[2][i], out[0][i]), (name, 2)


@pytest.mark.parametrize("n,l", [(6, 70), (4, 33)])
def test_sharded_and_emulated_ranks_keep_their_bits(eng, n, l):
    """A rank routes from the classes of its own site range: (6, 70) cut in 2 gives ranks of 35 sites (flat tiling),
    cut in 4 ranks of 17 or 18 (row tiling, compact tiles of one row); (4, 33) in 2 ranks of 16 or 17."""
    idx = batch(n, l)
    for call in (lambda: eng.forward_sharded(idx, 0, l, l), lambda: eng.forward_shards_emulated(idx, 2),
                 lambda: eng.forward_shards_emulated(idx, 4)):
        out = per_option(eng, call)
        assert same(out[1], out[0]) and same(out[2], out[0])
