"""-m gpu: the split route's row statistics once per distinct column of a pair row (option ``stats_dedup``, k_row_stats;
DESIGN.md section 4).

With the option at 1 an alignment on the split route with at most ``ROW_STATS_KMAX`` distinct columns gets its next-row
statistics from k_row_stats - v, q', k' once per distinct column, then every site reduced in place in the lanes and
slots of the original tiling; with more distinct columns, or with the option at 0, from the statistics launch
(k_main<MODE_STATS>).  No sum changes its order: everything here is ``np.array_equal`` on the float bits between the
option at 1 and at 0 - the distances and, under ``debug_keep``, the taps ``srow<k>``, ``x<k>``, ``ctx<k>`` and
``qrow<k>`` (q' of block k's row attention, per token).  The default kernels are forced (``precise`` 0).

Shapes: (6, 40) and (6, 70) flat tiling with tiles over two rows, (6, 64) row tiling, (2, 70) one pair,
(3, KMAX + 40) beyond the term table (the statistics launch, alone and beside k_row_stats in one block), (6, 80) for
the sharded forms.  ``main_dedup`` is 2 (every alignment split) unless a test says otherwise.
"""
import numpy as np
import pytest

from helpers import dedup_model as M
from helpers.row_stats_model import kmax
from oracle import pf_oracle as O
from phyloformer_amd.engine import Engine
from test_gpu_parity import _check, _record

pytestmark = pytest.mark.gpu
OPTIONS = (("stats_dedup", 1), ("main_dedup", 1), ("debug_keep", 0), ("head_fold", 1), ("two_streams", 1), ("profile", 0))


@pytest.fixture()
def eng(engines):
    e = engines("pf", precise=0)
    yield e
    for key, value in OPTIONS:
        e.set_option(key, value)


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def pairs(n):
    return n * (n - 1) // 2


def frozen(alns):
    idx = np.stack(alns)
    idx.setflags(write=False)
    return idx


def far_repeats(n, l, k):
    """k distinct columns in front, then repeats that step through the classes by 7: repeats whose first occurrence lies in
    another tile of the row and (k > 32) in the row's other compact tile than their neighbour's."""
    pool = M.distinct_columns(np.random.default_rng(7 * n + l), n, k)
    pick = np.r_[np.arange(k), (np.arange(l - k) * 7 + k - 1) % k]
    a = np.ascontiguousarray(pool[:, pick])
    srep, ulist, got = M.classes(a)
    assert got == k
    rep = np.flatnonzero(srep != np.arange(l))
    cidx = np.searchsorted(ulist, srep[rep])                # compact index of every repeat's class
    assert (rep // 32 != srep[rep] // 32).any() and (k <= 32 or ((cidx < 32).any() and (cidx >= 32).any()))
    return a


_BATCHES = {}


def batch(n, l):
    """1, 31, 32, 33 and L - 1 distinct columns, the repeats in front of, behind and between the first occurrences, and
    one alignment of far repeats; built once per shape and left unchanged."""
    if (n, l) not in _BATCHES:
        ks = sorted({1, 31, 32, 33, l - 1} & set(range(1, l)))
        alns = [M.alignment(n, l, k, p) for k in ks for p in (M.PLACEMENTS if k > 1 else M.PLACEMENTS[:1])]
        if n > 2:                                           # (two sequences: 484 columns, enough; six: plenty)
            alns.append(far_repeats(n, l, min(40, l - 8)))
        _BATCHES[n, l] = frozen(alns)
    return _BATCHES[n, l]


def tap_names(nb):
    return ([f"x{k}" for k in range(nb + 1)] + [f"srow{k}" for k in range(nb)] + [f"ctx{k}" for k in range(nb)] +
            [f"qrow{k}" for k in range(1, nb)])


def forward_with_taps(e, idx, nb):
    e.set_option("debug_keep", 1)
    d = e.forward(idx)
    out = [d] + [e.debug_read(name) for name in tap_names(nb)]
    e.set_option("debug_keep", 0)
    return out


def both(e, call):
    out = {}
    for opt in (0, 1):
        e.set_option("stats_dedup", opt)
        out[opt] = call()
    e.set_option("stats_dedup", 1)
    return out


def assert_taps_same(out, nb):
    for i, name in enumerate(["distances"] + tap_names(nb)):
        assert out[0][i].size and np.isfinite(out[0][i]).all(), name
        assert same(out[1][i], out[0][i]), name


@pytest.mark.parametrize("n,l", [(6, 40), (6, 70), (6, 64), (2, 70)])
@pytest.mark.parametrize("main_dedup", [2, 1])
def test_taps_and_distances_keep_their_bits(eng, weights, n, l, main_dedup):
    """(6, 40), (6, 70): flat tiling, tiles over two rows; (6, 64): row tiling; (2, 70): one pair, no neighbour row."""
    nb = weights("pf").n_blocks
    idx = batch(n, l)
    eng.set_option("main_dedup", main_dedup)
    assert_taps_same(both(eng, lambda: forward_with_taps(eng, idx, nb)), nb)


def big_shape():
    return 3, kmax() + 40


_BIG = {}


def big_batch():
    """(3, KMAX + 40): all distinct (the statistics launch); KMAX and KMAX + 1 distinct columns, the two sides of the
    term table's size; 5 distinct columns (k_row_stats)."""
    if not _BIG:
        n, l = big_shape()
        _BIG["idx"] = frozen([M.alignment(n, l, l, "front"), M.alignment(n, l, 5, "between"), M.alignment(n, l, kmax(), "between"),
                              M.alignment(n, l, kmax() + 1, "behind")])
    return _BIG["idx"]


def test_alignments_beyond_the_term_table_keep_the_statistics_launch(eng, weights):
    nb = weights("pf").n_blocks
    n, l = big_shape()
    idx = big_batch()
    eng.set_option("main_dedup", 2)
    alone = both(eng, lambda: forward_with_taps(eng, idx[:1], nb))      # nothing for k_row_stats
    assert_taps_same(alone, nb)
    mixed = both(eng, lambda: forward_with_taps(eng, idx, nb))          # both launches in every block
    assert_taps_same(mixed, nb)
    ns = M.read_plan(eng.debug_read("plan").view(np.int32), len(idx))[1]
    assert ns == len(idx)
    assert same(mixed[1][0][0], alone[1][0][0])
    eng.set_option("main_dedup", 0)
    assert same(eng.forward(idx), mixed[1][0])


@pytest.mark.parametrize("n,l", [(6, 70), (6, 64)])
def test_an_alignment_keeps_its_bits_alone_and_at_position_2_of_3(eng, n, l):
    idx = batch(n, l)
    eng.set_option("main_dedup", 2)
    eng.set_option("stats_dedup", 0)
    want = eng.forward(idx)
    eng.set_option("stats_dedup", 1)
    for b in range(0, len(idx), 2):
        assert same(eng.forward(idx[b]), want[b]), b
        assert same(eng.forward(np.stack([idx[-1], idx[0], idx[b]]))[2], want[b]), b


@pytest.mark.parametrize("two_streams", [0, 1])
@pytest.mark.parametrize("head_fold", [1, 0])
def test_schedules_and_the_unfolded_head_keep_their_bits(eng, two_streams, head_fold):
    idx = batch(6, 70)
    eng.set_option("main_dedup", 2)
    eng.set_option("two_streams", two_streams)
    eng.set_option("head_fold", head_fold)
    out = both(eng, lambda: eng.forward(idx))
    assert np.isfinite(out[0]).all() and same(out[1], out[0])


def test_sharded_and_emulated_ranks_keep_their_bits(eng):
    """(6, 80) cut in 2: ranks of 40 sites, flat tiling; a single-rank sharded call over the whole range."""
    idx = batch(6, 80)
    eng.set_option("main_dedup", 2)
    for call in (lambda: eng.forward_shards_emulated(idx, 2), lambda: eng.forward_sharded(idx, 0, 80, 80)):
        out = both(eng, call)
        assert np.isfinite(out[0]).all() and same(out[1], out[0])
    assert same(eng.forward(idx), out[1])


_ORACLE = {}


def test_oracle_parity_on_split_alignments(eng, weights):
    """Simulated columns, (6, 70), options at their defaults: the plan tap shows split alignments, the distances stay under
    the bound of DESIGN.md section 5 (``test_gpu_parity._check``) against the fp32 oracle."""
    n, l = 6, 70
    ks = [1, 31, 32, 33, l - 1, l]
    idx = frozen([M.alignment_simulated(n, l, k, p) for k in ks for p in (M.PLACEMENTS if 1 < k < l else M.PLACEMENTS[:1])])
    eng.set_option("debug_keep", 1)
    eng.forward(idx)
    nf, ns, *_ = M.read_plan(eng.debug_read("plan").view(np.int32), len(idx))
    assert ns >= 8 and nf > 0, (nf, ns)
    eng.set_option("debug_keep", 0)
    out = both(eng, lambda: eng.forward(idx))
    if "o" not in _ORACLE:
        w = weights("pf").tensors
        _ORACLE["o"] = O.forward_batch(w, idx), O.forward_batch(w, idx, dtype=np.float64)
    want, f64 = _ORACLE["o"]
    err, scale = _record(f"stats_dedup {n}x{l} batch {len(idx)} pf ({ns} split, {nf} fused)", out[1], want, f64=f64)
    _check(err, scale, (n, l))
    assert same(out[0], out[1])


@pytest.mark.parametrize("two_streams", [1, 0])
def test_profile_counts_one_main_per_block_and_run(weights, two_streams):
    idx = batch(6, 70)[[0, 3, 8, 12]]
    nb = weights("pf").n_blocks
    runs = 2 if two_streams else 1
    with Engine(weights("pf"), device=0) as e:
        e.set_option("precise", 0)
        e.set_option("two_streams", two_streams)
        e.set_option("profile", 1)
        for main_dedup in (1, 2):
            e.set_option("main_dedup", main_dedup)
            for opt in (0, 1):
                e.set_option("stats_dedup", opt)
                e.profile_reset()
                e.forward(idx)
                assert e.profile_get("main")[0] == nb * runs, (main_dedup, opt, e.profile_get("main"))
