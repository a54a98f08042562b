"""-m gpu: the sub-call driver of the taxon-axis analyses (leave-one-out, placement, tiling) where it really cuts - a
batch split into several sub-calls by option "sub_floats" against the same batch in one, bit for bit, with the number of
reductions as the proof of the split; the re-upload of what the range re-check replaced before a reduction reads it;
and the option itself."""
import numpy as np
import pytest

from helpers.profiled import Profiled
from phyloformer_amd import place as PL
from phyloformer_amd import taxa as T
from phyloformer_amd import tile as TL
from phyloformer_amd.engine import Engine
from phyloformer_amd.msa_sim import simulate_batch

pytestmark = pytest.mark.gpu
LOO_RTOL, LOO_ATOL = 2.0 ** -23, 1e-9            # test_gpu_taxa's: device statistics against the float64 twin
PLACE_RTOL, PLACE_ATOL = 1e-6, 1e-12             # test_gpu_place's


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"{what}: array {k} differs"


# ---- sub-calls that really split -----------------------------------------------------------------------------------
# B = 3 at the default cap (one sub-call), at a cap of two sources' distances (sub-calls of 2 and 1) and at a cap of one
# float (three sub-calls: one source always runs whole); (name, call, reduction's profile name, distances per source)

def _random(B, N, L, seed):
    return np.random.default_rng(seed).integers(0, 22, size=(B, N, L), dtype=np.uint8)


SPLITS = {
    # 5 x 40: per source N * P_{N-1} = 5 * 6; without keep_loo the cuts land in the internal temporary
    "loo_kept": (lambda e, idx: e.forward_leave_one_out(idx, keep_loo=True), "loo_stats", lambda: simulate_batch(3, 5, 40, seed=501), 30),
    "loo": (lambda e, idx: e.forward_leave_one_out(idx), "loo_stats", lambda: simulate_batch(3, 5, 40, seed=501), 30),
    # M = 5, Q = 2, L = 33: per source Q * P_{N+1} = 2 * 6
    "place_kept": (lambda e, idx: e.forward_place(idx, 2, keep_sets=True), "place_stats", lambda: simulate_batch(3, 5, 33, seed=502), 12),
    "place": (lambda e, idx: e.forward_place(idx, 2), "place_stats", lambda: simulate_batch(3, 5, 33, seed=502), 12),
    # N = 10, M = 6, L = 40: sets of 4, 5 and 6 rows, so three classes per sub-call
    "tiled": (lambda e, idx: e.forward_tiled(idx, 6), "tile_combine", lambda: _random(3, 10, 40, seed=503), TL.plan(10, 6).T),
}


@pytest.mark.parametrize("name", list(SPLITS))
def test_split_batch_gives_the_bits_of_one_sub_call(weights, name):
    call, reduction, make, per_source = SPLITS[name]
    idx = make()
    assert idx.shape[0] == 3
    runs = []
    with Engine(weights("pf"), 0) as e:
        for cap, n_sub in ((None, 1), (2 * per_source, 2), (1, 3)):
            if cap is not None:
                e.set_option("sub_floats", cap)
            with Profiled(e):
                runs.append(call(e, idx))
                n = e.profile_get(reduction)[0]
            print(f"{name}: sub_floats = {cap}: {n} {reduction} launches")
            assert n == n_sub, (cap, n)
    _same(runs[1], runs[0], f"{name}, sub-calls of 2 and 1 sources")
    _same(runs[2], runs[0], f"{name}, sub-calls of one source")


def test_split_leave_one_out_whole_on_default_kernels_cuts_in_float64(weights):
    """14 x 100: the whole alignment takes the default kernels, a cut (13 rows: 7,800 tokens) float64, so both routes
    cross a sub-call boundary."""
    idx = simulate_batch(3, 14, 100, seed=504)
    with Engine(weights("pf"), 0) as e:
        with Profiled(e):
            whole = e.forward_leave_one_out(idx, keep_loo=True)
            assert e.profile_get("main")[0] > 0 and e.profile_get("precise")[0] > 0 and e.profile_get("loo_stats")[0] == 1
        e.set_option("sub_floats", 1)
        with Profiled(e):
            split = e.forward_leave_one_out(idx, keep_loo=True)
            assert e.profile_get("loo_stats")[0] == 3
    _same(split, whole, "14 x 100")


# ---- the range re-check inside a reduction -------------------------------------------------------------------------
# B = 2 at 20 x 200: source 0 simulated, source 1 uniformly random residues (test_taxa_recheck_trips_in_the_random_source),
# whose cuts saturate above the threshold on the default kernels and are replaced on the host by their float64 values;
# the reduction must read those.  sub_floats = 1: each source is its own sub-call, only the second re-uploads.

def _recheck_batch(seed):
    idx = simulate_batch(2, 20, 200, seed=seed).copy()
    idx[1] = np.random.default_rng(7).integers(0, 20, size=(20, 200), dtype=np.uint8)
    return idx


@pytest.mark.parametrize("sub_floats", [0, 1])
def test_leave_one_out_reduces_what_the_recheck_left(weights, sub_floats):
    idx = _recheck_batch(505)
    with Engine(weights("pf"), 0) as e:
        e.set_option("sub_floats", sub_floats)
        with Profiled(e):
            out, infl, shift, ctx, loo = e.forward_leave_one_out(idx, keep_loo=True)
            n_call, n_stats = e.rechecked_count(), e.profile_get("loo_stats")[0]
            without = e.forward_leave_one_out(idx)
        e.profile_reset()
        want_out = e.forward(idx)
        n_whole = e.rechecked_count()
        want_loo = e.forward_taxa(idx, T.leave_one_out_sets(20))
    print(f"rechecked: {n_call} over the call, {n_whole} of them whole alignments; {n_stats} loo_stats launches; "
          f"largest cut distance {loo[1].max():.3f}")
    assert n_call >= 1 and n_call - n_whole >= 1                 # cuts were replaced: the re-upload ran
    assert n_stats == (2 if sub_floats else 1)
    assert np.array_equal(_bits(out), _bits(want_out)) and np.array_equal(_bits(loo), _bits(want_loo))
    for got, want, name in zip((infl, shift, ctx), T.loo_stats(out, loo), ("influence", "shift", "context")):
        print(f"{name}: max |device - twin| {float(np.abs(got.astype(np.float64) - want).max()):.3e}, largest value "
              f"{float(np.abs(want).max()):.3e}")
        assert np.allclose(got, want, rtol=LOO_RTOL, atol=LOO_ATOL), name
    _same(without, (out, infl, shift, ctx), "without keep_loo")


@pytest.mark.parametrize("sub_floats", [0, 1])
def test_placement_reduces_what_the_recheck_left(weights, sub_floats):
    idx = _recheck_batch(506)
    M, Q = 20, 2
    N = M - Q
    with Engine(weights("pf"), 0) as e:
        e.set_option("sub_floats", sub_floats)
        with Profiled(e):
            out, base, place, disturb, shift, joint, sets = e.forward_place(idx, Q, keep_sets=True)
            n_call, n_stats = e.rechecked_count(), e.profile_get("place_stats")[0]
            without = e.forward_place(idx, Q)
        e.profile_reset()
        want_out, want_base = e.forward(idx), e.forward(np.ascontiguousarray(idx[:, :N]))
        n_others = e.rechecked_count()
        want_sets = np.stack([np.stack([e.forward(PL.join_query(idx[b], N, q)) for q in range(Q)]) for b in range(2)])
    print(f"rechecked: {n_call} over the call, {n_others} of them wholes and backbones; {n_stats} place_stats launches; "
          f"largest set distance {sets[1].max():.3f}")
    assert n_call >= 1 and n_call - n_others >= 1                # sets were replaced: the re-upload ran
    assert n_stats == (2 if sub_floats else 1)
    assert np.array_equal(_bits(out), _bits(want_out)) and np.array_equal(_bits(base), _bits(want_base))
    assert np.array_equal(_bits(sets), _bits(want_sets))
    want = PL.place_stats(out, base, sets, N, Q)
    assert np.array_equal(_bits(place), _bits(want[0]))
    for got, w, name in zip((disturb, shift, joint), want[1:], ("disturb", "shift", "joint")):
        print(f"{name}: max |device - twin| {float(np.abs(got.astype(np.float64) - w).max()):.3e}, largest value "
              f"{float(np.abs(w).max()):.3e}")
        assert np.allclose(got, w, rtol=PLACE_RTOL, atol=PLACE_ATOL), name
    _same(without, (out, base, place, disturb, shift, joint), "without keep_sets")


# ---- the option ----------------------------------------------------------------------------------------------------

def test_sub_floats_zero_restores_the_default_and_unknown_options_are_refused(weights):
    idx = simulate_batch(3, 5, 40, seed=501)
    with Engine(weights("pf"), 0) as e:
        counts = []
        for value in (None, 1, 0):
            if value is not None:
                e.set_option("sub_floats", value)
            with Profiled(e):
                e.forward_leave_one_out(idx)
                counts.append(e.profile_get("loo_stats")[0])
        assert counts == [1, 3, 1]
        with pytest.raises(ValueError, match="unknown option 'sub_float'"):
            e.set_option("sub_float", 1)
        with Profiled(e):
            e.forward_leave_one_out(idx)
            assert e.profile_get("loo_stats")[0] == 1
