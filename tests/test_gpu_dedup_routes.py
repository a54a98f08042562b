"""-m gpu: the routes behind the column classes, read back and held against a model.

``test_gpu_site_dedup.py`` and ``test_gpu_main_dedup.py`` show that the options give the same float bits.  That holds
as well when nothing is routed at all, so here the route itself is read: with ``debug_keep`` 1 a forward leaves what
k_site_classes and k_main_plan wrote for its (one) run in the taps ``srep``, ``ulist``, ``ucount`` and ``plan`` (raw
int32 bits; no ``plan`` tap when the run is not routed), and ``helpers/dedup_model.py`` says what they must hold.

  a  the plan the forward used is the model's, at the threshold K * 20 <= L * 17 from both sides; the forwards that
     must stay fused leave no plan
  b  k_main_plan past one ballot round of 64 alignments, its lists and tile prefix carried across rounds
  c  the oracle in fp32, under the bound of ``test_gpu_parity._check``, on batches the plan tap shows to hold both routes
  d  every routed entry point, and a forward cut into workspace chunks, keeps its bits under every option
  e  the site-count edges of k_site_classes (1,024 threads per round, a table of 4,096 sites, the identity map behind
     it), one pair, one site, and pair counts of several k_colstats groups - through the forward
  f  the profile counters: one "main" per block and run, one "site_classes" per run

(2, 4096): two sequences have 22 x 22 = 484 different columns at the most, so that shape runs with K = 484 and the K = 4096
and K = 2000 cases of a full table run at (3, 4096).  ``same`` is ``np.array_equal`` on the uint32 view.
"""
import numpy as np
import pytest

from helpers import dedup_model as M
from helpers.profiled import Profiled
from oracle import pf_oracle as O
from phyloformer_amd.engine import Engine, EngineError
from test_gpu_parity import _check, _record

pytestmark = pytest.mark.gpu
OPTIONS = (("main_dedup", 1), ("site_dedup", 1), ("debug_keep", 0), ("head_fold", 1), ("two_streams", 1), ("materialize_x0", 0),
           ("profile", 0))


@pytest.fixture()
def eng(engines):
    e = engines("pf", precise=0)
    yield e
    for key, value in OPTIONS:
        e.set_option(key, value)


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def all_same(got, want):
    got, want = (x if isinstance(x, tuple) else (x,) for x in (got, want))
    return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))


def pairs(n):
    return n * (n - 1) // 2


def frozen(alns):
    idx = np.stack(alns)
    idx.setflags(write=False)
    return idx


def tap(e, name):
    return e.debug_read(name).view(np.int32)


def no_plan_tap(e):
    with pytest.raises(EngineError, match="no tap 'plan'"):
        e.debug_read("plan")
    return True


def check_class_taps(e, idx, dedup=True):
    """The srep / ulist / ucount taps of the last forward (one run over idx) against the model; returns ucount."""
    B, _, L = idx.shape
    srep, ulist, ucount = tap(e, "srep").reshape(B, L), tap(e, "ulist").reshape(B, L), tap(e, "ucount")
    assert ucount.shape == (B,)
    for b in range(B):
        if dedup and L <= 4096:
            want_srep, want_ulist, k = M.classes(idx[b])
        else:                                                   # the identity map
            want_srep = want_ulist = np.arange(L, dtype=np.int32)
            k = L
        assert ucount[b] == k, (b, ucount[b], k)
        assert np.array_equal(srep[b], want_srep), (b, np.flatnonzero(srep[b] != want_srep)[:8])
        assert np.array_equal(ulist[b, :k], want_ulist), (b, np.flatnonzero(ulist[b, :k] != want_ulist)[:8])
    return ucount


def check_plan_tap(e, ucount, P, L, mode):
    """The plan tap of the last forward against the model, field by field; returns it in the model's form."""
    got, want = M.read_plan(tap(e, "plan"), len(ucount)), M.plan(ucount, P, L, mode)
    for name, g, w in zip(("nf", "ns", "tiles", "flist", "slist", "cpre"), got, want):
        assert g == w, (name, mode, g, w)
    return got


def per_option(e, call, identity=True):
    """call() under main_dedup 0 / 1 / 2 (site_dedup 1) and, with ``identity``, under site_dedup 0 x main_dedup 0 / 1 / 2."""
    out = {}
    for sd in (1, 0) if identity else (1,):
        e.set_option("site_dedup", sd)
        for mode in (0, 1, 2):
            e.set_option("main_dedup", mode)
            out[mode, sd] = call()
    e.set_option("site_dedup", 1)
    e.set_option("main_dedup", 1)
    return out


# ---- a: the plan the forward used is the model's ---------------------------------------------------------------------

THRESHOLD = {40: (34, 35), 200: (170, 171)}            # (the largest K that splits, the smallest that stays fused)
_A = {}


def batch_a(l):
    if l not in _A:
        ks = [1, 31, 32, 33, *THRESHOLD[l], l - 1, l]
        _A[l] = ks, frozen([M.alignment(6, l, k, M.PLACEMENTS[i % 3]) for i, k in enumerate(ks)])
    return _A[l]


@pytest.mark.parametrize("l", [40, 200])
def test_the_plan_of_a_forward_is_the_models(eng, l):
    ks, idx = batch_a(l)
    P = pairs(6)
    eng.set_option("debug_keep", 1)
    for mode in (1, 2):
        eng.set_option("main_dedup", mode)
        eng.forward(idx)
        ucount = check_class_taps(eng, idx)
        assert ucount.tolist() == ks
        nf, ns, tiles, flist, slist, cpre = check_plan_tap(eng, ucount, P, l, mode)
        if mode == 1:
            lo, hi = THRESHOLD[l]
            assert ks.index(lo) in slist and ks.index(hi) in flist
            assert slist == [b for b, k in enumerate(ks) if k <= lo] and flist == [b for b, k in enumerate(ks) if k >= hi]
        else:
            assert nf == 0 and slist == list(range(len(ks))) and tiles == sum(M.compact_tiles(P, k) for k in ks)
    # site_dedup 0: every site its own class - nothing to split for option 1, everything for option 2
    eng.set_option("site_dedup", 0)
    for mode in (1, 2):
        eng.set_option("main_dedup", mode)
        eng.forward(idx)
        ucount = check_class_taps(eng, idx, dedup=False)
        assert np.all(ucount == l)
        nf, ns, tiles, *_ = check_plan_tap(eng, ucount, P, l, mode)
        assert (nf, ns, tiles) == ((len(ks), 0, 0) if mode == 1 else (0, len(ks), len(ks) * M.compact_tiles(P, l)))


@pytest.mark.parametrize("l", [40, 200])
def test_forwards_that_stay_fused_leave_no_plan(eng, l):
    """Each in turn behind a routed forward, whose plan tap it must take away."""
    ks, idx = batch_a(l)
    P = pairs(6)
    eng.set_option("debug_keep", 1)

    def routed():
        eng.forward(idx)
        check_plan_tap(eng, np.array(ks), P, l, 1)

    routed()
    eng.set_option("main_dedup", 0)
    want = eng.forward(idx)
    assert no_plan_tap(eng)
    check_class_taps(eng, idx)                              # (the classes are formed all the same: k_colstats walks them)
    eng.set_option("main_dedup", 1)

    routed()
    assert same(eng.forward_weighted(idx, np.ones((len(ks), l), np.float32)), want)     # unit weights: forward's bits
    assert no_plan_tap(eng)

    routed()
    dist, smap = eng.forward_site_map(idx)
    assert same(dist, want) and smap.shape == (len(ks), P, l)
    assert no_plan_tap(eng)

    routed()
    eng.set_option("materialize_x0", 1)
    assert same(eng.forward(idx), want)
    assert no_plan_tap(eng)
    eng.set_option("materialize_x0", 0)

    # head_fold 0: what the code does is a PLAN - the blocks in front of the last are routed.  Under debug_keep the last
    # block's launch writes x of every site and is the fused one for all alignments (phase_block),
    # without debug_keep it is routed too (test_gpu_main_dedup.py holds its bits either way).
    eng.set_option("head_fold", 0)
    eng.forward(idx)
    check_plan_tap(eng, np.array(ks), P, l, 1)


# ---- b: k_main_plan beyond one ballot round --------------------------------------------------------------------------

KS_B = (1, 20, 28, 29, 33)              # (3, 33): 28 * 20 <= 33 * 17 < 29 * 20 - three counts split, two stay fused
_B = {}


def batch_b(B):
    """Every five alignments hold the five counts, in a seeded order of their own."""
    if B not in _B:
        base = {(k, p): M.alignment(3, 33, k, p) for k in KS_B for p in M.PLACEMENTS}
        rng = np.random.default_rng(4206)
        ks = [int(k) for _ in range((B + 4) // 5) for k in rng.permutation(KS_B)][:B]
        _B[B] = ks, frozen([base[k, M.PLACEMENTS[b % 3]] for b, k in enumerate(ks)])
    return _B[B]


@pytest.mark.parametrize("B", [64, 65, 130])
def test_the_plan_is_carried_across_ballot_rounds(eng, B):
    ks, idx = batch_b(B)
    P, L = 3, 33
    rounds = [[M.split(k, L, 1) for k in ks[lo:lo + 64]] for lo in range(0, B, 64)]
    assert len(rounds) == (B + 63) // 64 and all(any(r) for r in rounds)       # a split alignment in every round of 64 ...
    assert all(not all(r) for r in rounds if len(r) > 1)                      # ... and a fused one: both lists cross every boundary
    eng.set_option("two_streams", 0)                        # one run of B alignments
    eng.set_option("debug_keep", 1)
    for mode in (1, 2):
        eng.set_option("main_dedup", mode)
        eng.forward(idx)
        ucount = check_class_taps(eng, idx)
        assert ucount.tolist() == ks
        nf, ns, tiles, flist, slist, cpre = check_plan_tap(eng, ucount, P, L, mode)
        if mode == 1:
            assert flist == [b for b, r in enumerate(sum(rounds, [])) if not r] and slist == [b for b, r in enumerate(sum(rounds, [])) if r]
    eng.set_option("debug_keep", 0)
    out = per_option(eng, lambda: eng.forward(idx), identity=False)
    assert np.isfinite(out[0, 1]).all()
    assert same(out[1, 1], out[0, 1]) and same(out[2, 1], out[0, 1])
    for b in sorted({0, 63, 64, 65, B - 1} & set(range(B))):
        assert same(eng.forward(idx[b]), out[0, 1][b]), b


# ---- c: the oracle on routes the test asserts ------------------------------------------------------------------------

_C = {}


def batch_c(n, l):
    """Columns of a simulated alignment: 1, 31, 32, 33, L - 1 and L of them distinct, repeats in front, behind, between."""
    if (n, l) not in _C:
        ks = sorted({1, 31, 32, 33, l - 1, l})
        _C[n, l] = frozen([M.alignment_simulated(n, l, k, p) for k in ks for p in (M.PLACEMENTS if 1 < k < l else M.PLACEMENTS[:1])])
    return _C[n, l]


_ORACLE = {}


def oracle_c(weights, n, l):
    if (n, l) not in _ORACLE:
        w, idx = weights("pf").tensors, batch_c(n, l)
        _ORACLE[n, l] = O.forward_batch(w, idx), O.forward_batch(w, idx, dtype=np.float64)
        for a in _ORACLE[n, l]:
            a.setflags(write=False)
    return _ORACLE[n, l]


@pytest.mark.parametrize("n,l", [(6, 70), (8, 200), (6, 64)])         # flat tiling twice, row tiling
def test_oracle_parity_on_both_routes(eng, weights, n, l):
    """Measured on the MI355X, 14 alignments per shape of which option 1 splits 10 (max-abs error against the fp32 oracle;
    GPU / fp32 oracle against the oracle's float64 evaluation; the parity table of DESIGN.md section 5):
    (6, 70) 1.05e-5 (5.6e-6 / 6.9e-6), (8, 200) 2.38e-5 (2.5e-5 / 3.2e-5), (6, 64) 7.6e-6 (6.3e-6 / 8.3e-6)."""
    idx = batch_c(n, l)
    eng.set_option("debug_keep", 1)
    eng.forward(idx)
    ucount = check_class_taps(eng, idx)
    nf, ns, *_ = check_plan_tap(eng, ucount, pairs(n), l, 1)
    assert nf > 0 and ns > 0, (nf, ns)                     # option 1: both routes in this batch
    eng.set_option("debug_keep", 0)
    out = per_option(eng, lambda: eng.forward(idx), identity=False)
    want, f64 = oracle_c(weights, n, l)
    err, scale = _record(f"dedup routes {n}x{l} batch {len(idx)} pf, main_dedup 1 ({ns} split, {nf} fused)", out[1, 1], want, f64=f64)
    _check(err, scale, (n, l))
    assert same(out[0, 1], out[1, 1]) and same(out[2, 1], out[1, 1])


# ---- d: every routed entry point ------------------------------------------------------------------------------------

def three(n, l=70):
    return frozen([M.alignment(n, l, k, p) for k, p in ((1, "front"), (l // 2, "between"), (l, "front"))])


def forward_device(e, idx):
    B, n, l = idx.shape
    out = np.empty((B, pairs(n)), np.float32)
    d_idx, d_out = e.malloc(idx.nbytes), e.malloc(out.nbytes)
    try:
        e.h2d(d_idx, idx)
        e.forward_device(d_idx, B, n, l, d_out)
        e.d2h(out, d_out)
    finally:
        e.free(d_idx)
        e.free(d_out)
    return out


SITES = np.stack([np.arange(40) % 13 * 5, np.r_[np.arange(35, 70), np.full(5, 69)]]).astype(np.int32)   # both repeat sites
TAXA = np.array([[0, 2, 3, 5], [4, 1, 1, 5]], np.int32)                                                     # a repeated taxon
ENTRY_POINTS = {                        # name: (sequences, call)
    "forward_device": (6, forward_device),
    "bootstrap": (6, lambda e, idx: e.bootstrap(idx, 4, seed=11)),
    "forward_sites": (6, lambda e, idx: e.forward_sites(idx, SITES)),
    "forward_windows": (6, lambda e, idx: e.forward_windows(idx, 32, 16)),
    "forward_taxa": (6, lambda e, idx: e.forward_taxa(idx, TAXA)),
    "forward_leave_one_out": (6, lambda e, idx: e.forward_leave_one_out(idx, keep_loo=True)),
    "forward_place": (6, lambda e, idx: e.forward_place(idx, 2, keep_sets=True)),
    "forward_tiled": (10, lambda e, idx: e.forward_tiled(idx, 6)),            # N > M: the smallest of test_gpu_tile.py
}


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_every_routed_entry_point_keeps_its_bits(eng, weights, name):
    n, call = ENTRY_POINTS[name]
    idx = three(n)
    assert [M.classes(a)[2] for a in idx] == [1, 35, 70]
    nb = weights("pf").n_blocks
    with Profiled(eng):                                     # (the default kernels ran, behind their class kernel)
        first = call(eng, idx)
        launches = {k: eng.profile_get(k)[0] for k in ("main", "site_classes", "precise")}
    assert launches["precise"] == 0 and launches["site_classes"] > 0 and launches["main"] == nb * launches["site_classes"], launches
    out = per_option(eng, lambda: call(eng, idx))
    for a in out[0, 1] if isinstance(out[0, 1], tuple) else (out[0, 1],):
        assert a.size and np.isfinite(a).all()
    assert all_same(first, out[1, 1])
    for key in ((1, 1), (2, 1), (1, 0)):
        assert all_same(out[key], out[0, 1]), (name, key)


def test_workspace_chunks_keep_their_bits(weights):
    idx = batch_c(8, 200)                                   # 14 alignments of 28 pairs x 200 sites, mixed K
    out = {}
    for limit in (0, 8):
        with Engine(weights("pf"), device=0) as e:
            e.set_option("precise", 0)
            e.set_option("two_streams", 0)                  # one run per chunk
            if limit:
                e.set_option("ws_limit_mb", limit)
            e.set_option("profile", 1)
            for mode in (0, 1, 2):
                e.set_option("main_dedup", mode)
                e.profile_reset()
                out[limit, mode] = e.forward(idx)
                runs = e.profile_get("site_classes")[0]
                assert runs >= 3 if limit else runs == 1, (limit, mode, runs)
    for mode in (0, 1, 2):
        assert same(out[8, mode], out[0, mode]) and same(out[0, mode], out[0, 0]), mode


# ---- e: site-count and pair-count edges through the forward ----------------------------------------------------------

def _p1(l, ks):
    return [M.alignment(2, l, k, M.PLACEMENTS[i % 3]) for i, k in enumerate(ks)]


def _two_rounds():
    """(3, 1100): the first occurrences of K = 1000 ... 1100 columns on both sides of site 1,024, where k_site_classes'
    second round of threads begins, and one alignment whose first 1,024 sites all repeat site 0."""
    alns = [M.alignment(3, 1100, k, p) for k in (1000, 1024, 1025) for p in ("behind", "between")]
    alns.append(M.alignment(3, 1100, 1100, "front"))
    late = M.alignment(3, 1100, 77, "behind")               # 77 distinct columns ...
    late = np.ascontiguousarray(late[:, np.r_[np.zeros(1024, int), np.arange(1, 77)]])     # ... 76 of them from site 1,024 on
    assert M.classes(late)[1].tolist() == [0] + list(range(1024, 1100))
    return alns + [late]


EDGES = {                               # name: (alignments, also one by one)
    "2x1": (lambda: [np.array([[3], [7]], np.uint8), np.array([[21], [21]], np.uint8)], True),
    "22x1": (lambda: [M.alignment(22, 1, 1, "front"), M.alignment(22, 1, 1, "front", seed=1)], True),
    "2x33": (lambda: _p1(33, [1, 28, 29, 32, 33]), False),                     # P = 1: a compact tile has no next row
    "2x70": (lambda: _p1(70, [1, 31, 32, 33, 59, 60, 69, 70]), False),
    "3x1100": (_two_rounds, False),
    "2x4096": (lambda: [M.alignment(2, 4096, 484, "between"), M.alignment(2, 4096, 31, "behind")], False),
    "3x4096": (lambda: [M.alignment(3, 4096, 4096, "front"), M.alignment(3, 4096, 2000, "between")], False),
    "2x4097": (lambda: [M.alignment(2, 4097, 1, "front"), M.alignment(2, 4097, 400, "between")], False),
    "17x40": (lambda: [M.alignment(17, 40, k, "between") for k in (1, 33, 40)], True),       # 136 pairs
    "33x12": (lambda: [M.alignment(33, 12, k, "between") for k in (1, 6, 12)], True),        # 528 pairs, K < 32
}
_E = {}


@pytest.mark.parametrize("name", list(EDGES))
def test_site_and_pair_count_edges_through_the_forward(eng, name):
    build, alone = EDGES[name]
    if name not in _E:
        _E[name] = frozen(build())
    idx = _E[name]
    B, n, l = idx.shape
    assert pairs(n) * l < 20000
    eng.set_option("debug_keep", 1)
    for mode in (1, 2):
        eng.set_option("main_dedup", mode)
        eng.forward(idx)
        ucount = check_class_taps(eng, idx)
        nf, ns, *_ = check_plan_tap(eng, ucount, pairs(n), l, mode)
        if l > 4096:                                        # the identity map: option 1 all fused, option 2 4,097 classes of one site
            assert np.all(ucount == l) and (nf, ns) == ((B, 0) if mode == 1 else (0, B))
    eng.set_option("debug_keep", 0)
    out = per_option(eng, lambda: eng.forward(idx))
    assert np.isfinite(out[0, 1]).all()
    for key, got in out.items():
        assert same(got, out[0, 1]), (name, key)
    if alone:
        for mode in (1, 2):
            eng.set_option("main_dedup", mode)
            for b in range(B):
                assert same(eng.forward(idx[b]), out[0, 1][b]), (name, mode, b)


# ---- f: profile accounting -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("two_streams", [1, 0])
def test_profile_counts_one_main_per_block_and_run(weights, two_streams):
    idx = batch_c(6, 70)[[0, 3, 8, 13]]                     # K = 1, 31, 33 and 70: both routes under option 1
    nb = weights("pf").n_blocks
    runs = 2 if two_streams else 1
    with Engine(weights("pf"), device=0) as e:
        e.set_option("precise", 0)
        e.set_option("two_streams", two_streams)
        e.set_option("profile", 1)
        for mode in (0, 1, 2):
            e.set_option("main_dedup", mode)
            e.profile_reset()
            e.forward(idx)
            assert e.profile_get("main")[0] == nb * runs, (mode, e.profile_get("main"))
            assert e.profile_get("site_classes")[0] == runs, (mode, e.profile_get("site_classes"))
