"""-m gpu: every distinct alignment column is walked once (k_site_classes, option ``site_dedup``).

k_colstats computes the column statistics of the first site of every class of equal columns only; k_colfin and k_main
read a repeated site's partials and q' at that first site.  No sum changes its order, so everything here is bit for bit:

  * ``pf_site_classes`` against first-occurrence classes formed in numpy (and ``weights_sites.compress_sites``);
  * the premise, on the hardware, with ``site_dedup = 0``: the tokens of a repeated column equal those of its first
    occurrence after every block (``x<k>``), and so do the column contexts (``ctx<k>``);
  * ``site_dedup = 1`` against ``0`` with ``np.array_equal`` on every path that goes through the blocks.

Alignments are built by hand from a few random columns.  Shapes: (4, 33) and (6, 70) flat tiling with tiles over two
rows and a ragged last chunk of sites, (5, 64) row tiling, (6, 40) and (7, 40) with ``colstats_fine`` forced both ways
((7, 40): 21 pairs, three runs of 8 - the smallest shape at which one block per run differs from one per group).
"""
import numpy as np
import pytest

from phyloformer_amd import weights_sites as ws

pytestmark = pytest.mark.gpu
SHAPES = [(4, 33), (6, 70), (5, 64), (6, 40)]
PATTERNS = ["none", "all", "big_class", "far", "last_seq", "first_seq", "mixed"]


def distinct_columns(rng, n, k):
    """k pairwise different columns of n residues, every code 0..21 (gaps, 21, included) in play."""
    cols = {}
    while len(cols) < k:
        c = rng.integers(0, 22, n).astype(np.uint8)
        cols.setdefault(c.tobytes(), c)
    return np.stack(list(cols.values()), axis=1)          # [n, k]


def alignment(n, l, pattern, seed=0):
    rng = np.random.default_rng(1000 * n + l + seed)
    pool = distinct_columns(rng, n, l)
    pick = np.arange(l)
    if pattern == "all":                                    # ucount = 1
        pick[:] = 0
    elif pattern == "big_class":                            # one class of more than 32 members, scattered
        members = rng.permutation(l)[:min(l - 2, 40)]
        pick[members] = members.min()
    elif pattern == "far":                                  # first occurrence as far back as the shape allows (>= 32 sites)
        pick[l - 1] = 0
        pick[l - 2] = 1 if l > 35 else pick[l - 2]
    elif pattern == "last_seq":                             # columns that differ in the last sequence only
        a = np.repeat(pool[:, :1], l, axis=1)
        a[n - 1] = (np.arange(l) * 5) % 22                  # (l > 22: repeats among them)
        return np.ascontiguousarray(a)
    elif pattern == "first_seq":                            # ... and in sequence 0 only
        a = np.repeat(pool[:, :1], l, axis=1)
        a[0] = (np.arange(l) * 7) % 22
        return np.ascontiguousarray(a)
    elif pattern == "mixed":                                # about l / 2 distinct columns
        pick = rng.integers(0, max(1, l // 2), l)
    return np.ascontiguousarray(pool[:, pick])


def classes(a):
    """(srep, ucount) of uint8[N, L]: the first site with an equal column."""
    seen, srep = {}, np.empty(a.shape[1], np.int32)
    for l in range(a.shape[1]):
        srep[l] = seen.setdefault(a[:, l].tobytes(), l)
    return srep, len(seen)


def three(n, l):
    """ucount = 1, about l / 2 and l in one batch."""
    return np.stack([alignment(n, l, "all"), alignment(n, l, "mixed"), alignment(n, l, "none")])


@pytest.fixture()
def eng(engines):
    e = engines("pf", precise=0)
    yield e
    for key, value in (("site_dedup", 1), ("debug_keep", 0), ("colstats_fine", -1), ("colstats_ring", 1), ("materialize_x0", 0)):
        e.set_option(key, value)


def on_off(e, call):
    e.set_option("site_dedup", 1)
    on = call()
    e.set_option("site_dedup", 0)
    off = call()
    e.set_option("site_dedup", 1)
    return on, off


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ---- the classes ----------------------------------------------------------------------------------------------------

# two rounds of the kernel's threads; its table full; one site; the sequence cap (the byte loops are unrolled by 8: 200 is a
# multiple of it, 9 is not)
@pytest.mark.parametrize("n,l", SHAPES + [(3, 1100), (3, 4096), (22, 1), (200, 40), (9, 40)])
def test_site_classes_are_numpys_first_occurrences(eng, n, l):
    alns = [alignment(n, l, p) for p in PATTERNS if l > 2] + [alignment(n, l, "mixed", seed=s) for s in (1, 2)]
    rng = np.random.default_rng(l)
    alns.append(rng.integers(0, 22, (n, l)).astype(np.uint8))
    alns.append(rng.integers(20, 22, (n, l)).astype(np.uint8))            # two letters, gaps among them: many repeats
    idx = np.stack(alns)
    srep, ucount = eng.site_classes(idx)
    for b, a in enumerate(alns):
        want, k = classes(a)
        assert np.array_equal(srep[b], want), (b, np.flatnonzero(srep[b] != want)[:8])
        assert ucount[b] == k == len(ws.compress_sites(a)[0])
        assert np.array_equal(np.flatnonzero(want == np.arange(l)), ws.compress_sites(a)[0])
    one_srep, one_k = eng.site_classes(alns[1])
    assert np.array_equal(one_srep, srep[1]) and one_k == ucount[1]
    eng.set_option("site_dedup", 0)
    srep, ucount = eng.site_classes(idx)
    assert np.array_equal(srep, np.tile(np.arange(l, dtype=np.int32), (len(alns), 1))) and np.all(ucount == l)


def test_equal_hashes_over_different_bytes_are_told_apart(eng):
    """Two different columns with the same 32-bit FNV-1a hash (the kernel's pre-filter; found here by birthday search
    over random bytes - pf_site_classes compares bytes as they are): the later one is a class of its own, its repeat
    joins IT, and a repeat of the earlier one still finds the earlier one behind the false candidate."""
    n, l = 6, 40
    rng = np.random.default_rng(7)
    cols = rng.integers(0, 256, (300_000, n)).astype(np.uint64)
    hv = np.full(len(cols), 0x811C9DC5, np.uint64)
    for k in range(n):
        hv = ((hv ^ cols[:, k]) * np.uint64(0x01000193)) & np.uint64(0xFFFFFFFF)
    order = np.argsort(hv, kind="stable")
    hit = np.flatnonzero((hv[order][1:] == hv[order][:-1]) & (cols[order][1:] != cols[order][:-1]).any(axis=1))
    assert len(hit), "no collision among 300,000 columns: 2^-33 per pair, about ten expected"
    ca, cb = cols[order[hit[0]]].astype(np.uint8), cols[order[hit[0] + 1]].astype(np.uint8)
    a = distinct_columns(rng, n, l)
    a[:, 0], a[:, 5], a[:, 9], a[:, 12], a[:, 39] = ca, cb, cb, ca, cb
    want, k = classes(a)
    assert want[5] == 5 and want[9] == 5 and want[12] == 0 and want[39] == 5 and k == l - 3
    srep, ucount = eng.site_classes(a)
    assert np.array_equal(srep, want) and ucount == k


def test_site_classes_beyond_the_table_are_the_identity(eng):
    idx = np.zeros((2, 2, 4097), np.uint8)
    srep, ucount = eng.site_classes(idx)
    assert np.array_equal(srep, np.tile(np.arange(4097, dtype=np.int32), (2, 1))) and np.all(ucount == 4097)
    with pytest.raises(ValueError):
        eng.site_classes(np.zeros((1, 2, 0), np.uint8))


# ---- the premise ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,l", SHAPES)
def test_repeated_columns_carry_equal_tokens_through_every_block(eng, weights, n, l):
    """site_dedup = 0: every site is computed; what the de-duplication relies on must hold on the hardware."""
    nb = weights("pf").n_blocks
    idx = np.stack([alignment(n, l, "mixed"), alignment(n, l, "big_class"), alignment(n, l, "last_seq")])
    P = n * (n - 1) // 2
    eng.set_option("site_dedup", 0)
    eng.set_option("debug_keep", 1)
    eng.forward(idx)
    for b in range(len(idx)):
        srep, k = classes(idx[b])
        assert k < l
        for blk in range(nb + 1):
            x = eng.debug_read(f"x{blk}").reshape(len(idx), P, l, 64)[b].view(np.uint32)
            assert np.array_equal(x, x[:, srep]), (b, blk)
        for blk in range(nb):
            c = eng.debug_read(f"ctx{blk}").reshape(len(idx), l, 64)[b].view(np.uint32)
            assert np.array_equal(c, c[srep]), (b, blk)


# ---- on against off -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,l", SHAPES)
def test_forward_keeps_its_bits_in_a_batch_and_alone(eng, n, l):
    idx = three(n, l)
    assert [classes(a)[1] for a in idx] == [1, classes(idx[1])[1], l] and 1 < classes(idx[1])[1] < l
    on, off = on_off(eng, lambda: eng.forward(idx))
    assert same(on, off)
    for b in range(3):
        assert same(eng.forward(idx[b]), on[b]), b


@pytest.mark.parametrize("n,l", SHAPES)
def test_sharded_and_emulated_shards_keep_their_bits(eng, n, l):
    idx = three(n, l)
    for call in (lambda: eng.forward_sharded(idx, 0, l, l),
                 lambda: eng.forward_shards_emulated(idx, 2),           # (the cuts go through the classes)
                 lambda: eng.forward_shards_emulated(idx, 4)):
        on, off = on_off(eng, call)
        assert same(on, off)


@pytest.mark.parametrize("n,l", SHAPES)
def test_weighted_forward_keeps_its_bits_with_different_weights_inside_a_class(eng, n, l):
    idx = three(n, l)
    wt = (1 + np.arange(3 * l, dtype=np.float32).reshape(3, l) % 5) * 0.5       # members of a class weigh differently
    wt[:, 1] = 0
    on, off = on_off(eng, lambda: eng.forward_weighted(idx, wt))
    assert same(on, off)


@pytest.mark.parametrize("n,l", SHAPES)
@pytest.mark.parametrize("option", ["colstats_ring", "materialize_x0"])
def test_register_prefetch_and_materialised_x0_keep_their_bits(eng, n, l, option):
    idx = three(n, l)
    want = eng.forward(idx)
    eng.set_option(option, 0 if option == "colstats_ring" else 1)
    on, off = on_off(eng, lambda: eng.forward(idx))
    assert same(on, off) and same(on, want)


@pytest.mark.parametrize("n,l", [(6, 40), (7, 40)])
@pytest.mark.parametrize("fine", [0, 1])
def test_blocks_per_group_and_per_run_keep_their_bits(eng, n, l, fine):
    idx = three(n, l)
    want = eng.forward(idx)
    eng.set_option("colstats_fine", fine)
    on, off = on_off(eng, lambda: eng.forward(idx))
    assert same(on, off) and same(on, want)
    assert same(eng.forward(idx[1]), on[1])


@pytest.mark.parametrize("n,l", SHAPES)
def test_taps_keep_their_bits(eng, weights, n, l):
    nb = weights("pf").n_blocks
    idx = three(n, l)
    names = [f"x{k}" for k in range(nb + 1)] + [f"ctx{k}" for k in range(nb)]
    eng.set_option("debug_keep", 1)

    def taps():
        eng.forward(idx)
        return [eng.debug_read(name) for name in names]
    on, off = on_off(eng, taps)
    for name, a, b in zip(names, on, off):
        assert a.size and same(a, b), name
