"""-m gpu: tiled inference on the device - pf_forward_tiled against pf_forward_taxa of every set fed through the host
twin tile.combine, bit for bit, where the sets take different routes in one call; batch and chunk invariance; the
combination alone on device arrays; refusals; the cap lifted for N; and the CLI's --tile on a temporary directory."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.profiled import Profiled as _Profiled
from phyloformer_amd import tile as TL
from phyloformer_amd.engine import Engine
from phyloformer_amd.taxa import pair_index

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("main", "precise", "gather_taxa", "tile_combine")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _random(B, N, L, seed):
    return np.random.default_rng(seed).integers(0, 22, size=(B, N, L), dtype=np.uint8)


def _set_distances(e, idx, M):
    """Every set of the plan through pf_forward_taxa - one call per set size, since a taxon table has one width - as the
    list of S arrays float32 [B, P_m] in (g, h) order."""
    p = TL.plan(idx.shape[1], M)
    rows = [p.set_rows(k) for k in range(p.S)]
    sets = [None] * p.S
    for m in sorted({len(r) for r in rows}):
        ks = [k for k in range(p.S) if len(rows[k]) == m]
        res = e.forward_taxa(idx, np.stack([rows[k] for k in ks]).astype(np.int32))
        for j, k in enumerate(ks):
            sets[k] = np.ascontiguousarray(res[:, j])
    return sets


def _assert_same(got, want, N, M, what=""):
    """out and spread bit for bit; the cross-group entries of out are direct copies of the sets' values."""
    out, spread = got
    assert out.dtype == spread.dtype == np.float32 and out.shape == spread.shape == want[0].shape
    assert np.array_equal(_bits(out), _bits(want[0])), f"{what}: out differs in {(_bits(out) != _bits(want[0])).sum()} entries"
    assert np.array_equal(_bits(spread), _bits(want[1])), f"{what}: spread differs in {(_bits(spread) != _bits(want[1])).sum()} entries"


def _assert_cross_copies(out, spread, sets, N, M):
    p = TL.plan(N, M)
    for k, (g, h) in enumerate(p.sets):
        ng = p.rows(g)
        for a, i in enumerate(range(p.bounds[g], p.bounds[g + 1])):
            for c, j in enumerate(range(p.bounds[h], p.bounds[h + 1])):
                q = pair_index(i, j, N)
                assert np.array_equal(_bits(out[:, q]), _bits(sets[k][:, pair_index(a, ng + c, ng + p.rows(h))])), (i, j)
                assert (_bits(spread[:, q]) == 0).all(), (i, j)          # +0.0 exactly


def _tiled(e, idx, M):
    with _Profiled(e):
        res = e.forward_tiled(idx, M)
        counts = {k: e.profile_get(k)[0] for k in KERNELS}
        counts["rechecked"] = e.rechecked_count()
    return res, counts


def test_three_set_sizes_on_the_float64_route(engines):
    """N = 10, M = 6, L = 40: groups of 2, 3, 2, 3 rows, sets of 4, 5 and 6 rows, all below 8,192 pair-site tokens."""
    e = engines("pf")
    N, M, L = 10, 6, 40
    idx = _random(2, N, L, seed=1906)
    p = TL.plan(N, M)
    assert np.diff(p.bounds).tolist() == [2, 3, 2, 3] and sorted({len(p.set_rows(k)) for k in range(p.S)}) == [4, 5, 6]
    got, counts = _tiled(e, idx, M)
    print(f"{N} x {L}, M = {M}: launches {counts}")
    assert counts["main"] == 0 and counts["precise"] > 0 and counts["gather_taxa"] >= 3 and counts["tile_combine"] == 1
    sets = _set_distances(e, idx, M)
    _assert_same(got, TL.combine(sets, N, M), N, M, "10 x 40")
    _assert_cross_copies(*got, sets, N, M)
    within = [pair_index(i, j, N) for g in range(p.G) for i in range(p.bounds[g], p.bounds[g + 1]) for j in range(i + 1, p.bounds[g + 1])]
    assert (got[1][:, within] > 0).all()                               # context dependence: the contexts disagree


@pytest.fixture(scope="module")
def mixed(engines):
    """N = 13, M = 8, L = 400, B = 2: sets of 6 rows (6,000 tokens: float64) and of 7 rows (8,400: the default kernels) in
    one call; computed once and left unchanged."""
    e = engines("pf")
    idx = _random(2, 13, 400, seed=1913)
    got, counts = _tiled(e, idx, 8)
    return idx, got, counts


def test_both_routes_in_one_call(engines, mixed):
    e = engines("pf")
    idx, got, counts = mixed
    p = TL.plan(13, 8)
    assert np.diff(p.bounds).tolist() == [3, 3, 3, 4] and sorted({len(p.set_rows(k)) for k in range(p.S)}) == [6, 7]
    print(f"13 x 400, M = 8: launches {counts}")
    assert counts["main"] > 0 and counts["precise"] > 0 and counts["tile_combine"] == 1
    sets = _set_distances(e, idx, 8)
    _assert_same(got, TL.combine(sets, 13, 8), 13, 8, "13 x 400")
    _assert_cross_copies(*got, sets, 13, 8)


def test_batch_and_chunk_invariance(weights, mixed):
    """Source 1 of B = 2 against the same source alone, and alone again under a workspace budget of 1 MB, which cuts each
    class into several chunks (more gathers)."""
    idx, whole, _counts = mixed
    with Engine(weights("pf"), 0) as e:
        alone, c_default = _tiled(e, idx[1], 8)
        e.set_option("ws_limit_mb", 1)
        chunked, c_chunked = _tiled(e, idx[1], 8)
    print(f"gather launches: {c_default['gather_taxa']} by default, {c_chunked['gather_taxa']} under ws_limit_mb = 1")
    assert c_chunked["gather_taxa"] > c_default["gather_taxa"] >= 2
    for name, a, c, w in zip(("out", "spread"), alone, chunked, whole):
        assert np.array_equal(_bits(a), _bits(w[1])), name
        assert np.array_equal(_bits(c), _bits(w[1])), name


def test_combine_device_alone_and_profile_count(weights):
    """N = 13, M = 8, L = 600: every set on the default kernels (6 rows: 9,000 tokens).  pf_tile_combine_device on the
    uploaded host-assembled [B][T] gives pf_forward_tiled's bits; the profile counts the launches."""
    N, M, L, B = 13, 8, 600, 2
    idx = _random(B, N, L, seed=1919)
    with Engine(weights("pf"), 0) as e:
        got, counts = _tiled(e, idx, M)
        print(f"{N} x {L}, M = {M}: launches {counts}")
        assert counts["main"] > 0 and counts["tile_combine"] == 1
        assert counts["precise"] == 0 or counts["rechecked"] > 0      # float64 only through the range re-check
        sets = _set_distances(e, idx, M)
        _assert_same(got, TL.combine(sets, N, M), N, M, "13 x 600")
        flat = TL.assemble(sets)
        p = TL.plan(N, M)
        assert flat.shape == (B, p.T)
        out, spread = np.empty((B, N * (N - 1) // 2), np.float32), np.empty((B, N * (N - 1) // 2), np.float32)
        bufs = [e.malloc(a.nbytes) for a in (flat, out, spread)]
        try:
            e.h2d(bufs[0], flat)
            with _Profiled(e):
                e.tile_combine_device(bufs[0], B, N, M, bufs[1], bufs[2])
                e.tile_combine_device(bufs[0], B, N, M, bufs[1], bufs[2])
                e.d2h(out, bufs[1])
                e.d2h(spread, bufs[2])
                e.synchronize()
                assert e.profile_get("tile_combine")[0] == 2
        finally:
            for ptr in bufs:
                e.free(ptr)
        _assert_same((out, spread), got, N, M, "pf_tile_combine_device")
        e.profile_reset()                                           # profiling off: nothing is counted
        e.forward_tiled(idx[0], M)
        assert e.profile_get("tile_combine")[0] == 0


def test_refusals_leave_outputs_untouched(weights):
    idx = _random(1, 202, 4, seed=1923)
    with Engine(weights("pf"), 0) as e:
        e.set_option("profile", 1)
        e.profile_reset()
        lib, h = e._lib, e._h
        out, spread = np.full(32768, -7.0, np.float32), np.full(32768, -7.0, np.float32)

        def refused(rc, text):
            assert rc == -1 and text.encode() in lib.pf_last_error(h), (rc, lib.pf_last_error(h))
            assert (out == -7.0).all() and (spread == -7.0).all()

        ptr = idx.ctypes.data
        refused(lib.pf_forward_tiled(h, ptr, 1, 6, 4, 6, out.ctypes.data, spread.ctypes.data), "call pf_forward")       # N == M
        refused(lib.pf_forward_tiled(h, ptr, 1, 5, 4, 6, out.ctypes.data, spread.ctypes.data), "call pf_forward")       # N < M
        refused(lib.pf_forward_tiled(h, ptr, 1, 10, 4, 1, out.ctypes.data, spread.ctypes.data), "M >= 2")
        refused(lib.pf_forward_tiled(h, ptr, 1, 202, 4, 201, out.ctypes.data, spread.ctypes.data),
                "n_seqs must be smaller or equal to 200")
        bad = idx.copy()
        bad[0, 9, 3] = 22
        refused(lib.pf_forward_tiled(h, bad.ctypes.data, 1, 10, 4, 6, out.ctypes.data, spread.ctypes.data), "residue index 22")
        refused(lib.pf_forward_tiled(h, ptr, 1, 10, 4, 6, out.ctypes.data, None), "null buffer")
        refused(lib.pf_forward_tiled(h, ptr, 1, 10, 4, 6, None, spread.ctypes.data), "null buffer")
        refused(lib.pf_forward_tiled(h, None, 1, 10, 4, 6, out.ctypes.data, spread.ctypes.data), "null buffer")
        refused(lib.pf_forward_tiled(h, ptr, 0, 10, 4, 6, out.ctypes.data, spread.ctypes.data), "bad dimensions")
        refused(lib.pf_forward_tiled(h, ptr, 1, 10, 0, 6, out.ctypes.data, spread.ctypes.data), "bad dimensions")
        assert all(e.profile_get(k)[0] == 0 for k in KERNELS)
        with pytest.raises(ValueError, match="call pf_forward"):
            e.forward_tiled(idx[:, :6], 6)
        with pytest.raises(ValueError, match="M >= 2"):
            e.forward_tiled(idx[:, :10], 1)
        # the handle still works
        small = np.ascontiguousarray(idx[:, :10])
        got = e.forward_tiled(small, 6)
        _assert_same(got, TL.combine(_set_distances(e, small, 6), 10, 6), 10, 6, "after the refusals")


def test_cap_is_checked_against_the_context_not_against_n(weights):
    """M = 200, max_seqs untouched, L = 8, N = 201: three sets of 134 rows, on the float64 route (fewer than 32 sites).
    pf_forward refuses the 201 rows; the sets are compared with pf_forward of the host-cut sets."""
    N, M, L = 201, 200, 8
    idx = _random(1, N, L, seed=1931)
    p = TL.plan(N, M)
    assert p.G == 3 and [len(p.set_rows(k)) for k in range(p.S)] == [134, 134, 134]
    with Engine(weights("pf"), 0) as e:
        with pytest.raises(ValueError, match="n_seqs must be smaller or equal to 200"):
            e.forward(idx)
        got, counts = _tiled(e, idx, M)
        print(f"{N} x {L}, M = {M}: launches {counts}")
        assert counts["main"] == 0 and counts["precise"] > 0 and counts["tile_combine"] == 1
        sets = [e.forward(s) for s in TL.cut_sets(idx, M)]
    assert got[0].shape == (1, N * (N - 1) // 2) and np.isfinite(got[0]).all() and (got[0] > 0).all()
    _assert_same(got, TL.combine(sets, N, M), N, M, "201 x 8")


# ---- CLI ---------------------------------------------------------------------------------------------------------------

def _write_fasta(path, idx):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">s{k}\n{''.join(alpha[int(v)] for v in row)}\n")


def test_cli_tile_on_a_large_and_a_small_file(tmp_path, engines):
    from phyloformer_amd.nj import neighbor_joining
    from phyloformer_amd.phylip import vec_to_phylip
    alns = {"big7": _random(1, 7, 40, seed=1941)[0], "small3": _random(1, 3, 40, seed=1942)[0]}
    msas = tmp_path / "msas"
    msas.mkdir()
    for stem, a in alns.items():
        _write_fasta(msas / f"{stem}.fa", a)
    r = subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf.ckpt"), str(msas),
                        "-o", str(tmp_path / "out"), "-t", "--tile", "4"], capture_output=True, text=True, cwd=REPO, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    files = {n: open(os.path.join(tmp_path / "out", n), "rb").read().decode() for n in sorted(os.listdir(tmp_path / "out"))}
    assert set(files) == {"big7.phy", "big7.nj.nwk", "big7.spread.phy", "big7.tile.tsv", "small3.phy", "small3.nj.nwk"}
    e = engines("pf")

    def tree(vec, ids):
        return neighbor_joining(vec_to_phylip(vec, ids)[0].astype("float64"), ids)

    ids7, ids3 = [f"s{k}" for k in range(7)], [f"s{k}" for k in range(3)]
    out, spread = e.forward_tiled(alns["big7"], 4)
    assert files["big7.phy"] == vec_to_phylip(out, ids7)[1] and files["big7.spread.phy"] == vec_to_phylip(spread, ids7)[1]
    assert files["big7.nj.nwk"] == tree(out, ids7) and files["big7.tile.tsv"] == TL.tile_tsv(ids7, 4)
    plain = e.forward(alns["small3"])
    assert files["small3.phy"] == vec_to_phylip(plain, ids3)[1] and files["small3.nj.nwk"] == tree(plain, ids3)
