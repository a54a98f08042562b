"""-m gpu: site maps on the device - k_gather_sites' bytes, the bit-identity of forward_windows / forward_sites with
forward of the host-cut alignments on every path, parity with the oracle, refusals, and the CLI's --windows on the 20
test MSAs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from phyloformer_amd import windows as pw
from phyloformer_amd.engine import Engine
from phyloformer_amd.msa_sim import simulate_batch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_sites(e, idx, sites):
    """forward_sites against forward of cut_sites, bit for bit; idx [B][N][L]."""
    B, N, _L = idx.shape
    S, K = np.asarray(sites).shape
    got = e.forward_sites(idx, sites)
    want = e.forward(pw.cut_sites(idx, sites).reshape(B * S, N, K)).reshape(B, S, -1)
    assert got.shape == want.shape == (B, S, N * (N - 1) // 2) and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want))
    return got


def _check_windows(e, idx, W, step):
    B, N, L = idx.shape
    sites = pw.window_sites(L, W, step)
    got = e.forward_windows(idx, W, step)
    want = e.forward(pw.cut_sites(idx, sites).reshape(B * len(sites), N, W)).reshape(B, len(sites), -1)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want))
    # the affine and the table map give the same bits
    assert np.array_equal(_bits(e.forward_sites(idx, sites)), _bits(got))
    return got


# ---- bit identity with forward of the host-cut alignments ----------------------------------------------------------

def test_windows_bitwise_default_kernels_row_tiling(engines):
    e = engines("pf")
    e.set_option("profile", 1)
    e.profile_reset()
    try:
        got = _check_windows(e, simulate_batch(1, 60, 512, seed=61), 128, 64)
        assert got.shape == (1, 7, 1770)
        assert e.profile_get("main")[0] > 0 and e.profile_get("precise")[0] == 0 and e.profile_get("gather")[0] >= 2
    finally:
        e.set_option("profile", 0)


def test_windows_bitwise_default_kernels_flat_tiling_anchored_last_window(engines):
    e = engines("pf")
    assert pw.window_starts(500, 200, 120) == [0, 120, 240, 300]
    idx = simulate_batch(1, 20, 500, seed=62)
    got = _check_windows(e, idx, 200, 120)
    # 2-D input gives [S][P]; the last window is the one anchored at L - W
    one = e.forward_windows(idx[0], 200, 120)
    assert one.shape == (4, 190) and np.array_equal(_bits(one), _bits(got[0]))
    assert np.array_equal(_bits(one[3]), _bits(e.forward(idx[0][:, 300:500])))


def test_windows_bitwise_float64_route_by_site_count(engines):
    e = engines("pf")
    e.set_option("profile", 1)
    e.profile_reset()
    try:
        _check_windows(e, simulate_batch(2, 20, 200, seed=63), 24, 20)
        assert e.profile_get("precise")[0] > 0 and e.profile_get("main")[0] == 0
    finally:
        e.set_option("profile", 0)


def test_windows_bitwise_float64_route_by_token_count(engines):
    e = engines("pf")
    e.set_option("profile", 1)
    e.profile_reset()
    try:
        _check_windows(e, simulate_batch(2, 8, 300, seed=64), 100, 70)        # 28 pairs x 100 sites < 8,192 tokens
        assert e.profile_get("precise")[0] > 0 and e.profile_get("main")[0] == 0
    finally:
        e.set_option("profile", 0)


def test_windows_three_sources_in_one_call_against_one_by_one(engines):
    e = engines("pf")
    idx = simulate_batch(3, 20, 500, seed=65)
    got = _check_windows(e, idx, 200, 120)
    for b in range(3):
        assert np.array_equal(_bits(e.forward_windows(idx[b:b + 1], 200, 120)[0]), _bits(got[b]))


@pytest.mark.parametrize("ws_mb", [24, 64, 400])
def test_windows_bitwise_across_chunks(weights, ws_mb):
    """A small workspace budget: the 9 windows of one source span several chunks (runs of one source's windows)."""
    with Engine(weights("pf"), 0) as e:
        e.set_option("ws_limit_mb", ws_mb)
        e.set_option("profile", 1)
        e.profile_reset()
        got = e.forward_windows(simulate_batch(2, 20, 520, seed=66), 200, 40)
        n_gather = e.profile_get("gather")[0]
        assert got.shape == (2, 9, 190)
        if ws_mb <= 64:                    # (fewer than S = 9 alignments of 20 x 200 fit: several chunks per source)
            assert n_gather >= 4
        _check_windows(e, simulate_batch(2, 20, 520, seed=66), 200, 40)


def test_sites_table_phases_reversed_and_repeated(engines):
    e = engines("pf")
    idx = simulate_batch(2, 20, 600, seed=67)
    rng = np.random.default_rng(67)
    sites = np.stack([np.arange(0, 600, 3), np.arange(1, 600, 3), np.arange(2, 600, 3),      # every third site, 3 phases
                      np.arange(399, 199, -1),                                             # a reversed window
                      np.sort(rng.integers(0, 600, size=200)) // 2 * 2])                    # repeated sites
    assert sites.shape == (5, 200) and np.unique(sites[4]).size < 200
    got = _check_sites(e, idx, sites)
    # int64 tables are accepted, and a reversed window is not the window (the model is not site-order invariant
    # bit for bit), but it is what forward gives for the reversed bytes - checked above
    assert np.array_equal(_bits(e.forward_sites(idx, sites.astype(np.int64))), _bits(got))


def test_windows_recheck_trips_in_exactly_one_window(weights):
    """One source whose third window holds uniformly random residues: that window's distances saturate far above the
    re-check threshold (default 8), the others stay far below; the flagged window is rebuilt from the resident source
    and recomputed in float64, exactly as pf_forward recomputes the host-cut window."""
    idx = simulate_batch(1, 20, 400, seed=51).copy()
    idx[0, :, 200:300] = np.random.default_rng(7).integers(0, 20, size=(20, 100), dtype=np.uint8)
    with Engine(weights("pf"), 0) as e:
        e.profile_reset()
        got = e.forward_windows(idx, 100, 100)
        n_win = e.rechecked_count()
        e.profile_reset()
        want = e.forward(pw.cut_sites(idx, pw.window_sites(400, 100, 100))[0])
        assert n_win == e.rechecked_count() == 1
        assert np.array_equal(_bits(got[0]), _bits(want))
        assert got[0, 2].max() > 8 and np.delete(got[0], 2, axis=0).max() < 8
        e.set_option("recheck_above", 0)
        off = e.forward_windows(idx, 100, 100)
        assert np.array_equal(_bits(np.delete(off[0], 2, axis=0)), _bits(np.delete(got[0], 2, axis=0)))


def test_windows_bitwise_generic_route(weights):
    with Engine(weights("pf"), 0) as e:
        e.set_option("generic", 1)
        e.set_option("profile", 1)
        e.profile_reset()
        _check_windows(e, simulate_batch(2, 10, 80, seed=68), 40, 30)
        assert e.profile_get("generic")[0] > 0 and e.profile_get("main")[0] == 0 and e.profile_get("precise")[0] == 0


# ---- the gather alone ----------------------------------------------------------------------------------------------

def _gather(e, src, sites=None, start=None, K=None, dst_offset=0):
    B, N, L = src.shape
    tab = np.ascontiguousarray(sites if sites is not None else start, dtype=np.int32)
    S = tab.shape[0]
    K = tab.shape[1] if sites is not None else K
    d_src, d_map, d_dst = e.malloc(src.nbytes), e.malloc(tab.nbytes), e.malloc(B * S * N * K + dst_offset)
    try:
        e.h2d(d_src, src)
        e.h2d(d_map, tab)
        e.gather_sites_device(d_src, B, N, L, d_map if sites is not None else None, d_map if sites is None else None, S, K,
                              d_dst + dst_offset)
        got = np.empty((B, S, N, K), np.uint8)
        e.d2h(got, d_dst + dst_offset)
        e.synchronize()
    finally:
        for p in (d_src, d_map, d_dst):
            e.free(p)
    return got


@pytest.mark.parametrize("dst_offset", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 64, 1023, 1024, 1029, 2048])
def test_gather_bytes_match_host_twin(engines, K, dst_offset):
    """K % 4 in {0, 1, 2, 3}, below / at / above one tile of 1024 sites, dst aligned and odd; affine starts of every
    alignment modulo 4 (the source rows are L = 2051 bytes apart: every row has another alignment too)."""
    e = engines("pf")
    rng = np.random.default_rng(K)
    B, N, L = 2, 5, 2051
    src = rng.integers(0, 22, size=(B, N, L), dtype=np.uint8)
    start = np.array([0, 1, 2, 3, L - K] + rng.integers(0, L - K + 1, size=4).tolist(), dtype=np.int32)
    want = pw.cut_sites(src, start[:, None] + np.arange(K)[None, :])
    assert np.array_equal(_gather(e, src, start=start, K=K, dst_offset=dst_offset), want)
    sites = rng.integers(0, L, size=(6, K))
    sites[0] = np.arange(K)[::-1]
    assert np.array_equal(_gather(e, src, sites=sites, dst_offset=dst_offset), pw.cut_sites(src, sites))


def test_gather_more_sets_than_one_grid(engines):
    """S above 65,535 with tiny N, K: the launches split over grid y."""
    e = engines("pf")
    rng = np.random.default_rng(3)
    src = rng.integers(0, 22, size=(1, 2, 5), dtype=np.uint8)
    S = 65535 + 4465
    sites = rng.integers(0, 5, size=(S, 3))
    assert np.array_equal(_gather(e, src, sites=sites), pw.cut_sites(src, sites))
    start = rng.integers(0, 3, size=S).astype(np.int32)
    assert np.array_equal(_gather(e, src, start=start, K=3), pw.cut_sites(src, start[:, None] + np.arange(3)[None, :]))


def test_gather_single_site_source(engines):
    e = engines("pf")
    src = np.arange(6, dtype=np.uint8).reshape(2, 3, 1)
    sites = np.zeros((4, 1), np.int32)
    assert np.array_equal(_gather(e, src, sites=sites), pw.cut_sites(src, sites))
    assert np.array_equal(_gather(e, src, start=np.zeros(4, np.int32), K=1), pw.cut_sites(src, sites))


def test_gather_device_entry_point_refusals(engines):
    e = engines("pf")
    with pytest.raises(ValueError, match="exactly one"):
        e.gather_sites_device(1, 1, 2, 8, 1, 1, 1, 4, 1)
    with pytest.raises(ValueError, match="exactly one"):
        e.gather_sites_device(1, 1, 2, 8, None, None, 1, 4, 1)
    with pytest.raises(ValueError, match="bad dimensions"):
        e.gather_sites_device(1, 1, 2, 8, 1, None, 1, 9, 1)
    with pytest.raises(ValueError, match="null buffer"):
        e.gather_sites_device(None, 1, 2, 8, 1, None, 1, 4, 1)


def test_gather_device_map_out_of_range_is_reported_not_dereferenced(weights):
    """A map that only ever existed on the device cannot be validated up front: an entry outside the source is never
    read through (site 0 stands in) and the next synchronisation says so, once."""
    src = np.arange(2 * 3 * 8, dtype=np.uint8).reshape(2, 3, 8) % 22
    with Engine(weights("pf"), 0) as e:
        for sites, start in ((np.array([[1, 8, 2, -5]]), None), (None, np.array([5], np.int32))):
            with pytest.raises(ValueError, match="site map"):
                _gather(e, src, sites=sites, start=start, K=4)
            e.synchronize()                                    # reported once
        ok = np.array([[1, 7, 2, 0]])
        assert np.array_equal(_gather(e, src, sites=ok), pw.cut_sites(src, ok))


# ---- against the oracle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["0_20_tips.fa", "1_20_tips.fa"])
def test_windows_reference_parity(weights, engines, name):
    from oracle import pf_oracle
    from phyloformer_amd.fasta import load_alignment
    idx, _ids = load_alignment(os.path.join(REPO, "data", "testdata", "msas", name))
    w = weights("pf")
    got = engines("pf").forward_windows(idx, 100, 50)
    cut = pw.cut_sites(idx, pw.window_sites(idx.shape[1], 100, 50))
    assert got.shape[0] == len(cut) == 4
    for s, win in enumerate(cut):
        err = float(np.abs(got[s] - pf_oracle.forward(w.tensors, win)).max())
        print(f"{name} window {s}: max-abs error vs oracle {err:.3e}")
        assert err <= 1e-4


# ---- validation ----------------------------------------------------------------------------------------------------

def test_refusals_leave_out_untouched_and_the_handle_usable(weights):
    idx = simulate_batch(1, 6, 30, seed=69)
    sites = np.ascontiguousarray(pw.window_sites(30, 10, 10), dtype=np.int32)
    with Engine(weights("pf"), 0) as e:
        e.set_option("profile", 1)
        e.profile_reset()
        lib, h = e._lib, e._h
        out = np.full((1, 8, 15), -7.0, np.float32)
        p_idx, p_out, p_sites = idx.ctypes.data, out.ctypes.data, sites.ctypes.data

        def refused(rc, text):
            assert rc == -1 and text.encode() in lib.pf_last_error(h), lib.pf_last_error(h)
            assert (out == -7.0).all()

        def table(entries, S=3, K=10):
            t = np.ascontiguousarray(entries, dtype=np.int32)
            return lib.pf_forward_sites(h, p_idx, 1, 6, 30, t.ctypes.data, S, K, p_out)

        refused(lib.pf_forward_sites(h, p_idx, 1, 6, 30, p_sites, 3, 0, p_out), "1 <= K <= L")
        refused(lib.pf_forward_sites(h, p_idx, 1, 6, 30, p_sites, 1, 31, p_out), "1 <= K <= L")
        refused(lib.pf_forward_sites(h, p_idx, 1, 6, 30, p_sites, 0, 10, p_out), "S >= 1")
        bad = sites.copy()
        bad[2, 9] = 30
        refused(table(bad), "site 30 at set 2, position 9 is outside [0, 30)")
        bad[2, 9], bad[0, 0] = 29, -1
        refused(table(bad), "site -1 at set 0, position 0 is outside [0, 30)")
        refused(lib.pf_forward_sites(h, p_idx, 1, 6, 30, None, 3, 10, p_out), "null buffer")
        refused(lib.pf_forward_sites(h, None, 1, 6, 30, p_sites, 3, 10, p_out), "null buffer")
        assert lib.pf_forward_sites(h, p_idx, 1, 6, 30, p_sites, 3, 10, None) == -1
        refused(lib.pf_forward_sites(h, p_idx, 0, 6, 30, p_sites, 3, 10, p_out), "bad dimensions")
        refused(lib.pf_forward_sites(h, p_idx, 1, 1, 30, p_sites, 3, 10, p_out), "bad dimensions")
        refused(lib.pf_forward_sites(h, p_idx, 1 << 30, 6, 30, p_sites, 1 << 30, 10, p_out), "overflow")
        refused(lib.pf_forward_windows(h, p_idx, 1, 6, 30, 10, 0, p_out, 8), "step >= 1")
        refused(lib.pf_forward_windows(h, p_idx, 1, 6, 30, 0, 5, p_out, 8), "1 <= K <= L")
        refused(lib.pf_forward_windows(h, p_idx, 1, 6, 30, 31, 5, p_out, 8), "1 <= K <= L")
        refused(lib.pf_forward_windows(h, p_idx, 1, 6, 30, 10, 3, p_out, 7), "out holds 7 windows")      # S = 8
        refused(lib.pf_forward_windows(h, p_idx, 1 << 30, 200, 2 ** 31 - 1, 1, 1, p_out, 2 ** 31 - 1), "overflow")
        res = idx.copy()
        res[0, 2, 5] = 22
        refused(lib.pf_forward_sites(h, res.ctypes.data, 1, 6, 30, p_sites, 3, 10, p_out), "residue index 22")
        refused(lib.pf_forward_windows(h, res.ctypes.data, 1, 6, 30, 10, 3, p_out, 8), "residue index 22")
        big = simulate_batch(1, 201, 8, seed=70)
        refused(lib.pf_forward_windows(h, big.ctypes.data, 1, 201, 8, 4, 4, p_out, 8), "n_seqs must be smaller or equal to 200")
        # nothing of all that reached the device
        assert e.profile_get("gather")[0] == 0 and e.profile_get("precise")[0] == 0 and e.profile_get("main")[0] == 0
        # the Python surface raises ValueError, also for what ctypes could not carry
        with pytest.raises(ValueError, match="outside"):
            e.forward_sites(idx, np.array([[0, 30]]))
        with pytest.raises(ValueError, match="outside"):
            e.forward_sites(idx, np.array([[0, 2 ** 40]]))
        with pytest.raises(ValueError):
            e.forward_sites(idx, np.array([[0.0, 1.0]]))
        with pytest.raises(ValueError, match="step >= 1"):
            e.forward_windows(idx, 10, 0)
        with pytest.raises(ValueError, match="1 <= K <= L"):
            e.forward_windows(idx, 31)
        assert e.profile_get("gather")[0] == 0
        # the handle still works
        assert lib.pf_forward_windows(h, p_idx, 1, 6, 30, 10, 3, p_out, 8) == 0
        want = e.forward(pw.cut_sites(idx, pw.window_sites(30, 10, 3))[0])
        assert np.array_equal(_bits(out[0]), _bits(want)) and e.profile_get("gather")[0] >= 1


# ---- CLI on the 20 test MSAs ---------------------------------------------------------------------------------------

def _run(args):
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, timeout=900)


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_cli_windows_on_test_msas(tmp_path, engines):
    from phyloformer_amd.fasta import load_alignment
    from phyloformer_amd.phylip import vec_to_phylip
    msas = os.path.join(REPO, "data", "testdata", "msas")
    plain = _run([msas, "-o", str(tmp_path / "plain"), "-t"])
    win = _run([msas, "-o", str(tmp_path / "win"), "-t", "--windows", "100:50"])
    assert plain.returncode == 0 and win.returncode == 0, plain.stderr[-2000:] + win.stderr[-2000:]
    p, w = _files(tmp_path / "plain"), _files(tmp_path / "win")
    stems = sorted(n[:-3] for n in os.listdir(msas) if n.endswith(".fa"))
    labels = ["w001-100", "w051-150", "w101-200", "w151-250"]                 # every test MSA has 250 sites
    want = set(p) | {f"{s}.windows.tsv" for s in stems} | {f"{s}.{lab}.{ext}" for s in stems for lab in labels
                                                           for ext in ("phy", "nj.nwk")}
    assert len(stems) == 20 and set(w) == want
    for name, data in p.items():
        assert w[name] == data, name                           # <stem>.phy and <stem>.nj.nwk unchanged
    e = engines("pf_base")
    for s in stems:
        idx, ids = load_alignment(os.path.join(msas, f"{s}.fa"))
        assert idx.shape[1] == 250
        cut = pw.cut_sites(idx, pw.window_sites(250, 100, 50))
        for lab, win_idx in zip(labels, cut):
            assert w[f"{s}.{lab}.phy"].decode() == vec_to_phylip(e.forward(win_idx), ids)[1], (s, lab)
        rows = w[f"{s}.windows.tsv"].decode().splitlines()
        assert rows[0] == "first\tlast\tmean_distance\trf_prev\trf_full" and len(rows) == 5
        assert [r.split("\t")[:2] for r in rows[1:]] == [["1", "100"], ["51", "150"], ["101", "200"], ["151", "250"]]
        assert rows[1].split("\t")[3] == "NA" and all(v.isdigit() for r in rows[2:] for v in r.split("\t")[3:])
    pyio = _run([msas, "-o", str(tmp_path / "pyio"), "-t", "--windows", "100:50", "--python-io"])
    assert pyio.returncode == 0 and _files(tmp_path / "pyio") == w, pyio.stderr[-2000:]
    one = _run([msas, "-o", str(tmp_path / "one"), "-t", "--windows", "100:50", "--batch", "1"])
    assert one.returncode == 0 and _files(tmp_path / "one") == w, one.stderr[-2000:]
