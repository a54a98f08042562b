"""-m gpu: site weights - pf_forward_weighted / _device, pf_forward_sites_weighted, pf_bootstrap_weighted
(k_main<.., WEIGHTED>, k_embed<WEIGHTED>, k_weight_sums, the weighted float64 kernels) and ``infer_alns.py --compress-sites``.

Bounds (none of them from what the code under test gives):
  * unit weights           pf_forward's bits on every path (1.f * x is exact, W = L is exact)
  * weights scaled by 1/4  the same bits (a power of two commutes with every rounding, nothing under- or overflows here)
  * against a yardstick    max |out - float64 oracle| <= 1e-4, the project's parity bound; the oracle sees the alignment the
                           weights stand for (integer weights: every site repeated; zero weights: the sites cut out;
                           bootstrap: the replicate of bootstrap.resample_sites), and pf_forward of that alignment is
                           held to the same bound
  * default vs float64     fractional weights have no expanded alignment: the default kernels against ``precise = 1`` on
                           the same weights, <= 1e-4
  * pf_bootstrap_weighted against pf_bootstrap: printed; both sit within 1e-4 of the oracle, so <= 2e-4 (the triangle)
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pf_oracle as O
from phyloformer_amd import weights_sites as ws
from phyloformer_amd.bootstrap import resample_sites
from phyloformer_amd.msa_sim import simulate_batch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSAS = os.path.join(REPO, "data", "testdata", "msas")
BOUND = 1e-4
SHAPES = [(20, 256), (20, 250), (24, 33), (20, 200)]         # row tiling, flat tiling, a tile over two rows, ragged row tiles (forced)
F64_SHAPES = [(5, 16), (10, 40)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _oracle_many(w, alns):
    """float64 oracle of a list of alignments (threads: numpy releases the GIL)."""
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda a: O.forward(w.tensors, a, n_blocks=w.n_blocks, n_heads=w.n_heads, dtype=np.float64), alns))


def _engine(weights, monkeypatch, n, l, precise=0):
    """A fresh engine; (20, 200) runs with row tiles forced, as tests/test_gpu_sitemap.py forces them."""
    from phyloformer_amd.engine import Engine
    if (n, l) == (20, 200):
        monkeypatch.setenv("PF_ROW_TILES", "1")
    e = Engine(weights("pf"), 0)
    e.set_option("precise", precise)
    return e


def _int_weights(rng, B, L):
    """Counts in 0..3 with at least one zero and one repeat per alignment."""
    wt = rng.integers(0, 4, (B, L)).astype(np.float32)
    wt[:, 0], wt[:, 1], wt[:, L // 2] = 2, 0, 3
    return wt


# ---- unit weights and scaling: bit for bit -------------------------------------------------------------------------

@pytest.mark.parametrize("n,l", SHAPES)
@pytest.mark.parametrize("fold", [1, 0])
def test_unit_weights_give_forwards_bits_on_the_default_kernels(weights, monkeypatch, n, l, fold):
    idx = simulate_batch(3, n, l, seed=n + l)
    rng = np.random.default_rng(n * l)
    with _engine(weights, monkeypatch, n, l) as e:
        e.set_option("head_fold", fold)
        e.set_option("profile", 1)
        e.profile_reset()
        want = e.forward(idx)
        got = e.forward_weighted(idx, np.ones((3, l), np.float32))
        assert e.profile_get("main")[0] in (12, 24) and e.profile_get("precise")[0] == 0 and e.profile_get("weight_sums")[0] == 1   # (two half-batches)
        assert same(got, want)
        wt = _int_weights(rng, 3, l) + rng.random((3, l), np.float32).round(3)
        wt[:, 1] = 0
        assert same(e.forward_weighted(idx, wt), e.forward_weighted(idx, 0.25 * wt))


@pytest.mark.parametrize("n,l", F64_SHAPES)
def test_unit_weights_give_forwards_bits_on_the_precise_route(engines, n, l):
    e = engines("pf")
    idx = simulate_batch(3, n, l, seed=n * l)
    e.set_option("profile", 1)
    try:
        e.profile_reset()
        assert same(e.forward_weighted(idx, np.ones((3, l))), e.forward(idx))
        assert e.profile_get("precise")[0] > 0 and e.profile_get("main")[0] == 0
        wt = np.random.default_rng(l).random((3, l), np.float32) * 2
        wt[:, 0] = 0
        assert same(e.forward_weighted(idx, wt), e.forward_weighted(idx, 0.25 * wt))
    finally:
        e.set_option("profile", 0)


def test_unit_weights_with_precise_always_and_on_a_generic_checkpoint(engines, golden):
    from phyloformer_amd.engine import Engine
    from test_arch_host import arch_weights, cases
    e = engines("pf", 1)
    for n, l in [(20, 250), (24, 33)]:
        idx = simulate_batch(2, n, l, seed=3)
        assert same(e.forward_weighted(idx, np.ones((2, l))), e.forward(idx))
        wt = _int_weights(np.random.default_rng(l), 2, l)
        assert same(e.forward_weighted(idx, wt), e.forward_weighted(idx, 0.25 * wt))
    g = golden("arch_variants.npz")
    with Engine(arch_weights(g, 0), 0) as ge:
        ge.set_option("profile", 1)
        for idx, _want in cases(g, 0):
            L = idx.shape[-1]
            assert same(ge.forward_weighted(idx, np.ones(L)), ge.forward(idx))
            wt = _int_weights(np.random.default_rng(L), 1, L)[0]
            assert same(ge.forward_weighted(idx, wt), ge.forward_weighted(idx, 0.25 * wt))
        assert ge.profile_get("generic")[0] > 0 and ge.profile_get("main")[0] == 0


# ---- integer, zero and fractional weights against a yardstick ------------------------------------------------------

_REFS = {}


def _int_case(weights, n, l):
    """(idx [2][n][l], counts, expanded alignments, their float64 oracle), computed once per shape."""
    if (n, l) not in _REFS:
        rng = np.random.default_rng(1000 * n + l)
        idx = simulate_batch(2, n, l, seed=17 + n + l)
        wt = _int_weights(rng, 2, l)
        big = [ws.expand(idx[b], wt[b]) for b in range(2)]
        for a in big:                                   # the expanded shapes stay on the default route
            assert a.shape[1] >= 32 and n * (n - 1) // 2 * a.shape[1] >= 8192
        _REFS[n, l] = (idx, wt, big, _oracle_many(weights("pf"), big))
    return _REFS[n, l]


@pytest.mark.parametrize("n,l", SHAPES)
@pytest.mark.parametrize("fold", [1, 0])
def test_integer_weights_against_the_oracle_of_the_expanded_alignment(weights, monkeypatch, n, l, fold):
    idx, wt, big, ref = _int_case(weights, n, l)
    with _engine(weights, monkeypatch, n, l) as e:
        e.set_option("head_fold", fold)
        got = e.forward_weighted(idx, wt)
        for b in range(2):
            plain = e.forward(big[b])
            err, err_plain = float(np.abs(got[b] - ref[b]).max()), float(np.abs(plain - ref[b]).max())
            print(f"{n} x {l} fold={fold} aln {b} (expanded to {big[b].shape[1]} sites, distances up to {ref[b].max():.2f}): "
                  f"weighted vs oracle {err:.3e}, pf_forward of the expansion vs oracle {err_plain:.3e}")
            assert err_plain <= BOUND            # or the inputs are wrong
            assert err <= BOUND


@pytest.mark.parametrize("n,l", F64_SHAPES)
def test_integer_weights_on_the_float64_route(engines, weights, n, l):
    e = engines("pf")
    idx = simulate_batch(2, n, l, seed=5 * l)
    wt = _int_weights(np.random.default_rng(l), 2, l)
    big = [ws.expand(idx[b], wt[b]) for b in range(2)]
    ref = _oracle_many(weights("pf"), big)
    got = e.forward_weighted(idx, wt)
    for b in range(2):
        err = float(np.abs(got[b] - ref[b]).max())
        print(f"{n} x {l} aln {b}: float64 route, weighted vs oracle of the expansion {err:.3e}")
        assert err <= BOUND


@pytest.mark.parametrize("n,l", SHAPES)
def test_fractional_weights_default_kernels_against_float64(weights, engines, monkeypatch, n, l):
    rng = np.random.default_rng(7 * n + l)
    idx = simulate_batch(2, n, l, seed=n * l + 1)
    wt = (rng.random((2, l)) * 2).astype(np.float32)
    wt[:, rng.integers(0, l, 5)] = 0                       # some exact zeros
    want = engines("pf", 1).forward_weighted(idx, wt)
    with _engine(weights, monkeypatch, n, l) as e:
        for fold in (1, 0):
            e.set_option("head_fold", fold)
            err = float(np.abs(e.forward_weighted(idx, wt) - want).max())
            print(f"{n} x {l} fold={fold}: fractional weights, default kernels vs precise = 1: {err:.3e}")
            assert err <= BOUND


@pytest.mark.parametrize("n,l", [(20, 250), (24, 66)])
def test_zero_weights_cut_the_sites(engines, weights, n, l):
    e = engines("pf", 0)
    rng = np.random.default_rng(l)
    idx = simulate_batch(1, n, l, seed=l)[0]
    keep = np.sort(rng.choice(l, (2 * l) // 3, replace=False))
    wt = np.zeros(l, np.float32)
    wt[keep] = 1
    ref = _oracle_many(weights("pf"), [idx[:, keep]])[0]
    got, cut = e.forward_weighted(idx, wt), e.forward_sites(idx, keep[None])[0]
    err, err_cut = float(np.abs(got - ref).max()), float(np.abs(cut - ref).max())
    print(f"{n} x {l}, {len(keep)} sites kept: zero-weighted vs oracle of the cut {err:.3e}, pf_forward_sites vs oracle {err_cut:.3e}, "
          f"one against the other {float(np.abs(got - cut).max()):.3e}")
    assert err_cut <= BOUND and err <= BOUND


# ---- batch and chunk invariance, the device call, the site-table call ----------------------------------------------

def test_batch_position_and_chunking_do_not_change_an_alignments_bits(weights):
    from phyloformer_amd.engine import Engine
    rng = np.random.default_rng(8)
    a = simulate_batch(1, 20, 250, seed=21)
    others = simulate_batch(6, 20, 250, seed=22)
    wa = _int_weights(rng, 1, 250) * 0.5
    wo = (rng.random((6, 250)) * 3).astype(np.float32)
    with Engine(weights("pf"), 0) as e:
        alone = e.forward_weighted(a, wa)
        for pos in (0, 6, 3):
            batch, wt = np.concatenate([others[:pos], a, others[pos:]]), np.concatenate([wo[:pos], wa, wo[pos:]])
            whole = e.forward_weighted(batch, wt)
            assert same(whole[pos], alone[0]), pos
        e.set_option("ws_limit_mb", 32)                  # x alone is 12 MB per alignment: at most two per chunk
        e.set_option("two_streams", 0)
        e.set_option("profile", 1)
        e.profile_reset()
        cut = e.forward_weighted(batch, wt)
        assert e.profile_get("main")[0] // 6 >= 3
        assert same(cut, whole)


def test_device_call_gives_the_host_calls_bits_and_flags_bad_weights(engines):
    e = engines("pf", 0)
    B, N, L = 3, 20, 250
    P = N * (N - 1) // 2
    idx = simulate_batch(B, N, L, seed=2)
    wt = (np.random.default_rng(2).random((B, L)) * 2).astype(np.float32)
    d_idx, d_w, d_out = e.malloc(idx.nbytes), e.malloc(wt.nbytes), e.malloc(B * P * 4)
    try:
        e.h2d(d_idx, idx)
        e.h2d(d_w, wt)
        e.forward_weighted_device(d_idx, B, N, L, d_w, d_out)
        out = np.empty((B, P), np.float32)
        e.d2h(out, d_out)
        assert same(out, e.forward_weighted(idx, wt))
        bad = wt.copy()
        bad[1, 7] = -1.0                                 # only the device can see it: the sticky flag reports it
        e.h2d(d_w, bad)
        e.forward_weighted_device(d_idx, B, N, L, d_w, d_out)
        with pytest.raises(ValueError, match="negative or non-finite"):
            e.synchronize()
        e.synchronize()                                  # reported once
    finally:
        for p in (d_idx, d_w, d_out):
            e.free(p)


@pytest.mark.parametrize("n,l,k", [(20, 250, 160), (24, 66, 33), (10, 40, 16)])
def test_sites_weighted_equals_forward_weighted_of_the_host_cut(engines, n, l, k):
    e = engines("pf")
    rng = np.random.default_rng(k)
    idx = simulate_batch(2, n, l, seed=k)
    sites = rng.integers(0, l, (5, k)).astype(np.int32)
    wt = (rng.random((5, k)) * 2).astype(np.float32)
    wt[:, -3:] = 0
    got = e.forward_sites_weighted(idx, sites, wt)
    assert got.shape == (2, 5, n * (n - 1) // 2)
    for b in range(2):
        want = e.forward_weighted(np.stack([idx[b][:, s] for s in sites]), wt)
        assert same(got[b], want), b


# ---- pf_bootstrap_weighted -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,l", [(14, 100), (20, 250)])
@pytest.mark.parametrize("seed", [0, 20260])
def test_bootstrap_weighted_against_the_oracle_of_the_replicates(engines, weights, n, l, seed):
    e = engines("pf")
    R = 8
    idx = simulate_batch(3, n, l, seed=l + 1)
    got = e.bootstrap_weighted(idx, R, seed)
    plain = e.bootstrap(idx, R, seed)
    assert got.shape == plain.shape == (3, R, n * (n - 1) // 2)
    reps = resample_sites(l, R, seed)
    ref = np.stack(_oracle_many(weights("pf"), [idx[0][:, reps[r]] for r in range(R)]))
    err, err_plain = float(np.abs(got[0] - ref).max()), float(np.abs(plain[0] - ref).max())
    gap = float(np.abs(got - plain).max())
    print(f"{n} x {l} seed {seed}: pf_bootstrap_weighted vs oracle {err:.3e}, pf_bootstrap vs oracle {err_plain:.3e}, "
          f"largest difference between the two calls {gap:.3e} (K = {ws.boot_tables(l, R, seed)[0].shape[1]})")
    assert err_plain <= BOUND and err <= BOUND
    assert gap <= 2 * BOUND                              # the triangle of the two bounds, nothing tighter
    for b in range(3):                                   # one call with B = 3 equals three calls with B = 1
        assert same(e.bootstrap_weighted(idx[b], R, seed), got[b]), b


# ---- range re-check ------------------------------------------------------------------------------------------------

def test_recheck_recomputes_a_saturated_weighted_alignment_in_float64(engines):
    """The saturated alignment of tests/test_gpu_precise.py (pf_selreg, 33 x 33 uniformly random residues) between two
    simulated ones, all three weighted."""
    e, e64, edef = engines("pf_selreg"), engines("pf_selreg", 1), engines("pf_selreg", 0)
    hot = np.random.default_rng(805854907).integers(0, 22, (1, 33, 33)).astype(np.uint8)
    sim = simulate_batch(2, 33, 33, seed=9)
    batch = np.concatenate([sim[:1], hot, sim[1:]])
    wt = (0.5 + np.random.default_rng(1).random((3, 33))).astype(np.float32)
    assert float(edef.forward_weighted(hot, wt[1:2]).max()) > 8.0
    e.profile_reset()
    out = e.forward_weighted(batch, wt)
    assert e.rechecked_count() == 1
    for b, ref in ((0, edef), (1, e64), (2, edef)):
        assert same(out[b], ref.forward_weighted(batch[b:b + 1], wt[b:b + 1])[0]), b
    e.profile_reset()
    sites = np.tile(np.arange(33, dtype=np.int32), (2, 1))
    got = e.forward_sites_weighted(hot, sites, wt[:2])
    assert e.rechecked_count() == 2
    assert same(got[0], e64.forward_weighted(np.repeat(hot, 2, axis=0), wt[:2]))


# ---- refusals ------------------------------------------------------------------------------------------------------

def test_refusals_leave_out_untouched(engines, weights):
    from phyloformer_amd.engine import PF_EINVAL, PF_ESTATE, Engine
    e = engines("pf")
    lib, h = e._lib, e._h
    B, N, L = 2, 6, 40
    P = N * (N - 1) // 2
    idx = simulate_batch(B, N, L, seed=1)
    ones = np.ones((B, L), np.float32)
    sites = np.tile(np.arange(L, dtype=np.int32), (3, 1))
    w3 = np.ones((3, L), np.float32)

    def refused(call, status, text):
        out = np.full((B, 8, P), -7777.0, np.float32)
        rc = call(out.ctypes.data)
        msg = (lib.pf_last_error(h) or b"").decode()
        print(f"status {rc}: {msg}")
        assert rc == status and text in msg, (rc, msg)
        assert (out == -7777.0).all()

    def fwd(idx_, w_, b=B, n=N, l=L):
        return lambda out: lib.pf_forward_weighted(h, idx_.ctypes.data if idx_ is not None else None, b, n, l,
                                                   w_.ctypes.data if w_ is not None else None, out)

    def sw(w_, s_=sites, S=3, K=L):
        return lambda out: lib.pf_forward_sites_weighted(h, idx.ctypes.data, B, N, L, s_.ctypes.data if s_ is not None else None,
                                                         w_.ctypes.data if w_ is not None else None, S, K, out)
    # what the unweighted twins refuse
    refused(fwd(idx, ones, b=0), PF_EINVAL, "bad dimensions")
    refused(fwd(None, ones), PF_EINVAL, "null buffer")
    refused(fwd(np.full((B, N, L), 22, np.uint8), ones), PF_EINVAL, "residue index")
    refused(fwd(np.zeros((1, 201, 2), np.uint8), np.ones((1, 2), np.float32), b=1, n=201, l=2), PF_EINVAL, "n_seqs must be smaller")
    refused(sw(w3, s_=None), PF_EINVAL, "null buffer")
    bad_sites = sites.copy()
    bad_sites[1, 2] = L
    refused(sw(w3, s_=bad_sites), PF_EINVAL, "set 1, position 2")
    refused(sw(w3, K=L + 1), PF_EINVAL, "1 <= K <= L")
    refused(lambda out: lib.pf_bootstrap_weighted(h, idx.ctypes.data, B, N, L, 0, 1, out), PF_EINVAL, "R >= 1")
    # the weights
    refused(fwd(idx, None), PF_EINVAL, "null buffer")
    refused(sw(None), PF_EINVAL, "null buffer")
    for bad_value in (-0.5, np.nan, np.inf):
        bad = ones.copy()
        bad[1, 17] = bad_value
        refused(fwd(idx, bad), PF_EINVAL, "alignment 1, position 17")
        bad3 = w3.copy()
        bad3[2, 5] = bad_value
        refused(sw(bad3), PF_EINVAL, "set 2, position 5")
    zero = ones.copy()
    zero[0] = 0
    refused(fwd(idx, zero), PF_EINVAL, "alignment 0 sum to 0")
    zero3 = w3.copy()
    zero3[1] = 0
    refused(sw(zero3), PF_EINVAL, "set 1 sum to 0")
    with pytest.raises(ValueError, match="must be a real array of shape"):
        e.forward_weighted(idx, np.ones((B, L + 1)))
    # PF_ESTATE: the handle's state forbids a weighted forward.  (The refusal of a communicator of more than one rank
    # shares check_weighted_handle with this one; it cannot be reached on a single GPU: a second rank would have to join.)
    with Engine(weights("pf"), 0) as e2:
        e2.set_option("embed_mfma", 1)
        out = np.full((B, P), -7777.0, np.float32)
        rc = e2._lib.pf_forward_weighted(e2._h, idx.ctypes.data, B, N, L, ones.ctypes.data, out.ctypes.data)
        assert rc == PF_ESTATE and "embed_mfma" in e2._lib.pf_last_error(e2._h).decode() and (out == -7777.0).all()
        rc = e2._lib.pf_bootstrap_weighted(e2._h, idx.ctypes.data, B, N, L, 2, 0, out.ctypes.data)
        assert rc == PF_ESTATE and (out == -7777.0).all()


# ---- CLI -----------------------------------------------------------------------------------------------------------

def _run(args):
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf.ckpt"), *args],
                          capture_output=True, text=True, cwd=REPO, timeout=600)


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _matrix(data):
    rows = data.decode().split("\n")[1:]
    return np.array([[float(v) for v in r.split()[1:]] for r in rows if r.strip()])


def test_cli_compress_sites_over_the_shipped_msas(engines, tmp_path):
    from phyloformer_amd.fasta import load_alignment
    from phyloformer_amd.phylip import vec_to_phylip
    plain = _run([MSAS, "-o", str(tmp_path / "plain"), "--batch", "4", "-t"])
    comp = _run([MSAS, "-o", str(tmp_path / "comp"), "--batch", "4", "-t", "--compress-sites"])
    assert plain.returncode == 0 and comp.returncode == 0, plain.stderr[-2000:] + comp.stderr[-3000:]
    base, files = _files(tmp_path / "plain"), _files(tmp_path / "comp")
    stems = sorted(n[:-3] for n in os.listdir(MSAS))
    assert len(stems) == 20 and set(files) == set(base) == {f"{s}.{x}" for s in stems for x in ("phy", "nj.nwk")}
    e = engines("pf")
    worst = 0.0
    for s in stems:
        diff = float(np.abs(_matrix(files[f"{s}.phy"]) - _matrix(base[f"{s}.phy"])).max())
        worst = max(worst, diff)
        assert diff <= BOUND + 1e-6, (s, diff)                       # (+ the files' own 6 decimals)
        idx, ids = load_alignment(os.path.join(MSAS, f"{s}.fa"))
        assert base[f"{s}.phy"].decode() == vec_to_phylip(e.forward(idx), ids)[1], s    # without the flag: the parent's bytes
    print(f"--compress-sites over the 20 shipped MSAs: largest distance difference to the plain run {worst:.3e}")
    p = _run([MSAS, "-o", str(tmp_path / "pyio"), "--batch", "4", "-t", "--compress-sites", "--python-io"])
    assert p.returncode == 0, p.stderr[-3000:]
    assert _files(tmp_path / "pyio") == files


def test_cli_bootstrap_with_compress_sites(tmp_path):
    import re
    src = tmp_path / "in"
    src.mkdir()
    for s in ("0_20_tips", "1_30_tips", "3_50_tips"):
        (src / f"{s}.fa").write_bytes(open(os.path.join(MSAS, f"{s}.fa"), "rb").read())
    a = _run([str(src), "-o", str(tmp_path / "a"), "--bootstrap", "8"])
    b = _run([str(src), "-o", str(tmp_path / "b"), "--bootstrap", "8", "--compress-sites"])
    assert a.returncode == 0 and b.returncode == 0, a.stderr[-2000:] + b.stderr[-3000:]
    fa, fb = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert set(fa) == set(fb) and sum(n.endswith(".sup.nwk") for n in fa) == 3

    def shape(t):        # the tree text apart from the support integers (an internal node's label: `)<int>:`)
        return re.sub(r"\)\d+:", "):", t.decode())
    for name in fa:
        if name.endswith(".sup.nwk"):
            assert shape(fa[name]) == shape(fb[name]), name


def test_cli_refused_flag_combinations(tmp_path):
    for extra, text in ((["--windows", "50"], "--compress-sites is not supported with --windows"),
                        (["--site-profile"], "--compress-sites is not supported with --site-profile"),
                        (["--leave-one-out"], "--compress-sites is not supported with --leave-one-out"),
                        (["--devices", "0,1", "--shard", "sites"], "--compress-sites is not supported with --shard sites")):
        r = _run([MSAS, "-o", str(tmp_path / "o"), "--compress-sites", *extra])
        assert r.returncode == 2 and text in r.stderr, (extra, r.stderr[-500:])
