"""-m gpu: site-resolved distances - pf_forward_site_map / _device, pf_forward_site_profile, pf_site_moments_device
(k_main<.., SITEMAP>, kg_head's map store, csrc/pf_sitemap.hip.h) and ``infer_alns.py --site-profile``.

Bounds (none of them from what the code under test gives):
  * out                    pf_forward's, bit for bit
  * map against a yardstick  max |map - ref| / max(1, |ref|) <= 1e-4 per token (the project's own "<= 1e-4 max-abs";
                           logits reach 23 - 44, where softplus is linear); the float64 paths at or below the fp32
                           oracle's own figure for the same case
  * map against out        | mean64_l(map[p]) - out[p] | <= (nparts + 8) 2^-24 mean_l |map[p]|, nparts = ceil(L / 32) + 1:
                           a 32-term tree plus nparts sequential fp32 additions (outpart / k_outsum); float64 paths
                           2 * 2^-24 relative (one rounding to float on each side)
  * se, profile            4 float ulp (2.4e-7 relative, 1e-30 absolute) of the float64 numpy twin; batch invariant bits
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import pf_oracle as O
from phyloformer_amd import siteprofile as sp
from phyloformer_amd.msa_sim import simulate_batch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSAS = os.path.join(REPO, "data", "testdata", "msas")


def _msa(stem):
    from phyloformer_amd.fasta import load_alignment
    return load_alignment(os.path.join(MSAS, f"{stem}.fa"))[0]


def _oracle_map(w, idx, dtype=np.float64):
    """softplus of the oracle's head logits [P][L] (tests/test_oracle.py pins the tap to the reference's golden)."""
    taps = {}
    O.forward(w.tensors, idx, n_blocks=w.n_blocks, n_heads=w.n_heads, dtype=dtype,
              tap=lambda k, v: taps.__setitem__(k, np.array(v)))
    return sp.softplus(taps["logits"])


def map_error(got, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def _moments_device(e, smap):
    """pf_site_moments_device on a host map [B][P][L]."""
    smap = np.ascontiguousarray(smap, np.float32)
    B, P, L = smap.shape
    d_map, d_se, d_prof = e.malloc(smap.nbytes), e.malloc(B * P * 4), e.malloc(B * L * 4)
    try:
        e.h2d(d_map, smap)
        e.site_moments_device(d_map, B, P, L, d_se, d_prof)
        se, prof = np.empty((B, P), np.float32), np.empty((B, L), np.float32)
        e.d2h(se, d_se)
        e.d2h(prof, d_prof)
    finally:
        for p in (d_map, d_se, d_prof):
            e.free(p)
    return se, prof


def _same_as_forward(e, idx):
    """Items 5 and 10 for one engine and batch: out is forward's, the profile call reduces the map call's map."""
    want = e.forward(idx)
    out, smap = e.forward_site_map(idx)
    out2, se, prof = e.forward_site_profile(idx)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out2.view(np.uint32), want.view(np.uint32))
    B, N, L = idx.shape
    assert smap.shape == (B, N * (N - 1) // 2, L) and np.isfinite(smap).all() and (smap >= 0).all()
    se_d, prof_d = _moments_device(e, smap)
    assert np.array_equal(se.view(np.uint32), se_d.view(np.uint32))
    assert np.array_equal(prof.view(np.uint32), prof_d.view(np.uint32))
    return out, smap, se, prof


def _agree(out, smap, f64_path):
    """Item 7: the map's site mean is the distance."""
    L = smap.shape[-1]
    m64 = smap.astype(np.float64)
    fac = 2.0 if f64_path else (-(-L // 32) + 1 + 8)
    bound = fac * 2.0 ** -24 * np.abs(m64).mean(axis=-1)
    diff = np.abs(m64.mean(axis=-1) - out.astype(np.float64))
    worst = float((diff / np.maximum(bound, 1e-300)).max())
    print(f"map vs out: L={L} worst diff / bound {worst:.3f}")
    assert (diff <= bound).all(), worst


# ---- 5, 7, 10: out is pf_forward's on every path; the map's mean is out; profile = moments of the map --------------

@pytest.mark.parametrize("n,l", [(20, 256), (20, 250), (60, 500)])
@pytest.mark.parametrize("fold", [1, 0])
def test_out_is_forwards_on_the_default_kernels(engines, n, l, fold):
    e = engines("pf", 0)
    idx = simulate_batch(2, n, l, seed=7 + n + l)
    try:
        e.set_option("head_fold", fold)
        e.set_option("profile", 1)
        e.profile_reset()
        out, smap, _se, _prof = _same_as_forward(e, idx)
        assert e.profile_get("main")[0] > 0 and e.profile_get("precise")[0] == 0 and e.profile_get("site_moments")[0] > 0
        _agree(out, smap, False)
        one = _same_as_forward(e, idx[:1])                     # B = 1
        assert np.array_equal(one[1], smap[:1]) and np.array_equal(one[0], out[:1])
    finally:
        e.set_option("head_fold", 1)
        e.set_option("profile", 0)


@pytest.mark.parametrize("n,l", [(5, 16), (10, 40)])
def test_out_is_forwards_on_the_precise_route(engines, n, l):
    e = engines("pf")
    try:
        e.set_option("profile", 1)
        e.profile_reset()
        out, smap, _se, _prof = _same_as_forward(e, simulate_batch(3, n, l, seed=n * l))
        assert e.profile_get("precise")[0] > 0 and e.profile_get("main")[0] == 0
        _agree(out, smap, True)
    finally:
        e.set_option("profile", 0)


def test_out_is_forwards_with_precise_always_and_on_a_generic_checkpoint(engines, golden):
    from phyloformer_amd.engine import Engine
    from test_arch_host import arch_weights, cases
    e = engines("pf", 1)
    out, smap, _se, _prof = _same_as_forward(e, simulate_batch(2, 20, 250, seed=3))
    _agree(out, smap, True)
    g = golden("arch_variants.npz")
    w = arch_weights(g, 0)
    with Engine(w, 0) as ge:
        ge.set_option("profile", 1)
        for idx, _want in cases(g, 0):
            out, smap, _se, _prof = _same_as_forward(ge, idx[None])
            _agree(out, smap, True)
        assert ge.profile_get("generic")[0] > 0 and ge.profile_get("main")[0] == 0


def test_chunked_batch_is_bit_identical(weights):
    """A small ws_limit_mb cuts 7 alignments of 20 x 250 into at least three chunks (counted by k_main launches, one
    stream): out is forward's, and every alignment's map / se / profile are those it gets alone."""
    from phyloformer_amd.engine import Engine
    idx = simulate_batch(7, 20, 250, seed=11)
    with Engine(weights("pf"), 0) as e:
        whole = _same_as_forward(e, idx)
        e.set_option("ws_limit_mb", 32)         # x alone is 12 MB per alignment: at most two per chunk
        e.set_option("two_streams", 0)
        e.set_option("profile", 1)
        e.profile_reset()
        e.forward_site_map(idx)
        chunks = e.profile_get("main")[0] // 6
        assert chunks >= 3, chunks
        cut = _same_as_forward(e, idx)
        for a, b in zip(whole, cut):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for b in (0, 3, 6):
            alone = _same_as_forward(e, idx[b:b + 1])
            for a, c in zip(alone, cut):
                assert np.array_equal(a[0].view(np.uint32), c[b].view(np.uint32))


# ---- 6: the map against the reference ------------------------------------------------------------------------------

def test_map_against_the_references_own_logits(engines, weights, golden):
    """taps_tiny.npz: the reference's head logits of a 5 x 16 alignment (the float64 route)."""
    g = golden("taps_tiny.npz")
    ref = sp.softplus(g["logits"])
    _out, smap = engines("pf").forward_site_map(g["idx"])
    err = map_error(smap, ref)
    f64 = _oracle_map(weights("pf"), g["idx"])
    own = map_error(_oracle_map(weights("pf"), g["idx"], np.float32), f64)
    err64 = map_error(smap, f64)
    print(f"tiny: map vs reference golden {err:.3e}; vs float64 oracle {err64:.3e} (fp32 oracle's own {own:.3e})")
    assert err <= 1e-4
    assert err64 <= own


@pytest.mark.parametrize("ckpt,stem", [("pf", "0_20_tips"), ("pf", "1_30_tips"), ("pf", "3_50_tips"), ("pf_base", "0_20_tips"),
                                       ("pf_indel", "1_20_tips")])
def test_map_against_the_float64_oracle(engines, weights, ckpt, stem):
    idx = _msa(stem)
    ref = _oracle_map(weights(ckpt), idx)
    out, smap = engines(ckpt, 0).forward_site_map(idx)
    err = map_error(smap, ref)
    print(f"{ckpt} {stem}: default kernels' map vs float64 oracle {err:.3e}")
    assert err <= 1e-4
    _agree(out, smap, False)
    if (ckpt, stem) == ("pf", "0_20_tips"):
        own = map_error(_oracle_map(weights(ckpt), idx, np.float32), ref)
        _o, m64 = engines(ckpt, 1).forward_site_map(idx)
        e64 = map_error(m64, ref)
        print(f"{ckpt} {stem}: float64 kernels' map vs float64 oracle {e64:.3e} (fp32 oracle's own {own:.3e})")
        assert e64 <= own


@pytest.mark.parametrize("stem", ["0_20_tips", "1_30_tips"])
def test_map_against_the_references_site_map_golden(engines, golden, stem):
    """tests/golden/site_map.npz: the reference's own per-site head output (fp32) for two shipped MSAs."""
    g = golden("site_map.npz")
    ref = sp.softplus(g[f"{stem}/logits"])
    for precise, name in ((0, "default"), (1, "float64")):
        _out, smap = engines("pf", precise).forward_site_map(g[f"{stem}/idx"])
        err = map_error(smap, ref)
        print(f"{stem}: {name} kernels' map vs reference golden {err:.3e}")
        assert err <= 1e-4


# ---- 8: batch invariance, bounds of the device map -----------------------------------------------------------------

def test_batch_position_does_not_change_an_alignments_bits(engines):
    e = engines("pf", 0)
    a = simulate_batch(1, 20, 200, seed=21)
    others = simulate_batch(4, 20, 200, seed=22)
    alone = (e.forward_site_map(a), e.forward_site_profile(a))
    for pos in (0, 4, 2):
        batch = np.concatenate([others[:pos], a, others[pos:]])
        (out, smap), (out2, se, prof) = e.forward_site_map(batch), e.forward_site_profile(batch)
        for got, want in ((out, alone[0][0]), (smap, alone[0][1]), (out2, alone[1][0]), (se, alone[1][1]), (prof, alone[1][2])):
            assert np.array_equal(got[pos].view(np.uint32), want[0].view(np.uint32)), pos


def _device_map_with_sentinels(e, idx):
    B, N, L = idx.shape
    P = N * (N - 1) // 2
    pad, nmap = 1024, B * P * L                                   # 4 KB of sentinel floats on either side
    host = np.full(pad + nmap + pad, -7777.0, np.float32)
    d_idx, d_out, d_buf = e.malloc(idx.nbytes), e.malloc(B * P * 4), e.malloc(host.nbytes)
    try:
        e.h2d(d_idx, idx)
        e.h2d(d_buf, host)
        e.forward_site_map_device(d_idx, B, N, L, d_out, d_buf + 4 * pad)
        e.synchronize()
        back, out = np.empty_like(host), np.empty((B, P), np.float32)
        e.d2h(back, d_buf)
        e.d2h(out, d_out)
    finally:
        for p in (d_idx, d_out, d_buf):
            e.free(p)
    assert (back[:pad] == -7777.0).all() and (back[-pad:] == -7777.0).all()
    smap = back[pad:pad + nmap].reshape(B, P, L)
    assert np.isfinite(smap).all() and (smap >= 0).all()          # no unwritten element, no trash-lane value
    return out, smap


@pytest.mark.parametrize("n,l,row", [(20, 200, True), (20, 200, False), (20, 250, False), (24, 33, False)])
def test_device_map_stays_inside_its_buffer(weights, monkeypatch, n, l, row):
    """Ragged row tiling (L = 200 with row tiles forced), flat tilings, L = 33: both sentinels survive, every element is
    written, and the device call's results are the host call's."""
    from phyloformer_amd.engine import Engine
    if row:
        monkeypatch.setenv("PF_ROW_TILES", "1")
    idx = simulate_batch(3, n, l, seed=5 * l + n)
    with Engine(weights("pf"), 0) as e:
        e.set_option("precise", 0)
        out, smap = _device_map_with_sentinels(e, idx)
        want_out, want_map = e.forward_site_map(idx)
        assert np.array_equal(out.view(np.uint32), e.forward(idx).view(np.uint32))
        assert np.array_equal(smap.view(np.uint32), want_map.view(np.uint32)) and np.array_equal(out, want_out)
        _agree(out, smap, False)


# ---- 9: k_site_moments alone ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,L", [(1, 1), (1, 7), (190, 200), (435, 33), (1770, 500), (19900, 64)])
def test_site_moments_kernels_against_the_numpy_twin(engines, P, L):
    e = engines("pf")
    rng = np.random.default_rng(P * 1000 + L)
    uniform = rng.random((P, L), np.float32) * 5.0
    heavy = np.exp(rng.standard_normal((P, L)) * 3.0 - 4.0).astype(np.float32)       # 1e-7 ... 40, never negative
    other = rng.random((P, L), np.float32)
    for smap in (uniform, heavy):
        batch = np.stack([smap, other, smap])
        se, prof = _moments_device(e, batch)
        want_se, want_prof = sp.site_moments(smap)
        for got, want, name in ((se[0], want_se, "se"), (prof[0], want_prof, "profile")):
            err = np.abs(got.astype(np.float64) - want)
            worst = float((err / np.maximum(np.abs(want), 1e-300)).max())
            print(f"{name} P={P} L={L}: worst relative {worst:.3e}")
            assert (err <= 2.4e-7 * np.abs(want) + 1e-30).all(), (name, worst)
        if L == 1:
            assert (se == 0).all()
        assert np.array_equal(se[0].view(np.uint32), se[2].view(np.uint32))          # another batch index, same bits
        assert np.array_equal(prof[0].view(np.uint32), prof[2].view(np.uint32))
        alone = _moments_device(e, smap[None])
        assert np.array_equal(alone[0][0], se[0]) and np.array_equal(alone[1][0], prof[0])


# ---- 11: range re-check --------------------------------------------------------------------------------------------

def test_recheck_replaces_map_se_and_profile_with_the_distances(engines):
    """The saturated alignment of tests/test_gpu_precise.py (pf_selreg, 33 x 33 uniformly random residues: largest
    distance above 8, not routed to float64 by shape) between two simulated ones."""
    e, e64, edef = engines("pf_selreg"), engines("pf_selreg", 1), engines("pf_selreg", 0)
    hot = np.random.default_rng(805854907).integers(0, 22, (1, 33, 33)).astype(np.uint8)
    sim = simulate_batch(2, 33, 33, seed=9)
    batch = np.concatenate([sim[:1], hot, sim[1:]])
    assert float(edef.forward(hot).max()) > 8.0
    e.profile_reset()
    out, smap = e.forward_site_map(batch)
    assert e.rechecked_count() == 1
    e.profile_reset()
    out2, se, prof = e.forward_site_profile(batch)
    assert e.rechecked_count() == 1
    assert np.array_equal(out.view(np.uint32), e.forward(batch).view(np.uint32)) and np.array_equal(out, out2)
    for b, ref in ((0, edef), (1, e64), (2, edef)):
        w_out, w_map = ref.forward_site_map(batch[b:b + 1])
        w_out2, w_se, w_prof = ref.forward_site_profile(batch[b:b + 1])
        for got, want in ((out[b], w_out[0]), (smap[b], w_map[0]), (out2[b], w_out2[0]), (se[b], w_se[0]), (prof[b], w_prof[0])):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), b


# ---- refusals ------------------------------------------------------------------------------------------------------

def test_refusals(engines):
    e = engines("pf")
    with pytest.raises(ValueError, match="residue index"):
        e.forward_site_map(np.full((1, 4, 8), 22, np.uint8))
    with pytest.raises(ValueError, match="null buffer"):
        e.site_moments_device(0, 1, 1, 1, 0, 0)
    with pytest.raises(ValueError, match="bad dimensions"):
        e.site_moments_device(1, 0, 1, 1, 1, 1)
    with pytest.raises(ValueError, match="null buffer"):
        e.forward_site_map_device(0, 1, 4, 8, 0, 0)
    with pytest.raises(ValueError, match="n_seqs must be smaller"):
        e.forward_site_profile(np.zeros((1, 201, 2), np.uint8))


# ---- 12: CLI -------------------------------------------------------------------------------------------------------

def _run(args):
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf.ckpt"), *args],
                          capture_output=True, text=True, cwd=REPO, timeout=600)


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_cli_site_profile_over_the_shipped_msas(engines, tmp_path):
    from phyloformer_amd.fasta import load_alignment
    plain = _run([MSAS, "-o", str(tmp_path / "plain"), "--batch", "4"])
    r = _run([MSAS, "-o", str(tmp_path / "o"), "--batch", "4", "--site-profile"])
    assert plain.returncode == 0 and r.returncode == 0, plain.stderr[-2000:] + r.stderr[-3000:]
    base, files = _files(tmp_path / "plain"), _files(tmp_path / "o")
    stems = sorted(n[:-3] for n in os.listdir(MSAS))
    assert len(stems) == 20 and set(base) == {f"{s}.phy" for s in stems}
    assert set(files) == set(base) | {f"{s}.{ext}" for s in stems for ext in ("sites.tsv", "se.phy")}
    for name, data in base.items():
        assert files[name] == data, name
    e = engines("pf")
    for s in stems:
        idx, ids = load_alignment(os.path.join(MSAS, f"{s}.fa"))
        _d, se, prof = e.forward_site_profile(idx)
        assert files[f"{s}.sites.tsv"].decode() == sp.sites_tsv(prof), s
        assert files[f"{s}.se.phy"].decode() == sp.se_phylip(se, ids), s
    p = _run([MSAS, "-o", str(tmp_path / "p"), "--batch", "4", "--site-profile", "--python-io"])
    assert p.returncode == 0, p.stderr[-3000:]
    assert _files(tmp_path / "p") == files
