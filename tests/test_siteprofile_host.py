"""Site-resolved distances on the host (no GPU): the numpy twins of csrc/pf_sitemap.hip.h, the reference's own per-site
head values, ``infer_alns.py --site-profile`` through the oracle engine, and the C ABI additions.

Metric of a map against a yardstick: ``max |map - ref| / max(1, |ref|)`` per token, bound 1e-4 (the project's own
"<= 1e-4 max-abs"; logits reach 23 - 44, where softplus is linear, so a pure absolute bound would be a relative one in
disguise)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from phyloformer_amd import siteprofile as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pf_forward_site_map", "pf_forward_site_map_device", "pf_forward_site_profile", "pf_site_moments_device")
MSAS = ("0_20_tips", "1_20_tips", "2_20_tips", "0_30_tips")


def map_error(got, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


# ---- the twins, pinned literally -----------------------------------------------------------------------------------

def test_site_moments_on_a_hand_written_map():
    m = np.array([[1.0, 2.0, 3.0, 6.0],
                  [0.5, 0.5, 0.5, 0.5],          # a constant row: se = 0
                  [0.0, 4.0, 0.0, 4.0]])
    se, prof = sp.site_moments(m)
    # row 0: mean 3, squared deviations 4 + 1 + 0 + 9 = 14, / (4 * 3); row 2: mean 2, 4 * 4 = 16, / 12
    assert np.allclose(se, [np.sqrt(14.0 / 12.0), 0.0, np.sqrt(16.0 / 12.0)], rtol=0, atol=1e-15)
    assert se[1] == 0.0
    assert np.allclose(prof, [1.5 / 3, 6.5 / 3, 3.5 / 3, 10.5 / 3], rtol=0, atol=1e-15)
    assert se.dtype == np.float64 and prof.dtype == np.float64
    # batched maps reduce per alignment
    se2, prof2 = sp.site_moments(np.stack([m, 2 * m]))
    assert se2.shape == (2, 3) and prof2.shape == (2, 4)
    assert np.array_equal(se2[0], se) and np.allclose(se2[1], 2 * se) and np.allclose(prof2[1], 2 * prof)


def test_site_moments_single_site_and_bad_shape():
    se, prof = sp.site_moments(np.array([[3.0], [5.0]]))
    assert np.array_equal(se, [0.0, 0.0]) and np.array_equal(prof, [4.0])
    with pytest.raises(ValueError):
        sp.site_moments(np.array([1.0, 2.0]))


def test_softplus_is_the_heads_activation():
    z = np.array([-50.0, -1.0, 0.0, 1.0, 19.9, 20.0, 20.1, 44.0])
    got = sp.softplus(z)
    assert got[2] == np.log(2.0) and got[6] == 20.1 and got[7] == 44.0       # threshold 20: linear above it
    assert np.allclose(got[:6], np.log1p(np.exp(z[:6])), rtol=1e-15)


def test_sites_tsv_and_se_phylip_formats():
    from phyloformer_amd.phylip import vec_to_phylip
    text = sp.sites_tsv(np.array([0.5, 1.5, 1.0], np.float32))
    assert text.splitlines() == ["site\tprofile\trelative", "1\t0.5000000000\t0.500000000000000",
                                 "2\t1.5000000000\t1.500000000000000", "3\t1.0000000000\t1.000000000000000"]
    assert sp.sites_tsv(np.zeros(2)).splitlines()[1:] == ["1\t0.0000000000\tNA", "2\t0.0000000000\tNA"]
    se = np.array([0.1, 0.2, 0.3], np.float32)
    assert sp.se_phylip(se, ["a", "b", "c"]) == vec_to_phylip(se, ["a", "b", "c"])[1]


# ---- against the reference ----------------------------------------------------------------------------------------

def test_reference_logits_decompose_the_reference_distances(golden, weights):
    """taps_tiny.npz holds the reference's own head logits [P][L] and distances: the site mean of softplus(logits) IS the
    distance (to fp32 rounding), and the oracle engine's map is the reference's within the bound."""
    from helpers.oracle_sitemap_engine import OracleSiteMapEngine, OracleSiteMapEngine64
    g = golden("taps_tiny.npz")
    ref = sp.softplus(g["logits"])
    dist = g["dist"].astype(np.float64)
    L = ref.shape[1]
    # a mean of L fp32 terms: (L + 1) roundings of 2^-24 relative at most
    assert np.abs(ref.mean(axis=1) - dist).max() <= (L + 1) * 2.0 ** -24 * np.abs(dist).max()
    for cls in (OracleSiteMapEngine, OracleSiteMapEngine64):
        d, m = cls(weights("pf"), 0).forward_site_map(g["idx"])
        err = map_error(m, ref)
        print(f"{cls.__name__}: map vs reference golden {err:.3e}")
        assert m.shape == ref.shape and m.dtype == np.float32 and err <= 1e-4
        assert np.abs(d - dist).max() <= 1e-4
        d2, se, prof = cls(weights("pf"), 0).forward_site_profile(g["idx"])
        want_se, want_prof = sp.site_moments(m)
        assert np.array_equal(d2, d) and np.array_equal(se, want_se.astype(np.float32))
        assert np.array_equal(prof, want_prof.astype(np.float32))


def test_site_map_golden_is_the_references_decomposition(golden, weights):
    """tests/golden/site_map.npz (tools/gen_golden_site_map.py): the reference's own head logits of two shipped MSAs.
    Their softplus averages to the reference's distances, and the float64 oracle's map sits within the bound."""
    from helpers.oracle_sitemap_engine import OracleSiteMapEngine64
    from phyloformer_amd.fasta import load_alignment
    g = golden("site_map.npz")
    for stem in ("0_20_tips", "1_30_tips"):
        idx, _ids = load_alignment(os.path.join(REPO, "data", "testdata", "msas", f"{stem}.fa"))
        assert np.array_equal(g[f"{stem}/idx"], idx)
        ref, dist = sp.softplus(g[f"{stem}/logits"]), g[f"{stem}/dist"].astype(np.float64)
        L = ref.shape[1]
        assert ref.shape == (len(dist), L)
        assert np.abs(ref.mean(axis=1) - dist).max() <= (L + 1) * 2.0 ** -24 * np.abs(dist).max()
        _d, m = OracleSiteMapEngine64(weights("pf"), 0).forward_site_map(idx)
        err = map_error(m, ref)
        print(f"{stem}: float64 oracle's map vs reference golden {err:.3e}")
        assert err <= 1e-4


# ---- CLI through the oracle engine --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def msa_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("site_alns")
    for stem in MSAS:
        shutil.copy(os.path.join(REPO, "data", "testdata", "msas", f"{stem}.fa"), d / f"{stem}.fa")
    return d


def _cli(args, tmp_path):
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_sitemap_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=1800)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def test_cli_site_profile_files(msa_dir, tmp_path, weights):
    from helpers.oracle_sitemap_engine import make
    from phyloformer_amd.fasta import load_alignment
    plain = _cli([str(msa_dir), "-o", str(tmp_path / "plain"), "-t"], tmp_path)
    r = _cli([str(msa_dir), "-o", str(tmp_path / "o"), "-t", "--site-profile"], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, plain.stderr[-2000:] + r.stderr[-3000:]
    files, base = _files(tmp_path / "o"), _files(tmp_path / "plain")
    assert set(files) == set(base) | {f"{s}.{ext}" for s in MSAS for ext in ("sites.tsv", "se.phy")}
    for name, data in base.items():
        assert files[name] == data, name                      # <stem>.phy / <stem>.nj.nwk exactly as without the flag
    eng = make(weights("pf"), 0)
    for stem in MSAS:
        idx, ids = load_alignment(os.path.join(REPO, "data", "testdata", "msas", f"{stem}.fa"))
        N, L = idx.shape
        rows = files[f"{stem}.sites.tsv"].decode().splitlines()
        assert rows[0].split("\t") == ["site", "profile", "relative"] and len(rows) == 1 + L
        cols = [r_.split("\t") for r_ in rows[1:]]
        assert [int(c[0]) for c in cols] == list(range(1, L + 1))
        prof = np.array([float(c[1]) for c in cols])
        rel = np.array([float(c[2]) for c in cols])
        assert abs(rel.mean() - 1.0) <= 1e-12
        _d, se, want_prof = eng.forward_site_profile(idx)
        assert files[f"{stem}.sites.tsv"].decode() == sp.sites_tsv(want_prof)
        assert np.abs(prof - want_prof.astype(np.float64)).max() <= 1e-10
        assert files[f"{stem}.se.phy"].decode() == sp.se_phylip(se, ids)
        phy = files[f"{stem}.se.phy"].decode().splitlines()
        assert phy[0] == str(N) and [l.split(" ")[0] for l in phy[1:]] == list(ids)
        assert [l.split(" ")[0] for l in files[f"{stem}.phy"].decode().splitlines()[1:]] == list(ids)
    p = _cli([str(msa_dir), "-o", str(tmp_path / "p"), "-t", "--site-profile", "--python-io"], tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _files(tmp_path / "p") == files


def test_cli_site_profile_refused_combinations(msa_dir, tmp_path):
    for extra, msg in ((["--bootstrap", "5"], "--site-profile is not supported with --bootstrap"),
                       (["--windows", "16"], "--site-profile is not supported with --windows"),
                       (["--devices", "0,1", "--shard", "sites"], "--site-profile is not supported with --shard sites"),
                       (["--shard", "sites"], "--site-profile is not supported with --shard sites")):
        r = _cli([str(msa_dir), "-o", str(tmp_path / "x"), "--site-profile", *extra], tmp_path)
        assert r.returncode == 2 and msg in r.stderr, r.stderr[-1000:]
        assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")


# ---- ABI -----------------------------------------------------------------------------------------------------------

def test_header_library_and_binding_have_the_four_entry_points():
    from phyloformer_amd import build as pf_build
    from phyloformer_amd import engine
    h = open(os.path.join(REPO, "include", "phyloformer_amd.h")).read()
    for name in SYMBOLS:
        assert re.search(rf"^int {name}\(", h, re.M), name
    assert re.search(r"^#define PF_ABI_VERSION 5$", h, re.M)
    lib = ctypes.CDLL(pf_build.build())
    for name in SYMBOLS:
        assert getattr(lib, name) is not None, name
        assert name in engine.SIGNATURES and name in engine.CALL_TIME_SYMBOLS
    assert lib.pf_abi_version() == 5 and engine.ABI_VERSION == 5
    # NULL handle: refused like every other entry point, nothing dereferenced
    lib.pf_site_moments_device.argtypes = engine.SIGNATURES["pf_site_moments_device"][1]
    assert lib.pf_site_moments_device(None, None, 1, 1, 1, None, None) == engine.PF_EINVAL


def test_a_library_without_the_symbols_fails_at_call_time():
    """An older ABI-5 library loads; the call through a missing symbol raises EngineError."""
    from phyloformer_amd import engine

    class Old:
        pass
    e = engine.Engine.__new__(engine.Engine)
    e._lib, e._h = Old(), None
    for call in (lambda: e.forward_site_map(np.zeros((3, 4), np.uint8)), lambda: e.forward_site_profile(np.zeros((3, 4), np.uint8)),
                 lambda: e.site_moments_device(0, 1, 1, 1, 0, 0), lambda: e.forward_site_map_device(0, 1, 2, 1, 0, 0)):
        with pytest.raises(engine.EngineError, match="does not export pf_"):
            call()
