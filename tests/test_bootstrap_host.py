"""Site bootstrap on the host (no GPU): the replicate stream, split supports on NJ trees (native and Python twins),
the CLI's --bootstrap plumbing through an oracle engine, and the ABI additions."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from phyloformer_amd import bootstrap as bs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = re.compile(r"\)(\d+)")


def _strip(text):
    return LABEL.sub(")", text)


# ---- the replicate stream ------------------------------------------------------------------------------------------

STREAM_TABLE = [
    (0, 0, 500, [140, 308, 120, 226, 34, 358, 417, 6]),
    (0, 1, 500, [44, 98, 315, 90, 52, 213, 39, 423]),
    (7, 0, 200, [91, 4, 141, 111, 123, 187, 13, 107]),
    (12345, 99, 2000, [836, 1636, 300, 1355, 226, 1811, 1683, 816]),
    (2 ** 64 - 1, 3, 1, [0] * 8),
]


def _site(seed, r, l, L):
    key = bs.stream_key(seed)
    z = int(bs.mix64(np.uint64(key ^ ((r << 32) | l))))
    return ((z >> 32) * L) >> 32


@pytest.mark.parametrize("seed,r,L,want", STREAM_TABLE)
def test_stream_literal_table(seed, r, L, want):
    assert [_site(seed, r, l, L) for l in range(8)] == want
    got = bs.resample_sites(L, r + 1, seed)[r]
    assert got[:8].tolist() == want[:L]


def test_stream_key_of_seed_zero():
    assert bs.stream_key(0) == 0xE220A8397B1DCDAF


def test_stream_is_independent_of_first():
    full = bs.resample_sites(300, 12, 5)
    for k in (0, 1, 7, 11):
        assert np.array_equal(bs.resample_sites(300, 12 - k, 5, first=k), full[k:])


@pytest.mark.parametrize("L", [1, 2, 3, 17, 200, 2001])
def test_stream_sites_in_range(L):
    s = bs.resample_sites(L, 50, 3)
    assert s.shape == (50, L) and s.dtype == np.int64 and s.min() >= 0 and s.max() < L


def test_stream_distinct_fraction():
    s = bs.resample_sites(500, 1000, 0)
    frac = np.array([np.unique(r).size / 500 for r in s])
    assert abs(frac.mean() - 0.632) <= 0.01
    assert round(float(frac.mean()), 4) == 0.6327


def test_resample_layout():
    rng = np.random.default_rng(1)
    idx = rng.integers(0, 22, size=(2, 4, 30), dtype=np.uint8)
    reps = bs.resample(idx, 3, 9)
    sites = bs.resample_sites(30, 3, 9)
    assert reps.shape == (2, 3, 4, 30)
    for b in range(2):
        for r in range(3):
            assert np.array_equal(reps[b, r], idx[b][:, sites[r]])
    assert np.array_equal(bs.resample(idx[0], 3, 9), reps[0])


# ---- supports ------------------------------------------------------------------------------------------------------

def _tree_dm(n, rng):
    """Distances of a random additive tree (distinct topology splits), as pairs i < j."""
    pts = rng.random((n, 3))
    d = np.abs(pts[:, None, :] - pts[None, :, :]).sum(-1)
    i, j = np.triu_indices(n, 1)
    return d[i, j].astype(np.float32)


def _both(preds, reps, ids):
    from phyloformer_amd.hostio import nj_support
    py = bs.support_newick_py(preds, reps, ids)
    nat = nj_support(preds, reps, ids, threads=3).decode()
    assert nat == py
    return nat


def test_support_all_100_when_replicates_equal_original():
    rng = np.random.default_rng(2)
    preds = _tree_dm(12, rng)
    text = _both(preds, np.stack([preds] * 5), [f"t{i}" for i in range(12)])
    labels = [int(v) for v in LABEL.findall(text)]
    assert len(labels) == 12 - 3 and all(v == 100 for v in labels)


def _pairs(d):
    i, j = np.triu_indices(d.shape[0], 1)
    return d[i, j].astype(np.float32)


def _caterpillar(order, n=6):
    """Path-metric distances of the caterpillar ((o0,o1),o2),o3),(o4,o5)): every leaf hangs off a spine."""
    pos = {leaf: k for k, leaf in enumerate(order)}
    d = np.zeros((n, n))
    for a in range(n):
        for b in range(n):
            if a != b:
                d[a, b] = abs(pos[a] - pos[b]) + 2.0
    return _pairs(d)


def test_support_hand_built_six_taxa():
    """Original tree: the caterpillar 0-1-2-3-4-5 with splits {0,1}, {0,1,2}, {0,1,2,3} (normalised to the side
    without 0: {2,3,4,5}, {3,4,5}, {4,5}).  R = 4 replicates: the same tree twice; 0-1-2-4-3-5 (splits {0,1},
    {0,1,2}, {0,1,2,4}); 0-2-1-3-4-5 ({0,2}, {0,1,2}, {0,1,2,3}).  So {0,1} is in 3 of 4 (75), {0,1,2} in 4 of 4
    (100), {0,1,2,3} in 3 of 4 (75)."""
    orig = _caterpillar([0, 1, 2, 3, 4, 5])
    reps = np.stack([orig, orig, _caterpillar([0, 1, 2, 4, 3, 5]), _caterpillar([0, 2, 1, 3, 4, 5])])
    ids = list("abcdef")
    text = _both(orig, reps, ids)
    from phyloformer_amd import nj
    from phyloformer_amd.phylip import vec_to_matrix
    joins, _final = nj.nj_joins(vec_to_matrix(orig, 6).astype(np.float64))
    splits = nj.join_splits(joins, 6)
    labels = [int(v) for v in LABEL.findall(text)]
    # count by hand: split sets of the four replicate caterpillars
    def cat_splits(order):
        full = 63
        out = set()
        for k in (2, 3, 4):       # the three internal edges of a 6-leaf caterpillar: first 2, 3, 4 leaves vs the rest
            m = sum(1 << o for o in order[:k])
            out.add(m ^ full if m & 1 else m)
        return out
    rs = [cat_splits([0, 1, 2, 3, 4, 5])] * 2 + [cat_splits([0, 1, 2, 4, 3, 5]), cat_splits([0, 2, 1, 3, 4, 5])]
    want = [bs.support_percent(sum(s in r for r in rs), 4) for s in splits]
    assert sorted(splits) == sorted(cat_splits([0, 1, 2, 3, 4, 5]))
    assert labels == want
    by_split = dict(zip(splits, labels))
    assert by_split == {0b111100: 75, 0b111000: 100, 0b110000: 75}


def test_support_rounding_rule():
    assert [bs.support_percent(c, 8) for c in range(9)] == [0, 13, 25, 38, 50, 63, 75, 88, 100]
    assert bs.support_percent(1, 3) == 33 and bs.support_percent(2, 3) == 67 and bs.support_percent(1, 200) == 1


def test_support_rounding_in_text():
    """c = 1 of R = 8 gives 13: one replicate equal to the tree, seven of a tree that shares no split with it."""
    orig = _caterpillar([0, 1, 2, 3, 4, 5])
    other = _caterpillar([0, 3, 5, 1, 4, 2])
    text = _both(orig, np.stack([orig] + [other] * 7), list("abcdef"))
    assert sorted(int(v) for v in LABEL.findall(text)) == [13, 13, 13]


def test_support_without_labels_is_nj_newick():
    from phyloformer_amd.hostio import nj_newick
    rng = np.random.default_rng(3)
    for n in (4, 5, 9, 20, 41):
        preds = rng.random(n * (n - 1) // 2).astype(np.float32)
        reps = preds[None] + 0.3 * rng.random((6, preds.size)).astype(np.float32)
        ids = [f"x{i}" for i in range(n)]
        assert _strip(_both(preds, reps, ids)).encode() == nj_newick(preds, ids)


@pytest.mark.parametrize("n", [2, 3])
def test_support_small_trees_have_no_labels(n):
    from phyloformer_amd.hostio import nj_newick
    preds = np.arange(1, n * (n - 1) // 2 + 1, dtype=np.float32)
    text = _both(preds, np.stack([preds * 2, preds]), ["a", "b", "c"][:n])
    assert not LABEL.search(text) and text.encode() == nj_newick(preds, ["a", "b", "c"][:n])


def test_support_duplicate_ids():
    rng = np.random.default_rng(4)
    preds = _tree_dm(8, rng)
    ids = ["same"] * 8
    text = _both(preds, np.stack([preds] * 3), ids)
    assert [int(v) for v in LABEL.findall(text)] == [100] * 5


def test_support_twins_on_random_cases_with_ties_and_zeros():
    rng = np.random.default_rng(5)
    for case in range(200):
        n = int(rng.integers(1, 16))
        P = n * (n - 1) // 2
        R = int(rng.integers(1, 7))
        if case % 3 == 0:
            preds = (rng.integers(0, 3, size=P) * 0.5).astype(np.float32)        # many ties
        else:
            preds = rng.random(P).astype(np.float32)
        preds[rng.random(P) < 0.2] = 0.0
        reps = np.stack([np.where(rng.random(P) < 0.25, 0.0, preds + rng.integers(-1, 2, size=P) * 0.5)
                         for _ in range(R)]).astype(np.float32)
        ids = [f"s{i % 4}" for i in range(n)]
        _both(preds, reps, ids)


def test_support_refuses_bad_replicates():
    from phyloformer_amd.hostio import nj_support
    with pytest.raises(ValueError):
        nj_support(np.zeros(6, np.float32), np.zeros((0, 6), np.float32), list("abcd"))
    with pytest.raises(ValueError):
        bs.support_newick_py(np.zeros(6, np.float32), np.zeros((2, 5), np.float32), list("abcd"))


# ---- CLI through the oracle engine (no GPU) ------------------------------------------------------------------------

def _write_fasta(path, idx, ids=None):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">{ids[k] if ids else f's{k}'}\n{''.join(alpha[int(v)] for v in row)}\n")


@pytest.fixture(scope="module")
def boot_dir(tmp_path_factory):
    from phyloformer_amd.msa_sim import simulate_batch
    d = tmp_path_factory.mktemp("boot_alns")
    for k, a in enumerate(simulate_batch(2, 6, 40, seed=21)):
        _write_fasta(d / f"a{k}.fa", a)
    _write_fasta(d / "b0.fa", simulate_batch(1, 5, 33, seed=22)[0])
    return d


def _cli(args, tmp_path):
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_boot_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=600)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def test_cli_bootstrap_zero_is_identical_to_no_flag(boot_dir, tmp_path):
    a = _cli([str(boot_dir), "-o", str(tmp_path / "a"), "-t"], tmp_path)
    b = _cli([str(boot_dir), "-o", str(tmp_path / "b"), "-t", "--bootstrap", "0"], tmp_path)
    assert a.returncode == 0 and b.returncode == 0, a.stderr[-2000:] + b.stderr[-2000:]
    assert _files(tmp_path / "a") == _files(tmp_path / "b") and len(_files(tmp_path / "a")) == 6


def test_cli_bootstrap_writes_one_support_tree_per_input(boot_dir, tmp_path):
    r = _cli([str(boot_dir), "-o", str(tmp_path / "o"), "-t", "--bootstrap", "5", "--seed", "2", "--bench"], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    files = _files(tmp_path / "o")
    assert sorted(n for n in files if n.endswith(".sup.nwk")) == ["a0.sup.nwk", "a1.sup.nwk", "b0.sup.nwk"]
    for stem in ("a0", "a1", "b0"):
        sup = files[f"{stem}.sup.nwk"].decode()
        assert _strip(sup).encode() == files[f"{stem}.nj.nwk"]
        labels = [int(v) for v in LABEL.findall(sup)]
        assert len(labels) == (3 if stem != "b0" else 2) and all(0 <= v <= 100 for v in labels)
    rep = json.loads([ln for ln in r.stderr.splitlines() if ln.startswith("{")][-1])
    assert rep["replicates"] == 5 and rep["bootstrap_s"] > 0
    # the same files through the Python I/O
    p = _cli([str(boot_dir), "-o", str(tmp_path / "p"), "-t", "--bootstrap", "5", "--seed", "2", "--python-io"], tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _files(tmp_path / "p") == files


def test_cli_bootstrap_refused_with_site_sharding(boot_dir, tmp_path):
    r = _cli([str(boot_dir), "-o", str(tmp_path / "s"), "--devices", "0,1", "--shard", "sites", "--bootstrap", "5"], tmp_path)
    assert r.returncode != 0 and "--bootstrap is not supported with --shard sites" in r.stderr
    assert not (tmp_path / "s").exists() or not os.listdir(tmp_path / "s")
    neg = _cli([str(boot_dir), "-o", str(tmp_path / "n"), "--bootstrap", "-1"], tmp_path)
    assert neg.returncode != 0 and "--bootstrap must be >= 0" in neg.stderr


# ---- ABI -----------------------------------------------------------------------------------------------------------

def test_header_declares_bootstrap_entry_points():
    h = open(os.path.join(REPO, "include", "phyloformer_amd.h")).read()
    assert re.search(r"^int pf_resample_sites_device\(pf_handle_t\* h, const uint8_t\* d_src, int32_t B, int32_t N, "
                     r"int32_t L,\s+int32_t r_begin, int32_t R, uint64_t seed, uint8_t\* d_dst\);", h, re.M)
    assert re.search(r"^int pf_bootstrap\(pf_handle_t\* h, const uint8_t\* idx, int32_t B, int32_t N, int32_t L, "
                     r"int32_t R,\s+uint64_t seed, float\* out\);", h, re.M)
    assert int(re.search(r"#define PF_ABI_VERSION (\d+)", h).group(1)) == 5
    from phyloformer_amd import build, engine
    assert "pf_boot.hip.h" in build.HEADERS and "pf_boot.hip.h" not in build.KERNEL_FILES
    assert {"pf_resample_sites_device", "pf_bootstrap"} <= set(engine.SIGNATURES) and engine.ABI_VERSION == 5
    build.build()
    lib = engine.load_library()
    assert hasattr(lib, "pf_bootstrap") and hasattr(lib, "pf_resample_sites_device") and lib.pf_abi_version() == 5
