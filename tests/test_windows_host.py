"""Site-window scans on the host (no GPU): the window rule (Python twin and the library's), cut_sites, the CLI's
--windows plumbing through an oracle engine, and the ABI additions."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from phyloformer_amd import windows as pw

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the window rule -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,W,step,want", [(10, 4, 4, [0, 4, 6]), (12, 4, 4, [0, 4, 8]), (10, 10, 3, [0]),
                                           (10, 4, 1, [0, 1, 2, 3, 4, 5, 6])])
def test_window_starts_literal(L, W, step, want):
    assert pw.window_starts(L, W, step) == want


def test_window_starts_default_step_is_width():
    assert pw.window_starts(10, 4) == pw.window_starts(10, 4, 4) == [0, 4, 6]
    assert pw.window_starts(500, 200, 120) == [0, 120, 240, 300]


@pytest.mark.parametrize("L,W,step", [(10, 11, 1), (10, 0, 1), (10, -3, 1), (10, 4, 0), (10, 4, -1)])
def test_window_starts_refusals(L, W, step):
    with pytest.raises(ValueError):
        pw.window_starts(L, W, step)


def test_window_starts_cover_every_site():
    """Regular starts step apart, all inside [0, L - W], the last window ends at L or is the regular one that does; with
    step <= W every site is in some window."""
    rng = np.random.default_rng(0)
    for _ in range(300):
        L = int(rng.integers(1, 400))
        W = int(rng.integers(1, L + 1))
        step = int(rng.integers(1, 2 * L + 2))
        st = pw.window_starts(L, W, step)
        regular = [s for s in range(0, L, step) if s + W <= L]
        assert st[:len(regular)] == regular and len(st) - len(regular) in (0, 1)
        assert st[-1] == L - W and st == sorted(set(st))
        if step <= W:
            covered = np.zeros(L, bool)
            for s in st:
                covered[s:s + W] = True
            assert covered.all()


def test_library_window_rule_agrees_with_twin():
    from phyloformer_amd import build, engine
    if not os.path.exists(build.LIB):
        pytest.skip("native library not built")
    lib = engine.load_library()
    rng = np.random.default_rng(1)
    triples = [(10, 4, 4), (12, 4, 4), (10, 10, 3), (10, 4, 1), (1, 1, 1), (2 ** 31 - 1, 1, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1, 1)]
    triples += [(int(L), int(rng.integers(1, L + 1)), int(rng.integers(1, 2 * L + 2))) for L in rng.integers(1, 5000, size=400)]
    for L, W, step in triples:
        st = pw.window_starts(L, W, step)
        assert lib.pf_window_count(L, W, step) == len(st), (L, W, step)
        assert [lib.pf_window_start(L, W, step, s) for s in range(len(st))] == st, (L, W, step)
        assert lib.pf_window_start(L, W, step, len(st)) == -1 and lib.pf_window_start(L, W, step, -1) == -1
    for L, W, step in [(10, 11, 1), (10, 0, 1), (10, 4, 0), (0, 1, 1), (10, -1, 1), (10, 4, -2)]:
        assert lib.pf_window_count(L, W, step) == -1 and lib.pf_window_start(L, W, step, 0) == -1
    assert lib.pf_window_count(2 ** 31 - 1, 1, 1) == 2 ** 31 - 1


# ---- cut_sites -----------------------------------------------------------------------------------------------------

def test_cut_sites_layout_and_refusals():
    rng = np.random.default_rng(2)
    idx = rng.integers(0, 22, size=(2, 4, 30), dtype=np.uint8)
    sites = np.array([[0, 29, 3, 3], [7, 6, 5, 4]])
    cut = pw.cut_sites(idx, sites)
    assert cut.shape == (2, 2, 4, 4) and cut.dtype == np.uint8 and cut.flags["C_CONTIGUOUS"]
    for b in range(2):
        for s in range(2):
            assert np.array_equal(cut[b, s], idx[b][:, sites[s]])
    assert np.array_equal(pw.cut_sites(idx[1], sites), cut[1])
    win = pw.cut_sites(idx, pw.window_sites(30, 8, 7))
    for k, st in enumerate(pw.window_starts(30, 8, 7)):
        assert np.array_equal(win[:, k], idx[:, :, st:st + 8])
    for bad in ([[30]], [[-1]], [[0.5]]):
        with pytest.raises(ValueError):
            pw.cut_sites(idx, np.array(bad))


def test_window_labels_are_one_based_and_padded():
    assert pw.window_label(40, 0, 16) == "w01-16" and pw.window_label(1000, 0, 100) == "w0001-0100"
    assert pw.window_label(999, 899, 100) == "w900-999" and pw.window_label(5, 4, 1) == "w5-5"
    assert pw.parse_windows_arg("100:50") == (100, 50) and pw.parse_windows_arg("7") == (7, 7)
    for bad in ("0", "5:0", "a", "1:2:3", ""):
        with pytest.raises(ValueError):
            pw.parse_windows_arg(bad)


# ---- CLI through the oracle engine (no GPU) ------------------------------------------------------------------------

def _write_fasta(path, idx, ids=None):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">{ids[k] if ids else f's{k}'}\n{''.join(alpha[int(v)] for v in row)}\n")


@pytest.fixture(scope="module")
def win_alns():
    from phyloformer_amd.msa_sim import simulate_batch
    a = simulate_batch(2, 6, 40, seed=41)
    return {"a0": a[0], "a1": a[1], "b0": simulate_batch(1, 5, 33, seed=42)[0]}


@pytest.fixture(scope="module")
def win_dir(tmp_path_factory, win_alns):
    d = tmp_path_factory.mktemp("win_alns")
    for stem, a in win_alns.items():
        _write_fasta(d / f"{stem}.fa", a)
    return d


def _cli(args, tmp_path):
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_windows_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=900)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def test_cli_windows_files_table_and_python_io(win_dir, win_alns, tmp_path):
    from helpers.oracle_windows_engine import make
    from phyloformer_amd import treecmp
    from phyloformer_amd.nj import neighbor_joining
    from phyloformer_amd.phylip import vec_to_phylip
    from phyloformer_amd.weights import load_weights
    plain = _cli([str(win_dir), "-o", str(tmp_path / "plain"), "-t"], tmp_path)
    r = _cli([str(win_dir), "-o", str(tmp_path / "o"), "-t", "--windows", "16:12"], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, plain.stderr[-2000:] + r.stderr[-3000:]
    files, base = _files(tmp_path / "o"), _files(tmp_path / "plain")
    labels = {40: ["w01-16", "w13-28", "w25-40"], 33: ["w01-16", "w13-28", "w18-33"]}
    want = set(base)
    for stem, a in win_alns.items():
        want |= {f"{stem}.windows.tsv"} | {f"{stem}.{lab}.{ext}" for lab in labels[a.shape[1]] for ext in ("phy", "nj.nwk")}
    assert set(files) == want
    for name, data in base.items():
        assert files[name] == data, name                         # <stem>.phy / <stem>.nj.nwk exactly as without the flag
    eng = make(load_weights(os.path.join(REPO, "models", "pf_base.ckpt")), 0)
    for stem, a in win_alns.items():
        N, L = a.shape
        ids = [f"s{k}" for k in range(N)]
        starts = pw.window_starts(L, 16, 12)
        cut = pw.cut_sites(a, pw.window_sites(L, 16, 12))
        rows = files[f"{stem}.windows.tsv"].decode().splitlines()
        assert rows[0].split("\t") == ["first", "last", "mean_distance", "rf_prev", "rf_full"] and len(rows) == 1 + len(starts)
        full = treecmp.parse_newick(files[f"{stem}.nj.nwk"].decode())
        prev = None
        for k, st in enumerate(starts):
            pred = eng.forward(cut[k])
            dm, text = vec_to_phylip(pred, ids)
            lab = labels[L][k]
            assert files[f"{stem}.{lab}.phy"].decode() == text
            nwk = neighbor_joining(dm.astype("float64"), ids)
            assert files[f"{stem}.{lab}.nj.nwk"].decode() == nwk
            tree = treecmp.parse_newick(nwk)
            first, last, mean, rf_prev, rf_full = rows[1 + k].split("\t")
            assert (int(first), int(last)) == (st + 1, st + 16)
            assert mean == f"{float(np.asarray(pred, np.float64).mean()):.10f}"
            assert rf_prev == ("NA" if k == 0 else str(treecmp.robinson_foulds(tree, prev)[0]))
            assert rf_full == str(treecmp.robinson_foulds(tree, full)[0])
            prev = tree
    # the same files through the Python I/O; without -t the table is the same and no window tree is written
    p = _cli([str(win_dir), "-o", str(tmp_path / "p"), "-t", "--windows", "16:12", "--python-io"], tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _files(tmp_path / "p") == files
    n = _cli([str(win_dir), "-o", str(tmp_path / "n"), "--windows", "16:12"], tmp_path)
    assert n.returncode == 0, n.stderr[-3000:]
    assert _files(tmp_path / "n") == {k: v for k, v in files.items() if not k.endswith(".nwk")}


def test_cli_windows_default_step_and_single_window(win_dir, tmp_path):
    """STEP defaults to W.  a0 / a1 have 40 sites: w01-33 and the anchored w08-40; b0 has 33: exactly one window."""
    r = _cli([str(win_dir), "-o", str(tmp_path / "o"), "--windows", "33"], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    files = _files(tmp_path / "o")
    assert {n for n in files if ".w" in n and n.endswith(".phy")} == {
        "b0.w01-33.phy", "a0.w01-33.phy", "a0.w08-40.phy", "a1.w01-33.phy", "a1.w08-40.phy"}
    assert files["b0.w01-33.phy"] == files["b0.phy"]
    rows = files["b0.windows.tsv"].decode().splitlines()
    assert len(rows) == 2 and rows[1].split("\t")[:2] == ["1", "33"] and rows[1].split("\t")[3:] == ["NA", "0"]


def test_cli_windows_short_file_is_an_error_in_file_order(tmp_path, win_alns):
    """glob order decides: every file in front of the short one gets its outputs, nothing behind it does."""
    from glob import glob
    d = tmp_path / "in"
    d.mkdir()
    for stem, a in win_alns.items():
        _write_fasta(d / f"{stem}.fa", a)
    order = [os.path.basename(p)[:-3] for p in glob(f"{d}/*")]
    for io in ([], ["--python-io"]):
        out = tmp_path / ("o" + "".join(io))
        r = _cli([str(d), "-o", str(out), "--windows", "36", *io], tmp_path)
        assert r.returncode != 0
        assert "b0.fa" in r.stderr and "L = 33" in r.stderr and "W = 36" in r.stderr, r.stderr[-2000:]
        done = {n.split(".")[0] for n in os.listdir(out)}
        assert done == set(order[:order.index("b0")])


def test_cli_windows_refused_combinations(win_dir, tmp_path):
    for extra, msg in ((["--bootstrap", "5"], "--windows is not supported with --bootstrap"),
                       (["--devices", "0,1", "--shard", "sites"], "--windows is not supported with --shard sites"),
                       (["--shard", "sites"], "--windows is not supported with --shard sites")):
        r = _cli([str(win_dir), "-o", str(tmp_path / "x"), "--windows", "16", *extra], tmp_path)
        assert r.returncode == 2 and msg in r.stderr, r.stderr[-1000:]
        assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")
    for bad in ("0", "16:0", "x", "16:4:2"):
        r = _cli([str(win_dir), "-o", str(tmp_path / "x"), "--windows", bad], tmp_path)
        assert r.returncode == 2 and "--windows" in r.stderr


# ---- ABI -----------------------------------------------------------------------------------------------------------

def test_header_declares_site_map_entry_points():
    h = open(os.path.join(REPO, "include", "phyloformer_amd.h")).read()
    for name in ("pf_window_count", "pf_window_start", "pf_gather_sites_device", "pf_forward_sites", "pf_forward_windows"):
        assert re.search(rf"^int {name}\(", h, re.M), name
    assert int(re.search(r"#define PF_ABI_VERSION (\d+)", h).group(1)) == 5
    from phyloformer_amd import build, engine
    assert {"pf_sites.hip.h", "pf_sites_host.h"} <= set(build.HEADERS)
    assert not {"pf_sites.hip.h", "pf_sites_host.h"} & set(build.KERNEL_FILES)       # the kernel hash does not move
    assert {"pf_window_count", "pf_window_start", "pf_gather_sites_device", "pf_forward_sites",
            "pf_forward_windows"} <= set(engine.SIGNATURES) and engine.ABI_VERSION == 5
    build.build()
    lib = engine.load_library()
    assert hasattr(lib, "pf_forward_windows") and hasattr(lib, "pf_gather_sites_device") and lib.pf_abi_version() == 5
