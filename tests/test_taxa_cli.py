"""``infer_alns.py --leave-one-out`` through an oracle engine (no GPU): the unchanged ``<stem>.phy``, ``<stem>.taxa.tsv``
and ``<stem>.context.phy`` against ``taxa.loo_stats`` of the oracle's distances, the refused flag combinations, and a
file with fewer than 3 sequences as a per-file error in file order."""
import os
import subprocess
import sys

import numpy as np
import pytest

from phyloformer_amd import taxa as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_fasta(path, idx, ids=None):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">{ids[k] if ids else f's{k}'}\n{''.join(alpha[int(v)] for v in row)}\n")


@pytest.fixture(scope="module")
def loo_alns():
    from phyloformer_amd.msa_sim import simulate_batch
    a = simulate_batch(2, 6, 40, seed=71)
    return {"a0": a[0], "a1": a[1], "c0": simulate_batch(1, 4, 40, seed=72)[0]}


@pytest.fixture(scope="module")
def loo_dir(tmp_path_factory, loo_alns):
    d = tmp_path_factory.mktemp("loo_alns")
    for stem, a in loo_alns.items():
        _write_fasta(d / f"{stem}.fa", a, ids=["dup", "dup"] + [f"s{k}" for k in range(2, len(a))] if stem == "a1" else None)
    return d


def _cli(args, tmp_path):
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_taxa_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=900)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def _phylip_upper(text, N):
    rows = text.splitlines()
    assert int(rows[0]) == N and len(rows) == N + 1
    m = np.array([[float(v) for v in r.split()[-N:]] for r in rows[1:]])
    assert np.array_equal(m, m.T) and not m.diagonal().any()
    return m[np.triu_indices(N, k=1)]


def test_cli_leave_one_out_files(loo_dir, loo_alns, tmp_path):
    from helpers.oracle_taxa_engine import make
    from phyloformer_amd.weights import load_weights
    plain = _cli([str(loo_dir), "-o", str(tmp_path / "plain"), "-t"], tmp_path)
    r = _cli([str(loo_dir), "-o", str(tmp_path / "o"), "-t", "--leave-one-out"], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, plain.stderr[-2000:] + r.stderr[-3000:]
    files, base = _files(tmp_path / "o"), _files(tmp_path / "plain")
    assert set(files) == set(base) | {f"{s}.{ext}" for s in loo_alns for ext in ("taxa.tsv", "context.phy")}
    for name, data in base.items():
        assert files[name] == data, name                         # <stem>.phy / <stem>.nj.nwk exactly as without the flag
    eng = make(load_weights(os.path.join(REPO, "models", "pf_base.ckpt")), 0)
    for stem, a in loo_alns.items():
        N = a.shape[0]
        dist, infl, shift, ctx, loo = eng.forward_leave_one_out(a, keep_loo=True)
        want = T.loo_stats(dist, np.stack([eng.forward(c) for c in T.cut_taxa(a, T.leave_one_out_sets(N))]))
        assert all(np.array_equal(x, y) for x, y in zip((infl, shift, ctx), want))
        rows = [r.split("\t") for r in files[f"{stem}.taxa.tsv"].decode().splitlines()]
        assert rows[0] == ["index", "id", "influence", "shift", "relative", "rf_pruned"] and len(rows) == N + 1
        ids = ["dup", "dup"] + [f"s{k}" for k in range(2, N)] if stem == "a1" else [f"s{k}" for k in range(N)]
        for k, row in enumerate(rows[1:]):
            assert row[:2] == [str(k), ids[k]]
            assert row[2] == f"{float(infl[k]):.10f}" and row[3] == f"{float(shift[k]):.10f}"
            assert row[4] == f"{float(infl[k]) / float(np.asarray(infl, np.float64).mean()):.15f}"
            assert row[5] == "NA" if N - 1 < 4 else row[5].isdigit()          # (duplicate ids: index labels)
        assert abs(sum(float(r[4]) for r in rows[1:]) / N - 1.0) < 1e-12
        got_ctx = _phylip_upper(files[f"{stem}.context.phy"].decode(), N)
        assert np.array_equal(got_ctx, np.array([float(f"{float(v):.10f}") for v in ctx]))
        assert infl.min() > 0 and ctx.min() > 0
    # the same files through the Python I/O; without -t the table has no rf_pruned column
    p = _cli([str(loo_dir), "-o", str(tmp_path / "p"), "-t", "--leave-one-out", "--python-io"], tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _files(tmp_path / "p") == files
    n = _cli([str(loo_dir), "-o", str(tmp_path / "n"), "--leave-one-out", "--batch", "1"], tmp_path)
    assert n.returncode == 0, n.stderr[-3000:]
    nf = _files(tmp_path / "n")
    assert set(nf) == {k for k in files if not k.endswith(".nwk")}
    for k, v in nf.items():
        if k.endswith(".taxa.tsv"):
            assert v.decode().splitlines() == ["\t".join(r.split("\t")[:5]) for r in files[k].decode().splitlines()]
        else:
            assert v == files[k], k


def test_cli_leave_one_out_two_sequence_file_is_an_error_in_file_order(tmp_path, loo_alns):
    """glob order decides: every file in front of the 2-sequence one gets its outputs, nothing behind it does."""
    from glob import glob
    d = tmp_path / "in"
    d.mkdir()
    for stem, a in loo_alns.items():
        _write_fasta(d / f"{stem}.fa", a)
    _write_fasta(d / "b2.fa", loo_alns["a0"][:2])
    order = [os.path.basename(p)[:-3] for p in glob(f"{d}/*")]
    for io in ([], ["--python-io"]):
        out = tmp_path / ("o" + "".join(io))
        r = _cli([str(d), "-o", str(out), "--leave-one-out", *io], tmp_path)
        assert r.returncode != 0
        assert "b2.fa" in r.stderr and "N = 2" in r.stderr and "--leave-one-out" in r.stderr, r.stderr[-2000:]
        done = {n.split(".")[0] for n in os.listdir(out)}
        assert done == set(order[:order.index("b2")])
        for stem in done:
            assert {f"{stem}.phy", f"{stem}.taxa.tsv", f"{stem}.context.phy"} <= set(os.listdir(out))
    # the other files are written whatever the order: without the short file every one of them is
    (d / "b2.fa").unlink()
    r = _cli([str(d), "-o", str(tmp_path / "all"), "--leave-one-out"], tmp_path)
    assert r.returncode == 0 and {n.split(".")[0] for n in os.listdir(tmp_path / "all")} == set(loo_alns)


def test_cli_leave_one_out_refused_combinations(loo_dir, tmp_path):
    for extra, msg in ((["--bootstrap", "5"], "--leave-one-out is not supported with --bootstrap"),
                       (["--windows", "16"], "--leave-one-out is not supported with --windows"),
                       (["--site-profile"], "--leave-one-out is not supported with --site-profile"),
                       (["--devices", "0,1", "--shard", "sites"], "--leave-one-out is not supported with --shard sites"),
                       (["--shard", "sites"], "--leave-one-out is not supported with --shard sites")):
        r = _cli([str(loo_dir), "-o", str(tmp_path / "x"), "--leave-one-out", *extra], tmp_path)
        assert r.returncode == 2 and msg in r.stderr, r.stderr[-1000:]
        assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")
