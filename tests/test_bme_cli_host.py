"""The CLI's and the scheduler's side of ``--bme``, without a GPU: a stand-in engine whose distances depend on the
residues alone, whose ``nj_joins`` is ``nj.nj_joins`` and whose ``bme_nni`` is ``bme.bme_nni``.  ``--bme`` needs ``-t``,
writes ``<stem>.bme.nwk`` with the same bytes natively and with ``--python-io``, leaves every other file's bytes alone,
runs beside ``--bootstrap``, ``--windows`` and ``--tile``, counts what it did, and takes the device branch from
``BME_DEVICE_MIN`` sequences on - with the host's bytes, and the host's path for a flagged source."""
import os

import numpy as np
import pytest

import infer_alns
from helpers.nj_table import table_of
from phyloformer_amd import analyses, bme, scheduler

M, BIG, SMALL, L = 4, 9, 3, 12


class Engine:
    def __init__(self, flag_first=False):
        self.bme_calls, self.bme_sources, self.nj_sources, self.flag_first = 0, 0, 0, flag_first

    @staticmethod
    def _dist(batch, salt, extra=()):
        batch = np.asarray(batch)
        out = np.empty((len(batch), *extra, batch.shape[1] * (batch.shape[1] - 1) // 2), np.float32)
        for b, a in enumerate(batch):
            out[b] = np.random.default_rng(int(a.astype(np.int64).sum()) + salt).uniform(0.05, 2.0, size=out.shape[1:])
        return out

    def forward(self, batch):
        return self._dist(batch, 1)

    def forward_tiled(self, batch, m):
        out = self._dist(batch, 1)
        return out, (out * 0.125).astype(np.float32)

    def bootstrap(self, batch, replicates, seed):
        return self._dist(batch, 3 + seed, (replicates,))

    def forward_windows(self, batch, width, step):
        from phyloformer_amd.windows import window_starts
        return self._dist(batch, 4, (len(window_starts(np.asarray(batch).shape[2], width, step)),))

    def nj_joins(self, preds):
        self.nj_sources += len(preds)
        n = (1 + int(round((1 + 8 * preds.shape[1]) ** 0.5))) // 2
        tables = [table_of(p, n) for p in preds]
        flag = np.zeros(len(preds), bool)
        if self.flag_first:
            flag[0] = True
            tables[0] = (np.full_like(tables[0][0], -1), np.full_like(tables[0][1], np.nan))      # unspecified
        return np.stack([t[0] for t in tables]), np.stack([t[1] for t in tables]), flag

    def bme_nni(self, preds, starts):
        self.bme_calls += 1
        self.bme_sources += len(preds)
        n = (1 + int(round((1 + 8 * preds.shape[1]) ** 0.5))) // 2
        res = [bme.bme_nni(bme.matrix_of_preds(p, n), s) for p, s in zip(preds, starts)]   # (ValueError for a bad table)
        if self.flag_first:
            t = 2 * (n - 3) + 3
            res[0] = (np.zeros(t, np.int32), np.zeros(t), 0, 0.0, bme.NONFINITE)
        return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.int32),
                np.array([r[3] for r in res]), np.array([r[4] for r in res], np.uint8))


def _write_fasta(path, idx):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">s{k % 7}\n{''.join(alpha[int(v)] for v in row)}\n")       # (duplicate ids)


@pytest.fixture(scope="module")
def alns(tmp_path_factory):
    d = tmp_path_factory.mktemp("bme_cli")
    rng = np.random.default_rng(78)
    for stem, n in (("big_a", BIG), ("big_b", BIG), ("small", SMALL)):
        _write_fasta(d / f"{stem}.fa", rng.integers(0, 20, size=(n, L)))
    return sorted(str(d / f) for f in os.listdir(d))


def _run(paths, out, engine, native_io, bme_flag=True, modes=(), batch=0):
    if native_io:
        from phyloformer_amd import build
        build.build()
    os.makedirs(out)
    runner = scheduler.DirectoryRunner(engine, str(out), trees=True, native_io=native_io, batch=batch, modes=list(modes), bme=bme_flag)
    stats = runner.run(paths)
    return {n: open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out))}, stats


def test_bme_needs_trees(tmp_path, capsys):
    with pytest.raises(SystemExit):
        infer_alns.main(["w.ckpt", str(tmp_path), "-o", str(tmp_path / "o"), "--bme"])
    assert "--bme refines the tree of --trees" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--bme"):
        scheduler.DirectoryRunner(Engine(), str(tmp_path), trees=False, bme=True)
    args = infer_alns.build_parser().parse_args(["w.ckpt", "d", "-t", "--bme"])
    assert args.bme and args.trees and not infer_alns.build_parser().parse_args(["w.ckpt", "d", "-t"]).bme
    assert analyses.MODES[-1] is analyses.Tile and all(m.flag != "--bme" for m in analyses.MODES)


def test_native_and_python_io_write_the_same_trees_and_nothing_else_changes(alns, tmp_path, monkeypatch):
    monkeypatch.setattr(bme, "BME_DEVICE_MIN", None)
    plain, plain_stats = _run(alns, tmp_path / "plain", Engine(), True, bme_flag=False)
    native, stats = _run(alns, tmp_path / "native", Engine(), True)
    python, py_stats = _run(alns, tmp_path / "python", Engine(), False)
    stems = ("big_a", "big_b", "small")
    assert set(plain) == {f"{s}.{x}" for s in stems for x in ("phy", "nj.nwk")}
    assert set(native) == set(plain) | {f"{s}.bme.nwk" for s in stems}
    assert all(native[k] == v for k, v in plain.items())                     # every other file keeps its bytes
    assert native == python
    for stem, n in (("big_a", BIG), ("big_b", BIG), ("small", SMALL)):
        assert native[f"{stem}.bme.nwk"].endswith(b";\n") and native[f"{stem}.bme.nwk"].count(b",") == n - 1
    assert native["big_a.bme.nwk"] != native["big_a.nj.nwk"]                  # balanced lengths, if not another tree
    for s in (stats, py_stats):
        assert s["bme"] == 3 and s["bme_steps"] >= 0 and s["bme_device"] == 0 and s["bme_device_s"] == 0.0
    assert stats["bme_steps"] == py_stats["bme_steps"]
    assert not any(k.startswith("bme") for k in plain_stats)
    assert {"bme", "bme_steps", "bme_device", "bme_device_s"} <= set(scheduler.summarize(stats))
    assert not any(k.startswith("bme") for k in scheduler.summarize(plain_stats))


@pytest.mark.parametrize("native_io", [True, False])
def test_beside_bootstrap_windows_and_tile(alns, tmp_path, monkeypatch, native_io):
    monkeypatch.setattr(bme, "BME_DEVICE_MIN", None)
    monkeypatch.setattr(analyses, "NJ_DEVICE_MIN", None)
    base, _ = _run(alns, tmp_path / "base", Engine(), native_io)
    for name, modes in (("boot", [analyses.Bootstrap(5, 1)]), ("win", [analyses.Windows(6, 6)]), ("tile", [analyses.Tile(M)])):
        without, _ = _run(alns, tmp_path / f"{name}_off", Engine(), native_io, bme_flag=False, modes=modes)
        with_, stats = _run(alns, tmp_path / f"{name}_on", Engine(), native_io, modes=modes)
        assert set(with_) == set(without) | {f"{s}.bme.nwk" for s in ("big_a", "big_b", "small")}, name
        assert all(with_[k] == v for k, v in without.items()), name
        # the whole alignment's tree only, and the same one whatever the mode beside it
        assert all(with_[f"{s}.bme.nwk"] == base[f"{s}.bme.nwk"] for s in ("big_a", "big_b", "small")), name
        assert stats["bme"] == 3
    for flags in (["--leave-one-out"], ["--site-profile"], ["--bootstrap", "5"]):           # the parser refuses none of them
        args = infer_alns.build_parser().parse_args(["w", "d", "-t", "--bme", *flags])
        assert len(analyses.modes_from_args(args, lambda text: pytest.fail(text))) == 1 and args.bme


@pytest.mark.parametrize("native_io", [True, False])
def test_device_branch_from_the_threshold_on_with_the_hosts_bytes(alns, tmp_path, monkeypatch, native_io):
    monkeypatch.setattr(bme, "BME_DEVICE_MIN", None)
    off_engine = Engine()
    off, off_stats = _run(alns, tmp_path / "off", off_engine, native_io)
    assert off_engine.bme_calls == 0 and off_stats["bme_device"] == 0

    monkeypatch.setattr(bme, "BME_DEVICE_MIN", 5)                             # 3 < 5 <= 9
    engine = Engine()
    on, stats = _run(alns, tmp_path / "on", engine, native_io)
    assert on == off
    assert engine.bme_calls == 1 and engine.bme_sources == 2 and engine.nj_sources == 2
    assert stats["bme_device"] == 2 and stats["bme_device_s"] > 0 and stats["bme"] == 3
    assert stats["bme_steps"] == off_stats["bme_steps"]

    engine = Engine(flag_first=True)                                          # a flagged source keeps the host's path
    flagged, stats = _run(alns, tmp_path / "flagged", engine, native_io)
    assert flagged == off and engine.bme_calls == 1 and stats["bme_device"] == 1 and stats["bme"] == 3

    monkeypatch.setattr(bme, "BME_DEVICE_MIN", BIG + 1)
    engine = Engine()
    below, stats = _run(alns, tmp_path / "below", engine, native_io)
    assert below == off and engine.bme_calls == 0 and stats["bme_device"] == 0

    monkeypatch.setattr(bme, "BME_DEVICE_MIN", 1)                             # fewer than three sequences have no table
    engine = Engine()
    tiny, stats = _run(alns, tmp_path / "tiny", engine, native_io, batch=1)
    assert tiny == off and engine.bme_calls == 3 and stats["bme_device"] == 3
