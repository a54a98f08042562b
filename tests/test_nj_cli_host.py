"""The scheduler's side of the device neighbour joining, without a GPU: ``--tile M -t`` over a file above the threshold
through a stand-in engine whose ``nj_joins`` is ``nj.nj_joins``.  The tree's bytes are those of the run with the device
path switched off, it is computed once, the stats count it, a flagged source falls back to the host, and a run without
``--tile`` never asks for joins."""
import os

import numpy as np
import pytest

from helpers.nj_table import table_of
from phyloformer_amd import analyses, scheduler

M, BIG, SMALL, L = 4, 9, 3, 12


class Engine:
    """forward / forward_tiled: distances that depend on the residues alone; nj_joins: nj.nj_joins per source."""

    def __init__(self, flag_first=False):
        self.nj_calls, self.nj_sources, self.flag_first = 0, 0, flag_first

    @staticmethod
    def _dist(batch, salt):
        out = np.empty((len(batch), batch.shape[1] * (batch.shape[1] - 1) // 2), np.float32)
        for b, a in enumerate(batch):
            out[b] = np.random.default_rng(int(a.astype(np.int64).sum()) + salt).uniform(0.05, 2.0, size=out.shape[1])
        return out

    def forward(self, batch):
        return self._dist(np.asarray(batch), 1)

    def forward_tiled(self, batch, m):
        assert m == M and batch.shape[1] > m
        out = self._dist(np.asarray(batch), 2)
        return out, (out * 0.125).astype(np.float32)

    def nj_joins(self, preds):
        self.nj_calls += 1
        self.nj_sources += len(preds)
        n = BIG
        tables = [table_of(p, n) for p in preds]
        flag = np.zeros(len(preds), bool)
        if self.flag_first:
            flag[0] = True
            tables[0] = (np.full_like(tables[0][0], -1), np.full_like(tables[0][1], np.nan))      # unspecified
        return np.stack([t[0] for t in tables]), np.stack([t[1] for t in tables]), flag


def _write_fasta(path, idx):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">s{k % 7}\n{''.join(alpha[int(v)] for v in row)}\n")       # (duplicate ids)


@pytest.fixture(scope="module")
def alns(tmp_path_factory):
    d = tmp_path_factory.mktemp("nj_cli")
    rng = np.random.default_rng(77)
    for stem, n in (("big_a", BIG), ("big_b", BIG), ("small", SMALL)):
        _write_fasta(d / f"{stem}.fa", rng.integers(0, 20, size=(n, L)))
    return sorted(str(d / f) for f in os.listdir(d))


def _run(paths, out, engine, native_io, tile=True, monkeypatch=None, batch=0):
    """One run; returns (files, stats, host trees computed): the host neighbour joinings of the default writer and of
    the modes - ``DirectoryRunner.nj`` calls plus the tree paths handed to the native writer."""
    os.makedirs(out)
    host = []
    real_nj = scheduler.DirectoryRunner.nj
    monkeypatch.setattr(scheduler.DirectoryRunner, "nj", lambda self, vec, ids: (host.append(len(ids)), real_nj(self, vec, ids))[1])
    if native_io:
        from phyloformer_amd import hostio
        real_wp = hostio.write_phylip

        def write_phylip(entries, n, preds, out_paths, threads=8, tree_paths=None):
            host.extend([n] * (len(tree_paths) if tree_paths is not None else 0))
            return real_wp(entries, n, preds, out_paths, threads, tree_paths)
        monkeypatch.setattr(hostio, "write_phylip", write_phylip)
    runner = scheduler.DirectoryRunner(engine, str(out), trees=True, native_io=native_io, batch=batch,
                                       modes=[analyses.Tile(M)] if tile else [])
    stats = runner.run(paths)
    return {n: open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out))}, stats, host


@pytest.mark.parametrize("native_io", [True, False])
def test_device_tree_is_the_hosts_bytes_and_is_computed_once(alns, tmp_path, monkeypatch, native_io):
    if native_io:
        from phyloformer_amd import build
        build.build()
    monkeypatch.setattr(analyses, "NJ_DEVICE_MIN", None)                      # the device path switched off
    off_engine = Engine()
    off, off_stats, off_host = _run(alns, tmp_path / "off", off_engine, native_io, monkeypatch=monkeypatch)
    assert off_engine.nj_calls == 0 and off_stats["nj_device"] == 0 and sorted(off_host) == [SMALL, BIG, BIG]
    assert set(off) == {f"{s}.{x}" for s in ("big_a", "big_b") for x in ("phy", "nj.nwk", "spread.phy", "tile.tsv")} | {"small.phy", "small.nj.nwk"}

    monkeypatch.setattr(analyses, "NJ_DEVICE_MIN", 5)                         # 3 < 5 <= 9
    engine = Engine()
    on, stats, host = _run(alns, tmp_path / "on", engine, native_io, monkeypatch=monkeypatch)
    assert on == off                                                          # every file, byte for byte
    assert b"s0" in on["big_a.nj.nwk"] and on["big_a.nj.nwk"] != on["big_b.nj.nwk"]
    assert engine.nj_calls == 1 and engine.nj_sources == 2                     # one call for the launch's two files
    assert host == [SMALL]                                                     # the host joined the small file's tree only
    assert stats["nj_device"] == 2 and stats["nj_device_s"] > 0 and stats["tiled"] == 2

    # one file per launch; N below the threshold: today's path
    engine = Engine()
    one, stats, host = _run(alns, tmp_path / "one", engine, native_io, monkeypatch=monkeypatch, batch=1)
    assert one == off and engine.nj_calls == 2 and stats["nj_device"] == 2 and host == [SMALL]
    monkeypatch.setattr(analyses, "NJ_DEVICE_MIN", BIG + 1)
    engine = Engine()
    below, stats, host = _run(alns, tmp_path / "below", engine, native_io, monkeypatch=monkeypatch)
    assert below == off and engine.nj_calls == 0 and stats["nj_device"] == 0 and sorted(host) == [SMALL, BIG, BIG]


@pytest.mark.parametrize("native_io", [True, False])
def test_a_flagged_source_falls_back_to_the_host(alns, tmp_path, monkeypatch, native_io):
    if native_io:
        from phyloformer_amd import build
        build.build()
    monkeypatch.setattr(analyses, "NJ_DEVICE_MIN", None)
    off, _stats, _host = _run(alns, tmp_path / "off", Engine(), native_io, monkeypatch=monkeypatch)
    monkeypatch.setattr(analyses, "NJ_DEVICE_MIN", 5)
    engine = Engine(flag_first=True)
    on, stats, host = _run(alns, tmp_path / "on", engine, native_io, monkeypatch=monkeypatch)
    assert on == off
    assert engine.nj_calls == 1 and stats["nj_device"] == 1 and sorted(host) == [SMALL, BIG]


def test_without_tile_joins_are_never_asked_for(alns, tmp_path, monkeypatch):
    monkeypatch.setattr(analyses, "NJ_DEVICE_MIN", 2)
    engine = Engine()
    files, stats, host = _run(alns, tmp_path / "plain", engine, False, tile=False, monkeypatch=monkeypatch)
    assert engine.nj_calls == 0 and "nj_device" not in stats and sorted(host) == [SMALL, BIG, BIG]
    assert set(files) == {f"{s}.{x}" for s in ("big_a", "big_b", "small") for x in ("phy", "nj.nwk")}


def test_the_constant_and_the_question():
    assert analyses.NJ_DEVICE_MIN is None or analyses.NJ_DEVICE_MIN >= 201
    assert analyses.Analysis().writes_tree((5000, 10)) is False
    t = analyses.Tile(100)
    if analyses.NJ_DEVICE_MIN is not None:
        assert t.writes_tree((analyses.NJ_DEVICE_MIN, 10)) and not t.writes_tree((analyses.NJ_DEVICE_MIN - 1, 10))
    assert not t.writes_tree((100, 10)) and not analyses.Tile(200).writes_tree((200, 10))
    src = open(scheduler.__file__).read()
    assert "Tile" not in src and "NJ_DEVICE_MIN" not in src                 # the runner names no mode
