"""The CLI's and the scheduler's side of ``--bionj``, without a GPU: a stand-in engine whose distances depend on the
residues alone, whose ``bionj_joins`` is ``bionj.bionj_joins`` and whose searches are ``bme.py``'s.  ``--bionj`` needs
``-t``, writes ``<stem>.bionj.nwk`` - and with ``--bme`` / ``--spr`` ``<stem>.bionj.bme.nwk`` / ``<stem>.bionj.spr.nwk`` -
with the same bytes natively and with ``--python-io``, leaves every other file's bytes alone, counts what it did, and
takes the device branch from ``BIONJ_DEVICE_MIN`` sequences on - with the host's bytes, and the host's path for a flagged
source."""
import os

import numpy as np
import pytest

import infer_alns
from helpers.bionj_table import table_of
from helpers.nj_table import table_of as nj_table_of
from phyloformer_amd import bionj, bme, scheduler

BIG, SMALL, L = 9, 3, 12
STEMS = ("big_a", "big_b", "small")


class Engine:
    def __init__(self, flag_first=False):
        self.calls = {"bionj_joins": 0, "nj_joins": 0, "bme_nni": 0, "bme_spr": 0}
        self.flag_first = flag_first

    def forward(self, batch):
        batch = np.asarray(batch)
        out = np.empty((len(batch), batch.shape[1] * (batch.shape[1] - 1) // 2), np.float32)
        for b, a in enumerate(batch):
            out[b] = np.random.default_rng(int(a.astype(np.int64).sum()) + 1).uniform(0.05, 2.0, size=out.shape[1])
        return out

    def _joins(self, name, table, preds):
        self.calls[name] += 1
        n = (1 + int(round((1 + 8 * preds.shape[1]) ** 0.5))) // 2
        tables = [table(p, n) for p in preds]
        flag = np.zeros(len(preds), bool)
        if self.flag_first:
            flag[0] = True
            tables[0] = (np.full_like(tables[0][0], -1), np.full_like(tables[0][1], np.nan))      # unspecified
        return np.stack([t[0] for t in tables]), np.stack([t[1] for t in tables]), flag

    def bionj_joins(self, preds):
        return self._joins("bionj_joins", table_of, preds)

    def nj_joins(self, preds):
        return self._joins("nj_joins", nj_table_of, preds)

    def _refine(self, name, search, preds, starts):
        self.calls[name] += 1
        n = (1 + int(round((1 + 8 * preds.shape[1]) ** 0.5))) // 2
        res = [search(bme.matrix_of_preds(p, n), s) for p, s in zip(preds, starts)]           # (ValueError for a bad table)
        if self.flag_first:
            t = 2 * (n - 3) + 3
            res[0] = (np.zeros(t, np.int32), np.zeros(t), 0, 0.0, bme.NONFINITE)
        return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.int32),
                np.array([r[3] for r in res]), np.array([r[4] for r in res], np.uint8))

    def bme_nni(self, preds, starts):
        return self._refine("bme_nni", bme.bme_nni, preds, starts)

    def bme_spr(self, preds, starts):
        return self._refine("bme_spr", bme.bme_spr, preds, starts)


def _write_fasta(path, idx):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">s{k % 7}\n{''.join(alpha[int(v)] for v in row)}\n")       # (duplicate ids)


@pytest.fixture(scope="module")
def alns(tmp_path_factory):
    d = tmp_path_factory.mktemp("bionj_cli")
    rng = np.random.default_rng(79)
    for stem, n in (("big_a", BIG), ("big_b", BIG), ("small", SMALL)):
        _write_fasta(d / f"{stem}.fa", rng.integers(0, 20, size=(n, L)))
    return sorted(str(d / f) for f in os.listdir(d))


def _run(paths, out, engine, native_io, batch=0, **flags):
    if native_io:
        from phyloformer_amd import build
        build.build()
    os.makedirs(out)
    runner = scheduler.DirectoryRunner(engine, str(out), trees=True, native_io=native_io, batch=batch, **flags)
    stats = runner.run(paths)
    return {n: open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out))}, stats


@pytest.fixture(autouse=True)
def host_refinements(monkeypatch):
    """The NJ-started refinements stay on the host in every test here: their device branch is test_bme_cli_host's."""
    monkeypatch.setattr(bme, "BME_DEVICE_MIN", None)
    monkeypatch.setattr(bme, "SPR_DEVICE_MIN", None)


def test_usage_errors(tmp_path, capsys):
    with pytest.raises(SystemExit):
        infer_alns.main(["w.ckpt", str(tmp_path), "-o", str(tmp_path / "o"), "--bionj"])
    assert "--bionj writes a tree beside that of --trees" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        infer_alns.main(["w.ckpt", str(tmp_path), "-o", str(tmp_path / "o"), "-t", "--bionj", "--devices", "0,1", "--shard", "sites"])
    assert "--bionj cannot be combined with --shard sites" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--bionj"):
        scheduler.DirectoryRunner(Engine(), str(tmp_path), trees=False, bionj=True)
    args = infer_alns.build_parser().parse_args(["w.ckpt", "d", "-t", "--bionj", "--spr"])
    assert args.bionj and args.spr and not args.bme and not infer_alns.build_parser().parse_args(["w.ckpt", "d", "-t"]).bionj


def test_files_names_bytes_and_stats(alns, tmp_path, monkeypatch):
    monkeypatch.setattr(bionj, "BIONJ_DEVICE_MIN", None)
    plain, plain_stats = _run(alns, tmp_path / "plain", Engine(), True, bme=True, spr=True)
    native, stats = _run(alns, tmp_path / "native", Engine(), True, bme=True, spr=True, bionj=True)
    python, py_stats = _run(alns, tmp_path / "python", Engine(), False, bme=True, spr=True, bionj=True)
    assert set(plain) == {f"{s}.{x}" for s in STEMS for x in ("phy", "nj.nwk", "bme.nwk", "spr.nwk")}
    assert set(native) == set(plain) | {f"{s}.{x}" for s in STEMS for x in ("bionj.nwk", "bionj.bme.nwk", "bionj.spr.nwk")}
    assert all(native[k] == v for k, v in plain.items())                     # every existing output keeps its bytes
    assert native == python                                                  # --python-io: byte-identical
    only, only_stats = _run(alns, tmp_path / "only", Engine(), True, bionj=True)
    assert set(only) == {f"{s}.{x}" for s in STEMS for x in ("phy", "nj.nwk", "bionj.nwk")}
    assert all(native[k] == v for k, v in only.items())
    for stem, n in (("big_a", BIG), ("big_b", BIG), ("small", SMALL)):
        for x in ("bionj.nwk", "bionj.bme.nwk", "bionj.spr.nwk"):
            assert native[f"{stem}.{x}"].endswith(b";\n") and native[f"{stem}.{x}"].count(b",") == n - 1
    assert native["big_a.bionj.nwk"] != native["big_a.nj.nwk"]
    assert native["big_a.bionj.bme.nwk"] != native["big_a.bionj.nwk"]        # balanced lengths, if not another tree
    for s in (stats, py_stats, only_stats):
        assert s["bionj"] == 3 and s["bionj_device"] == 0 and s["bionj_device_s"] == 0.0
    assert stats["bme"] == plain_stats["bme"] == 3 and stats["bme_steps"] == plain_stats["bme_steps"]
    assert not any(k.startswith("bionj") for k in plain_stats)
    assert {"bionj", "bionj_device", "bionj_device_s"} <= set(scheduler.summarize(stats))
    assert not any(k.startswith("bionj") for k in scheduler.summarize(plain_stats))


@pytest.mark.parametrize("native_io", [True, False])
def test_device_branch_from_the_threshold_on_with_the_hosts_bytes(alns, tmp_path, monkeypatch, native_io):
    monkeypatch.setattr(bionj, "BIONJ_DEVICE_MIN", None)
    off_engine = Engine()
    off, off_stats = _run(alns, tmp_path / "off", off_engine, native_io, bme=True, spr=True, bionj=True)
    assert not any(off_engine.calls.values()) and off_stats["bionj_device"] == 0

    monkeypatch.setattr(bionj, "BIONJ_DEVICE_MIN", 5)                        # 3 < 5 <= 9
    engine = Engine()
    on, stats = _run(alns, tmp_path / "on", engine, native_io, bme=True, spr=True, bionj=True)
    assert on == off
    assert engine.calls == {"bionj_joins": 1, "nj_joins": 0, "bme_nni": 0, "bme_spr": 0}     # the searches stay on the host
    assert stats["bionj_device"] == 2 and stats["bionj_device_s"] > 0 and stats["bionj"] == 3

    monkeypatch.setattr(bme, "BME_DEVICE_MIN", 5)                            # the refinements of the device's table follow
    monkeypatch.setattr(bme, "SPR_DEVICE_MIN", BIG + 1)                      # each from its own minimum on
    engine = Engine()
    on, stats = _run(alns, tmp_path / "on_bme", engine, native_io, bme=True, spr=True, bionj=True)
    assert on == off
    assert engine.calls == {"bionj_joins": 1, "nj_joins": 1, "bme_nni": 2, "bme_spr": 0}      # (--bme itself: nj_joins + bme_nni)
    monkeypatch.setattr(bme, "SPR_DEVICE_MIN", 5)

    engine = Engine(flag_first=True)                                         # a flagged source keeps the host's path
    flagged, stats = _run(alns, tmp_path / "flagged", engine, native_io, bme=True, spr=True, bionj=True)
    assert flagged == off and engine.calls["bionj_joins"] == 1 and engine.calls["bme_spr"] == 2
    assert stats["bionj_device"] == 1 and stats["bionj"] == 3

    monkeypatch.setattr(bionj, "BIONJ_DEVICE_MIN", BIG + 1)
    engine = Engine()
    below, stats = _run(alns, tmp_path / "below", engine, native_io, bionj=True)
    assert all(off[k] == v for k, v in below.items()) and engine.calls["bionj_joins"] == 0 and stats["bionj_device"] == 0

    monkeypatch.setattr(bionj, "BIONJ_DEVICE_MIN", 1)                        # fewer than three sequences have no table
    engine = Engine()
    tiny, stats = _run(alns, tmp_path / "tiny", engine, native_io, batch=1, bionj=True)
    assert all(off[k] == v for k, v in tiny.items()) and engine.calls["bionj_joins"] == 3 and stats["bionj_device"] == 3


def test_the_measured_minimum_changes_no_path_without_tile():
    assert bionj.BIONJ_DEVICE_MIN is None or bionj.BIONJ_DEVICE_MIN >= 201
