"""The CLI's and the scheduler's side of ``--spr``, without a GPU: tests/test_bme_cli_host.py's stand-in engine with
``bme_spr`` = ``bme.bme_spr`` on top.  ``--spr`` needs ``-t``, is refused with ``--shard sites``, writes ``<stem>.spr.nwk``
with the same bytes natively and with ``--python-io``, leaves every other file's bytes alone - ``--bme``'s included -,
runs beside ``--bme`` and ``--tile``, counts what it did, and takes the device branch from ``SPR_DEVICE_MIN`` sequences
on - with the host's bytes, and the host's path for a flagged source."""
import os

import numpy as np
import pytest

import infer_alns
from phyloformer_amd import analyses, bme, scheduler
from test_bme_cli_host import BIG, M, SMALL, Engine as BmeEngine, alns  # noqa: F401  (alns: the fixture)

STEMS = ("big_a", "big_b", "small")


class Engine(BmeEngine):
    def __init__(self, flag_first=False):
        super().__init__(flag_first)
        self.spr_calls, self.spr_sources = 0, 0

    def bme_spr(self, preds, starts):
        self.spr_calls += 1
        self.spr_sources += len(preds)
        n = (1 + int(round((1 + 8 * preds.shape[1]) ** 0.5))) // 2
        res = [bme.bme_spr(bme.matrix_of_preds(p, n), s) for p, s in zip(preds, starts)]   # (ValueError for a bad table)
        if self.flag_first:
            t = 2 * (n - 3) + 3
            res[0] = (np.zeros(t, np.int32), np.zeros(t), 0, 0.0, bme.NONFINITE)
        return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.int32),
                np.array([r[3] for r in res]), np.array([r[4] for r in res], np.uint8))


def _run(paths, out, engine, native_io, spr=True, bme_flag=False, modes=(), batch=0):
    if native_io:
        from phyloformer_amd import build
        build.build()
    os.makedirs(out)
    runner = scheduler.DirectoryRunner(engine, str(out), trees=True, native_io=native_io, batch=batch, modes=list(modes), bme=bme_flag,
                                       spr=spr)
    stats = runner.run(paths)
    return {n: open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out))}, stats


def test_spr_needs_trees_and_is_refused_with_site_shards(tmp_path, capsys):
    with pytest.raises(SystemExit):
        infer_alns.main(["w.ckpt", str(tmp_path), "-o", str(tmp_path / "o"), "--spr"])
    assert "--spr refines the tree of --trees" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        infer_alns.main(["w.ckpt", str(tmp_path), "-o", str(tmp_path / "o"), "-t", "--spr", "--shard", "sites"])
    assert "--spr cannot be combined with --shard sites" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--spr"):
        scheduler.DirectoryRunner(Engine(), str(tmp_path), trees=False, spr=True)
    parse = infer_alns.build_parser().parse_args
    args = parse(["w.ckpt", "d", "-t", "--spr"])
    assert args.spr and args.trees and not args.bme and not parse(["w.ckpt", "d", "-t", "--bme"]).spr
    both = parse(["w.ckpt", "d", "-t", "--spr", "--bme"])
    assert both.spr and both.bme
    assert all(m.flag != "--spr" for m in analyses.MODES)


def test_native_and_python_io_write_the_same_trees_and_nothing_else_changes(alns, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setattr(bme, "SPR_DEVICE_MIN", None)
    monkeypatch.setattr(bme, "BME_DEVICE_MIN", None)
    plain, plain_stats = _run(alns, tmp_path / "plain", Engine(), True, spr=False)
    native, stats = _run(alns, tmp_path / "native", Engine(), True)
    python, py_stats = _run(alns, tmp_path / "python", Engine(), False)
    assert set(plain) == {f"{s}.{x}" for s in STEMS for x in ("phy", "nj.nwk")}
    assert set(native) == set(plain) | {f"{s}.spr.nwk" for s in STEMS}
    assert all(native[k] == v for k, v in plain.items())                     # every other file keeps its bytes
    assert native == python
    for stem, n in (("big_a", BIG), ("big_b", BIG), ("small", SMALL)):
        assert native[f"{stem}.spr.nwk"].endswith(b";\n") and native[f"{stem}.spr.nwk"].count(b",") == n - 1
    assert native["big_a.spr.nwk"] != native["big_a.nj.nwk"]                  # balanced lengths, if not another tree
    for s in (stats, py_stats):
        assert s["spr"] == 3 and s["spr_steps"] >= 0 and s["spr_device"] == 0 and s["spr_device_s"] == 0.0
    assert stats["spr_steps"] == py_stats["spr_steps"]
    assert not any(k.startswith(("spr", "bme")) for k in plain_stats) and not any(k.startswith("bme") for k in stats)
    assert {"spr", "spr_steps", "spr_device", "spr_device_s"} <= set(scheduler.summarize(stats))
    assert not any(k.startswith("spr") for k in scheduler.summarize(plain_stats))


@pytest.mark.parametrize("native_io", [True, False])
def test_beside_bme_and_tile(alns, tmp_path, monkeypatch, native_io):  # noqa: F811
    monkeypatch.setattr(bme, "SPR_DEVICE_MIN", None)
    monkeypatch.setattr(bme, "BME_DEVICE_MIN", None)
    monkeypatch.setattr(analyses, "NJ_DEVICE_MIN", None)
    base, _ = _run(alns, tmp_path / "base", Engine(), native_io)
    for name, modes, bme_flag in (("bme", [], True), ("tile", [analyses.Tile(M)], False), ("tile_bme", [analyses.Tile(M)], True)):
        without, off_stats = _run(alns, tmp_path / f"{name}_off", Engine(), native_io, spr=False, bme_flag=bme_flag, modes=modes)
        with_, stats = _run(alns, tmp_path / f"{name}_on", Engine(), native_io, bme_flag=bme_flag, modes=modes)
        assert set(with_) == set(without) | {f"{s}.spr.nwk" for s in STEMS}, name
        assert all(with_[k] == v for k, v in without.items()), name            # --bme's files among them
        assert (f"{STEMS[0]}.bme.nwk" in with_) == bme_flag
        # the whole alignment's tree only, and the same one whatever stands beside it
        assert all(with_[f"{s}.spr.nwk"] == base[f"{s}.spr.nwk"] for s in STEMS), name
        assert stats["spr"] == 3 and stats.get("bme", 0) == (3 if bme_flag else 0) and "spr" not in off_stats
    for flags in (["--leave-one-out"], ["--site-profile"], ["--bootstrap", "5"], ["--bme"]):   # the parser refuses none of them
        args = infer_alns.build_parser().parse_args(["w", "d", "-t", "--spr", *flags])
        assert len(analyses.modes_from_args(args, lambda text: pytest.fail(text))) == (0 if flags == ["--bme"] else 1) and args.spr


@pytest.mark.parametrize("native_io", [True, False])
def test_device_branch_from_the_threshold_on_with_the_hosts_bytes(alns, tmp_path, monkeypatch, native_io):  # noqa: F811
    monkeypatch.setattr(bme, "BME_DEVICE_MIN", None)
    monkeypatch.setattr(bme, "SPR_DEVICE_MIN", None)
    off_engine = Engine()
    off, off_stats = _run(alns, tmp_path / "off", off_engine, native_io)
    assert off_engine.spr_calls == 0 and off_stats["spr_device"] == 0

    monkeypatch.setattr(bme, "SPR_DEVICE_MIN", 5)                             # 3 < 5 <= 9
    engine = Engine()
    on, stats = _run(alns, tmp_path / "on", engine, native_io)
    assert on == off
    assert engine.spr_calls == 1 and engine.spr_sources == 2 and engine.nj_sources == 2 and engine.bme_calls == 0
    assert stats["spr_device"] == 2 and stats["spr_device_s"] > 0 and stats["spr"] == 3
    assert stats["spr_steps"] == off_stats["spr_steps"]

    engine = Engine(flag_first=True)                                          # a flagged source keeps the host's path
    flagged, stats = _run(alns, tmp_path / "flagged", engine, native_io)
    assert flagged == off and engine.spr_calls == 1 and stats["spr_device"] == 1 and stats["spr"] == 3

    monkeypatch.setattr(bme, "SPR_DEVICE_MIN", BIG + 1)
    engine = Engine()
    below, stats = _run(alns, tmp_path / "below", engine, native_io)
    assert below == off and engine.spr_calls == 0 and stats["spr_device"] == 0

    monkeypatch.setattr(bme, "BME_DEVICE_MIN", 5)                             # each flag has its own threshold
    engine = Engine()
    both, stats = _run(alns, tmp_path / "both", engine, native_io, bme_flag=True)
    assert engine.spr_calls == 0 and engine.bme_calls == 1 and stats["bme_device"] == 2 and stats["spr_device"] == 0
    assert all(both[k] == v for k, v in off.items())
