"""Split supports without a GPU: the statement (``supports.split_supports``) on a case worked by hand, its serial native
twin (``hostio.join_supports_host``), the labels, the refusals, and the CLI's ``--tbe`` / ``--bootstrap-refined`` through a
stand-in engine.  Every comparison is equality."""
import os
import shutil

import numpy as np
import pytest

import infer_alns
from helpers import bme_check as bc
from helpers import support_inputs as si
from phyloformer_amd import analyses, bme, bootstrap, fasta, hostio, scheduler, supports


def _native():
    from phyloformer_amd import build
    build.build()


def test_a_case_worked_by_hand():
    """N = 8.  Reference: (1,2) (3,4) (1,3) (5,6) (1,5), then 0, 1, 7 - the splits (sides without sequence 0)
    {1,2}, {3,4}, {1,2,3,4}, {5,6}, {1..6} of depth 2, 2, 4, 2, 2.  Replicate A: (1,2) (3,5) (1,3) (4,6) (1,4), then
    0, 1, 7 - the splits {1,2}, {3,5}, {1,2,3,5}, {4,6}, {1..6}.
      {1,2} and {1..6} are in A: delta 0.
      {3,4}: the closest of A are {3,5} and {4,6}, two sequences away; the cap p - 1 = 1 decides: delta 1.
      {1,2,3,4} (p = 4, cap 3): {1,2,3,5} differs in {4,5}, {1,2} in {3,4}, {1..6} in {5,6}: delta 2 - strictly between
      0 and the cap.
      {5,6}: {3,5} and {4,6} are two away, the cap decides: delta 1.
    Replicate B is passed with its flag and a table of zeros: delta = p - 1 = 1, 1, 3, 1, 1 (the cap, for p = 4 too).
    Replicate C is the reference: delta 0 everywhere.
    count = 2, 1, 1, 1, 2; transfer = 0+1+0, 1+1+0, 2+3+0, 1+1+0, 0+1+0; for {1,2,3,4} D = 3 * 3 = 9 and the transfer
    support is 1 - 5/9 = 44.4 %, Felsenstein's 1/3 = 33.3 %."""
    ref = [1, 2, 3, 4, 1, 3, 5, 6, 1, 5, 0, 1, 7]
    a = [1, 2, 3, 5, 1, 3, 4, 6, 1, 4, 0, 1, 7]
    count, transfer, depth = supports.split_supports(ref, [a, [0] * 13, ref], 8, [False, True, False])
    assert depth == [2, 2, 4, 2, 2]
    assert count == [2, 1, 1, 1, 2]
    assert transfer == [1, 2, 5, 2, 1]
    assert supports.split_supports(ref, [a], 8) == ([1, 0, 0, 0, 1], [0, 1, 2, 1, 0], depth)
    fbp, tbe = supports.labels_of(count, transfer, depth, 3)
    assert fbp == [67, 33, 33, 33, 67] and tbe == [67, 33, 44, 33, 67]
    _native()
    got = hostio.join_supports_host(ref, [a, [0] * 13, ref], [False, True, False])
    assert [x.tolist() for x in got[:3]] == [count, transfer, depth] and got[3] == 0


@pytest.mark.parametrize("n", [4, 5, 9, 64, 65, 137])
def test_the_serial_twin_equals_the_statement(n):
    _native()
    for r in (1, 5):
        ref, reps, flag = si.sources(n, r)
        got = hostio.join_supports_host(ref, reps, flag)
        assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[2].dtype == np.int32 and not got[3].any()
        for b in range(2):
            want = supports.split_supports(ref[b], reps[b], n, flag[b])
            assert [x[b].tolist() for x in got[:3]] == [list(w) for w in want], (n, r, b)
        if r == 5:
            count, transfer, depth = (x for x in got[:3])
            assert count[0].min() >= 1                          # the reference is one of source 0's replicates
            assert count[1].max() <= 4 and (transfer[1] >= depth[1] - 1).all()      # source 1's flagged replicate
            assert (depth >= 2).all() and (depth <= n // 2).all()
    # every branch of the definition is reached: partial counts, deltas at the cap and strictly inside it
    if n >= 9:
        ref, noisy = si.noisy_tables(n, 5)
        count = supports.split_supports(ref, noisy, n)[0]
        assert any(0 < c < 5 for c in count)
        deep = []
        for one in si.unrelated_tables(n, 3):                   # (one replicate: transfer is its delta)
            _c, delta, depth = supports.split_supports(ref, [one], n)
            deep += [(d, p) for d, p in zip(delta, depth) if p > 2]
        assert any(d == p - 1 for d, p in deep) and any(0 < d < p - 1 for d, p in deep)


def test_counts_reproduce_the_bootstrap_oracle_byte_for_byte(golden):
    """``bootstrap.support_newick_py`` counts with a set of Python ints and knows nothing of this module: the Felsenstein
    text from ``count`` on NJ tables - the Python twins' and the native twins' - has its bytes, on two shipped 20-tip
    distance vectors with six noisy replicates each."""
    _native()
    gold = golden("e2e_testdata.npz")
    for k, stem in enumerate(("0_20_tips", "1_20_tips")):
        pred = np.asarray(gold[f"pf/{stem}"], dtype=np.float32)
        n = 20
        assert pred.size == n * (n - 1) // 2
        ids = [f"t{i}" for i in range(n)]
        g = np.random.default_rng(k).standard_normal((6, pred.size))
        reps = (pred[None, :] * (1 + 0.15 * g)).astype(np.float32)
        want = bootstrap.support_newick_py(pred, reps, ids)
        texts = supports.support_newicks(pred, reps, ids, kinds=("nj",), tbe=True)
        assert texts["sup.nwk"] == want and texts["tbe.nwk"] != want
        slots, lengths, bad = hostio.nj_joins_host(np.concatenate([pred[None, :], reps]))
        assert not bad.any()
        res = hostio.join_supports_host(slots[0], slots[1:])
        assert supports.support_texts(slots[0], lengths[0], ids, *res[:3], 6)[0] == want
        assert want.encode() == hostio.nj_support(pred, reps, ids)
        assert 0 < sum(0 < c < 6 for c in res[0])               # (the labels are not all 0 or 100)


def test_tbe_percent_at_its_ends_and_half_way():
    assert supports.tbe_percent(0, 7, 5) == 100
    assert supports.tbe_percent(28, 7, 5) == 0                   # S = D = R (p - 1)
    assert supports.tbe_percent(1, 1, 201) == 100                # 99.5 rounds up
    assert supports.tbe_percent(3, 1, 201) == 99                 # 98.5 rounds up
    assert supports.tbe_percent(1, 4, 3) == 88                   # 87.5 rounds up
    assert supports.tbe_percent(199, 1, 201) == 1                # 0.5 rounds up
    assert supports.tbe_percent(5, 3, 4) == 44                   # 44.4 rounds down


def test_invalid_tables_and_too_few_sequences_are_refused():
    _native()
    n = 9
    ref, reps, flag = si.sources(n, 5)
    for where, k, v in (("rep", 3, n), ("rep", 0, -1), ("ref", 0, n), ("ref", 2 * (n - 3), None)):
        r, q = ref.copy(), reps.copy()
        if where == "rep":
            q[0, 1, k] = v
        else:
            r[:, k] = r[:, k + 1] if v is None else v            # (None: two equal slots at the trifurcation)
        with pytest.raises(ValueError):
            hostio.join_supports_host(r, q, flag)
        with pytest.raises(ValueError):
            supports.split_supports(r[1], q[1], n, flag[1]) if where == "ref" else supports.split_supports(r[0], q[0], n, flag[0])
    q = reps.copy()
    q[1, 4, :] = -7                                              # the flagged replicate's table is never read
    assert all(np.array_equal(x, y) for x, y in zip(hostio.join_supports_host(ref, q, flag), hostio.join_supports_host(ref, reps, flag)))
    three = np.array([[0, 1, 2]], dtype=np.int32)
    with pytest.raises(ValueError):
        hostio.join_supports_host(three, three[None])
    with pytest.raises(ValueError):
        supports.split_supports([0, 1, 2], [[0, 1, 2]], 3)
    with pytest.raises(ValueError):
        supports.split_supports(ref[0], [], n)


def test_usage_errors_of_the_two_flags(tmp_path, capsys):
    base = ["w.ckpt", str(tmp_path), "-o", str(tmp_path / "o")]
    for flags, text in ((["--tbe"], "--tbe labels the tree of --bootstrap: give --bootstrap R as well"),
                        (["-t", "--bme", "--bootstrap-refined"],
                         "--bootstrap-refined counts over the replicates of --bootstrap: give --bootstrap R as well"),
                        (["-t", "--bootstrap", "5", "--bootstrap-refined"],
                         "--bootstrap-refined supports the trees of --bme / --spr: give at least one of them as well"),
                        (["--bootstrap", "5", "--tbe", "--windows", "50"], "--windows is not supported with --bootstrap")):
        with pytest.raises(SystemExit):
            infer_alns.main(base + flags)
        assert text in capsys.readouterr().err
    parse = infer_alns.build_parser().parse_args
    mode, = analyses.modes_from_args(parse(["w", "d", "-t", "--spr", "--bootstrap", "5", "--tbe", "--bootstrap-refined"]), pytest.fail)
    assert mode.tbe and mode.refined and mode.extend is not None
    assert set(mode.stats()) == {"replicates", "bootstrap_s", "tbe", "refined_supports", "supports_device", "supports_device_s"}
    plain, = analyses.modes_from_args(parse(["w", "d", "--bootstrap", "5", "--seed", "2"]), pytest.fail)
    assert plain.extend is None and set(plain.stats()) == {"replicates", "bootstrap_s"} and not plain.tbe and not plain.refined
    assert [m.flag for m in analyses.MODES] == ["--bootstrap", "--windows", "--site-profile", "--leave-one-out", "--compress-sites",
                                                "--place", "--tile"]


class Engine:
    """A stand-in with the Engine's interface: fixed distances, one replicate with a NaN, the device searches by their
    host twins."""

    def __init__(self):
        self.calls = {"nj_joins": 0, "bme_nni": 0, "bme_spr": 0, "join_supports": 0}

    def forward(self, batch):
        return np.stack([bc.random_tree_distances(batch.shape[1], 3 + b) for b in range(len(batch))])

    def bootstrap(self, batch, replicates, seed=0):
        rng = np.random.default_rng(seed)
        base = self.forward(batch)
        out = (base[:, None, :] * (1 + 0.2 * rng.standard_normal((len(batch), replicates, base.shape[1])))).astype(np.float32)
        out[0, 2, 5] = np.nan
        return out

    def nj_joins(self, preds):
        self.calls["nj_joins"] += 1
        return hostio.nj_joins_host(preds)

    def bme_nni(self, preds, starts):
        self.calls["bme_nni"] += 1
        return hostio.bme_nni_host(preds, starts)

    def bme_spr(self, preds, starts):
        self.calls["bme_spr"] += 1
        return hostio.bme_spr_host(preds, starts)

    def join_supports(self, ref, reps, flag=None):
        self.calls["join_supports"] += 1
        return hostio.join_supports_host(ref, reps, flag)


def _run(paths, out, native_io, engine, **flags):
    os.makedirs(out)
    runner = scheduler.DirectoryRunner([engine], str(out), trees=True, native_io=native_io, modes=[analyses.Bootstrap(6, 1, **flags)],
                                       bme=True, spr=True)
    stats = runner.run(paths)
    return {n: open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out))}, stats


@pytest.mark.parametrize("native_io", [True, False])
def test_cli_writes_the_twins_texts_on_every_path(repo, tmp_path, monkeypatch, native_io):
    """Two shipped 20-tip files (one launch) under ``-t --bme --spr --bootstrap 6 --seed 1``: with ``--tbe
    --bootstrap-refined`` every earlier file keeps its bytes - ``.sup.nwk`` among them -, the five new files per
    alignment are ``supports.support_newicks`` of the Python twins, and they are the same bytes when the thresholds send
    the replicate searches and the matching through the engine."""
    _native()
    stems = ("0_20_tips", "1_20_tips")
    ind = tmp_path / "in"
    ind.mkdir()
    for stem in stems:
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    paths = [str(ind / f"{s}.fa") for s in stems]
    for name in ("BME_DEVICE_MIN", "SPR_DEVICE_MIN"):
        monkeypatch.setattr(bme, name, None)
    monkeypatch.setattr(supports, "SUPPORT_DEVICE_MIN", None)
    plain, plain_stats = _run(paths, tmp_path / "plain", native_io, Engine())
    host_engine = Engine()
    new, stats = _run(paths, tmp_path / "new", native_io, host_engine, tbe=True, refined=True)
    assert not any(host_engine.calls.values())
    added = ("tbe.nwk", "bme.sup.nwk", "bme.tbe.nwk", "spr.sup.nwk", "spr.tbe.nwk")
    assert sorted(new) == sorted(list(plain) + [f"{s}.{x}" for s in stems for x in added])
    assert all(new[k] == v for k, v in plain.items())
    assert (stats["tbe"], stats["refined_supports"], stats["supports_device"], stats["supports_device_s"]) == (6, 4, 0, 0.0)
    assert not {"tbe", "refined_supports", "supports_device", "supports_device_s"} & set(plain_stats)
    assert {"tbe", "refined_supports", "supports_device", "supports_device_s"} <= set(scheduler.summarize(stats))
    assert "tbe" not in scheduler.summarize(plain_stats)
    batch = np.stack([fasta.load_alignment(p)[0] for p in paths])
    preds, reps = Engine().forward(batch), Engine().bootstrap(batch, 6, 1)
    for b, stem in enumerate(stems):
        ids = fasta.load_alignment(paths[b])[1]
        want = supports.support_newicks(preds[b], reps[b], ids, kinds=("nj", "bme", "spr"), tbe=True)
        for suffix, text in want.items():
            assert new[f"{stem}.{suffix}"] == text.encode(), (stem, suffix)
    only_tbe, _ = _run(paths, tmp_path / "tbe", native_io, Engine(), tbe=True)
    assert sorted(only_tbe) == sorted(list(plain) + [f"{s}.tbe.nwk" for s in stems])
    assert all(new[k] == v for k, v in only_tbe.items())
    # the device branches, each alone and all together: the same bytes
    for lowered in (("BME_DEVICE_MIN",), ("SPR_DEVICE_MIN",), ("SUPPORT_DEVICE_MIN",), ("BME_DEVICE_MIN", "SPR_DEVICE_MIN", "SUPPORT_DEVICE_MIN")):
        for name in ("BME_DEVICE_MIN", "SPR_DEVICE_MIN"):
            monkeypatch.setattr(bme, name, 4 if name in lowered else None)
        monkeypatch.setattr(supports, "SUPPORT_DEVICE_MIN", 4 if "SUPPORT_DEVICE_MIN" in lowered else None)
        engine = Engine()
        got, dev_stats = _run(paths, tmp_path / "_".join(lowered), native_io, engine, tbe=True, refined=True)
        assert got == new, lowered
        match = "SUPPORT_DEVICE_MIN" in lowered
        kinds = 1 + ("BME_DEVICE_MIN" in lowered) + ("SPR_DEVICE_MIN" in lowered)
        assert engine.calls["join_supports"] == (kinds if match else 0) and dev_stats["supports_device"] == (2 * kinds if match else 0)
        # (one call for the file's own tree, by the runner, and one for all the launch's trees, by the mode)
        assert engine.calls["bme_nni"] == (2 if "BME_DEVICE_MIN" in lowered else 0)
        assert engine.calls["bme_spr"] == (2 if "SPR_DEVICE_MIN" in lowered else 0)
