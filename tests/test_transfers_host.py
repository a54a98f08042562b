"""Per-taxon transfer counts without a GPU: the statement (``supports.transfer_taxa``) on a case worked by hand, its serial
native twin (``hostio.join_transfers_host``), the identity that ties the counts to the transfer sums, a planted rogue
taxon, the label, the refusals, and the CLI's ``--instability`` through a stand-in engine.  Every comparison is
equality."""
import os
import shutil

import numpy as np
import pytest

import infer_alns
from helpers import bme_check as bc
from helpers import support_inputs as si
from helpers import transfer_inputs as ti
from phyloformer_amd import analyses, bme, hostio, scheduler, supports


def _native():
    from phyloformer_amd import build
    build.build()


def test_a_case_worked_by_hand():
    """N = 6.  Reference: (1,2) (1,3) (4,5), then 0, 1, 4 - the splits s0 = {1,2}, s1 = {1,2,3}, s2 = {4,5} of depth
    2, 3, 2, so p - 1 = 1, 2, 1.
    Replicate A: (1,3) (1,2) (4,5), then 0, 1, 4 - q0 = {1,3}, q1 = {1,2,3}, q2 = {4,5}.
      s0: h = 2, 1, 4, so m = 2, 1, 2: j* = 1, and m = 1 = p - 1 - the internal split is preferred to the leaf edges:
          not capped, delta 1, X = {1,2} xor {1,2,3} = {3}.
      s1 = q1 and s2 = q2: delta 0, X empty.
    Replicate B: (2,3) (4,5) (2,4), then 0, 1, 2 - q0 = {2,3}, q1 = {4,5}, q2 = {2,3,4,5}.
      s0: h = 2, 4, 4, so m = 2, 2, 2 > p - 1: capped, delta 1.
      s1: h = 1, 5, 3: m = 1 (side 0), 1 (side 1), 3 (h = N - h: side 0).  q0 and q1 are equally close and the lower j
          wins: j* = 0, X = {1,2,3} xor {2,3} = {1}, delta 1 <= p - 1 = 2.  (Had q1 won, X would be the complement of
          {1,2,3,4,5} = {0}.)
      s2 = q1: delta 0.
    count = 0, 1, 2; transfer = 2, 1, 0.  At cutoff 100 every pair is used: used = 2, 2, 2; capped = 1, 0, 0;
    branch_moves = {3: 1}, {1: 1}, {}; moves = 1 for sequences 1 and 3.  At cutoff 50, (s0, A) and (s0, B) have
    100 * 1 > 50 * 1 and are not used, (s1, B) has 100 * 1 <= 50 * 2 and is.  At 30 and 0 only the delta = 0 pairs are."""
    n = 6
    ref = [1, 2, 1, 3, 4, 5, 0, 1, 4]
    a = [1, 3, 1, 2, 4, 5, 0, 1, 4]
    b = [2, 3, 4, 5, 2, 4, 0, 1, 2]
    same = {"count": [0, 1, 2], "transfer": [2, 1, 0], "depth": [2, 3, 2]}
    want = {100: dict(same, used=[2, 2, 2], capped=[1, 0, 0], moves=[0, 1, 0, 1, 0, 0],
                      branch_moves=[[0, 0, 0, 1, 0, 0], [0, 1, 0, 0, 0, 0], [0] * 6]),
            50: dict(same, used=[0, 2, 2], capped=[0, 0, 0], moves=[0, 1, 0, 0, 0, 0],
                     branch_moves=[[0] * 6, [0, 1, 0, 0, 0, 0], [0] * 6]),
            30: dict(same, used=[0, 1, 2], capped=[0, 0, 0], moves=[0] * 6, branch_moves=[[0] * 6] * 3)}
    want[0] = want[30]
    assert supports.split_supports(ref, [a, b], n) == (same["count"], same["transfer"], same["depth"])
    _native()
    for cutoff, w in want.items():
        assert supports.transfer_taxa(ref, [a, b], n, cutoff=cutoff) == w, cutoff
        assert ti.as_lists(hostio.join_transfers_host(ref, [a, b], None, cutoff)) == dict(w, status=0), cutoff
    # the same replicate passed with its flag: capped wherever it stood
    flagged = supports.transfer_taxa(ref, [a, b], n, [True, False], 100)
    assert flagged["capped"] == [2, 1, 1] and flagged["moves"] == [0, 1, 0, 0, 0, 0] and flagged["transfer"] == [2, 3, 1]


@pytest.mark.parametrize("n", [4, 5, 8, 63, 64, 65, 129, 137])
def test_the_serial_twin_equals_the_statement(n):
    """Two unrelated random trees, the reference itself, a flagged replicate and a noisy copy of the reference, at the
    cutoffs 0, 30 and 100; ``count``, ``transfer`` and ``depth`` are ``join_supports_host``'s arrays."""
    _native()
    ref, reps, flag = ti.mixed(n)
    plain = hostio.join_supports_host(ref, reps, flag)
    for cutoff in ti.CUTOFFS:
        want = supports.transfer_taxa(ref, reps, n, flag, cutoff)
        got = hostio.join_transfers_host(ref, reps, flag, cutoff)
        assert [x.dtype for x in got] == [np.int32, np.int64, np.int32, np.int64, np.int32, np.int32, np.int32, np.uint8]
        assert got[6].shape == (n - 3, n)
        assert ti.as_lists(got) == dict(want, status=0), (n, cutoff)
        for g, p in zip(got[:3], plain[:3]):
            assert g.dtype == p.dtype and np.array_equal(g, p)
        without = hostio.join_transfers_host(ref, reps, flag, cutoff, branch_moves=False)
        assert without[6] is None
        ti.assert_same(without[:6] + without[7:], got[:6] + got[7:])
        if cutoff == 100:                                       # the identity: every transfer is attributed or capped
            assert want["used"] == [5] * (n - 3)
            for t in range(n - 3):
                assert sum(want["branch_moves"][t]) + (want["depth"][t] - 1) * want["capped"][t] == want["transfer"][t]
            assert min(want["capped"]) >= 1                     # (the flagged replicate)
        # the reference among its own replicates is used at any cutoff and moves nothing
        alone = supports.transfer_taxa(ref, [ref], n, None, cutoff)
        assert alone["used"] == [1] * (n - 3) and not any(alone["moves"]) and not any(alone["capped"])
        assert min(want["used"]) >= 1
    # sources side by side are the sources one by one
    ref2, reps2, flag2 = si.sources(n, 5)
    both = hostio.join_transfers_host(ref2, reps2, flag2, 30)
    for b in range(2):
        assert ti.as_lists([x[b] for x in both]) == dict(ti.statement(n, 5, b, 30), status=0)


def test_every_branch_of_the_definition_is_reached():
    """On ordinary inputs: ties between equally close splits, both sides, capped and uncapped pairs, pairs beyond the
    cutoff."""
    n = 65
    ref, reps, flag = ti.mixed(n)
    splits = supports.table_splits(ref, n)
    ties = sides = 0
    for rep in (reps[0], reps[4]):
        qs = supports.table_splits(rep, n)
        for s in splits:
            ms = [min(bin(s ^ q).count("1"), n - bin(s ^ q).count("1")) for q in qs]
            ties += ms.count(min(ms)) > 1
            j = ms.index(min(ms))
            sides += 2 * bin(s ^ qs[j]).count("1") > n
    assert ties > 0 and sides > 0
    full, some = supports.transfer_taxa(ref, reps, n, flag, 100), supports.transfer_taxa(ref, reps, n, flag, 30)
    assert any(0 < c < 5 for c in full["capped"]) and any(full["moves"])
    assert any(u < 5 for u in some["used"]) and sum(some["moves"]) < sum(full["moves"])


@pytest.mark.parametrize("n", [8, 20, 65, 130])
def test_a_planted_rogue_taxon_has_the_most_moves(n):
    """One random tree on ``n - 1`` sequences; the last sequence is regrafted on a random edge in the reference and in
    each of ten replicates: it has strictly more moves than any other sequence."""
    _native()
    ref, reps = ti.planted_rogue(n)
    moves = hostio.join_transfers_host(ref, reps)[3]
    assert moves.tolist() == supports.transfer_taxa(ref, reps, n)["moves"]
    assert moves[n - 1] > moves[:n - 1].max(), moves.tolist()


def test_instability_permille():
    assert supports.instability_permille(0, 7) == 0
    assert supports.instability_permille(7, 7) == 1000
    assert supports.instability_permille(1, 2000) == 1          # 0.5 rounds up
    assert supports.instability_permille(1, 2001) == 0
    assert supports.instability_permille(1, 3) == 333
    assert supports.instability_permille(2, 3) == 667
    assert supports.instability_permille(5, 0) == 0             # no pair used
    assert supports.instability_permille(3, 2) == 1500          # a sequence may move for several branches of a replicate


def test_refusals():
    _native()
    n = 9
    ref, reps, flag = si.sources(n, 5)
    for cutoff in (-1, 101):
        with pytest.raises(ValueError):
            hostio.join_transfers_host(ref, reps, flag, cutoff)
        with pytest.raises(ValueError):
            supports.transfer_taxa(ref[0], reps[0], n, flag[0], cutoff)
    for where, k, v in (("rep", 3, n), ("rep", 0, -1), ("ref", 0, n)):
        r, q = ref.copy(), reps.copy()
        if where == "rep":
            q[0, 1, k] = v
        else:
            r[:, k] = v
        with pytest.raises(ValueError):
            hostio.join_transfers_host(r, q, flag)
        with pytest.raises(ValueError):
            supports.transfer_taxa(r[0], q[0], n, flag[0])
    q = reps.copy()
    q[1, 4, :] = -7                                              # the flagged replicate's table is never read
    ti.assert_same(hostio.join_transfers_host(ref, q, flag), hostio.join_transfers_host(ref, reps, flag))
    three = np.array([[0, 1, 2]], dtype=np.int32)
    with pytest.raises(ValueError):
        hostio.join_transfers_host(three, three[None])
    with pytest.raises(ValueError):
        supports.transfer_taxa([0, 1, 2], [[0, 1, 2]], 3)
    with pytest.raises(ValueError):
        supports.transfer_taxa(ref[0], [], n)


def test_usage_errors_of_the_flag(tmp_path, capsys):
    base = ["w.ckpt", str(tmp_path), "-o", str(tmp_path / "o")]
    for flags, text in ((["--instability"], "--instability counts over the replicates of --bootstrap: give --bootstrap R as well"),
                        (["--bootstrap", "5", "--instability", "101"], "--instability takes a cutoff of 0 to 100 percent (got 101)"),
                        (["--bootstrap", "5", "--instability", "-1"], "--instability takes a cutoff of 0 to 100 percent (got -1)"),
                        (["--bootstrap", "5", "--instability", "--windows", "50"], "--windows is not supported with --bootstrap")):
        with pytest.raises(SystemExit):
            infer_alns.main(base + flags)
        assert text in capsys.readouterr().err
    parse = infer_alns.build_parser().parse_args
    mode, = analyses.modes_from_args(parse(["w", "d", "--bootstrap", "5", "--instability"]), pytest.fail)
    assert mode.instability == 30 and mode.extend is not None and not mode.tbe
    assert set(mode.stats()) == {"replicates", "bootstrap_s", "tbe", "refined_supports", "supports_device", "supports_device_s",
                                 "instability", "transfers_device"}
    mode, = analyses.modes_from_args(parse(["w", "d", "--bootstrap", "5", "--instability", "0"]), pytest.fail)
    assert mode.instability == 0
    plain, = analyses.modes_from_args(parse(["w", "d", "--bootstrap", "5", "--tbe"]), pytest.fail)
    assert plain.instability is None and not {"instability", "transfers_device"} & set(plain.stats())
    assert [m.flag for m in analyses.MODES] == ["--bootstrap", "--windows", "--site-profile", "--leave-one-out", "--compress-sites",
                                                "--place", "--tile"]
    assert supports.TRANSFER_DEVICE_MIN is None or supports.TRANSFER_DEVICE_MIN >= 4


class Engine:
    """A stand-in with the Engine's interface: fixed distances, one replicate with a NaN, the device searches by their
    host twins."""

    def __init__(self):
        self.calls = {"nj_joins": 0, "bme_nni": 0, "bme_spr": 0, "join_supports": 0, "join_transfers": 0}

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

    def join_transfers(self, ref, reps, flag=None, cutoff=100, branch_moves=True):
        self.calls["join_transfers"] += 1
        return hostio.join_transfers_host(ref, reps, flag, cutoff, branch_moves)


def _run(paths, out, native_io, engine, **flags):
    os.makedirs(out)
    runner = scheduler.DirectoryRunner([engine], str(out), trees=True, native_io=native_io, modes=[analyses.Bootstrap(6, 1, **flags)],
                                       bme=True, spr=True)
    stats = runner.run(paths)
    return {n: open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out))}, stats


@pytest.mark.parametrize("native_io", [True, False])
def test_cli_writes_the_statements_files_on_every_path(repo, tmp_path, monkeypatch, native_io):
    """Two shipped 20-tip files (one launch) under ``-t --bme --spr --bootstrap 6 --seed 1 --tbe --bootstrap-refined``:
    with ``--instability 40`` every earlier file keeps its bytes - ``.sup.nwk`` and ``.tbe.nwk`` among them -, the nine
    new files per alignment are ``supports.instability_texts`` of the statement on the Python twins' tables, and they are
    the same bytes when the threshold sends the counting through the engine: one ``join_transfers`` call per kind of tree
    and no ``join_supports`` call."""
    _native()
    stems = ("0_20_tips", "1_20_tips")
    ind = tmp_path / "in"
    ind.mkdir()
    for stem in stems:
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    paths = [str(ind / f"{s}.fa") for s in stems]
    for name in ("BME_DEVICE_MIN", "SPR_DEVICE_MIN"):
        monkeypatch.setattr(bme, name, None)
    monkeypatch.setattr(supports, "SUPPORT_DEVICE_MIN", 4)
    monkeypatch.setattr(supports, "TRANSFER_DEVICE_MIN", None)
    before_engine = Engine()
    before, before_stats = _run(paths, tmp_path / "before", native_io, before_engine, tbe=True, refined=True)
    assert before_engine.calls["join_supports"] == 1 and before_engine.calls["join_transfers"] == 0
    assert not {"instability", "transfers_device"} & set(before_stats)
    host_engine = Engine()
    new, stats = _run(paths, tmp_path / "new", native_io, host_engine, tbe=True, refined=True, instability=40)
    # (below its own threshold the flag keeps the matching off the device altogether: it would run twice)
    assert host_engine.calls["join_supports"] == 0 and host_engine.calls["join_transfers"] == 0
    kinds = ("nj", "bme", "spr")
    added = [x for k in kinds for x in supports.INSTABILITY_SUFFIXES[k]]
    assert added[:3] == ["instability.tsv", "branches.tsv", "branches.nwk"] and added[3] == "bme.instability.tsv"
    assert sorted(new) == sorted(list(before) + [f"{s}.{x}" for s in stems for x in added])
    assert all(new[k] == v for k, v in before.items())
    assert (stats["instability"], stats["transfers_device"]) == (6, 0)
    assert {"instability", "transfers_device"} <= set(scheduler.summarize(stats)) and "instability" not in scheduler.summarize(before_stats)
    batch = np.stack([fasta_idx(p) for p in paths])
    preds, reps = Engine().forward(batch), Engine().bootstrap(batch, 6, 1)
    for b, stem in enumerate(stems):
        ids = fasta_ids(paths[b])
        for kind in kinds:
            slots, lengths, rep_slots, rep_flag = supports.kind_tables(preds[b], reps[b], 20, kind)
            res = supports.transfer_tuple(supports.transfer_taxa(slots, rep_slots, 20, rep_flag, 40))
            want = supports.instability_texts(slots, lengths, ids, res, 6)
            for suffix, text in zip(supports.INSTABILITY_SUFFIXES[kind], want):
                assert new[f"{stem}.{suffix}"] == text.encode(), (stem, suffix)
            lines = want[0].splitlines()
            assert lines[0] == "id\tmoves\tpermille" and [l.split("\t")[0] for l in lines[1:]] == list(ids)
            assert len(want[1].splitlines()) == 1 + 17 and want[2].count(")") == 18
        assert b != 0 or rep_flag[2]                             # (the replicate with the NaN is flagged)
    assert any(int(l.split("\t")[1]) > 0 for l in new["0_20_tips.instability.tsv"].decode().splitlines()[1:])
    # the device path: the same bytes
    monkeypatch.setattr(supports, "TRANSFER_DEVICE_MIN", 4)
    engine = Engine()
    got, dev_stats = _run(paths, tmp_path / "device", native_io, engine, tbe=True, refined=True, instability=40)
    assert got == new
    assert engine.calls["join_transfers"] == 1 and engine.calls["join_supports"] == 0
    assert (dev_stats["instability"], dev_stats["transfers_device"], dev_stats["supports_device"]) == (6, 2, 2)
    for name in ("BME_DEVICE_MIN", "SPR_DEVICE_MIN"):
        monkeypatch.setattr(bme, name, 4)
    engine = Engine()
    got, dev_stats = _run(paths, tmp_path / "all", native_io, engine, tbe=True, refined=True, instability=40)
    assert got == new
    assert engine.calls["join_transfers"] == 3 and engine.calls["join_supports"] == 0 and dev_stats["transfers_device"] == 6
    # the flag alone: the NJ tree's three files and .sup.nwk
    only, _ = _run(paths, tmp_path / "only", native_io, Engine(), instability=40)
    assert sorted(set(only) - set(before)) == sorted(f"{s}.{x}" for s in stems for x in added[:3])
    assert all(new[k] == v for k, v in only.items())


def fasta_idx(path):
    from phyloformer_amd import fasta
    return fasta.load_alignment(path)[0]


def fasta_ids(path):
    from phyloformer_amd import fasta
    return fasta.load_alignment(path)[1]
