"""Majority-rule consensus trees without a GPU: the statement (``consensus.join_consensus``) on a case worked by hand and
on its own invariants, its serial native twin (``hostio.join_consensus_host``: integers equal, doubles bit-equal), the
text, the refusals, and the CLI's ``--consensus`` through a stand-in engine."""
import os
import shutil

import numpy as np
import pytest

import infer_alns
from helpers import bme_check as bc
from helpers import support_inputs as si
from phyloformer_amd import analyses, bme, consensus, fasta, hostio, scheduler, supports

GRID_N, GRID_R = (4, 5, 9, 64, 65, 137, 300), (1, 5, 6)


def _native():
    from phyloformer_amd import build
    build.build()


def table(joins, final):
    return [x for j in joins for x in j] + list(final)


WORKED = [table([(1, 2), (3, 4), (1, 3)], (0, 1, 5)), table([(1, 2), (3, 4), (3, 5)], (0, 1, 3)),
          table([(1, 2), (4, 5), (3, 4)], (0, 1, 3)), table([(0, 5), (1, 2), (3, 4)], (0, 1, 3))]
WORKED_LENGTHS = [[r + 1.0] * 9 for r in range(4)]


def lengths_of(shape, seed):
    """Seeded branch lengths, negative ones among them."""
    return np.random.default_rng(seed).standard_normal(shape)


def assert_same(got, want, what=""):
    """A twin's arrays of one source against the statement's ``Consensus``: integers equal, doubles bit for bit."""
    assert int(got[0]) == want.n_splits and int(got[7]) == want.status, what
    for k in (1, 2, 3, 5):
        assert got[k].dtype == np.int32 and got[k].tolist() == list(want[k]), (what, k)
    for k in (4, 6):
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].dtype == np.float64 and got[k].tobytes() == np.asarray(want[k], dtype=np.float64).tobytes(), (what, k)


def test_a_case_worked_by_hand():
    """N = 6, R = 4, every length of replicate r equal to r + 1.  Counts: {1,2}: 4, {3,4}: 3, {1,2,3,4}: 2 (replicate 3's
    {0,5} normalises to it), {3,4,5}: 2, {4,5}: 1."""
    got = consensus.join_consensus(WORKED, 6, WORKED_LENGTHS)
    assert got.n_splits == 2 and got.status == 0
    assert got.count == [4, 3, 0] and got.size == [2, 2, 0] and got.parent == [-1, -1, 0]
    assert got.leaf_parent == [-1, 0, 0, 1, 1, -1]
    assert got.split_length == [2.5, 7 / 3, 0.0] and got.leaf_length == [2.5] * 6
    assert consensus.newick_of_consensus("abcdef", got, 4) == "(a:2.5,(b:2.5,c:2.5)100:2.5,(d:2.5,e:2.5)75:2.3333333333333335,f:2.5);\n"
    assert consensus.newick_of_consensus("abcdef", consensus.join_consensus(WORKED, 6), 4) == "(a,(b,c)100,(d,e)75,f);\n"
    high = consensus.join_consensus(WORKED, 6, WORKED_LENGTHS, percent=75)
    assert high.n_splits == 1 and high.count == [4, 0, 0] and high.leaf_parent == [-1, 0, 0, -1, -1, -1]
    assert consensus.newick_of_consensus("abcdef", high, 4) == "(a:2.5,(b:2.5,c:2.5)100:2.5,d:2.5,e:2.5,f:2.5);\n"
    # a negative mean is clamped at writing, not before
    neg = consensus.join_consensus(WORKED, 6, [[-1.0] * 9] * 4)
    assert neg.split_length[:2] == [-1.0, -1.0]
    assert consensus.newick_of_consensus("abcdef", neg, 4) == "(a:0.0,(b:0.0,c:0.0)100:0.0,(d:0.0,e:0.0)75:0.0,f:0.0);\n"
    assert consensus.newick_of_consensus("abcdef", neg, 4, clamp_negative=False).startswith("(a:-1.0,(b:-1.0,")
    assert consensus.newick_of_consensus("abc", consensus.star(3), 4) == "(a,b,c);\n"
    _native()
    for percent, want in ((50, got), (75, high)):
        assert_same(hostio.join_consensus_host(WORKED, WORKED_LENGTHS, None, percent), want, percent)
    assert_same(hostio.join_consensus_host(WORKED), consensus.join_consensus(WORKED, 6))


@pytest.mark.parametrize("n", GRID_N)
def test_the_statements_invariants_and_the_serial_twin(n):
    """Selected counts over the threshold, pairwise compatible, ``M <= N - 3``; the inputs cover partial resolution, the
    excluded tie and the star; the twin equals the statement, with and without lengths, at two thresholds."""
    _native()
    for r in GRID_R:
        _ref, reps, flag = si.sources(n, r)
        lengths = lengths_of(reps.shape, 10 * n + r)
        assert (lengths < 0).any()
        got = hostio.join_consensus_host(reps, lengths, flag)
        bare = hostio.join_consensus_host(reps, None, flag, 70)
        for b in range(2):
            want = consensus.join_consensus(reps[b], n, lengths[b], flag[b])
            assert_same([x[b] for x in got], want, (n, r, b))
            assert_same([None if x is None else x[b] for x in bare], consensus.join_consensus(reps[b], n, None, flag[b], 70), (n, r, b))
            m = want.n_splits
            assert m <= n - 3 and all(2 * c > r for c in want.count[:m]) and not any(want.count[m:])
            trees = [None if f else supports.table_splits(s, n) for s, f in zip(reps[b], flag[b])]
            tally = {}
            for s in (s for splits in trees if splits for s in splits):
                tally[s] = tally.get(s, 0) + 1
            chosen = sorted((s for s, c in tally.items() if 2 * c > r), key=lambda s: (bin(s).count("1"), (s & -s).bit_length()))
            assert len(chosen) == m and [tally[s] for s in chosen] == want.count[:m]
            assert all(a & c in (0, a, c) for a in chosen for c in chosen)
            assert [bin(s).count("1") for s in chosen] == want.size[:m]
            for i in range(m):
                p = want.parent[i]
                assert p == -1 or (p > i and chosen[p] & chosen[i] == chosen[i])
            assert want.leaf_parent[0] == -1
        m0, m1 = int(got[0][0]), int(got[0][1])
        if n >= 64 and r == 5:
            assert 0 < m0 < n - 3                               # source 0, noisy replicates: partial resolution
        if n >= 64 and r == 6:
            assert got[1][0][:m0].min() == 4                    # a split in exactly half (3 of 6) is not selected
        if r >= 5:
            assert m1 == 0 and (got[5][1] == -1).all()          # source 1, unrelated replicates: the star


def test_partial_resolution_is_what_it_was_measured_to_be():
    got = {n: consensus.join_consensus(si.sources(n, 5)[1][0], n).n_splits for n in (64, 65, 137, 300)}
    assert got == {64: 56, 65: 59, 137: 132, 300: 290}


def test_identical_replicates_give_their_own_tree():
    _native()
    n, r = 65, 7
    ref, _noisy = si.noisy_tables(n, 5)
    reps = np.stack([ref] * r)
    lengths = np.stack([np.arange(2 * (n - 3) + 3, dtype=np.float64) + 1.0] * r)
    got = hostio.join_consensus_host(reps, lengths)
    assert_same(got, consensus.join_consensus(reps, n, lengths))
    assert got[0] == n - 3 and (got[1] == r).all()
    ids = [f"t{i}" for i in range(n)]
    from phyloformer_amd import treecmp
    own = supports.support_texts(ref, lengths[0], ids, [r] * (n - 3), [0] * (n - 3), [2] * (n - 3), r)[0]
    text = consensus.newick_of_consensus(ids, got, r)
    a, b = treecmp.parse_newick(text), treecmp.parse_newick(own)
    assert treecmp.robinson_foulds(a, b)[0] == 0 and treecmp.branch_score(a, b) == 0.0
    # every branch keeps its length: the mean of r equal numbers
    assert sorted(got[4].tolist() + got[6].tolist()) == sorted(lengths[0].tolist())


def test_a_table_that_is_none_gives_status_one_and_zeros():
    _native()
    n = 9
    _ref, reps, flag = si.sources(n, 5)
    lengths = lengths_of(reps.shape, 3)
    for k, v in ((3, n), (0, -1), (2 * (n - 3), None), (4, 1 << 30)):
        q = reps.copy()
        q[0, 1, k] = q[0, 1, k + 1] if v is None else v         # (None: two equal slots at the trifurcation)
        got = hostio.join_consensus_host(q, lengths, flag)
        assert got[7].tolist() == [1, 0]
        assert not any(np.asarray(x[0]).any() for x in got[:7])
        assert_same([x[0] for x in got], consensus.join_consensus(q[0], n, lengths[0], flag[0]))
        assert_same([x[1] for x in got], consensus.join_consensus(q[1], n, lengths[1], flag[1]))
    q = reps.copy()
    q[1, 4, :] = -7                                              # the flagged replicate's table is never read
    assert all(np.array_equal(x, y) for x, y in zip(hostio.join_consensus_host(q, lengths, flag), hostio.join_consensus_host(reps, lengths, flag)))
    every = np.ones((1, 5), dtype=bool)                          # no replicate with a tree: the star, lengths 0.0
    got = hostio.join_consensus_host(q[1:], lengths[1:], every)
    assert_same([x[0] for x in got], consensus.join_consensus(q[1], n, lengths[1], every[0]))
    assert got[0][0] == 0 and not got[6].any()
    assert consensus.newick_of_consensus("abcdefghi", [x[0] for x in got], 5) == "(" + ",".join(f"{c}:0.0" for c in "abcdefghi") + ");\n"


def test_refusals():
    _native()
    n = 9
    _ref, reps, flag = si.sources(n, 5)
    for percent in (49, 100, 0, -3):
        with pytest.raises(ValueError):
            hostio.join_consensus_host(reps, None, flag, percent)
        with pytest.raises(ValueError):
            consensus.join_consensus(reps[0], n, None, flag[0], percent)
    three = np.array([[[0, 1, 2]]], dtype=np.int32)
    with pytest.raises(ValueError):
        hostio.join_consensus_host(three)
    with pytest.raises(ValueError):
        consensus.join_consensus([[0, 1, 2]], 3)
    with pytest.raises(ValueError):
        consensus.join_consensus([], n)
    with pytest.raises(ValueError):
        hostio.join_consensus_host(reps[:, :0])


def test_usage_errors_and_the_interface(tmp_path, capsys):
    from phyloformer_amd import build, engine
    base = ["w.ckpt", str(tmp_path), "-o", str(tmp_path / "o")]
    for flags, text in ((["--consensus"], "--consensus is the consensus of the replicate trees of --bootstrap: give --bootstrap R as well"),
                        (["--bootstrap", "5", "--consensus", "49"], "--consensus takes a threshold of 50 to 99 percent (got 49)"),
                        (["--bootstrap", "5", "--consensus", "100"], "--consensus takes a threshold of 50 to 99 percent (got 100)"),
                        (["--bootstrap", "5", "--consensus", "--windows", "50"], "--windows is not supported with --bootstrap")):
        with pytest.raises(SystemExit):
            infer_alns.main(base + flags)
        assert text in capsys.readouterr().err
    parse = infer_alns.build_parser().parse_args
    mode, = analyses.modes_from_args(parse(["w", "d", "--bootstrap", "5", "--consensus"]), pytest.fail)
    assert mode.consensus == 50 and mode.extend is not None and {"consensus", "consensus_device"} <= set(mode.stats())
    mode, = analyses.modes_from_args(parse(["w", "d", "--bootstrap", "5", "--consensus", "80"]), pytest.fail)
    assert mode.consensus == 80
    plain, = analyses.modes_from_args(parse(["w", "d", "--bootstrap", "5"]), pytest.fail)
    assert plain.consensus is None and plain.extend is None and set(plain.stats()) == {"replicates", "bootstrap_s"}
    names = ("pf_join_consensus", "pf_join_consensus_device", "pf_join_consensus_host")
    assert set(names) <= set(engine.SIGNATURES) and set(names) <= engine.CALL_TIME_SYMBOLS and engine.ABI_VERSION == 5
    new = {"pf_consensus.hip.h", "pf_consensus_host.h"}
    assert new <= set(build.HEADERS) and not new & set(build.KERNEL_FILES)           # the kernel hash does not move
    assert consensus.CONSENSUS_DEVICE_MIN is None or consensus.CONSENSUS_DEVICE_MIN >= 4


class Engine:
    """A stand-in with the Engine's interface: fixed distances, one replicate with a NaN, the device calls by their host
    twins."""

    def __init__(self):
        self.calls = {"nj_joins": 0, "bme_nni": 0, "bme_spr": 0, "join_supports": 0, "join_consensus": 0}

    def forward(self, batch):
        return np.stack([bc.random_tree_distances(batch.shape[1], 3 + b) for b in range(len(batch))])

    def bootstrap(self, batch, replicates, seed=0):
        rng = np.random.default_rng(seed)
        base = self.forward(batch)
        out = (base[:, None, :] * (1 + 0.2 * rng.standard_normal((len(batch), replicates, base.shape[1])))).astype(np.float32)
        out[0, 2, min(5, base.shape[1] - 1)] = np.nan
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

    def join_consensus(self, reps, lengths=None, flag=None, percent=50):
        self.calls["join_consensus"] += 1
        return hostio.join_consensus_host(reps, lengths, flag, percent)


def _run(paths, out, native_io, engine, **flags):
    os.makedirs(out)
    runner = scheduler.DirectoryRunner([engine], str(out), trees=True, native_io=native_io, modes=[analyses.Bootstrap(6, 1, **flags)],
                                       bme=True, spr=True)
    stats = runner.run(paths)
    return {n: open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out))}, stats


def _want(pred, reps, ids, kind, percent):
    """``<stem>[.<kind>].con.nwk`` by the Python twins alone."""
    n = len(ids)
    _s, _l, rep_slots, rep_flag, rep_lengths = supports.kind_tables(pred, reps, n, kind, with_lengths=True)
    return consensus.newick_of_consensus(ids, consensus.join_consensus(rep_slots, n, rep_lengths, rep_flag, percent), len(reps)).encode()


@pytest.mark.parametrize("native_io", [True, False])
def test_cli_writes_the_statements_text_on_every_path(repo, tmp_path, monkeypatch, native_io):
    """Two shipped 20-tip files under ``-t --bme --spr --bootstrap 6 --seed 1``: a run without ``--consensus`` keeps
    every byte and every stat of the parent's code path (the mode constructed as the parent constructs it); with
    ``--consensus`` every earlier file keeps its bytes and ``<stem>.con.nwk`` is the statement's text on the Python twins'
    tables; with ``--bootstrap-refined`` ``.bme.con.nwk`` / ``.spr.con.nwk`` too; the same bytes when the thresholds send
    the work through the engine."""
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
    monkeypatch.setattr(consensus, "CONSENSUS_DEVICE_MIN", None)
    plain, plain_stats = _run(paths, tmp_path / "plain", native_io, Engine())
    assert sorted(plain) == sorted(f"{s}.{x}" for s in stems for x in ("phy", "nj.nwk", "sup.nwk", "bme.nwk", "spr.nwk"))
    assert not {"consensus", "consensus_device", "tbe"} & set(plain_stats) and "consensus" not in scheduler.summarize(plain_stats)
    batch = np.stack([fasta.load_alignment(p)[0] for p in paths])
    preds, reps = Engine().forward(batch), Engine().bootstrap(batch, 6, 1)
    ids = [fasta.load_alignment(p)[1] for p in paths]
    # the parent's bytes of <stem>.sup.nwk, from the writer the parent's plain mode uses
    for b, stem in enumerate(stems):
        want = hostio.nj_support(preds[b], reps[b], ids[b]) if native_io else supports.support_newicks(preds[b], reps[b], ids[b], tbe=False)["sup.nwk"].encode()
        assert plain[f"{stem}.sup.nwk"] == want

    host_engine = Engine()
    con, stats = _run(paths, tmp_path / "con", native_io, host_engine, consensus=50)
    assert not any(host_engine.calls.values())
    assert sorted(con) == sorted(list(plain) + [f"{s}.con.nwk" for s in stems])
    assert all(con[k] == v for k, v in plain.items())
    assert (stats["consensus"], stats["consensus_device"]) == (2, 0)
    assert {"consensus", "consensus_device"} <= set(scheduler.summarize(stats))
    for b, stem in enumerate(stems):
        assert con[f"{stem}.con.nwk"] == _want(preds[b], reps[b], ids[b], "nj", 50), stem
    # (file 0's replicate 2 has a NaN: it has no tree and counts in R, so no split of file 0 reaches 6 of 6)
    assert b")83:" in con["0_20_tips.con.nwk"] and b")100:" not in con["0_20_tips.con.nwk"] and b")100:" in con["1_20_tips.con.nwk"]

    new, stats = _run(paths, tmp_path / "new", native_io, Engine(), consensus=60, refined=True, tbe=True)
    added = ("tbe.nwk", "bme.sup.nwk", "bme.tbe.nwk", "spr.sup.nwk", "spr.tbe.nwk", "con.nwk", "bme.con.nwk", "spr.con.nwk")
    assert sorted(new) == sorted(list(plain) + [f"{s}.{x}" for s in stems for x in added])
    assert all(new[k] == v for k, v in plain.items())
    assert (stats["consensus"], stats["consensus_device"], stats["tbe"]) == (6, 0, 6)
    for b, stem in enumerate(stems):
        for kind in ("nj", "bme", "spr"):
            assert new[f"{stem}.{consensus.SUFFIXES[kind]}"] == _want(preds[b], reps[b], ids[b], kind, 60), (stem, kind)
    # the device branches, each alone and all together: the same bytes, the tables joined and refined once
    for lowered in (("CONSENSUS_DEVICE_MIN",), ("BME_DEVICE_MIN", "CONSENSUS_DEVICE_MIN"),
                    ("BME_DEVICE_MIN", "SPR_DEVICE_MIN", "SUPPORT_DEVICE_MIN", "CONSENSUS_DEVICE_MIN")):
        for name in ("BME_DEVICE_MIN", "SPR_DEVICE_MIN"):
            monkeypatch.setattr(bme, name, 4 if name in lowered else None)
        monkeypatch.setattr(supports, "SUPPORT_DEVICE_MIN", 4 if "SUPPORT_DEVICE_MIN" in lowered else None)
        monkeypatch.setattr(consensus, "CONSENSUS_DEVICE_MIN", 4)
        engine = Engine()
        got, dev_stats = _run(paths, tmp_path / "_".join(lowered), native_io, engine, consensus=60, refined=True, tbe=True)
        assert got == new, lowered
        kinds = 1 + ("BME_DEVICE_MIN" in lowered) + ("SPR_DEVICE_MIN" in lowered)
        assert engine.calls["join_consensus"] == kinds and dev_stats["consensus_device"] == 2 * kinds and dev_stats["consensus"] == 6
        assert engine.calls["nj_joins"] == 1 + ("BME_DEVICE_MIN" in lowered) + ("SPR_DEVICE_MIN" in lowered)
        assert engine.calls["bme_nni"] == (2 if "BME_DEVICE_MIN" in lowered else 0)


def test_fewer_than_four_sequences_get_the_star(tmp_path):
    _native()
    ind = tmp_path / "in"
    ind.mkdir()
    (ind / "three.fa").write_text(">x\nACDEFGHIKL\n>y\nACDEFGHIKV\n>z\nACDEFGHIVV\n")
    for native_io in (True, False):
        got, stats = _run([str(ind / "three.fa")], tmp_path / f"o{int(native_io)}", native_io, Engine(), consensus=50)
        assert got["three.con.nwk"] == b"(x,y,z);\n" and stats["consensus"] == 1
