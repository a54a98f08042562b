"""Tree distances on the CPU: the statement (``treedist.join_distances_py``) by hand and against ``treecmp`` - an
independent reader of the written Newick text -, its properties, the serial twin (``pf_join_distances_host``) against it
bit for bit, and ``treedist.table_of_newick`` on the shipped trees."""
import glob
import math
import os

import numpy as np
import pytest

from helpers import bme_check as bc
from helpers import treedist_inputs as ti
from phyloformer_amd import bionj, bme, fasta, hostio, treecmp, treedist
from phyloformer_amd.nj import table_of_joins

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def statement(slots, lengths, flag, n):
    w = treedist.join_distances_py(slots, lengths, flag, n)
    return w.shared, w.kf, w.wrf, np.uint8(w.status)


# ---- hand cases, exact bits ------------------------------------------------------------------------------------------

def test_two_five_leaf_tables_by_hand():
    """A = ((0,1),(2,3),4), B = ((0,1),2,(3,4)) on dyadic lengths: they share {2,3,4}; the terms are 3, 8 | 0, -3 | 0, 1, 0,
    -1.75, -1.875."""
    slots = np.array([[0, 1, 2, 3, 0, 2, 4], [0, 1, 3, 4, 0, 2, 3]], dtype=np.int32)
    lengths = np.array([[1, 2, 0.5, 0.25, 4, 8, 0.125], [1, 1, 2, 2, 1, 0.5, 3]])
    for got in (statement(slots, lengths, None, 5), hostio.join_distances_host(slots, lengths)):
        assert got[0].tolist() == [[2, 1], [1, 2]] and got[3] == 0
        assert got[1].tolist() == [[0.0, math.sqrt(89.578125)], [math.sqrt(89.578125), 0.0]]
        assert got[2].tolist() == [[0.0, 18.625], [18.625, 0.0]]
    assert treedist.rf_of(1, 5) == 2


@pytest.mark.parametrize("n", [4, 8, 67])
def test_a_tree_against_itself(n):
    slots, lengths = ti.mixed(n, 1)
    got = statement(np.repeat(slots, 2, axis=0), np.repeat(lengths, 2, axis=0), None, n)
    assert (got[0] == n - 3).all() and got[1].tobytes() == np.zeros((2, 2)).tobytes() and not got[2].any()


def test_caterpillar_against_balanced_of_eight():
    """The caterpillar's clusters are {0,1}, {0,1,2}, ... ; the balanced table's are {0,1}, {2,3}, {4,5}, {6,7}, {0,1,2,3}:
    both hold {0,1} (as {2..7}), {0,1,2,3} (as {4..7}) and - the caterpillar's {0..5} - {6,7}, and nothing else."""
    slots = np.stack([bme.caterpillar_slots(8), ti.balanced_slots(8)])
    got = treedist.join_distances_py(slots, np.ones(slots.shape), None, 8)
    assert got.shared.tolist() == [[5, 3], [3, 5]]
    assert got.wrf[0, 1] == 4.0 and got.kf[0, 1] == 2.0               # (two unshared splits each, all other terms 0)


# ---- the statement against treecmp -----------------------------------------------------------------------------------

def tables_of(n):
    """NJ, BIONJ, BNNI, caterpillar, balanced and random tables of ``n`` sequences with non-negative lengths."""
    dm = bme.matrix_of_preds(bc.random_tree_distances(n, 3) * (1 + 0.2 * np.random.default_rng(n).standard_normal(n * (n - 1) // 2)).astype(np.float32), n)
    nj = table_of_joins(*bme.nj_joins(dm))
    rows = [nj, table_of_joins(*bionj.bionj_joins(dm)), bme.bme_nni(dm, nj[0])[:2]]
    slots = np.stack([np.asarray(r[0], dtype=np.int32) for r in rows] + [bme.caterpillar_slots(n), ti.balanced_slots(n), ti.random_tables(n, 1, n)[0]])
    lengths = np.abs(np.stack([np.asarray(r[1], dtype=np.float64) for r in rows] + list(np.random.default_rng(n + 1).standard_normal((3, slots.shape[1])))))
    return slots, lengths


@pytest.mark.parametrize("n", [4, 5, 31, 64, 65, 66, 67, 68, 130])
def test_statement_against_treecmp(n):
    slots, lengths = tables_of(n)
    ids = [f"t{x}" for x in range(n)]
    trees = [treecmp.parse_newick(hostio.newick_of_joins_py(s, l, ids)) for s, l in zip(slots, lengths)]
    got = treedist.join_distances_py(slots, lengths, None, n)
    assert got.status == 0
    for i in range(len(trees)):
        for j in range(len(trees)):
            assert treecmp.robinson_foulds(trees[i], trees[j])[0] == treedist.rf_of(got.shared[i, j], n), (i, j)
            kf = got.kf[i, j]
            assert abs(treecmp.branch_score(trees[i], trees[j]) - kf) <= 1e-12 * max(1.0, kf), (i, j)
    assert (got.wrf >= got.kf - 1e-12).all()                    # (the 1-norm is no less than the 2-norm)


# ---- properties ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [9, 65])
def test_symmetry_and_the_triangle_inequality(n):
    slots, lengths = ti.mixed(n, 7)
    got = treedist.join_distances_py(slots, lengths, None, n)
    rf = 2 * (n - 3) - 2 * got.shared.astype(np.int64)
    for m in (rf, got.kf, got.wrf):
        assert (m == m.T).all()
    assert (np.diag(rf) == 0).all() and (rf >= 0).all()
    for a in range(7):
        for b in range(7):
            for c in range(7):
                assert rf[a, c] <= rf[a, b] + rf[b, c]


def test_a_flagged_tree_is_never_read():
    n, k = 9, 4
    slots, lengths = (a.copy() for a in ti.mixed(n, k))
    slots[2] = np.iinfo(np.int32).min
    flag = [False, False, True, False]
    for got in (statement(slots, lengths, flag, n), hostio.join_distances_host(slots, lengths, flag)):
        assert got[3] == 0 and (got[0][2] == -1).all() and (got[0][:, 2] == -1).all()
        assert np.isnan(got[1][2]).all() and np.isnan(got[2][:, 2]).all()
        keep = [0, 1, 3]
        assert ti.same(tuple(a[np.ix_(keep, keep)] for a in got[:3]), statement(slots[keep], lengths[keep], None, n)[:3])


@pytest.mark.parametrize("where, value", [(3, 9), (0, -1), (4, 1 << 30), (14, 9), (13, 0)])
def test_status_1_for_a_table_that_is_none(where, value):
    n = 9
    slots, lengths = (a.copy() for a in ti.mixed(n, 3))
    slots[1] = bme.caterpillar_slots(n)
    slots[1, where] = value                                      # (13: the trifurcation names slot 0 twice)
    for got in (statement(slots, lengths, None, n), hostio.join_distances_host(slots, lengths)):
        assert got[3] == 1 and not got[0].any() and not got[1].any() and not got[2].any()


def test_status_1_for_a_join_of_a_dead_slot():
    n = 9
    slots, lengths = (a.copy() for a in ti.mixed(n, 3))
    slots[2] = bme.caterpillar_slots(n)
    slots[2, 2 * 3] = 1                                          # join 3 names the slot that join 0 joined away
    for got in (statement(slots, lengths, None, n), hostio.join_distances_host(slots, lengths)):
        assert got[3] == 1 and not got[0].any()


# ---- the twin against the statement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3, 7, 33])
@pytest.mark.parametrize("n", [4, 5, 64, 65, 67, 130])
def test_twin_equals_the_statement(n, k):
    slots, lengths = ti.mixed(n, k)
    flag = np.zeros(k, dtype=bool)
    flag[k // 2] = k > 2
    want = statement(slots, lengths, flag, n)
    assert ti.same(hostio.join_distances_host(slots, lengths, flag), want)
    none = hostio.join_distances_host(slots, None, flag)
    assert none[1] is None and none[2] is None and np.array_equal(none[0], want[0])
    three = hostio.join_distances_host(np.stack([slots, slots[::-1], slots]), np.stack([lengths, lengths[::-1], lengths]),
                                       np.stack([flag, flag[::-1], flag]))
    assert ti.same(tuple(a[0] for a in three), want) and ti.same(tuple(a[2] for a in three), want)
    assert ti.same(tuple(a[1] for a in three), statement(slots[::-1], lengths[::-1], flag[::-1], n))


def test_host_sides_answer_alike():
    from phyloformer_amd.treekinds import NativeHost, PythonHost
    slots, lengths = ti.mixed(9, 3)
    assert ti.same(NativeHost().join_distances(slots, lengths), PythonHost().join_distances(slots, lengths))
    with pytest.raises(ValueError):
        hostio.join_distances_host(np.zeros((4097, 5), dtype=np.int32))


# ---- a tree the user already has -------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(REPO, "data/testdata/trees/*.nwk"))))
def test_shipped_trees(path):
    stem = os.path.basename(path)[:-4]
    _idx, ids = fasta.load_alignment(os.path.join(REPO, "data/testdata/msas", f"{stem}.fa"))
    text = open(path).read()
    slots, lengths = treedist.table_of_newick(text, ids)
    back = treecmp.parse_newick(hostio.newick_of_joins_py(slots, lengths, ids, clamp_negative=False))
    given = treecmp.parse_newick(text)
    assert treecmp.robinson_foulds(back, given)[0] == 0
    assert treecmp.branch_score(back, given) <= 1e-12
    got = treedist.join_distances_py(np.stack([slots, slots]), np.stack([lengths, lengths]), None, len(ids))
    assert got.shared[0, 1] == len(ids) - 3 and got.kf[0, 1] == 0.0


def test_table_of_newick_roots_names_and_refusals():
    ids = ["a", "b c", "d", "e'f", "g"]
    three = "(a:1,'b c':2,((d:0.5,'e''f':0.25):4,g):8);"
    two = "((a:1,'b c':2):3,((d:0.5,'e''f':0.25):4,g):5);"
    s3, l3 = treedist.table_of_newick(three, ids)
    s2, l2 = treedist.table_of_newick(two, ids)
    assert s3.tolist() == s2.tolist() and sorted(l3) == sorted(l2) == [0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0]      # (3 + 5: one edge)
    got = treedist.join_distances_py(np.stack([s3, s2]), np.stack([l3, l2]), None, 5)
    assert got.shared[0, 1] == 2 and got.kf[0, 1] == 0.0
    for text, reason in (("(a,'b c',d,('e''f',g));", "children"), ("(a,'b c',(d,'e''f',g));", "children"),
                         ("(a,'b c',(d,('e''f',x)));", "not the alignment's"), ("(a,'b c',(d,'e''f'));", "not the alignment's"),
                         ("(a,a,(d,('e''f',g)));", "duplicate"), ("(a,'b c',((d),('e''f',g)));", "children"), ("(a,b", "must end")):
        with pytest.raises(ValueError, match=reason) as err:
            treedist.table_of_newick(text, ids)
        assert "\n" not in str(err.value)
    with pytest.raises(ValueError, match="fewer than four"):
        treedist.table_of_newick("(a,b,c);", ["a", "b", "c"])


def test_the_files():
    n = 9
    slots, lengths = ti.mixed(n, 3)
    dist = statement(slots, lengths, [False, False, True], n)
    text = treedist.treedist_tsv(["nj", "bme", "ref"], n, dist, [None, None, "no such file"])
    rows = [line.split("\t") for line in text.splitlines()]
    assert rows[0] == list(treedist.COLUMNS) and len(rows) == 4
    rf = treedist.rf_of(dist[0][0, 1], n)
    assert rows[1][:6] == ["nj", "bme", str(rf), repr(rf / 12), repr(float(dist[2][0, 1])), repr(float(dist[1][0, 1]))]
    assert rows[2][2:6] == ["NA"] * 4 and rows[2][6] == "ref: no such file"
    reps = treedist.reps_tsv(n, dist).splitlines()
    assert reps[0] == "rep\trf\tkf\tmean_rf" and reps[1].split("\t")[:2] == ["1", str(rf)] and reps[2] == "2\tNA\tNA\tNA"
    phy = treedist.rf_phylip(n, dist).splitlines()
    assert phy[0] == "3" and phy[1].split() == ["nj", "0", str(rf), "-1"]


# ---- the CLI through a stand-in engine -------------------------------------------------------------------------------

import json
import shutil
import subprocess
import sys

SHIPPED = ("0_20_tips", "1_20_tips")


def _write_fasta(path, idx):
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    with open(path, "w") as fh:
        for k, row in enumerate(idx):
            fh.write(f">s{k}\n{''.join(alpha[int(v)] for v in row)}\n")


@pytest.fixture(scope="module")
def shipped_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("treedist_alns")
    for stem in SHIPPED:
        shutil.copy(os.path.join(REPO, "data/testdata/msas", f"{stem}.fa"), d / f"{stem}.fa")
    return d


def _cli(args, tmp_path):
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_treedist_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=900)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def _rows(data):
    rows = [line.split("\t") for line in data.decode().split("\n")[:-1]]
    assert rows[0] == list(treedist.COLUMNS)
    return {(r[0], r[1]): r[2:] for r in rows[1:]}


def test_cli_reference_trees_against_treecmp_and_every_other_file_keeps_its_bytes(shipped_dir, tmp_path):
    """``-t --bme --bionj --fit --ols --bootstrap 3 --treedist-ref data/testdata/trees`` on two shipped files: every line
    of ``<stem>.treedist.tsv`` against ``treecmp`` on the written ``.nwk`` files and the shipped tree; the replicate files;
    every file of the run without the flag keeps its bytes."""
    base = [str(shipped_dir), "-t", "--bme", "--bionj", "--fit", "--ols", "--bootstrap", "3", "--seed", "2"]
    plain = _cli(base + ["-o", str(tmp_path / "plain")], tmp_path)
    r = _cli(base + ["-o", str(tmp_path / "o"), "--treedist-ref", os.path.join(REPO, "data/testdata/trees"), "--bench"], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, plain.stderr[-2000:] + r.stderr[-3000:]
    files, before = _files(tmp_path / "o"), _files(tmp_path / "plain")
    added = {f"{s}.treedist.{x}" for s in SHIPPED for x in ("tsv", "reps.tsv", "rf.phy")}
    assert set(files) == set(before) | added and not added & set(before)
    assert {"0_20_tips.sup.nwk", "0_20_tips.fit.tsv", "0_20_tips.ols.tsv"} <= set(before)
    assert all(files[name] == before[name] for name in before)
    names = ["nj", "bme", "bionj", "bionj.bme", "ref"]
    for stem in SHIPPED:
        trees = {k: treecmp.parse_newick(files[f"{stem}.{k}.nwk"].decode()) for k in names[:-1]}
        trees["ref"] = treecmp.parse_newick(open(os.path.join(REPO, "data/testdata/trees", f"{stem}.nwk")).read())
        rows = _rows(files[f"{stem}.treedist.tsv"])
        assert list(rows) == [(a, b) for i, a in enumerate(names) for b in names[i + 1:]]
        for (a, b), (rf, nrf, wrf, kf, note) in rows.items():
            want = treecmp.robinson_foulds(trees[a], trees[b])[0]
            assert int(rf) == want and float(nrf) == want / 34 and note == "", (stem, a, b)
            if "ref" in (a, b) or all(":-" not in files[f"{stem}.{k}.nwk"].decode() for k in (a, b)):
                # (the written files clamp negative lengths, the table does not: compared where nothing was clamped)
                score = treecmp.branch_score(trees[a], trees[b])
                assert "ref" in (a, b) or abs(score - float(kf)) <= 1e-12 * max(1.0, score), (stem, a, b)
            assert float(wrf) >= float(kf) - 1e-12
        reps = files[f"{stem}.treedist.reps.tsv"].decode().splitlines()
        assert reps[0] == "rep\trf\tkf\tmean_rf" and [line.split("\t")[0] for line in reps[1:]] == ["1", "2", "3"]
        assert all(int(line.split("\t")[1]) % 2 == 0 and float(line.split("\t")[3]) >= 0 for line in reps[1:])
        phy = files[f"{stem}.treedist.rf.phy"].decode().splitlines()
        assert phy[0] == "4" and [line.split()[0] for line in phy[1:]] == ["nj", "rep1", "rep2", "rep3"]
        assert [line.split()[1] for line in phy[2:]] == [line.split("\t")[1] for line in reps[1:]]
    report = json.loads([line for line in r.stderr.splitlines() if line.startswith("{")][-1])
    assert report["treedist"] == 2 and report["treedist_s"] > 0 and report["treedist_ref_missing"] == 0
    # through the Python I/O and one alignment per launch: the same files
    q = _cli(base + ["-o", str(tmp_path / "p"), "--treedist-ref", os.path.join(REPO, "data/testdata/trees"), "--python-io", "--batch", "1"],
             tmp_path)
    assert q.returncode == 0, q.stderr[-3000:]
    assert _files(tmp_path / "p") == files


def test_cli_refusals_and_the_usage_error(shipped_dir, tmp_path):
    for args, text in ((["--treedist"], treedist.NEEDS_TREES), (["-t", "--treedist-ref", "x", "--shard", "sites"], treedist.SHARD_SITES),
                       (["-t", "--treedist"], treedist.NOTHING_TO_COMPARE)):
        r = _cli([str(shipped_dir), "-o", str(tmp_path / "o"), *args], tmp_path)
        assert r.returncode == 2 and text in r.stderr and "usage:" in r.stderr, (args, r.stderr[-500:])
    assert "--bme, --spr and --bionj" in treedist.NOTHING_TO_COMPARE and "--treedist-ref" in treedist.NOTHING_TO_COMPARE
    assert "--bootstrap" in treedist.NOTHING_TO_COMPARE
    assert not os.path.exists(tmp_path / "o") or not os.listdir(tmp_path / "o")
    from phyloformer_amd.scheduler import DirectoryRunner, SiteShardedRunner
    with pytest.raises(ValueError, match="--treedist cannot be combined with --shard sites"):
        SiteShardedRunner(None, None, 0, 1, str(tmp_path), trees=True, bme=True, treedist=True)
    with pytest.raises(ValueError, match="--treedist compares the trees of --trees: give -t as well"):
        DirectoryRunner(None, str(tmp_path), treedist=True)
    with pytest.raises(ValueError, match="--treedist has nothing to compare"):
        DirectoryRunner(None, str(tmp_path), trees=True, treedist=True)


def test_runner_takes_both_routes_and_notes_what_is_missing(tmp_path, monkeypatch):
    """With the thresholds at 4 sequences the kinds' tables are made on the GPU thread and one ``Engine.join_distances`` serves
    a launch; the files are those of the host route.  A missing and a polytomous reference tree, three sequences and distances
    that are not finite give ``NA`` with a note, and the run goes on."""
    from helpers.oracle_treedist_engine import OracleTreedistEngine
    from phyloformer_amd import bionj as bionj_mod
    from phyloformer_amd.msa_sim import simulate_batch
    from phyloformer_amd.scheduler import DirectoryRunner
    from phyloformer_amd.weights import load_weights
    assert treedist.TREEDIST_DEVICE_MIN is None or treedist.TREEDIST_DEVICE_MIN in (20, 60, 200, 512, 1024, 4096)
    w = load_weights(os.path.join(REPO, "models", "pf_base.ckpt"))
    alns = {"six": simulate_batch(1, 6, 20, seed=401)[0], "nine": simulate_batch(1, 9, 20, seed=402)[0],
            "poly": simulate_batch(1, 6, 20, seed=404)[0], "three": simulate_batch(1, 3, 20, seed=403)[0]}
    for stem, a in alns.items():
        _write_fasta(tmp_path / f"{stem}.fa", a)
    refs = tmp_path / "refs"
    refs.mkdir()
    (refs / "six.nwk").write_text("((s0:1,s1:1):1,(s2:1,(s3:1,(s4:1,s5:1):1):1):1);\n")
    (refs / "poly.nwk").write_text("(s0,s1,s2,(s3,s4,s5));\n")
    (refs / "three.nwk").write_text("(s0,s1,s2);\n")
    paths = [str(tmp_path / f"{stem}.fa") for stem in alns]
    outs = {}
    for name, minimum in (("host", None), ("device", 4)):
        monkeypatch.setattr(bme, "BME_DEVICE_MIN", minimum)
        monkeypatch.setattr(bionj_mod, "BIONJ_DEVICE_MIN", minimum)
        monkeypatch.setattr(treedist, "TREEDIST_DEVICE_MIN", minimum)
        OracleTreedistEngine.distance_calls = 0
        out = tmp_path / name
        out.mkdir()
        stats = DirectoryRunner(OracleTreedistEngine(w, 0), str(out), trees=True, bme=True, bionj=True, treedist_ref=str(refs)).run(paths)
        assert stats["treedist"] == 4 and stats["treedist_s"] > 0 and stats["treedist_ref_missing"] == 2     # (nine: missing; poly: refused; three is never read)
        assert OracleTreedistEngine.distance_calls == (2 if minimum else 0)      # (the launches of six and of nine sequences)
        outs[name] = _files(out)
    assert outs["host"] == outs["device"]
    six, nine, poly, three = (_rows(outs["host"][f"{s}.treedist.tsv"]) for s in ("six", "nine", "poly", "three"))
    assert all(r[4] == "" and r[0] != "NA" for r in six.values()) and len(six) == 10
    assert nine["nj", "bme"][0] != "NA" and nine["nj", "ref"][:4] == ["NA"] * 4 and nine["nj", "ref"][4].startswith("ref: no reference tree")
    assert poly["bme", "ref"][:4] == ["NA"] * 4 and "children" in poly["bme", "ref"][4] and poly["nj", "bionj"][0] != "NA"
    assert all(r == ["NA"] * 4 + ["; ".join(f"{x}: {treedist.FEW_SEQUENCES}" for x in pair)] for pair, r in three.items()) and len(three) == 10

    class NanEngine(OracleTreedistEngine):
        def forward(self, idx):
            return np.full((len(idx), idx.shape[1] * (idx.shape[1] - 1) // 2), np.nan, dtype=np.float32)

    out = tmp_path / "nan"
    out.mkdir()
    DirectoryRunner(NanEngine(w, 0), str(out), trees=True, bme=True, treedist_ref=str(refs), native_io=False).run(paths[:1])
    rows = _rows((out / "six.treedist.tsv").read_bytes())
    assert rows["nj", "bme"] == ["NA"] * 4 + [f"nj: {treedist.NOT_FINITE}; bme: {treedist.NOT_FINITE}"]
    assert rows["bme", "ref"] == ["NA"] * 4 + [f"bme: {treedist.NOT_FINITE}"]


def test_bootstrap_files_on_both_routes(tmp_path, monkeypatch):
    """``--bootstrap 4 --tbe --treedist``: the replicate call beside ``Bootstrap._extend``'s device calls with the thresholds
    lowered, the host side's otherwise - the same files, and ``.sup.nwk`` / ``.tbe.nwk`` as without the flag."""
    from helpers.oracle_treedist_engine import OracleTreedistEngine
    from phyloformer_amd import supports
    from phyloformer_amd.analyses import Bootstrap
    from phyloformer_amd.msa_sim import simulate_batch
    from phyloformer_amd.scheduler import DirectoryRunner
    from phyloformer_amd.weights import load_weights
    assert treedist.reps_minimum(101) == treedist.TREEDIST_REPS_DEVICE_MIN and treedist.reps_minimum(100) == treedist.TREEDIST_DEVICE_MIN
    assert treedist.TREEDIST_REPS_DEVICE_MIN is None or treedist.TREEDIST_REPS_DEVICE_MIN in (20, 60, 200, 512, 1024, 4096)
    w = load_weights(os.path.join(REPO, "models", "pf_base.ckpt"))
    _write_fasta(tmp_path / "nine.fa", simulate_batch(1, 9, 20, seed=402)[0])
    _write_fasta(tmp_path / "three.fa", simulate_batch(1, 3, 20, seed=403)[0])
    paths = [str(tmp_path / "nine.fa"), str(tmp_path / "three.fa")]
    outs = {}
    for name, minimum, flag in (("plain", None, False), ("host", None, True), ("device", 4, True)):
        monkeypatch.setattr(supports, "SUPPORT_DEVICE_MIN", minimum)
        monkeypatch.setattr(treedist, "TREEDIST_DEVICE_MIN", minimum)        # (five trees go by the threshold of few trees)
        OracleTreedistEngine.distance_calls = 0
        out = tmp_path / name
        out.mkdir()
        DirectoryRunner(OracleTreedistEngine(w, 0), str(out), trees=True, treedist=flag, modes=[Bootstrap(4, 1, tbe=True)]).run(paths)
        assert OracleTreedistEngine.distance_calls == (1 if minimum else 0)
        outs[name] = _files(out)
    assert outs["host"] == outs["device"]
    added = {f"{s}.treedist.{x}" for s in ("nine", "three") for x in ("tsv", "reps.tsv", "rf.phy")}
    assert set(outs["host"]) == set(outs["plain"]) | added and "nine.tbe.nwk" in outs["plain"]
    assert all(outs["host"][f] == outs["plain"][f] for f in outs["plain"])
    assert outs["host"]["nine.treedist.tsv"].decode() == "\t".join(treedist.COLUMNS) + "\n"      # (one tree: no pair)
    assert outs["host"]["three.treedist.reps.tsv"].decode().splitlines()[1:] == [f"{r}\tNA\tNA\tNA" for r in range(1, 5)]
    assert outs["host"]["three.treedist.rf.phy"].decode().splitlines()[1].split() == ["nj", "-1", "-1", "-1", "-1", "-1"]
    assert outs["host"]["nine.treedist.rf.phy"].decode().splitlines()[1].split()[:2] == ["nj", "0"]
