"""-m gpu: the balanced SPR search on the device (``pf_bme_spr``, ``pf_bme_spr_device``) against its serial twin
(``pf_bme_spr_host``: the same bodies without a device) - slots, steps and status equal, lengths and tree length equal
as uint64 - and the CLI's ``--spr`` end to end."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import bme_check as bc
from phyloformer_amd import bme, hostio

pytestmark = pytest.mark.gpu


def assert_same(got, want):
    for name, g, w in zip(("slots", "lengths", "steps", "tree_length", "status"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), name


def eng_of(engines):
    from phyloformer_amd import build
    build.build()
    return engines()


# 137: the recursive split of the sums; 300: beyond a 256-thread workgroup of target edges and the sequence cap (there
# the sources are the path lengths of random trees, one move from their NJ trees: the serial twin stays quick)
@pytest.mark.parametrize("n", [3, 4, 6, 9, 137, 300])
def test_device_equals_the_serial_twin(engines, n):
    eng = eng_of(engines)
    if n < 300:
        preds = bc.uniform_preds(n, n * 100 + 256, 2)
    else:
        preds = np.stack([bc.random_tree_distances(n, s) * np.random.default_rng(s).uniform(0.9, 1.1, n * (n - 1) // 2).astype(np.float32)
                          for s in (1, 2)])
    nj_slots, _lengths, nonfinite = eng.nj_joins(preds)
    assert not nonfinite.any()
    eng.profile_reset()
    got = eng.bme_spr(preds, nj_slots)
    assert eng.profile_get("bme_spr")[0] == 1 and eng.profile_get("bme_nni")[0] == 0
    assert_same(got, hostio.bme_spr_host(preds, nj_slots))
    assert not got[4].any() and (n < 137 or got[2].min() >= 1)
    print(n, "steps", got[2])


def test_the_two_pair_table_kernels_give_the_same_bits(engines):
    eng = eng_of(engines)
    n = 137
    preds = bc.uniform_preds(n, 7, 1)
    start = eng.nj_joins(preds)[0]
    tiled = eng.bme_spr(preds, start)
    eng.set_option("spr_pairs_simple", 1)
    try:
        simple = eng.bme_spr(preds, start)
    finally:
        eng.set_option("spr_pairs_simple", 0)
    assert_same(tiled, simple)
    assert tiled[2][0] >= 1


def test_more_than_one_round_from_a_caterpillar(engines):
    eng = eng_of(engines)
    n = 65
    preds = np.stack([bc.uniform_preds(n, 6503, 1)[0], bc.random_tree_distances(n, 2)])
    starts = np.stack([bc.caterpillar_slots(n)] * 2)
    got = eng.bme_spr(preds, starts)
    assert_same(got, hostio.bme_spr_host(preds, starts))
    assert not got[4].any() and got[2].max() > 32
    print("steps", got[2])


def test_a_lowered_cap_stops_the_search(engines):
    eng = eng_of(engines)
    n = 17
    preds = bc.uniform_preds(n, 1956, 2)
    starts = np.stack([bc.caterpillar_slots(n)] * 2)
    free = eng.bme_spr(preds, starts)
    assert free[2].min() >= 3 and not free[4].any()
    eng.set_option("spr_step_cap", 2)
    try:
        got = eng.bme_spr(preds, starts)
    finally:
        eng.set_option("spr_step_cap", 0)
    assert got[2].tolist() == [2, 2] and got[4].tolist() == [bme.CAPPED, bme.CAPPED]
    for b in range(2):                                          # the tree after two moves, with its balanced lengths
        tree = bme.Tree(starts[b], n)
        dm = bme.matrix_of_preds(preds[b], n)
        for _ in range(2):
            best = min(bme.spr_candidates(bme.PairTable(dm, tree).t.tolist(), tree), key=lambda c: c[:3])
            bme.spr_move(tree, best[1], best[3])
        table = bme.Table(dm, tree)
        slots, lengths = bme.joins_of_tree(tree, table.lengths)
        assert np.array_equal(got[0][b], slots) and got[1][b].tobytes() == lengths.tobytes()
    assert_same(eng.bme_spr(preds, starts), free)


def test_chunks_under_a_small_workspace_limit(engines):
    """``ws_limit_mb = 1``: one source of 65 sequences fits (762,384 bytes), so three run in three chunks; 137 are
    refused, with the bytes in the message."""
    eng = eng_of(engines)
    n = 65
    preds = np.concatenate([bc.uniform_preds(n, 1, 2), bc.random_tree_distances(n, 3)[None, :]])
    starts = np.stack([bme.nj_start(bme.matrix_of_preds(p, n)) for p in preds])
    want = hostio.bme_spr_host(preds, starts)
    eng.set_option("ws_limit_mb", 1)
    try:
        assert_same(eng.bme_spr(preds, starts), want)
        with pytest.raises(ValueError, match=r"balanced SPR of N=137 sequences needs \d+ bytes of state per source"):
            eng.bme_spr(bc.uniform_preds(137, 1, 1), bc.caterpillar_slots(137)[None, :])
    finally:
        eng.set_option("ws_limit_mb", 24 << 10)
    assert_same(eng.bme_spr(preds, starts), want)


def test_the_three_searches_alternate_on_one_workspace(engines):
    """Balanced SPR, balanced NNI and - in a buffer of its own - neighbour joining carve their states from grow-only
    buffers of one engine; SPR and NNI share one, with different layouts.  Under ``ws_limit_mb = 1``: SPR (N = 9, B = 3),
    NNI (N = 65, B = 3: 240,944 bytes per source, so the three fit one chunk where SPR's 762,384 would make three), NJ
    (N = 65), then the first SPR call again.  Every result has the bytes of its serial twin, the two SPR results those
    of each other."""
    from helpers.nj_table import table_of
    eng = eng_of(engines)
    small = bc.uniform_preds(9, 909, 3)
    small_starts = np.stack([bc.caterpillar_slots(9)] * 3)
    n = 65
    preds = np.concatenate([bc.uniform_preds(n, 1, 2), bc.random_tree_distances(n, 3)[None, :]])
    starts = np.stack([bme.nj_start(bme.matrix_of_preds(p, n)) for p in preds])
    eng.set_option("ws_limit_mb", 1)
    try:
        first = eng.bme_spr(small, small_starts)
        nni = eng.bme_nni(preds, starts)
        slots, lengths, nonfinite = eng.nj_joins(preds)
        again = eng.bme_spr(small, small_starts)
    finally:
        eng.set_option("ws_limit_mb", 24 << 10)
    assert_same(first, hostio.bme_spr_host(small, small_starts))
    assert_same(nni, hostio.bme_nni_host(preds, starts))
    assert not nonfinite.any()
    for b in range(3):
        want_s, want_l = table_of(preds[b], n)
        assert_same((slots[b], lengths[b]), (want_s, want_l))
    assert_same(again, first)


def test_device_arrays(engines):
    eng = eng_of(engines)
    n, b = 17, 3
    t = 2 * (n - 3) + 3
    preds = np.stack([bc.random_tree_distances(n, s) for s in (1, 2, 3)])
    starts = np.stack([bc.caterpillar_slots(n)] * b)
    want = hostio.bme_spr_host(preds, starts)
    sizes = [preds.nbytes, starts.nbytes, b * t * 4, b * t * 8, b * 4, b * 8, b]
    ptrs = [eng.malloc(s) for s in sizes]
    try:
        eng.h2d(ptrs[0], preds)
        eng.h2d(ptrs[1], starts)
        eng.bme_spr_device(ptrs[0], ptrs[1], b, n, *ptrs[2:])
        got = [np.zeros((b, t), np.int32), np.zeros((b, t), np.float64), np.zeros(b, np.int32), np.zeros(b, np.float64), np.zeros(b, np.uint8)]
        for arr, p in zip(got, ptrs[2:]):
            eng.d2h(arr, p)
    finally:
        for p in ptrs:
            eng.free(p)
    assert_same(got, want)
    assert got[2].min() >= 1


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_source_next_to_a_finite_one(engines, bad):
    eng = eng_of(engines)
    n = 9
    preds = bc.uniform_preds(n, 9, 3)
    preds[1, 17] = bad
    starts = np.stack([bc.caterpillar_slots(n)] * 3)
    got = eng.bme_spr(preds, starts)
    assert got[4].tolist() == [0, 1, 0]
    assert not got[0][1].any() and not got[1][1].any()
    assert_same(got, hostio.bme_spr_host(preds, starts))


def test_refusals(engines):
    eng = eng_of(engines)
    n = 6
    preds = bc.uniform_preds(n, 6, 1)
    good = bc.caterpillar_slots(n)[None, :]
    for k, v in ((0, n), (0, -1), (3, 1), (8, 0)):
        bad = good.copy()
        bad[0, k] = v
        with pytest.raises(ValueError, match="start table"):
            eng.bme_spr(preds, bad)
    with pytest.raises(ValueError, match="N >= 3"):
        eng.bme_spr(np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int32))
    assert_same(eng.bme_spr(preds, good), hostio.bme_spr_host(preds, good))


def _cli(repo, args):
    return subprocess.run([sys.executable, os.path.join(repo, "infer_alns.py"), *args], capture_output=True, text=True, cwd=repo)


def test_cli_spr_end_to_end(repo, tmp_path, golden):
    """``infer_alns.py -t --spr`` on two shipped alignments: ``<stem>.spr.nwk`` has the topology of FastME ``-m N -s`` on
    the reference's distances of the same file, within the 1 % of the splits that tests/test_cli_gpu.py grants
    GPU-versus-reference distances (of these two files' 2 * (37 + 37) splits that is less than one: RF 0).  Then
    ``--tile 20 --spr --bme``: both refinements of the tiled distances, each the text the host writes for the ``.phy``
    beside it.  (That no other file changes its bytes is tests/test_spr_cli_host.py's.)"""
    from phyloformer_amd import fasta, treecmp
    from phyloformer_amd.phylip import vec_to_matrix
    ind, outd, tiled = (tmp_path / x for x in ("in", "out", "tiled"))
    ind.mkdir()
    stems = ("0_40_tips", "3_40_tips")
    for stem in stems:
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    ckpt = os.path.join(repo, "models/pf.ckpt")
    r = _cli(repo, [ckpt, str(ind), "-o", str(outd), "-t", "--spr", "--bench"])
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stderr.strip().splitlines()[-1])
    assert stats["spr"] == 2 and stats["spr_steps"] >= 0 and stats["spr_device"] == 0 and "bme" not in stats
    with open(os.path.join(repo, "tests", "golden", "fastme_nj_spr.json")) as fh:
        trees = json.load(fh)
    gold = golden("e2e_testdata.npz")
    rf, total = 0, 0
    for stem in stems:
        _idx, ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"))
        n = len(ids)
        dm = vec_to_matrix(gold[f"pf/{stem}"], n).astype(np.float64)
        key = hashlib.sha256(hostio.format_phylip(dm[np.triu_indices(n, 1)], ids)).hexdigest()
        mine = treecmp.parse_newick(open(outd / f"{stem}.spr.nwk").read())
        rf += treecmp.robinson_foulds(treecmp.parse_newick(trees[key]["tree"]), mine)[0]
        total += 2 * (n - 3)
    assert sorted(os.listdir(outd)) == sorted(f"{s}.{x}" for s in stems for x in ("phy", "nj.nwk", "spr.nwk"))
    print("RF summed over the two trees:", rf, "of", total, "splits")
    assert rf <= int(0.01 * total)
    r = _cli(repo, [ckpt, str(ind), "-o", str(tiled), "-t", "--tile", "20", "--spr", "--bme", "--bench"])
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stderr.strip().splitlines()[-1])
    assert stats["spr"] == 2 and stats["bme"] == 2
    names = set(os.listdir(tiled))
    assert {f"{s}.{x}" for s in stems for x in ("phy", "nj.nwk", "spr.nwk", "bme.nwk")} <= names
    for stem in stems:
        for kind in ("spr", "bme"):
            tree = treecmp.parse_newick(open(tiled / f"{stem}.{kind}.nwk").read())
            assert set(treecmp.splits(tree)) and open(tiled / f"{stem}.{kind}.nwk").read().count(",") == 39


def test_cli_takes_the_device_path_with_the_hosts_bytes(repo, tmp_path, monkeypatch):
    """A file of 70 sequences x 32 sites under ``-t --spr``: from ``SPR_DEVICE_MIN`` sequences on the tree is refined on
    the GPU thread, and ``<stem>.spr.nwk`` - like every other file - has the bytes of the run with the device path off.
    In one process, so that the constant can be set."""
    import infer_alns
    assert bme.SPR_DEVICE_MIN is not None and bme.SPR_DEVICE_MIN <= 70
    ind = tmp_path / "in"
    ind.mkdir()
    rng = np.random.default_rng(70)
    base = rng.integers(0, 20, size=32)
    alpha = "ARNDCQEGHILKMFPSTWYV"
    with open(ind / "big.fa", "w") as fh:
        for k in range(70):
            row = np.where(rng.random(32) < 0.3, rng.integers(0, 20, size=32), base)
            fh.write(f">s{k}\n{''.join(alpha[int(v)] for v in row)}\n")
    outs = {}
    for name, minimum in (("host", None), ("device", bme.SPR_DEVICE_MIN)):
        monkeypatch.setattr(bme, "SPR_DEVICE_MIN", minimum)
        out = tmp_path / name
        seen = []
        real = __import__("phyloformer_amd.scheduler", fromlist=["x"]).DirectoryRunner.book
        monkeypatch.setattr("phyloformer_amd.scheduler.DirectoryRunner.book",
                            lambda self, _real=real, _seen=seen, **kw: (_seen.append(kw), _real(self, **kw))[1])
        assert infer_alns.main([os.path.join(repo, "models/pf.ckpt"), str(ind), "-o", str(out), "-t", "--spr", "--gpu-streams", "1"]) == 0
        monkeypatch.setattr("phyloformer_amd.scheduler.DirectoryRunner.book", real)
        outs[name] = {f: open(out / f, "rb").read() for f in sorted(os.listdir(out))}
        device = sum(kw.get("spr_device", 0) for kw in seen)
        assert device == (1 if minimum else 0) and sum(kw.get("spr", 0) for kw in seen) == 1
    assert outs["host"] == outs["device"] and "big.spr.nwk" in outs["host"]
    assert outs["host"]["big.spr.nwk"] != outs["host"]["big.nj.nwk"]
