"""-m gpu: tree fit on the device - pf_tree_fit and pf_tree_fit_device against pf_tree_fit_host (itself pinned to fit.py in
tests/test_fit_host.py), every array bit for bit; both sides of the LDS / global switch of the pair kernel; patristic NULL
against non-NULL; a batch against single calls; chunks under a small workspace limit; trees with a status among fine ones;
the refusals and the call counter; Engine.tree_fit on the engine's own tables against the statement; the CLI end to end."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers.fit_inputs import balanced_slots, pairs_of, same, table_len, trees, uniform
from phyloformer_amd import bme
from phyloformer_amd import fit as F
from phyloformer_amd import fasta, hostio
from phyloformer_amd.engine import Engine

pytestmark = pytest.mark.gpu

_inputs = {}


def inputs(n, b, m):
    """The trees of a shape and the host twin's arrays, computed once."""
    if (n, b, m) not in _inputs:
        preds, slots, lengths = trees(n, 5000 + n, b, m)
        _inputs[n, b, m] = preds, slots, lengths, hostio.tree_fit_host(preds, slots, lengths)
    return _inputs[n, b, m]


def on_device(e, preds, slots, lengths, patristic=True):
    """pf_tree_fit_device on device arrays, the results filled with a pattern first."""
    b, m, t = slots.shape
    n = (t + 3) // 2
    out = (np.empty((b, m, pairs_of(n)), np.float64), np.empty((b, m, n, F.COLS), np.float64), np.empty((b, m, n), np.int32),
           np.empty((b, m), np.uint8))
    bufs = [e.malloc(a.nbytes) for a in (preds, slots, lengths, *out)]
    try:
        for host, dev in zip((preds, slots, lengths), bufs):
            e.h2d(dev, host)
        for host, dev in zip(out, bufs[3:]):
            e.h2d(dev, np.full(host.shape, 0x55, dtype=np.uint8).astype(host.dtype))
        e.tree_fit_device(*bufs[:3], b, m, n, bufs[3] if patristic else 0, *bufs[4:])
        for host, dev in zip(out, bufs[3:]):
            e.d2h(host, dev)
        e.synchronize()
    finally:
        for p in bufs:
            e.free(p)
    return out if patristic else (None, *out[1:])


# 3: no join; 4, 5: one and two; 31: half a wave of partners; 64 / 65: the edge of the 64 accumulators; 130: three passes
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n", [3, 4, 5, 31, 64, 65, 130])
def test_both_entry_points_equal_the_host_twin_bit_for_bit(engines, n, b, m):
    e = engines("pf")
    preds, slots, lengths, want = inputs(n, b, m)
    assert not want[3].any()
    assert same(e.tree_fit(preds, slots, lengths), want)
    assert same(on_device(e, preds, slots, lengths), want)


def test_a_caterpillar_and_a_balanced_table_of_130(engines):
    n = 130
    rng = np.random.default_rng(9)
    preds = uniform(n, 77, 1)
    slots = np.stack([bme.caterpillar_slots(n), balanced_slots(n)])[None]
    lengths = rng.uniform(-0.05, 1.0, size=slots.shape)
    assert F.table_status(slots[0, 1], n) == 0
    want = hostio.tree_fit_host(preds, slots, lengths)
    assert not want[3].any() and same(engines("pf").tree_fit(preds, slots, lengths), want)
    assert same(want[:1], (np.stack([F.patristic_py(slots[0, k], lengths[0, k], n) for k in range(2)])[None],))


def test_both_sides_of_the_lds_switch(weights):
    """The node arrays of 65 sequences take 128 x 12 bytes: with that much LDS allowed 65 sequences are staged and 66 are read
    from global memory (the product's switch is between 6,827 and 6,828)."""
    with Engine(weights("pf"), 0) as e:
        e.set_option("fit_lds_bytes", 128 * 12)
        for n in (65, 66):
            preds, slots, lengths = trees(n, 600 + n, 2, 3)
            want = hostio.tree_fit_host(preds, slots, lengths)
            assert same(e.tree_fit(preds, slots, lengths), want)
            assert same(on_device(e, preds, slots, lengths), want)
        e.set_option("fit_lds_bytes", 12)                   # nothing fits: global for every size
        preds, slots, lengths, want = inputs(31, 3, 3)
        assert same(e.tree_fit(preds, slots, lengths), want)


def test_without_patristic_the_rows_are_the_same(engines):
    e = engines("pf")
    for n, b, m in ((5, 3, 3), (65, 3, 3), (130, 1, 3)):
        preds, slots, lengths, want = inputs(n, b, m)
        got = e.tree_fit(preds, slots, lengths, patristic=False)
        assert got[0] is None and same(got[1:], want[1:])
        assert same(on_device(e, preds, slots, lengths, patristic=False)[1:], want[1:])


def test_a_batch_equals_single_calls_and_runs_repeat(engines):
    e = engines("pf")
    preds, slots, lengths, want = inputs(31, 3, 3)
    whole = e.tree_fit(preds, slots, lengths)
    again = e.tree_fit(preds, slots, lengths)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(whole, again))
    for k in range(3):
        assert same(e.tree_fit(preds[k:k + 1], slots[k:k + 1], lengths[k:k + 1]), tuple(x[k:k + 1] for x in whole))
        assert same(e.tree_fit(preds[k], slots[k], lengths[k]), tuple(x[k] for x in whole))
        assert same(e.tree_fit(preds[k], slots[k, 1], lengths[k, 1]), tuple(x[k, 1] for x in whole))


def test_chunks_under_a_small_workspace_limit(weights):
    """130 sequences: 71,216 bytes of state per tree without the caller's patristic, 4,136 with it; 18 trees under 1 MiB run in
    two chunks of 14 and 4 (the second starts inside source 4), with the patristic array in one."""
    n = 130
    preds, slots, lengths = trees(n, 808, 6, 3)
    want = hostio.tree_fit_host(preds, slots, lengths)
    with Engine(weights("pf"), 0) as e:
        e.set_option("ws_limit_mb", 1)
        got = e.tree_fit(preds, slots, lengths, patristic=False)
        assert same(got[1:], want[1:])
        assert same(on_device(e, preds, slots, lengths, patristic=False)[1:], want[1:])
        assert same(e.tree_fit(preds, slots, lengths), want)


def test_trees_with_a_status_leave_their_neighbours_unchanged(engines):
    e = engines("pf")
    n = 31
    preds, slots, lengths, clean = inputs(n, 3, 3)
    preds, slots, lengths = preds.copy(), slots.copy(), lengths.copy()
    preds[1, 40] = np.nan                  # every tree of source 1: status 1
    lengths[0, 1, 7] = np.inf              # one tree of source 0: status 1
    slots[2, 0, 4] = n                     # out of range: status 2
    slots[2, 2, 3] = slots[2, 2, 2]        # a == b: status 2
    want = hostio.tree_fit_host(preds, slots, lengths)
    assert want[3].tolist() == [[0, 1, 0], [1, 1, 1], [2, 0, 2]]
    for got in (e.tree_fit(preds, slots, lengths), on_device(e, preds, slots, lengths)):
        assert same(got, want)
        for b, m in ((0, 0), (0, 2), (2, 1)):
            assert same(tuple(x[b, m] for x in got), tuple(x[b, m] for x in clean))
        for b, m in ((0, 1), (1, 0), (1, 2), (2, 0), (2, 2)):
            assert not any(x[b, m].any() for x in got[:3])
    # tables of slots far out of range, negative, and of one slot only
    wild = np.stack([np.full(table_len(n), 2 ** 31 - 1), np.full(table_len(n), -2 ** 31), np.zeros(table_len(n))]).astype(np.int32)[None]
    got = e.tree_fit(preds[:1], wild, lengths[:1])
    assert got[3].tolist() == [[2, 2, 2]] and not any(x.any() for x in got[:3])


def test_refusals_and_call_counter(weights):
    n = 4
    preds, slots, lengths = trees(n, 3, 1, 1)
    with Engine(weights("pf"), 0) as e:
        e.profile_reset()
        assert e.profile_get("tree_fit")[0] == 0
        e.tree_fit(preds, slots, lengths)
        on_device(e, preds, slots, lengths)
        assert e.profile_get("tree_fit")[0] == 2
        with pytest.raises(ValueError, match=r"tree fit needs N >= 3 sequences \(got 2\)"):
            e.tree_fit(np.ones((1, 1), np.float32), np.zeros((1, 1, 1), np.int32), np.zeros((1, 1, 1)))
        # the library, before any device work: nothing counted, nothing written
        out = (np.full((1, 1, 6), -7.0), np.full((1, 1, n, 6), -7.0), np.full((1, 1, n), -7, np.int32), np.full((1, 1), 9, np.uint8))
        ptrs = [a.ctypes.data for a in out]
        ins = [preds.ctypes.data, slots.ctypes.data, lengths.ctypes.data]
        for fn in (e._lib.pf_tree_fit, e._lib.pf_tree_fit_device):
            for (b, m, k), text in (((1, 1, 2), "tree fit needs N >= 3 sequences (got 2)"),
                                    ((1, 1, 8193), "tree fit takes at most 8192 sequences (got 8193)"),
                                    ((1, 1, 65537), "tree fit takes at most 8192 sequences (got 65537)"),
                                    ((0, 1, n), "tree fit needs B >= 1 sources (got 0)"),
                                    ((1, 0, n), "tree fit needs M >= 1 trees per source (got 0)")):
                assert fn(e._h, *ins, b, m, k, *ptrs) == -1
                assert e._lib.pf_last_error(e._h).decode() == text
            for hole in (0, 1, 2, 4, 5, 6):                      # (3 is patristic: it may be NULL)
                args = [*ins, *ptrs]
                args[hole] = None
                assert fn(e._h, *args[:3], 1, 1, n, *args[3:]) == -1
                assert e._lib.pf_last_error(e._h).decode() == "null buffer"
        e.set_option("ws_limit_mb", 1)
        # 600 sequences without the caller's patristic: 1,198 nodes x 16 + 179,700 distances x 8 bytes of state for one tree
        assert e._lib.pf_tree_fit(e._h, *ins, 1, 1, 600, None, *ptrs[1:]) == -1
        assert "above the workspace limit of 1048576 bytes" in e._lib.pf_last_error(e._h).decode()
        e.set_option("ws_limit_mb", 24 << 10)
        assert e.profile_get("tree_fit")[0] == 2 and all((a == a.flat[0]).all() for a in out)
        assert same(e.tree_fit(preds, slots, lengths), hostio.tree_fit_host(preds, slots, lengths))      # the handle still works
        e.profile_reset()
        assert e.profile_get("tree_fit")[0] == 0


def test_the_engines_own_tables_of_a_real_forward_against_the_statement(engines, repo):
    e = engines("pf")
    idx, _ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas/0_20_tips.fa"))
    pred = e.forward(idx)
    start, start_len, flag = e.nj_joins(pred[None])
    assert not flag.any()
    refined = e.bme_nni(pred[None], start)
    slots, lengths = np.stack([start[0], refined[0][0]]), np.stack([start_len[0], refined[1][0]])
    got = e.tree_fit(pred, slots, lengths)
    assert got[3].tolist() == [0, 0]
    for k in range(2):
        assert same(tuple(x[k] for x in got), F.tree_fit_py(pred, slots[k], lengths[k], 20))
        s = F.fit_scores(pred, got[1][k], got[2][k], 20)
        assert s.explained <= 1 and 0 < s.correlation <= 1 + 1e-12 and s.rmse > 0 and s.worst[0] < s.worst[1]


def _cli(repo, args):
    return subprocess.run([sys.executable, os.path.join(repo, "infer_alns.py"), *args], capture_output=True, text=True, cwd=repo)


def test_cli_end_to_end_on_two_test_alignments(repo, tmp_path, engines):
    """``infer_alns.py -t --bme --bionj --fit``: ``<stem>.fit.tsv`` holds one line per written kind, every value is
    ``fit_scores`` of the written table, and every other output keeps the bytes of a run without the flag."""
    from helpers.fit_inputs import check_fit_files
    from phyloformer_amd.phylip import vec_to_phylip
    ind = tmp_path / "in"
    ind.mkdir()
    stems = ("0_20_tips", "0_30_tips")
    for stem in stems:
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    ckpt = os.path.join(repo, "models/pf.ckpt")
    r = _cli(repo, [ckpt, str(ind), "-o", str(tmp_path / "fit"), "-t", "--bme", "--bionj", "--fit", "--bench"])
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stderr.strip().splitlines()[-1])
    assert stats["fit"] == 2 and stats["fit_s"] > 0
    plain = _cli(repo, [ckpt, str(ind), "-o", str(tmp_path / "plain"), "-t", "--bme", "--bionj"])
    assert plain.returncode == 0, plain.stderr
    files = {n: (tmp_path / "fit" / n).read_bytes() for n in sorted(os.listdir(tmp_path / "fit"))}
    base = {n: (tmp_path / "plain" / n).read_bytes() for n in sorted(os.listdir(tmp_path / "plain"))}
    kinds = ["nj", "bme", "bionj", "bionj.bme"]
    added = {f"{s}.fit.tsv" for s in stems} | {f"{s}.{'' if k == 'nj' else k + '.'}{end}" for s in stems for k in kinds
                                               for end in ("fit.taxa.tsv", "patristic.phy")}
    assert set(files) == set(base) | added and all(files[n] == base[n] for n in base)
    for stem in stems:
        idx, ids = fasta.load_alignment(str(ind / f"{stem}.fa"))
        pred = engines("pf").forward(idx)
        assert files[f"{stem}.phy"].decode() == vec_to_phylip(pred, ids)[1]
        lines = check_fit_files(files, stem, pred, ids, kinds)
        assert len(lines) == 4 and all(0 < v[0] and v[1] <= 1 for v in lines.values())
