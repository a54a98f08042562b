"""-m gpu: least-squares branch lengths on the device - pf_tree_ols and pf_tree_ols_device against pf_tree_ols_host (itself
pinned to ols.py in tests/test_ols_host.py), bit for bit; a caterpillar and a balanced table; a batch against single calls;
chunks under a small workspace limit; trees with a status among fine ones; the refusals and the call counter; Engine.tree_ols
on the engine's own tables against the statement; the CLI end to end.  (The kernels have no size switch.)"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers.fit_inputs import same
from helpers.ols_inputs import SIZES, balanced_slots, check_ols_files, table_len, tables, uniform
from phyloformer_amd import bme
from phyloformer_amd import fit as F
from phyloformer_amd import ols as O
from phyloformer_amd import fasta, hostio
from phyloformer_amd.engine import Engine

pytestmark = pytest.mark.gpu

_inputs = {}


def inputs(n, b, m):
    """The tables of a shape and the host twin's arrays, computed once."""
    if (n, b, m) not in _inputs:
        preds, slots = tables(n, 7000 + n, b, m)
        _inputs[n, b, m] = preds, slots, hostio.tree_ols_host(preds, slots)
    return _inputs[n, b, m]


def on_device(e, preds, slots):
    """pf_tree_ols_device on device arrays, the results filled with a pattern first."""
    b, m, t = slots.shape
    n = (t + 3) // 2
    out = (np.empty((b, m, t), np.float64), np.empty((b, m), np.uint8))
    bufs = [e.malloc(a.nbytes) for a in (preds, slots, *out)]
    try:
        for host, dev in zip((preds, slots), bufs):
            e.h2d(dev, host)
        for host, dev in zip(out, bufs[2:]):
            e.h2d(dev, np.full(host.shape, 0x55, dtype=np.uint8).astype(host.dtype))
        e.tree_ols_device(*bufs[:2], b, m, n, *bufs[2:])
        for host, dev in zip(out, bufs[2:]):
            e.d2h(host, dev)
        e.synchronize()
    finally:
        for p in bufs:
            e.free(p)
    return out


# 3, 4: the last node's children are leaves; 5: a join below a join; 31: half a wave; 64 / 65: the edge of the 64 accumulators;
# 130: three passes
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_both_entry_points_equal_the_host_twin_bit_for_bit(engines, n, b, m):
    e = engines("pf")
    preds, slots, want = inputs(n, b, m)
    assert not want[1].any() and want[0].any()
    assert same(e.tree_ols(preds, slots), want)
    assert same(on_device(e, preds, slots), want)


def test_a_caterpillar_and_a_balanced_table_of_130(engines):
    n = 130
    preds = uniform(n, 78, 1)
    slots = np.stack([bme.caterpillar_slots(n), balanced_slots(n)])[None]
    assert F.table_status(slots[0, 1], n) == 0
    want = hostio.tree_ols_host(preds, slots)
    assert not want[1].any() and same(engines("pf").tree_ols(preds, slots), want)
    assert same(want[:1], (np.stack([O.tree_ols_py(preds[0], slots[0, k], n)[0] for k in range(2)])[None],))


def test_a_batch_equals_single_calls_and_runs_repeat(engines):
    e = engines("pf")
    preds, slots, _want = inputs(31, 3, 3)
    whole = e.tree_ols(preds, slots)
    again = e.tree_ols(preds, slots)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(whole, again))
    for k in range(3):
        assert same(e.tree_ols(preds[k:k + 1], slots[k:k + 1]), tuple(x[k:k + 1] for x in whole))
        assert same(e.tree_ols(preds[k], slots[k]), tuple(x[k] for x in whole))
        assert same(e.tree_ols(preds[k], slots[k, 1]), tuple(x[k, 1] for x in whole))


def test_chunks_under_a_small_workspace_limit(weights):
    """130 sequences: 258 x 130 doubles of column sums and 7 N int32 of node arrays, about 272 KB of state per tree; nine trees
    need 2.4 MB and run under 1 MiB in three chunks of three.  120 sequences: 232 KB; four trees a chunk, so the second chunk
    starts inside source 1 and the third holds one tree."""
    with Engine(weights("pf"), 0) as e:
        e.set_option("ws_limit_mb", 1)
        for n in (130, 120):
            preds, slots = tables(n, 909, 3, 3)
            want = hostio.tree_ols_host(preds, slots)
            assert same(e.tree_ols(preds, slots), want)
            assert same(on_device(e, preds, slots), want)


def test_trees_with_a_status_leave_their_neighbours_unchanged(engines):
    e = engines("pf")
    n = 31
    preds, slots, clean = inputs(n, 3, 3)
    preds, slots = preds.copy(), slots.copy()
    preds[1, 40] = np.inf                  # every tree of source 1: status 1
    slots[2, 0, 4] = n                     # out of range: status 2
    slots[2, 2, 3] = slots[2, 2, 2]        # a == b: status 2
    slots[0, 1, -1] = slots[0, 1, -2]      # a repeated last slot: status 2
    want = hostio.tree_ols_host(preds, slots)
    assert want[1].tolist() == [[0, 2, 0], [1, 1, 1], [2, 0, 2]]
    for got in (e.tree_ols(preds, slots), on_device(e, preds, slots)):
        assert same(got, want)
        for b, m in ((0, 0), (0, 2), (2, 1)):
            assert same(tuple(x[b, m] for x in got), tuple(x[b, m] for x in clean))
        for b, m in ((0, 1), (1, 0), (1, 2), (2, 0), (2, 2)):
            assert not got[0][b, m].any()
    # a table that is none in a source that is not finite: the table is checked first
    slots[1, 1, 0] = -1
    assert e.tree_ols(preds, slots)[1].tolist() == [[0, 2, 0], [1, 2, 1], [2, 0, 2]]
    # tables of slots far out of range, negative, and of one slot only
    wild = np.stack([np.full(table_len(n), 2 ** 31 - 1), np.full(table_len(n), -2 ** 31), np.zeros(table_len(n))]).astype(np.int32)[None]
    got = e.tree_ols(preds[:1], wild)
    assert got[1].tolist() == [[2, 2, 2]] and not got[0].any()


def test_refusals_and_call_counter(weights):
    n = 4
    preds, slots = tables(n, 3, 1, 1)
    with Engine(weights("pf"), 0) as e:
        e.profile_reset()
        assert e.profile_get("tree_ols")[0] == 0
        e.tree_ols(preds, slots)
        on_device(e, preds, slots)
        assert e.profile_get("tree_ols")[0] == 2
        with pytest.raises(ValueError, match=r"tree OLS needs N >= 3 sequences \(got 2\)"):
            e.tree_ols(np.ones((1, 1), np.float32), np.zeros((1, 1, 1), np.int32))
        # the library, before any device work: nothing counted, nothing written
        out = (np.full((1, 1, table_len(n)), -7.0), np.full((1, 1), 9, np.uint8))
        ptrs = [a.ctypes.data for a in out]
        ins = [preds.ctypes.data, slots.ctypes.data]
        for fn in (e._lib.pf_tree_ols, e._lib.pf_tree_ols_device):
            for (b, m, k), text in (((1, 1, 2), "tree OLS needs N >= 3 sequences (got 2)"),
                                    ((1, 1, 8193), "tree OLS takes at most 8192 sequences (got 8193)"),
                                    ((1, 1, 65537), "tree OLS takes at most 8192 sequences (got 65537)"),
                                    ((0, 1, n), "tree OLS needs B >= 1 sources (got 0)"),
                                    ((1, 0, n), "tree OLS needs M >= 1 trees per source (got 0)")):
                assert fn(e._h, *ins, b, m, k, *ptrs) == -1
                assert e._lib.pf_last_error(e._h).decode() == text
            for hole in range(4):
                args = [*ins, *ptrs]
                args[hole] = None
                assert fn(e._h, *args[:2], 1, 1, n, *args[2:]) == -1
                assert e._lib.pf_last_error(e._h).decode() == "null buffer"
        e.set_option("ws_limit_mb", 1)
        # 600 sequences: 1,198 x 600 doubles of column sums, 5.75 MB of state for one tree
        assert e._lib.pf_tree_ols(e._h, *ins, 1, 1, 600, *ptrs) == -1
        text = e._lib.pf_last_error(e._h).decode()
        assert "tree OLS of N=600 sequences needs 57" in text and "above the workspace limit of 1048576 bytes" in text
        e.set_option("ws_limit_mb", 24 << 10)
        assert e.profile_get("tree_ols")[0] == 2 and all((a == a.flat[0]).all() for a in out)
        assert same(e.tree_ols(preds, slots), hostio.tree_ols_host(preds, slots))      # the handle still works
        e.profile_reset()
        assert e.profile_get("tree_ols")[0] == 0


def test_the_engines_own_tables_of_a_real_forward_against_the_statement(engines, repo):
    e = engines("pf")
    idx, _ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas/0_20_tips.fa"))
    pred = e.forward(idx)
    start, start_len, flag = e.nj_joins(pred[None])
    other, other_len, other_flag = e.bionj_joins(pred[None])
    assert not flag.any() and not other_flag.any()
    refined = e.bme_nni(pred[None], start)
    slots = np.stack([start[0], other[0], refined[0][0]])
    lengths = np.stack([start_len[0], other_len[0], refined[1][0]])
    got = e.tree_ols(pred, slots)
    assert got[1].tolist() == [0, 0, 0]
    fits = e.tree_fit(pred, np.concatenate([slots, slots]), np.concatenate([lengths, got[0]]), patristic=False)
    for k in range(3):
        assert same(tuple(x[k] for x in got), O.tree_ols_py(pred, slots[k], 20))
        s = O.ols_scores(pred, lengths[k], got[0][k], fits[1][[k, 3 + k]], fits[2][[k, 3 + k]], 20)
        assert 0 < s.rmse_ols <= s.rmse and s.explained <= s.explained_ols <= 1 and s.max_change > 0


def _cli(repo, args):
    return subprocess.run([sys.executable, os.path.join(repo, "infer_alns.py"), *args], capture_output=True, text=True, cwd=repo)


def test_cli_end_to_end_on_two_test_alignments(repo, tmp_path, engines):
    """``infer_alns.py -t --bme --bionj --ols``: per written kind ``<stem>[.<kind>].ols.nwk`` is the kind's table with the OLS
    lengths - it parses to the kind's own topology -, ``<stem>.ols.tsv`` holds ``ols_scores`` of the written tables with
    ``rmse_ols <= rmse``, and every other output keeps the bytes of a run without the flag."""
    from phyloformer_amd.phylip import vec_to_phylip
    from phyloformer_amd.treecmp import parse_newick, robinson_foulds
    ind = tmp_path / "in"
    ind.mkdir()
    stems = ("0_20_tips", "0_30_tips")
    for stem in stems:
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    ckpt = os.path.join(repo, "models/pf.ckpt")
    r = _cli(repo, [ckpt, str(ind), "-o", str(tmp_path / "ols"), "-t", "--bme", "--bionj", "--ols", "--bench"])
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stderr.strip().splitlines()[-1])
    assert stats["ols"] == 2 and stats["ols_s"] > 0
    plain = _cli(repo, [ckpt, str(ind), "-o", str(tmp_path / "plain"), "-t", "--bme", "--bionj"])
    assert plain.returncode == 0, plain.stderr
    files = {n: (tmp_path / "ols" / n).read_bytes() for n in sorted(os.listdir(tmp_path / "ols"))}
    base = {n: (tmp_path / "plain" / n).read_bytes() for n in sorted(os.listdir(tmp_path / "plain"))}
    kinds = ["nj", "bme", "bionj", "bionj.bme"]
    added = {f"{s}.ols.tsv" for s in stems} | {f"{s}.{'' if k == 'nj' else k + '.'}ols.nwk" for s in stems for k in kinds}
    assert set(files) == set(base) | added and all(files[n] == base[n] for n in base)
    for stem in stems:
        idx, ids = fasta.load_alignment(str(ind / f"{stem}.fa"))
        pred = engines("pf").forward(idx)
        assert files[f"{stem}.phy"].decode() == vec_to_phylip(pred, ids)[1]
        lines = check_ols_files(files, stem, pred, ids, kinds)
        assert len(lines) == 4 and all(0 < s.rmse_ols <= s.rmse for s in lines.values())
        for k in kinds:
            prefix = "" if k == "nj" else k + "."
            best, own = (parse_newick(files[f"{stem}.{name}"].decode()) for name in (f"{prefix}ols.nwk", f"{k}.nwk"))
            assert robinson_foulds(best, own)[0] == 0
