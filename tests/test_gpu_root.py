"""-m gpu: tree rooting on the device - pf_tree_root and pf_tree_root_device against pf_tree_root_host (itself pinned to root.py
in tests/test_root_host.py), bit for bit, at the house's sizes and the two around k_root_score's tile of 256; a batch against
single calls; chunks under a small workspace limit; trees with a status among fine ones; the refusals and the call counter;
Engine.tree_root on the engine's own tables against the statement; the CLI end to end."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers.root_inputs import GPU_SIZES, same, table_len, tables
from phyloformer_amd import fasta, hostio
from phyloformer_amd import root as R
from phyloformer_amd.engine import Engine

pytestmark = pytest.mark.gpu

_inputs = {}


def inputs(n, b, m):
    """The tables of a shape and the host twin's arrays, computed once."""
    if (n, b, m) not in _inputs:
        slots, lengths = tables(n, 7100 + n, b, m)
        _inputs[n, b, m] = slots, lengths, hostio.tree_root_host(slots, lengths)
    return _inputs[n, b, m]


def on_device(e, slots, lengths):
    """pf_tree_root_device on device arrays, the results filled with a pattern first."""
    b, m, t = slots.shape
    n = (t + 3) // 2
    out = (np.empty((b, m, t), np.float64), np.empty((b, m, t), np.float64), np.empty((b, m, R.MID), np.float64), np.empty((b, m), np.uint8))
    bufs = [e.malloc(a.nbytes) for a in (slots, lengths, *out)]
    try:
        for host, dev in zip((slots, lengths), bufs):
            e.h2d(dev, host)
        for host, dev in zip(out, bufs[2:]):
            e.h2d(dev, np.full(host.shape, 0x55, dtype=np.uint8).astype(host.dtype))
        e.tree_root_device(*bufs[:2], b, m, n, *bufs[2:])
        for host, dev in zip(out, bufs[2:]):
            e.d2h(host, dev)
        e.synchronize()
    finally:
        for p in bufs:
            e.free(p)
    return out


# 3: leaf branches only; 4, 5: a join below a join; 31: half a wave; 64 / 65: the edge of the 64 accumulators; 130: three passes;
# 256 / 257: the edge of the score kernel's group of places and chunk of partners.  With b = m = 3 all four kinds of table run.
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n", GPU_SIZES)
def test_both_entry_points_equal_the_host_twin_bit_for_bit(engines, n, b, m):
    e = engines("pf")
    slots, lengths, want = inputs(n, b, m)
    assert not want[3].any() and want[0].any() and want[2].any()
    assert same(e.tree_root(slots, lengths), want)
    assert same(on_device(e, slots, lengths), want)


def test_a_batch_equals_single_calls_and_runs_repeat(engines):
    e = engines("pf")
    slots, lengths, _want = inputs(31, 3, 3)
    whole = e.tree_root(slots, lengths)
    again = e.tree_root(slots, lengths)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(whole, again))
    for k in range(3):
        assert same(e.tree_root(slots[k:k + 1], lengths[k:k + 1]), tuple(x[k:k + 1] for x in whole))
        assert same(e.tree_root(slots[k], lengths[k]), tuple(x[k] for x in whole))
        assert same(e.tree_root(slots[k, 1], lengths[k, 1]), tuple(x[k, 1] for x in whole))


def test_chunks_under_a_small_workspace_limit(weights):
    """130 sequences: 258 x 130 + 130 x 130 doubles and the node arrays, about 410 KB of state per tree: two trees a chunk under
    1 MiB.  Sources of two trees are aligned with the chunks, sources of three are not and the last chunk holds one tree."""
    with Engine(weights("pf"), 0) as e:
        e.set_option("ws_limit_mb", 1)
        for b, m in ((3, 2), (3, 3)):
            slots, lengths = tables(130, 909, b, m)
            want = hostio.tree_root_host(slots, lengths)
            assert same(e.tree_root(slots, lengths), want)
            assert same(on_device(e, slots, lengths), want)


def test_trees_with_a_status_leave_their_neighbours_unchanged(engines):
    e = engines("pf")
    n = 31
    slots, lengths, clean = inputs(n, 3, 3)
    slots, lengths = slots.copy(), lengths.copy()
    lengths[1, 0, 7] = np.inf              # status 1
    lengths[1, 2, 0] = np.nan              # status 1
    slots[2, 0, 4] = n                     # out of range: status 2
    slots[2, 2, 3] = slots[2, 2, 2]        # a == b: status 2
    slots[0, 1, -1] = slots[0, 1, -2]      # a repeated last slot: status 2
    want = hostio.tree_root_host(slots, lengths)
    assert want[3].tolist() == [[0, 2, 0], [1, 0, 1], [2, 0, 2]]
    for got in (e.tree_root(slots, lengths), on_device(e, slots, lengths)):
        assert same(got, want)
        for b, m in ((0, 0), (0, 2), (1, 1), (2, 1)):
            assert same(tuple(x[b, m] for x in got), tuple(x[b, m] for x in clean))
        for b, m in ((0, 1), (1, 0), (1, 2), (2, 0), (2, 2)):
            assert not any(x[b, m].any() for x in got[:3])
    # a table that is none with lengths that are not finite: the table is checked first
    slots[1, 0, 0] = -1
    assert e.tree_root(slots, lengths)[3].tolist() == [[0, 2, 0], [2, 0, 1], [2, 0, 2]]
    # tables of slots far out of range, negative, and of one slot only
    wild = np.stack([np.full(table_len(n), 2 ** 31 - 1), np.full(table_len(n), -2 ** 31), np.zeros(table_len(n))]).astype(np.int32)[None]
    got = e.tree_root(wild, lengths[:1])
    assert got[3].tolist() == [[2, 2, 2]] and not any(x.any() for x in got[:3])


def test_refusals_and_call_counter(weights):
    n = 4
    slots, lengths = tables(n, 3, 1, 1)
    with Engine(weights("pf"), 0) as e:
        e.profile_reset()
        assert e.profile_get("tree_root")[0] == 0
        e.tree_root(slots, lengths)
        on_device(e, slots, lengths)
        assert e.profile_get("tree_root")[0] == 2
        with pytest.raises(ValueError, match=r"tree root needs N >= 3 sequences \(got 2\)"):
            e.tree_root(np.zeros((1, 1, 1), np.int32), np.ones((1, 1, 1)))
        # the library, before any device work: nothing counted, nothing written
        out = (np.full((1, 1, table_len(n)), -7.0), np.full((1, 1, table_len(n)), -7.0), np.full((1, 1, R.MID), -7.0), np.full((1, 1), 9, np.uint8))
        ptrs = [a.ctypes.data for a in out]
        ins = [slots.ctypes.data, lengths.ctypes.data]
        for fn in (e._lib.pf_tree_root, e._lib.pf_tree_root_device):
            for (b, m, k), text in (((1, 1, 2), "tree root needs N >= 3 sequences (got 2)"),
                                    ((1, 1, 8193), "tree root takes at most 8192 sequences (got 8193)"),
                                    ((1, 1, 65537), "tree root takes at most 8192 sequences (got 65537)"),
                                    ((0, 1, n), "tree root needs B >= 1 sources (got 0)"),
                                    ((1, 0, n), "tree root needs M >= 1 trees per source (got 0)")):
                assert fn(e._h, *ins, b, m, k, *ptrs) == -1
                assert e._lib.pf_last_error(e._h).decode() == text
            for hole in range(6):
                args = [*ins, *ptrs]
                args[hole] = None
                assert fn(e._h, *args[:2], 1, 1, n, *args[2:]) == -1
                assert e._lib.pf_last_error(e._h).decode() == "null buffer"
        e.set_option("ws_limit_mb", 1)
        # 600 sequences: 1,198 x 600 + 600 x 600 doubles, 8.67 MB of state for one tree
        assert e._lib.pf_tree_root(e._h, *ins, 1, 1, 600, *ptrs) == -1
        text = e._lib.pf_last_error(e._h).decode()
        assert "tree root of N=600 sequences needs 8668760 bytes" in text and "above the workspace limit of 1048576 bytes" in text
        e.set_option("ws_limit_mb", 24 << 10)
        assert e.profile_get("tree_root")[0] == 2 and all((a == a.flat[0]).all() for a in out)
        assert same(e.tree_root(slots, lengths), hostio.tree_root_host(slots, lengths))      # the handle still works
        e.profile_reset()
        assert e.profile_get("tree_root")[0] == 0


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
    got = e.tree_root(slots, lengths)
    assert got[3].tolist() == [0, 0, 0]
    for k in range(3):
        assert same(tuple(x[k] for x in got), R.tree_root_py(slots[k], lengths[k], 20))
        s = R.root_scores(slots[k], lengths[k], got[0][k], got[1][k], got[2][k], 20)
        assert 0 < s.ambiguity <= 1 and 0 <= s.root_pos <= s.root_length and s.mad > 0 and s.mid_diameter > 0


def _cli(repo, args):
    return subprocess.run([sys.executable, os.path.join(repo, "infer_alns.py"), *args], capture_output=True, text=True, cwd=repo)


def test_cli_end_to_end_on_two_test_alignments(repo, tmp_path, engines):
    """``infer_alns.py -t --bme --bionj --root mad``: per written kind ``<stem>[.<kind>].rooted.nwk`` is the kind's tree with a root of
    two children - RF 0 to the kind's own text -, ``<stem>.root.tsv`` holds ``root_scores`` of the written tables, and every other
    output keeps the bytes of a run without the flag."""
    from helpers.fit_inputs import kind_table
    from phyloformer_amd.treecmp import parse_newick, robinson_foulds
    ind = tmp_path / "in"
    ind.mkdir()
    stems = ("0_20_tips", "0_30_tips")
    for stem in stems:
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    ckpt = os.path.join(repo, "models/pf.ckpt")
    r = _cli(repo, [ckpt, str(ind), "-o", str(tmp_path / "root"), "-t", "--bme", "--bionj", "--root", "mad", "--bench"])
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stderr.strip().splitlines()[-1])
    assert stats["root"] == 2 and stats["root_s"] > 0
    plain = _cli(repo, [ckpt, str(ind), "-o", str(tmp_path / "plain"), "-t", "--bme", "--bionj"])
    assert plain.returncode == 0, plain.stderr
    files = {n: (tmp_path / "root" / n).read_bytes() for n in sorted(os.listdir(tmp_path / "root"))}
    base = {n: (tmp_path / "plain" / n).read_bytes() for n in sorted(os.listdir(tmp_path / "plain"))}
    kinds = ["nj", "bme", "bionj", "bionj.bme"]
    added = {f"{s}.root.tsv" for s in stems} | {f"{s}.{'' if k == 'nj' else k + '.'}rooted.nwk" for s in stems for k in kinds}
    assert set(files) == set(base) | added and all(files[n] == base[n] for n in base)
    for stem in stems:
        idx, ids = fasta.load_alignment(str(ind / f"{stem}.fa"))
        pred = engines("pf").forward(idx)
        text = files[f"{stem}.root.tsv"].decode()
        assert text.startswith(R.ROOT_HEAD) and list(R.parse_root_tsv(text)) == kinds
        for row, k in zip(text.splitlines(keepends=True)[1:], kinds):
            slots, lengths = kind_table(k, pred)
            s = R.root_scores(slots, lengths, *hostio.tree_root_host(slots, lengths)[:3], len(ids))
            assert row == R.root_line(k, "mad", s, ids)
            prefix = "" if k == "nj" else k + "."
            assert files[f"{stem}.{prefix}rooted.nwk"].decode() == R.rooted_newick(ids, slots, lengths, s.root_k, s.root_pos)
            rooted, own = (parse_newick(files[f"{stem}.{name}"].decode()) for name in (f"{prefix}rooted.nwk", f"{k}.nwk"))
            assert robinson_foulds(rooted, own) == (0, 0.0)
