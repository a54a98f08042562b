"""-m gpu: BIONJ on the device - pf_bionj_joins against pf_bionj_joins_host (the same bodies run serially, themselves
pinned to bionj.py in tests/test_bionj_native.py), bit for bit (slots equal, lengths equal as uint64); the sources of a
call are independent; chunks under a workspace budget; the entry point on device arrays and the call counter; the
non-finite flag; duplicated rows; the refinements of the device's table; and the CLI end to end."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.bionj_table import assert_table, assert_tables_equal, duplicated_rows, uniform
from helpers.nj_table import tie_cases
from phyloformer_amd import bionj, hostio
from phyloformer_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _same(a, b):
    assert_tables_equal(a, b)
    assert np.array_equal(a[2], b[2])


# no join; the under-8 sums; eight accumulators; the recursive split of both sums on the way down from 137; 300: more
# rows than one workgroup of the minima has threads, and 256 partial minima for the pick and the join to reduce
@pytest.mark.parametrize("N", [3, 4, 9, 137, 300])
def test_joins_equal_the_host_twin_bit_for_bit_and_sources_are_independent(engines, N):
    e = engines("pf")
    preds = uniform(N, 2600 + N, 2)
    want = hostio.bionj_joins_host(preds)
    got = e.bionj_joins(preds)
    assert got[0].shape == got[1].shape == (2, 2 * (N - 3) + 3) and got[0].dtype == np.int32 and got[1].dtype == np.float64
    assert got[2].tolist() == [False, False]
    _same(got, want)
    if N <= 137:                                     # (the statement itself: seconds at 300)
        assert_table(got[0][0], got[1][0], preds[0], N)
    alone = e.bionj_joins(preds[1])
    _same(alone, (want[0][1], want[1][1], want[2][1]))


def test_duplicated_rows_all_equal_distances_and_negative_zeros(engines):
    """The window with more than one pair in it, and v_ab = 0 (lambda = 1/2)."""
    n = 23
    preds = np.concatenate([tie_cases(n), duplicated_rows(n, 7)[None, :]])
    got = engines("pf").bionj_joins(preds)
    assert not got[2].any()
    _same(got, hostio.bionj_joins_host(preds))
    for b in range(len(preds)):
        assert_table(got[0][b], got[1][b], preds[b], n)


def test_chunks_under_a_workspace_budget_give_the_same_bits(weights):
    """N = 200: 640 KB of matrices per source, so ws_limit_mb = 1 runs the three sources one after the other; one
    source of 300 no longer fits it, and the refusal names its bytes."""
    preds = uniform(200, 2651, 3)
    with Engine(weights("pf"), 0) as e:
        whole = e.bionj_joins(preds)
        e.set_option("ws_limit_mb", 1)
        chunked = e.bionj_joins(preds)
        _same(whole, chunked)
        with pytest.raises(ValueError, match=r"BIONJ of N=300 sequences needs \d+ bytes of state per source \(2 N\^2 doubles\), "
                                             r"above the workspace limit of 1048576 bytes"):
            e.bionj_joins(uniform(300, 1))
    _same(whole, hostio.bionj_joins_host(preds))


def test_device_entry_point_and_call_counter(weights):
    B, N = 2, 37
    T = 2 * (N - 3) + 3
    preds = uniform(N, 2637, B)
    with Engine(weights("pf"), 0) as e:
        e.profile_reset()
        want = e.bionj_joins(preds)
        assert e.profile_get("bionj_joins")[0] == 1 and e.profile_get("nj_joins")[0] == 0
        slots, lengths, flag = np.empty((B, T), np.int32), np.empty((B, T), np.float64), np.full(B, 7, np.uint8)
        bufs = [e.malloc(a.nbytes) for a in (preds, slots, lengths, flag)]
        try:
            e.h2d(bufs[0], preds)
            e.bionj_joins_device(bufs[0], B, N, bufs[1], bufs[2], bufs[3])
            e.bionj_joins_device(bufs[0], B, N, bufs[1], bufs[2], bufs[3])
            for host, dev in zip((slots, lengths, flag), bufs[1:]):
                e.d2h(host, dev)
            e.synchronize()
        finally:
            for ptr in bufs:
                e.free(ptr)
        assert e.profile_get("bionj_joins")[0] == 3
        _same((slots, lengths, flag.astype(bool)), want)
        nj = e.nj_joins(preds)                       # the two joiners share their state's buffer: one after the other
        _same(e.bionj_joins(preds), want)
        assert not np.array_equal(nj[0], want[0])
        e.profile_reset()
        assert e.profile_get("bionj_joins")[0] == 0
    _same(want, hostio.bionj_joins_host(preds))


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_flags_that_source_only(engines, bad):
    N = 40
    preds = uniform(N, 2640, 3)
    want = hostio.bionj_joins_host(preds)
    dirty = preds.copy()
    dirty[1, 333] = bad
    slots, lengths, flag = engines("pf").bionj_joins(dirty)
    assert flag.tolist() == [False, True, False]
    for b in (0, 2):
        assert_tables_equal((slots[b], lengths[b]), (want[0][b], want[1][b]))


def test_refusals(weights):
    preds = uniform(9, 9)
    T = 2 * (9 - 3) + 3
    slots, lengths, flag = np.full(T, -7, np.int32), np.full(T, -7.0), np.full(1, 7, np.uint8)
    with Engine(weights("pf"), 0) as e:
        lib, h = e._lib, e._h
        p, s, l, f = preds.ctypes.data, slots.ctypes.data, lengths.ctypes.data, flag.ctypes.data

        def refused(rc, text):
            assert rc == -1 and text.encode() in lib.pf_last_error(h), (rc, lib.pf_last_error(h))
            assert (slots == -7).all() and (lengths == -7.0).all() and flag[0] == 7

        for fn in (lib.pf_bionj_joins, lib.pf_bionj_joins_device):
            refused(fn(h, p, 1, 2, s, l, f), "BIONJ needs N >= 3 sequences (got 2)")
            refused(fn(h, p, 0, 9, s, l, f), "bad dimensions B=0 N=9")
            refused(fn(h, None, 1, 9, s, l, f), "null buffer")
            refused(fn(h, p, 1, 9, None, l, f), "null buffer")
            refused(fn(h, p, 1, 9, s, None, f), "null buffer")
            refused(fn(h, p, 1, 9, s, l, None), "null buffer")
            refused(fn(h, p, 1, 65537, s, l, f), "their 2147516416 pairs each overflow a distance vector")
            refused(fn(h, p, 1, 60000, s, l, f), "(2 N^2 doubles), above the workspace limit of 25769803776 bytes (option ws_limit_mb)")
        assert e.profile_get("bionj_joins")[0] == 0
        got = e.bionj_joins(preds[0])                # the handle still works
    assert_table(got[0], got[1], preds[0], 9)


def test_refinements_of_the_devices_table_equal_the_host_chain(engines):
    """Engine.bionj_joins -> Engine.bme_nni / Engine.bme_spr against pf_bionj_joins_host -> pf_bme_nni_host /
    pf_bme_spr_host at N = 65."""
    e = engines("pf")
    preds = uniform(65, 2665, 2)
    start = e.bionj_joins(preds)[0]
    host_start = hostio.bionj_joins_host(preds)[0]
    assert np.array_equal(start, host_start)
    for device, host in ((e.bme_nni, hostio.bme_nni_host), (e.bme_spr, hostio.bme_spr_host)):
        got, want = device(preds, start), host(preds, host_start)
        assert_tables_equal(got, want)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[4], want[4]) and got[2].sum() > 0
        assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))


def _cli(repo, args):
    return subprocess.run([sys.executable, os.path.join(repo, "infer_alns.py"), *args], capture_output=True, text=True, cwd=repo)


def test_cli_end_to_end_on_the_20_test_alignments(repo, tmp_path, engines):
    """``infer_alns.py -t --bionj`` on the shipped alignments: ``<stem>.bionj.nwk`` is byte-identical to ``--python-io``'s,
    every other file keeps its bytes, and the tree has RF 0 to FastME ``-m I`` of the GPU distances of an earlier run
    (tests/golden/fastme_bionj.json) where this run's distances give the same PHYLIP text, else to ``bionj.py`` of this
    run's own distances."""
    from phyloformer_amd import fasta, treecmp
    msas = os.path.join(repo, "data/testdata/msas")
    ckpt = os.path.join(repo, "models/pf.ckpt")
    native, python, plain = tmp_path / "native", tmp_path / "python", tmp_path / "plain"
    r = _cli(repo, [ckpt, msas, "-o", str(native), "-t", "--bionj", "--bench"])
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stderr.strip().splitlines()[-1])
    assert stats["bionj"] == 20 and stats["bionj_device"] == 0
    r = _cli(repo, [ckpt, msas, "-o", str(python), "-t", "--bionj", "--python-io"])
    assert r.returncode == 0, r.stderr
    r = _cli(repo, [ckpt, msas, "-o", str(plain), "-t"])
    assert r.returncode == 0, r.stderr
    with open(os.path.join(repo, "tests", "golden", "fastme_bionj.json")) as fh:
        trees = json.load(fh)
    stems = sorted(f[:-3] for f in os.listdir(msas))
    assert sorted(os.listdir(native)) == sorted(f"{s}.{x}" for s in stems for x in ("phy", "nj.nwk", "bionj.nwk"))
    assert sorted(os.listdir(plain)) == sorted(f"{s}.{x}" for s in stems for x in ("phy", "nj.nwk"))
    keyed = 0
    for stem in stems:
        for suffix in ("phy", "nj.nwk"):
            assert open(native / f"{stem}.{suffix}", "rb").read() == open(plain / f"{stem}.{suffix}", "rb").read()
        text = open(native / f"{stem}.bionj.nwk", "rb").read()
        assert text == open(python / f"{stem}.bionj.nwk", "rb").read(), stem
        phy = open(native / f"{stem}.phy", "rb").read()
        mine = treecmp.parse_newick(text.decode())
        entry = trees.get(hashlib.sha256(phy).hexdigest())
        if entry is not None and entry["source"].startswith("gpu_distances_r02"):
            keyed += 1
            ref = treecmp.parse_newick(entry["bionj"])
        else:
            # the run's own distances: the same forward in this process (the PHYLIP text says that they are the same)
            idx, ids = fasta.load_alignment(os.path.join(msas, f"{stem}.fa"))
            vec = engines("pf").forward(idx[None])[0]
            assert hostio.format_phylip(vec, ids) == phy, stem
            ref = treecmp.parse_newick(bionj.bionj_newick_py(vec, ids))
        assert treecmp.robinson_foulds(ref, mine)[0] == 0, stem
    print("files whose distances are those of the recorded run:", keyed, "of 20")


def test_cli_tile_takes_the_device_path_with_the_hosts_bytes(repo, tmp_path, monkeypatch):
    """A file of 300 sequences x 32 sites under ``--tile 200 -t --bionj --bme``: with ``BIONJ_DEVICE_MIN`` at 256 the
    BIONJ tree is joined and refined on the GPU thread, and ``<stem>.bionj.nwk`` and ``<stem>.bionj.bme.nwk`` - like every
    other file - have the bytes of the run with the device path off.  (``--spr`` takes the same branch:
    tests/test_bionj_cli_host.py; its host search of 300 sequences would take this test's seconds alone.)  In one process, so that the constant can be set."""
    import infer_alns
    ind = tmp_path / "in"
    ind.mkdir()
    rng = np.random.default_rng(300)
    base = rng.integers(0, 20, size=32)
    alpha = "ARNDCQEGHILKMFPSTWYV"
    with open(ind / "big.fa", "w") as fh:
        for k in range(300):
            row = np.where(rng.random(32) < 0.3, rng.integers(0, 20, size=32), base)
            fh.write(f">s{k}\n{''.join(alpha[int(v)] for v in row)}\n")
    outs = {}
    for name, minimum in (("host", None), ("device", 256)):
        monkeypatch.setattr(bionj, "BIONJ_DEVICE_MIN", minimum)
        out = tmp_path / name
        seen = []
        real = __import__("phyloformer_amd.scheduler", fromlist=["x"]).DirectoryRunner.book
        monkeypatch.setattr("phyloformer_amd.scheduler.DirectoryRunner.book",
                            lambda self, _real=real, _seen=seen, **kw: (_seen.append(kw), _real(self, **kw))[1])
        assert infer_alns.main([os.path.join(repo, "models/pf.ckpt"), str(ind), "-o", str(out), "-t", "--bionj", "--bme",
                                "--tile", "200", "--gpu-streams", "1"]) == 0
        monkeypatch.setattr("phyloformer_amd.scheduler.DirectoryRunner.book", real)
        outs[name] = {f: open(out / f, "rb").read() for f in sorted(os.listdir(out))}
        device = sum(kw.get("bionj_device", 0) for kw in seen)
        assert device == (1 if minimum else 0) and sum(kw.get("bionj", 0) for kw in seen) == 1
    assert outs["host"] == outs["device"]
    assert {"big.bionj.nwk", "big.bionj.bme.nwk", "big.bme.nwk", "big.nj.nwk"} <= set(outs["host"])
    assert outs["host"]["big.bionj.nwk"] != outs["host"]["big.nj.nwk"]
    assert outs["host"]["big.bionj.bme.nwk"] != outs["host"]["big.bionj.nwk"]
