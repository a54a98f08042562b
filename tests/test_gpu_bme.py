"""-m gpu: balanced NNI refinement on the device (``pf_bme_nni``, ``pf_bme_nni_device``) against its serial twin
(``pf_bme_nni_host``: the same bodies without a device) - slots, steps and status equal, lengths and tree length equal
as uint64 - and the CLI's ``--bme`` end to end."""
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


def bad_case(n):
    """Two sources and starts far from their optimum: the caterpillar on the path lengths of a random tree (hundreds of
    moves at 137); at 300 - where the serial twin would take a minute from there - the NJ table of noisy distances."""
    if n <= 137:
        return np.stack([bc.random_tree_distances(n, s) for s in (1, 2)]), np.stack([bc.caterpillar_slots(n)] * 2)
    preds = bc.uniform_preds(n, n, 2)
    return preds, np.stack([bc.noisy_start(p, n, 7) for p in preds])


# 65: beyond one wave; 137: the recursive split of the sums; 300: beyond a 256-thread workgroup and the sequence cap
@pytest.mark.parametrize("n", [3, 4, 5, 9, 65, 137, 300])
def test_device_equals_the_serial_twin(engines, n):
    eng = eng_of(engines)
    preds = bc.uniform_preds(n, n * 100 + 256, 2)
    nj_slots, _lengths, nonfinite = eng.nj_joins(preds)
    assert not nonfinite.any()
    eng.profile_reset()
    got = eng.bme_nni(preds, nj_slots)
    assert eng.profile_get("bme_nni")[0] == 1
    assert_same(got, hostio.bme_nni_host(preds, nj_slots))
    assert not got[4].any() and (n < 65 or got[2].min() >= 1)
    preds, starts = bad_case(n)
    got = eng.bme_nni(preds, starts)
    assert_same(got, hostio.bme_nni_host(preds, starts))
    assert not got[4].any()
    if n in (65, 137):
        assert got[2].min() > 32                                   # more than one round
    print(n, "steps", got[2])


def eng_of(engines):
    from phyloformer_amd import build
    build.build()
    return engines()


def test_chunks_under_a_small_workspace_limit(engines):
    """``ws_limit_mb = 1``: four sources of 65 sequences fit side by side, six run in two chunks; 300 are refused, with
    the bytes in the message."""
    eng = eng_of(engines)
    n = 65
    preds = np.concatenate([bc.uniform_preds(n, 1, 3), np.stack([bc.random_tree_distances(n, s) for s in (1, 2, 3)])])
    starts = np.stack([bc.caterpillar_slots(n)] * 6)
    want = hostio.bme_nni_host(preds, starts)
    eng.set_option("ws_limit_mb", 1)
    try:
        assert_same(eng.bme_nni(preds, starts), want)
        with pytest.raises(ValueError, match="5060568 bytes of state per source"):
            eng.bme_nni(bc.uniform_preds(300, 1, 1), bc.caterpillar_slots(300)[None, :])
    finally:
        eng.set_option("ws_limit_mb", 24 << 10)
    assert_same(eng.bme_nni(preds, starts), want)


def test_device_arrays(engines):
    eng = eng_of(engines)
    n, b = 17, 3
    t = 2 * (n - 3) + 3
    preds = np.stack([bc.random_tree_distances(n, s) for s in (1, 2, 3)])
    starts = np.stack([bc.caterpillar_slots(n)] * b)
    want = hostio.bme_nni_host(preds, starts)
    sizes = [preds.nbytes, starts.nbytes, b * t * 4, b * t * 8, b * 4, b * 8, b]
    ptrs = [eng.malloc(s) for s in sizes]
    try:
        eng.h2d(ptrs[0], preds)
        eng.h2d(ptrs[1], starts)
        eng.bme_nni_device(ptrs[0], ptrs[1], b, n, *ptrs[2:])
        got = [np.zeros((b, t), np.int32), np.zeros((b, t), np.float64), np.zeros(b, np.int32), np.zeros(b, np.float64), np.zeros(b, np.uint8)]
        for arr, p in zip(got, ptrs[2:]):
            eng.d2h(arr, p)
    finally:
        for p in ptrs:
            eng.free(p)
    assert_same(got, want)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_source_next_to_a_finite_one(engines, bad):
    eng = eng_of(engines)
    n = 9
    preds = bc.uniform_preds(n, 9, 3)
    preds[1, 17] = bad
    starts = np.stack([bc.caterpillar_slots(n)] * 3)
    got = eng.bme_nni(preds, starts)
    assert got[4].tolist() == [0, 1, 0]
    assert_same(got, hostio.bme_nni_host(preds, starts))


def test_a_from_scratch_table_resumes_the_search(engines):
    """``bme_check.star_tie_preds``: the input on which the serial driver reports from-scratch tables that resumed the
    search (tests/test_bme_native.py asserts that it does); the device walks the same way."""
    eng = eng_of(engines)
    n = 40
    vec = bc.star_tie_preds(n, 2)[None, :]
    start = bc.caterpillar_slots(n)[None, :]
    got = eng.bme_nni(vec, start)
    assert_same(got, hostio.bme_nni_host(vec, start))
    assert got[4][0] == 0 and got[2][0] >= 2


def test_refusals(engines):
    eng = eng_of(engines)
    n = 6
    preds = bc.uniform_preds(n, 6, 1)
    good = bc.caterpillar_slots(n)[None, :]
    for k, v in ((0, n), (0, -1), (3, 1), (8, 0)):
        bad = good.copy()
        bad[0, k] = v
        with pytest.raises(ValueError, match="start table"):
            eng.bme_nni(preds, bad)
    with pytest.raises(ValueError, match="N >= 3"):
        eng.bme_nni(np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int32))
    assert_same(eng.bme_nni(preds, good), hostio.bme_nni_host(preds, good))


def _cli(repo, args):
    return subprocess.run([sys.executable, os.path.join(repo, "infer_alns.py"), *args], capture_output=True, text=True, cwd=repo)


def test_cli_bme_end_to_end(repo, tmp_path, golden):
    """``infer_alns.py -t --bme`` on two shipped alignments: ``<stem>.bme.nwk`` has the topology of FastME ``-m N -n B``
    on the reference's distances of the same file.  tests/test_cli_gpu.py grants GPU-versus-reference distances 1 % of
    the splits; of these two files' 2 * (37 + 37) that is less than one split, so RF 0 is what applies - and what the
    GPU distances of an earlier run (tests/golden/gpu_distances_r02.npz) give on the CPU for both files."""
    from phyloformer_amd import fasta, treecmp
    from phyloformer_amd.phylip import vec_to_matrix
    ind, outd, plain = tmp_path / "in", tmp_path / "out", tmp_path / "plain"
    ind.mkdir()
    stems = ("0_40_tips", "3_40_tips")
    for stem in stems:
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    r = _cli(repo, [os.path.join(repo, "models/pf.ckpt"), str(ind), "-o", str(outd), "-t", "--bme", "--bench"])
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stderr.strip().splitlines()[-1])
    assert stats["bme"] == 2 and stats["bme_steps"] >= 1 and stats["bme_device"] == 0
    r = _cli(repo, [os.path.join(repo, "models/pf.ckpt"), str(ind), "-o", str(plain), "-t"])
    assert r.returncode == 0, r.stderr
    with open(os.path.join(repo, "tests", "golden", "fastme_nj_bnni.json")) as fh:
        trees = json.load(fh)
    gold = golden("e2e_testdata.npz")
    rf, total = 0, 0
    for stem in stems:
        for suffix in ("phy", "nj.nwk"):
            assert open(outd / f"{stem}.{suffix}", "rb").read() == open(plain / f"{stem}.{suffix}", "rb").read()
        _idx, ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"))
        n = len(ids)
        dm = vec_to_matrix(gold[f"pf/{stem}"], n).astype(np.float64)
        key = hashlib.sha256(hostio.format_phylip(dm[np.triu_indices(n, 1)], ids)).hexdigest()
        mine = treecmp.parse_newick(open(outd / f"{stem}.bme.nwk").read())
        rf += treecmp.robinson_foulds(treecmp.parse_newick(trees[key]["tree"]), mine)[0]
        total += 2 * (n - 3)
    assert sorted(os.listdir(plain)) == sorted(f"{s}.{x}" for s in stems for x in ("phy", "nj.nwk"))
    print("RF summed over the two trees:", rf, "of", total, "splits")
    assert rf <= int(0.01 * total)


def test_cli_tile_takes_the_device_path_with_the_hosts_bytes(repo, tmp_path, monkeypatch):
    """A file of 300 sequences x 32 sites under ``--tile 200 -t --bme``: with ``BME_DEVICE_MIN`` at 256 the tree is
    refined on the GPU thread, and ``<stem>.bme.nwk`` - like every other file - has the bytes of the run with the
    device path off.  In one process, so that the constant can be set."""
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
        monkeypatch.setattr(bme, "BME_DEVICE_MIN", minimum)
        out = tmp_path / name
        seen = []
        real = __import__("phyloformer_amd.scheduler", fromlist=["x"]).DirectoryRunner.book
        monkeypatch.setattr("phyloformer_amd.scheduler.DirectoryRunner.book",
                            lambda self, _real=real, _seen=seen, **kw: (_seen.append(kw), _real(self, **kw))[1])
        assert infer_alns.main([os.path.join(repo, "models/pf.ckpt"), str(ind), "-o", str(out), "-t", "--bme", "--tile", "200",
                                "--gpu-streams", "1"]) == 0
        monkeypatch.setattr("phyloformer_amd.scheduler.DirectoryRunner.book", real)
        outs[name] = {f: open(out / f, "rb").read() for f in sorted(os.listdir(out))}
        device = sum(kw.get("bme_device", 0) for kw in seen)
        assert device == (1 if minimum else 0) and sum(kw.get("bme", 0) for kw in seen) == 1
    assert outs["host"] == outs["device"] and "big.bme.nwk" in outs["host"]
    assert outs["host"]["big.bme.nwk"] != outs["host"]["big.nj.nwk"]
