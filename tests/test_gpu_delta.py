"""-m gpu: delta scores on the device - pf_delta and pf_delta_device against pf_delta_host (every quartet once, serially;
itself pinned to delta.py in tests/test_delta_host.py), all three arrays bit for bit; the sources of a call are
independent; two runs give the same bytes; the design without atomics on the pair sums gives the same integers; the refusals and the call
counter; Engine.delta on the engine's own distances against the statement; and the CLI end to end."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers.delta_inputs import check_delta_files, mixed, pairs_of, small_integers, uniform
from phyloformer_amd import delta as D
from phyloformer_amd import fasta, hostio
from phyloformer_amd.engine import Engine

pytestmark = pytest.mark.gpu

_inputs = {}


def sources(n, b):
    """The sources of a shape and the host twin's arrays for every K, computed once: b = 3 is a random source, a
    non-finite one and one of small integers with ties."""
    if (n, b) not in _inputs:
        preds = mixed(n, 4000 + n, b) if b == 3 else uniform(n, 4000 + n, b)
        _inputs[n, b] = preds, {k: hostio.delta_host(preds, bins=k) for k in (1, 20, 64)}
    return _inputs[n, b]


def same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype and x.shape == y.shape for x, y in zip(a, b))


def on_device(e, preds, n, bins):
    """pf_delta_device on device arrays, filled with a pattern first."""
    b = len(preds)
    out = (np.empty((b, pairs_of(n)), np.int64), np.empty((b, bins), np.int64), np.empty(b, np.uint8))
    bufs = [e.malloc(a.nbytes) for a in (preds, *out)]
    try:
        e.h2d(bufs[0], preds)
        for host, dev in zip(out, bufs[1:]):
            e.h2d(dev, np.full(host.shape, 0x55, dtype=host.dtype))
        e.delta_device(bufs[0], b, n, bins, *bufs[1:])
        for host, dev in zip(out, bufs[1:]):
            e.d2h(host, dev)
        e.synchronize()
    finally:
        for p in bufs:
            e.free(p)
    return out


# one quartet; one partial wave; the 64 / 65 edge of a wave on the partner loop (2,016 and 2,080 pairs: 8 passes of a
# workgroup and a ninth); 130: up to 33 passes, rows of the triangle longer and shorter than a pass
@pytest.mark.parametrize("bins", [1, 20, 64])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n", [4, 5, 31, 64, 65, 130])
def test_both_entry_points_equal_the_host_twin_bit_for_bit(engines, n, b, bins):
    e = engines("pf")
    preds, want = sources(n, b)
    got = e.delta(preds, bins=bins)
    assert same(got, want[bins])
    assert same(on_device(e, preds, n, bins), want[bins])
    if b == 3:
        assert got[2].tolist() == [0, 1, 0] and not got[0][1].any() and not got[1][1].any()
        assert got[1][0].sum() == got[1][2].sum() > 0                          # the neighbours are untouched
        assert n < 31 or (got[0][0].any() and got[0][2].any() and got[1][2][0] > 0 and got[1][2][-1] > 0)     # ties present


def test_small_integer_matrices_with_many_ties(engines):
    for n, top in ((9, 2), (33, 3), (70, 5)):
        preds = small_integers(n, 4100 + n, 2, top)
        assert same(engines("pf").delta(preds), hostio.delta_host(preds))


def test_a_batch_equals_single_calls_and_runs_repeat(engines):
    e = engines("pf")
    n = 31
    preds, want = sources(n, 3)
    whole = e.delta(preds)
    again = e.delta(preds)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(whole, again))
    for k in range(3):
        one = e.delta(preds[k])
        assert same(one, tuple(x[k] for x in whole))
        assert same(e.delta(preds[k:k + 1]), tuple(x[k:k + 1] for x in whole))


def test_the_design_without_atomics_on_the_pair_sums_gives_the_same_integers(weights):
    with Engine(weights("pf"), 0) as e:
        e.set_option("delta_atomic", 0)
        for n, b in ((4, 1), (5, 3), (65, 3), (130, 1)):
            preds, want = sources(n, b)
            assert same(e.delta(preds, bins=20), want[20])
            assert same(on_device(e, preds, n, 64), want[64])


def test_refusals_and_call_counter(weights):
    p6 = np.ones((1, 6), dtype=np.float32)
    with Engine(weights("pf"), 0) as e:
        e.profile_reset()
        assert e.profile_get("delta")[0] == 0
        e.delta(p6)
        on_device(e, p6, 4, 20)
        assert e.profile_get("delta")[0] == 2
        # the binding's own checks say the same as the library's
        with pytest.raises(ValueError, match=r"delta scores take 4 <= N <= 2048 sequences \(got 3\)"):
            e.delta(np.ones(3, dtype=np.float32))
        with pytest.raises(ValueError, match=r"delta scores take 1 <= K <= 64 bins \(got 65\)"):
            e.delta(p6, bins=65)
        # the library, before any device work: nothing counted, nothing written
        out = (np.full((1, 6), -7, np.int64), np.full((1, 20), -7, np.int64), np.full(1, 9, np.uint8))
        ptrs = [a.ctypes.data for a in out]
        for fn in (e._lib.pf_delta, e._lib.pf_delta_device):
            for (b, n, k), text in (((1, 3, 20), "delta scores take 4 <= N <= 2048 sequences (got 3)"),
                                    ((1, 2049, 20), "delta scores take 4 <= N <= 2048 sequences (got 2049)"),
                                    ((0, 4, 20), "bad dimensions B=0 N=4"),
                                    ((1, 4, 0), "delta scores take 1 <= K <= 64 bins (got 0)"),
                                    ((1, 4, 65), "delta scores take 1 <= K <= 64 bins (got 65)")):
                assert fn(e._h, p6.ctypes.data, b, n, k, *ptrs) == -1
                assert e._lib.pf_last_error(e._h).decode() == text
            for hole in range(4):
                args = [p6.ctypes.data, *ptrs]
                args[hole] = None
                assert fn(e._h, args[0], 1, 4, 20, *args[1:]) == -1
                assert e._lib.pf_last_error(e._h).decode() == "null buffer"
        assert e.profile_get("delta")[0] == 2 and all((a == a.flat[0]).all() for a in out)
        assert same(e.delta(p6), hostio.delta_host(p6))             # the handle still works
        e.profile_reset()
        assert e.profile_get("delta")[0] == 0


def test_engine_delta_of_the_engines_own_distances_equals_the_statement(engines, repo):
    e = engines("pf")
    idx, _ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas/0_20_tips.fa"))
    pred = e.forward(idx)
    got = e.delta(pred)
    assert same(got, D.delta_py(pred, 20))
    s = D.delta_scores(got[0], got[1], 20)
    assert 0 < s.overall < 0.5 and s.quartets == 4845


def _cli(repo, args):
    return subprocess.run([sys.executable, os.path.join(repo, "infer_alns.py"), *args], capture_output=True, text=True, cwd=repo)


def test_cli_end_to_end_on_two_test_alignments(repo, tmp_path, engines):
    """``infer_alns.py -t --delta``: the three files hold the statement's values for the engine's distances, ``.phy`` and
    ``.nj.nwk`` keep the bytes of a run without the flag."""
    from phyloformer_amd.phylip import vec_to_phylip
    ind = tmp_path / "in"
    ind.mkdir()
    stems = ("0_20_tips", "0_30_tips")
    for stem in stems:
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    ckpt = os.path.join(repo, "models/pf.ckpt")
    r = _cli(repo, [ckpt, str(ind), "-o", str(tmp_path / "delta"), "-t", "--delta", "--bench"])
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stderr.strip().splitlines()[-1])
    assert stats["delta"] == 2 and stats["delta_s"] > 0
    plain = _cli(repo, [ckpt, str(ind), "-o", str(tmp_path / "plain"), "-t"])
    assert plain.returncode == 0, plain.stderr
    files = {n: (tmp_path / "delta" / n).read_bytes() for n in sorted(os.listdir(tmp_path / "delta"))}
    base = {n: (tmp_path / "plain" / n).read_bytes() for n in sorted(os.listdir(tmp_path / "plain"))}
    assert set(files) == set(base) | {f"{s}.delta.{k}" for s in stems for k in ("tsv", "phy", "hist.tsv")}
    assert all(files[n] == base[n] for n in base) and {f"{s}.phy" for s in stems} <= set(base)
    for stem in stems:
        idx, ids = fasta.load_alignment(str(ind / f"{stem}.fa"))
        pred = engines("pf").forward(idx)
        assert files[f"{stem}.phy"].decode() == vec_to_phylip(pred, ids)[1]
        check_delta_files(files, stem, pred, ids)
