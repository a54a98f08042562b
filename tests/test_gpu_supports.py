"""-m gpu: split supports of join tables on the device (``pf_join_supports``, ``pf_join_supports_device``) against their
serial twin (``pf_join_supports_host``: the same bodies without a device) - every result is an integer and every
comparison equality - and the CLI's ``--tbe`` / ``--bootstrap-refined`` end to end."""
import os
import shutil

import numpy as np
import pytest

from helpers import bme_check as bc
from helpers import support_inputs as si
from phyloformer_amd import bme, hostio, supports

pytestmark = pytest.mark.gpu


def assert_same(got, want):
    for name, g, w in zip(("count", "transfer", "depth", "status"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(g, w), name


def eng_of(engines):
    from phyloformer_amd import build
    build.build()
    return engines()


def random_tables(n: int, r: int, seed: int) -> np.ndarray:
    """``int32 [r][T]``: valid join tables of random joins (no distances behind them)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((r, 2 * (n - 3) + 3), dtype=np.int32)
    for k in range(r):
        alive = list(range(n))
        for t in range(n - 3):
            i, j = sorted(rng.choice(len(alive), size=2, replace=False).tolist())
            out[k, 2 * t], out[k, 2 * t + 1] = alive[i], alive[j]
            alive.pop(j)
        out[k, 2 * (n - 3):] = alive
    return out


# 64 / 65: the word boundary and a one-bit tail; 137: three words; 300: more splits than a 256-thread workgroup and more
# than one tile of reference splits
@pytest.mark.parametrize("r", [1, 5])
@pytest.mark.parametrize("n", [4, 5, 9, 64, 65, 137, 300])
def test_device_equals_the_serial_twin(engines, n, r):
    eng = eng_of(engines)
    ref, reps, flag = si.sources(n, r)
    want = hostio.join_supports_host(ref, reps, flag)
    eng.profile_reset()
    got = eng.join_supports(ref, reps, flag)
    assert eng.profile_get("join_supports")[0] == 1
    assert_same(got, want)
    assert not got[3].any()
    if r > 1:                                                   # (the reference itself is among source 0's replicates)
        assert got[0][0].min() >= 1 and got[0][1].max() <= r - 1
    one = eng.join_supports(ref[1], reps[1], flag[1])            # B = 1: the same integers
    assert_same(one, [w[1] for w in want])


def test_chunks_of_replicates_under_a_small_workspace_limit(engines):
    """``ws_limit_mb = 1``, N = 300, R = 100: a source's 101 bitset tables of 13,080 bytes and its deltas take
    1,441,472 bytes, so every source runs alone in two chunks of 72 and 28 replicates; the result is the unchunked
    one.  A reference and one replicate of 2,100 sequences (two tables of 562,008 bytes) are refused with the bytes in
    the message."""
    eng = eng_of(engines)
    n, r = 300, 100
    ref, noisy = si.noisy_tables(n, 5)
    reps = random_tables(n, 2 * r, 300).reshape(2, r, -1)
    reps[0, 10:15] = noisy
    reps[1, 80] = ref
    flag = np.zeros((2, r), dtype=bool)
    flag[0, 75] = flag[1, 3] = True
    refs = np.stack([ref, ref])
    want = hostio.join_supports_host(refs, reps, flag)
    whole = eng.join_supports(refs, reps, flag)
    eng.set_option("ws_limit_mb", 1)
    try:
        chunked = eng.join_supports(refs, reps, flag)
        big = bc.caterpillar_slots(2100)
        with pytest.raises(ValueError, match=r"split supports of N=2100 sequences needs \d+ bytes of state per source"):
            eng.join_supports(big[None, :], big[None, None, :])
    finally:
        eng.set_option("ws_limit_mb", 24 << 10)
    assert_same(whole, want)
    assert_same(chunked, want)
    assert want[0][1].max() >= 1 and 0 < want[1][0].min()


def test_device_arrays_and_tables_that_are_none(engines):
    """``pf_join_supports_device``: three sources; the reference of the first names slot ``N``, a replicate of the
    second slot ``-1`` - the kernel's own check gives them status 1 and zeros - and the third has the twin's results."""
    eng = eng_of(engines)
    n, r, b = 65, 5, 3
    ref2, reps2, _flag = si.sources(n, r)
    ref = np.stack([ref2[0], ref2[0], ref2[1]])
    reps = np.stack([reps2[0], reps2[0], reps2[1]])
    flag = np.zeros((b, r), dtype=np.uint8)
    flag[2, r - 1] = 1
    ref[0, 7] = n
    reps[1, 2, 40] = -1
    want = hostio.join_supports_host(ref[2], reps[2], flag[2])
    s = n - 3
    outs = [np.zeros((b, s), np.int32), np.zeros((b, s), np.int64), np.zeros((b, s), np.int32), np.zeros(b, np.uint8)]
    ptrs = [eng.malloc(a.nbytes) for a in (ref, reps, flag, *outs)]
    try:
        for p, a in zip(ptrs, (ref, reps, flag)):
            eng.h2d(p, a)
        eng.join_supports_device(ptrs[0], ptrs[1], ptrs[2], b, r, n, *ptrs[3:])
        eng.synchronize()
        for a, p in zip(outs, ptrs[3:]):
            eng.d2h(a, p)
    finally:
        for p in ptrs:
            eng.free(p)
    assert outs[3].tolist() == [1, 1, 0]
    for a in outs[:3]:
        assert not a[:2].any()
    assert_same([a[2] for a in outs], want)


def test_host_entry_refusals(engines):
    eng = eng_of(engines)
    n = 9
    ref, reps, flag = si.sources(n, 5)
    bad = reps.copy()
    bad[0, 1, 3] = n
    with pytest.raises(ValueError, match="not a join table"):
        eng.join_supports(ref, bad, flag)
    bad = ref.copy()
    bad[1, 0] = -1
    with pytest.raises(ValueError, match="not a join table"):
        eng.join_supports(bad, reps, flag)
    assert_same(eng.join_supports(ref, reps, flag), hostio.join_supports_host(ref, reps, flag))


def _inputs(repo, tmp_path):
    ind = tmp_path / "in"
    ind.mkdir()
    for stem in ("0_20_tips", "1_20_tips"):
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    return ind


@pytest.mark.parametrize("lowered", [False, True])
def test_cli_tbe_and_refined_supports(repo, tmp_path, monkeypatch, lowered):
    """``-t --bme --spr --bootstrap 8 --seed 1 --tbe --bootstrap-refined`` on two shipped 20-tip files: ``.sup.nwk``,
    ``.bme.nwk``, ``.spr.nwk``, ``.nj.nwk`` and ``.phy`` keep the bytes of a run without the two new flags, and the five
    new files are ``supports.support_newicks`` of the Python twins on the run's own distances.  Once as it is (20
    sequences: the host twins on the writer threads) and once with the three device thresholds lowered, so that the
    replicate refinements and the matching run on the GPU thread."""
    import infer_alns
    from phyloformer_amd import fasta
    from phyloformer_amd.engine import Engine
    ind = _inputs(repo, tmp_path)
    ckpt = os.path.join(repo, "models/pf.ckpt")
    base = [ckpt, str(ind), "-t", "--bme", "--spr", "--bootstrap", "8", "--seed", "1", "--gpu-streams", "1"]
    assert infer_alns.main(base + ["-o", str(tmp_path / "plain")]) == 0
    if lowered:
        monkeypatch.setattr(bme, "BME_DEVICE_MIN", 4)
        monkeypatch.setattr(bme, "SPR_DEVICE_MIN", 4)
        monkeypatch.setattr(supports, "SUPPORT_DEVICE_MIN", 4)
    booked, forwards, boots = [], [], []
    real = __import__("phyloformer_amd.scheduler", fromlist=["x"]).DirectoryRunner.book
    monkeypatch.setattr("phyloformer_amd.scheduler.DirectoryRunner.book",
                        lambda self, _real=real, **kw: (booked.append(kw), _real(self, **kw))[1])
    # the run's own distances, as its engine returned them: what the Python twins are given below
    fwd, boot = Engine.forward, Engine.bootstrap
    monkeypatch.setattr(Engine, "forward", lambda self, idx: (forwards.append((np.array(idx), fwd(self, idx))), forwards[-1][1])[1])
    monkeypatch.setattr(Engine, "bootstrap", lambda self, idx, r, seed=0: (boots.append((np.array(idx), boot(self, idx, r, seed))), boots[-1][1])[1])
    assert infer_alns.main(base + ["--tbe", "--bootstrap-refined", "-o", str(tmp_path / "new")]) == 0
    monkeypatch.undo()
    device = sum(kw.get("supports_device", 0) for kw in booked)
    assert device == (6 if lowered else 0)                      # (two files, three kinds of tree)
    assert sum(kw.get("tbe", 0) for kw in booked) == 6 and sum(kw.get("refined_supports", 0) for kw in booked) == 4
    plain = {f: open(tmp_path / "plain" / f, "rb").read() for f in sorted(os.listdir(tmp_path / "plain"))}
    new = {f: open(tmp_path / "new" / f, "rb").read() for f in sorted(os.listdir(tmp_path / "new"))}
    stems = ("0_20_tips", "1_20_tips")
    added = ("tbe.nwk", "bme.sup.nwk", "bme.tbe.nwk", "spr.sup.nwk", "spr.tbe.nwk")
    assert sorted(plain) == sorted(f"{s}.{x}" for s in stems for x in ("phy", "nj.nwk", "sup.nwk", "bme.nwk", "spr.nwk"))
    assert sorted(new) == sorted(list(plain) + [f"{s}.{x}" for s in stems for x in added])
    for f in plain:
        assert new[f] == plain[f], f

    def row_of(calls, idx):
        return next(out[b] for batch, out in calls for b in range(len(batch)) if np.array_equal(batch[b], idx))
    for stem in stems:
        idx, ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"))
        want = supports.support_newicks(row_of(forwards, idx), row_of(boots, idx), ids, kinds=("nj", "bme", "spr"), tbe=True)
        assert want["sup.nwk"].encode() == new[f"{stem}.sup.nwk"]
        for suffix in added:
            assert new[f"{stem}.{suffix}"] == want[suffix].encode(), (stem, suffix)
        assert new[f"{stem}.tbe.nwk"] != new[f"{stem}.sup.nwk"]
