"""-m gpu: majority-rule consensus trees on the device (``pf_join_consensus``, ``pf_join_consensus_device``) against their
serial twin (``pf_join_consensus_host``: the same bodies without a device) - integers equal, doubles bit for bit - and the
CLI's ``--consensus`` end to end."""
import os
import shutil

import numpy as np
import pytest

from helpers import bme_check as bc
from helpers import support_inputs as si
from phyloformer_amd import bme, consensus, hostio, supports

pytestmark = pytest.mark.gpu

NAMES = ("n_splits", "count", "size", "parent", "split_length", "leaf_parent", "leaf_length", "status")


def assert_same(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert (g is None) == (w is None), name
        if g is None:
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert g.tobytes() == w.tobytes(), name                 # (the doubles bit for bit)


def eng_of(engines):
    from phyloformer_amd import build
    build.build()
    return engines()


def random_tables(n: int, r: int, seed: int) -> np.ndarray:
    """``int32 [r][T]``: valid join tables of random joins (no distances behind them): unrelated trees."""
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


def lengths_of(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape)


# 64 / 65: the word boundary and a one-bit tail; 137: three words; 300: more splits than a 256-thread workgroup and more
# than one tile of selected splits
@pytest.mark.parametrize("r", [1, 5, 6])
@pytest.mark.parametrize("n", [4, 5, 9, 64, 65, 137, 300])
def test_device_equals_the_serial_twin(engines, n, r):
    eng = eng_of(engines)
    _ref, reps, flag = si.sources(n, r)
    lengths = lengths_of(reps.shape, 10 * n + r)
    want = hostio.join_consensus_host(reps, lengths, flag)
    eng.profile_reset()
    got = eng.join_consensus(reps, lengths, flag)
    assert eng.profile_get("join_consensus")[0] == 1
    assert_same(got, want)
    assert not got[7].any()
    if n >= 64 and r == 5:
        assert 0 < got[0][0] < n - 3 and got[0][1] == 0        # partial resolution beside the star
    one = eng.join_consensus(reps[1], lengths[1], flag[1])       # B = 1: the same results
    assert_same(one, [w[1] for w in want])
    assert_same(eng.join_consensus(reps, None, flag, 70), hostio.join_consensus_host(reps, None, flag, 70))


def test_identical_replicates_every_slot_claimed_once_and_hit_99_times(engines):
    eng = eng_of(engines)
    n, r = 300, 100
    ref, _noisy = si.noisy_tables(n, 5)
    reps = np.stack([ref] * r)[None]
    lengths = lengths_of(reps.shape, 7)
    got = eng.join_consensus(reps, lengths)
    assert_same(got, hostio.join_consensus_host(reps, lengths))
    assert got[0][0] == n - 3 and (got[1] == r).all()


def test_unrelated_replicates_the_table_at_its_fullest(engines):
    eng = eng_of(engines)
    n, r = 300, 100
    reps = random_tables(n, r, 301)[None]
    flag = np.zeros((1, r), dtype=bool)
    flag[0, 17] = True
    lengths = lengths_of(reps.shape, 8)
    got = eng.join_consensus(reps, lengths, flag)
    assert_same(got, hostio.join_consensus_host(reps, lengths, flag))
    assert got[0][0] == 0 and (got[5] == -1).all()
    distinct = len({s for tab, f in zip(reps[0], flag[0]) if not f for s in supports.table_splits(tab, n)})
    assert distinct > 0.9 * (r - 1) * (n - 3)                    # (nearly every split is its own slot)


def test_sources_side_by_side_under_a_small_workspace_limit(engines):
    """``ws_limit_mb = 1``, N = 137, R = 20: a source's state (about 276 KB) fits three times, so five sources run in two
    chunks of three and two; the result is the unchunked one.  A source of R = 100 replicates of 300 sequences (1.3 MB of
    bitset tables alone) is refused with the bytes in the message."""
    eng = eng_of(engines)
    n, r, b = 137, 20, 5
    reps = random_tables(n, b * r, 65).reshape(b, r, -1)
    _ref, noisy = si.noisy_tables(n, 5)
    reps[1, :15] = np.tile(noisy, (3, 1))                        # (a split of four of the five noisy trees: 12 of 20)
    reps[3, :] = noisy[0]
    flag = np.zeros((b, r), dtype=bool)
    flag[2, 5] = flag[4, 0] = True
    lengths = lengths_of(reps.shape, 9)
    want = hostio.join_consensus_host(reps, lengths, flag)
    whole = eng.join_consensus(reps, lengths, flag)
    eng.set_option("ws_limit_mb", 1)
    try:
        chunked = eng.join_consensus(reps, lengths, flag)
        big = np.stack([bc.caterpillar_slots(300)] * 100)[None]
        with pytest.raises(ValueError, match=r"consensus of R=100 replicates of N=300 sequences needs \d+ bytes of state per source"):
            eng.join_consensus(big)
    finally:
        eng.set_option("ws_limit_mb", 24 << 10)
    assert_same(whole, want)
    assert_same(chunked, want)
    assert want[0][3] == n - 3 and 0 < want[0][1] < n - 3


def test_device_arrays_and_tables_that_are_none(engines):
    """``pf_join_consensus_device``: three sources; a replicate of the first names slot ``N`` and another slot ``-1`` -
    the kernel's own check gives the source status 1 and zeros - and its neighbours have the twin's results."""
    eng = eng_of(engines)
    n, r, b = 65, 5, 3
    _ref, reps2, _flag = si.sources(n, r)
    reps = np.ascontiguousarray(np.stack([reps2[0], reps2[0], reps2[1]]))
    flag = np.zeros((b, r), dtype=np.uint8)
    flag[2, r - 1] = 1
    lengths = np.ascontiguousarray(lengths_of(reps.shape, 11))
    want = hostio.join_consensus_host(reps[1:], lengths[1:], flag[1:])
    reps[0, 1, 7] = n
    reps[0, 3, 40] = -1
    s = n - 3
    outs = [np.zeros(b, np.int32), np.zeros((b, s), np.int32), np.zeros((b, s), np.int32), np.zeros((b, s), np.int32),
            np.zeros((b, s), np.float64), np.zeros((b, n), np.int32), np.zeros((b, n), np.float64), np.zeros(b, np.uint8)]
    ptrs = [eng.malloc(a.nbytes) for a in (reps, lengths, flag, *outs)]
    try:
        for p, a in zip(ptrs, (reps, lengths, flag)):
            eng.h2d(p, a)
        eng.join_consensus_device(ptrs[0], ptrs[1], ptrs[2], b, r, n, 50, *ptrs[3:])
        eng.synchronize()
        for a, p in zip(outs, ptrs[3:]):
            eng.d2h(a, p)
    finally:
        for p in ptrs:
            eng.free(p)
    assert outs[7].tolist() == [1, 0, 0]
    for a in outs[:7]:
        assert not a[0].any()
    assert_same([a[1:] for a in outs], want)
    assert want[0][0] > 0


def test_host_entry_refusals(engines):
    eng = eng_of(engines)
    n = 9
    _ref, reps, flag = si.sources(n, 5)
    bad = reps.copy()
    bad[0, 1, 3] = n
    with pytest.raises(ValueError, match="not a join table"):
        eng.join_consensus(bad, None, flag)
    for percent in (49, 100):
        with pytest.raises(ValueError, match="percent from 50 to 99"):
            eng.join_consensus(reps, None, flag, percent)
    assert_same(eng.join_consensus(reps, None, flag), hostio.join_consensus_host(reps, None, flag))


def _inputs(repo, tmp_path):
    ind = tmp_path / "in"
    ind.mkdir()
    for stem in ("0_20_tips", "1_20_tips"):
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    return ind


@pytest.mark.parametrize("lowered", [False, True])
def test_cli_consensus(repo, tmp_path, monkeypatch, lowered):
    """``-t --bme --bootstrap 8 --seed 1 --bootstrap-refined --consensus`` on two shipped 20-tip files, as it is (the host
    twins on the writer threads) and with the device thresholds lowered to 4 (the GPU thread): the bytes of the
    ``--python-io`` run, where the statement itself writes the consensus; every file of a run without ``--consensus``
    keeps its bytes."""
    import infer_alns
    ind = _inputs(repo, tmp_path)
    ckpt = os.path.join(repo, "models/pf.ckpt")
    base = [ckpt, str(ind), "-t", "--bme", "--bootstrap", "8", "--seed", "1", "--bootstrap-refined", "--gpu-streams", "1"]
    assert infer_alns.main(base + ["-o", str(tmp_path / "plain")]) == 0
    assert infer_alns.main(base + ["--consensus", "--python-io", "-o", str(tmp_path / "python")]) == 0
    if lowered:
        monkeypatch.setattr(bme, "BME_DEVICE_MIN", 4)
        monkeypatch.setattr(supports, "SUPPORT_DEVICE_MIN", 4)
        monkeypatch.setattr(consensus, "CONSENSUS_DEVICE_MIN", 4)
    else:
        monkeypatch.setattr(consensus, "CONSENSUS_DEVICE_MIN", None)
    booked = []
    real = __import__("phyloformer_amd.scheduler", fromlist=["x"]).DirectoryRunner.book
    monkeypatch.setattr("phyloformer_amd.scheduler.DirectoryRunner.book",
                        lambda self, _real=real, **kw: (booked.append(kw), _real(self, **kw))[1])
    assert infer_alns.main(base + ["--consensus", "-o", str(tmp_path / "new")]) == 0
    monkeypatch.undo()
    assert sum(kw.get("consensus_device", 0) for kw in booked) == (4 if lowered else 0)      # (two files, two kinds of tree)
    assert sum(kw.get("consensus", 0) for kw in booked) == 4
    read = lambda d: {f: open(tmp_path / d / f, "rb").read() for f in sorted(os.listdir(tmp_path / d))}
    plain, python, new = read("plain"), read("python"), read("new")
    stems = ("0_20_tips", "1_20_tips")
    assert sorted(new) == sorted(list(plain) + [f"{s}.{x}" for s in stems for x in ("con.nwk", "bme.con.nwk")])
    for f in plain:
        assert new[f] == plain[f], f
    for s in stems:
        for x in ("con.nwk", "bme.con.nwk"):
            assert new[f"{s}.{x}"] == python[f"{s}.{x}"], (s, x)
            assert new[f"{s}.{x}"].count(b"(") >= 2 and new[f"{s}.{x}"].endswith(b");\n")
