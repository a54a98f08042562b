"""-m gpu: per-taxon transfer counts on the device (``pf_join_transfers``, ``pf_join_transfers_device``) against their
serial twin (``pf_join_transfers_host``: the same bodies without a device) - every result is an integer and every
comparison equality - and the CLI's ``--instability`` end to end."""
import os
import shutil

import numpy as np
import pytest

from helpers import bme_check as bc
from helpers import support_inputs as si
from helpers import transfer_inputs as ti
from phyloformer_amd import bme, hostio, supports

pytestmark = pytest.mark.gpu


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


# 4: one split; 5, 17: fewer splits than a tile, and more than one tile; 64 / 65: the word boundary and a one-bit tail;
# 129: three words; 300: five words, and more splits than a 256-thread workgroup, so that a thread walks more than one j
# and more than one sequence
@pytest.mark.parametrize("r", [1, 5])
@pytest.mark.parametrize("n", [4, 5, 17, 64, 65, 129, 300])
def test_device_equals_the_serial_twin(engines, n, r):
    eng = eng_of(engines)
    ref, reps, flag = si.sources(n, r)
    plain = eng.join_supports(ref, reps, flag)
    for cutoff in ti.CUTOFFS:
        want = hostio.join_transfers_host(ref, reps, flag, cutoff)
        eng.profile_reset()
        got = eng.join_transfers(ref, reps, flag, cutoff)
        assert eng.profile_get("join_transfers")[0] == 1 and eng.profile_get("join_supports")[0] == 0
        ti.assert_same(got, want)
        assert not got[7].any()
        without = eng.join_transfers(ref, reps, flag, cutoff, branch_moves=False)
        assert without[6] is None
        ti.assert_same(without[:6] + without[7:], want[:6] + want[7:])
        ti.assert_same(got[:3] + got[7:], plain)                # (pf_join_supports' three arrays and its status)
    if r > 1:                                                   # (the reference itself is among source 0's replicates)
        assert got[4][0].min() >= 1
        assert got[3].any() or n < 17                           # (the comparison is not one of zeros)
    one = eng.join_transfers(ref[1], reps[1], flag[1], 30)       # B = 1: the same integers
    ti.assert_same(one, [w[1] for w in hostio.join_transfers_host(ref, reps, flag, 30)])
    ti.assert_same(eng.join_supports(ref, reps, flag), plain)    # (and pf_join_supports after it)
    ti.assert_same(plain, hostio.join_supports_host(ref, reps, flag))


def test_chunks_of_replicates_under_a_small_workspace_limit(engines):
    """``ws_limit_mb = 1``, N = 300, R = 100: a source's 101 bitset tables of 13,080 bytes and its deltas and keys exceed
    the limit, so every source runs alone in chunks of replicates - the counts accumulate from chunk to chunk; the result
    is the unchunked one.  A reference and one replicate of 2,100 sequences are refused with the bytes in the message."""
    eng = eng_of(engines)
    n, r = 300, 100
    ref, noisy = si.noisy_tables(n, 5)
    reps = random_tables(n, 2 * r, 300).reshape(2, r, -1)
    reps[0, 10:15] = noisy
    reps[1, 80] = ref
    flag = np.zeros((2, r), dtype=bool)
    flag[0, 75] = flag[1, 3] = True
    refs = np.stack([ref, ref])
    want = hostio.join_transfers_host(refs, reps, flag, 30)
    whole = eng.join_transfers(refs, reps, flag, 30)
    eng.set_option("ws_limit_mb", 1)
    try:
        chunked = eng.join_transfers(refs, reps, flag, 30)
        big = bc.caterpillar_slots(2100)
        with pytest.raises(ValueError, match=r"transfer counts of N=2100 sequences needs \d+ bytes of state per source"):
            eng.join_transfers(big[None, :], big[None, None, :], branch_moves=False)
    finally:
        eng.set_option("ws_limit_mb", 24 << 10)
    ti.assert_same(whole, want)
    ti.assert_same(chunked, want)
    assert want[3].any() and want[4].max() > want[4].min() and want[5].sum() == 0 and want[4][1].min() >= 1


def test_device_arrays_and_tables_that_are_none(engines):
    """``pf_join_transfers_device``: three sources; the reference of the first names slot ``N``, a replicate of the
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
    want = hostio.join_transfers_host(ref[2], reps[2], flag[2], 100)
    outs, _ptrs = hostio.transfer_outputs(b, n)
    for a in outs:
        a[...] = 77                                             # (every element is written)
    ptrs = [eng.malloc(a.nbytes) for a in (ref, reps, flag, *outs)]
    try:
        for p, a in zip(ptrs, (ref, reps, flag, *outs)):
            eng.h2d(p, a)
        eng.join_transfers_device(ptrs[0], ptrs[1], ptrs[2], b, r, n, 100, *ptrs[3:])
        eng.synchronize()
        for a, p in zip(outs, ptrs[3:]):
            eng.d2h(a, p)
    finally:
        for p in ptrs:
            eng.free(p)
    assert outs[7].tolist() == [1, 1, 0]
    for a in outs[:7]:
        assert not a[:2].any()
    ti.assert_same([a[2] for a in outs], want)


def test_host_entry_refusals(engines):
    eng = eng_of(engines)
    n = 9
    ref, reps, flag = si.sources(n, 5)
    bad = reps.copy()
    bad[0, 1, 3] = n
    with pytest.raises(ValueError, match="not a join table"):
        eng.join_transfers(ref, bad, flag)
    bad = ref.copy()
    bad[1, 0] = -1
    with pytest.raises(ValueError, match="not a join table"):
        eng.join_transfers(bad, reps, flag)
    for cutoff in (-1, 101):
        with pytest.raises(ValueError, match="cutoff is a percent from 0 to 100"):
            eng.join_transfers(ref, reps, flag, cutoff)
    ti.assert_same(eng.join_transfers(ref, reps, flag), hostio.join_transfers_host(ref, reps, flag))


def test_cli_instability_end_to_end(repo, tmp_path, monkeypatch):
    """``-t --bme --bootstrap 8 --seed 1 --tbe --bootstrap-refined`` on two shipped 20-tip files: with ``--instability``
    every earlier file - ``.sup.nwk`` and ``.tbe.nwk`` among them - keeps its bytes, the six new files per alignment are
    there, and with the device thresholds lowered, so that ``pf_join_transfers`` counts on the GPU thread, they are the
    files of the host path."""
    import infer_alns
    ind = tmp_path / "in"
    ind.mkdir()
    stems = ("0_20_tips", "1_20_tips")
    for stem in stems:
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    ckpt = os.path.join(repo, "models/pf.ckpt")
    base = [ckpt, str(ind), "-t", "--bme", "--bootstrap", "8", "--seed", "1", "--tbe", "--bootstrap-refined", "--gpu-streams", "1"]
    monkeypatch.setattr(supports, "TRANSFER_DEVICE_MIN", None)
    assert infer_alns.main(base + ["-o", str(tmp_path / "plain")]) == 0
    assert infer_alns.main(base + ["--instability", "-o", str(tmp_path / "host")]) == 0
    booked = []
    real = __import__("phyloformer_amd.scheduler", fromlist=["x"]).DirectoryRunner.book
    monkeypatch.setattr("phyloformer_amd.scheduler.DirectoryRunner.book",
                        lambda self, _real=real, **kw: (booked.append(kw), _real(self, **kw))[1])
    monkeypatch.setattr(bme, "BME_DEVICE_MIN", 4)
    monkeypatch.setattr(supports, "TRANSFER_DEVICE_MIN", 4)
    assert infer_alns.main(base + ["--instability", "-o", str(tmp_path / "device")]) == 0
    monkeypatch.undo()
    assert sum(kw.get("transfers_device", 0) for kw in booked) == 4 and sum(kw.get("instability", 0) for kw in booked) == 4
    plain, host, device = ({f: open(tmp_path / d / f, "rb").read() for f in sorted(os.listdir(tmp_path / d))}
                           for d in ("plain", "host", "device"))
    added = [x for k in ("nj", "bme") for x in supports.INSTABILITY_SUFFIXES[k]]
    assert sorted(host) == sorted(list(plain) + [f"{s}.{x}" for s in stems for x in added])
    assert all(host[f] == plain[f] for f in plain)
    assert device == host
    rows = [line.split("\t") for line in host["0_20_tips.instability.tsv"].decode().splitlines()]
    assert rows[0] == ["id", "moves", "permille"] and len(rows) == 21
    assert len(host["0_20_tips.branches.tsv"].decode().splitlines()) == 18
