"""-m gpu: distances between join tables on the device (``pf_join_distances``, ``pf_join_distances_device``) against their
serial twin (``pf_join_distances_host``: the same bodies without a device) - integers equal, doubles bit for bit - and the
engine's own tables against the statement."""
import os

import numpy as np
import pytest

from helpers import treedist_inputs as ti
from phyloformer_amd import bme, hostio, treedist

pytestmark = pytest.mark.gpu


def eng_of(engines):
    from phyloformer_amd import build
    build.build()
    return engines()


def device_form(eng, slots, lengths, flag):
    """``pf_join_distances_device`` on copies of the arrays: ``(shared, kf, wrf, status)``."""
    b, k, t = slots.shape
    n = (t + 3) // 2
    ins = [np.ascontiguousarray(slots, dtype=np.int32), np.ascontiguousarray(lengths, dtype=np.float64),
           np.ascontiguousarray(flag, dtype=np.uint8)]
    outs = [np.full((b, k, k), 7, np.int32), np.full((b, k, k), 7.0), np.full((b, k, k), 7.0), np.full(b, 7, np.uint8)]
    ptrs = [eng.malloc(a.nbytes) for a in ins + outs]
    try:
        for p, a in zip(ptrs, ins + outs):
            eng.h2d(p, a)
        eng.join_distances_device(*ptrs[:3], b, k, n, *ptrs[3:])
        eng.synchronize()
        for a, p in zip(outs, ptrs[3:]):
            eng.d2h(a, p)
    finally:
        for p in ptrs:
            eng.free(p)
    return tuple(outs)


# 64 / 65 / 67: the word boundary, and N - 3 = 61 / 62 / 64 against the 64 accumulators; 130: three words, more than one
# round of every lane
@pytest.mark.parametrize("k", [1, 2, 3, 33])
@pytest.mark.parametrize("n", [4, 5, 64, 65, 67, 130])
def test_both_device_forms_equal_the_serial_twin(engines, n, k):
    eng = eng_of(engines)
    slots, lengths = (np.stack([a, a[::-1]]) for a in ti.mixed(n, k))
    flag = np.zeros((2, k), dtype=bool)
    if k > 2:
        flag[1, 1] = True
        slots[1, 1] = np.iinfo(np.int32).min                    # (never read)
    want = hostio.join_distances_host(slots, lengths, flag)
    assert not want[3].any() and (want[0][0] >= 0).all()
    eng.profile_reset()
    assert ti.same(eng.join_distances(slots, lengths, flag), want)
    assert ti.same(device_form(eng, slots, lengths, flag), want)
    assert eng.profile_get("join_distances")[0] == 2
    only = eng.join_distances(slots[0], None, None)               # one source, no lengths
    assert only[1] is None and only[2] is None and np.array_equal(only[0], want[0][0]) and only[3] == 0


def test_identical_trees_every_slot_claimed_once(engines):
    eng = eng_of(engines)
    n, k = 130, 33
    slots, lengths = ti.mixed(n, 1)
    slots, lengths = np.repeat(slots, k, axis=0), np.repeat(lengths, k, axis=0)
    got = eng.join_distances(slots, lengths)
    assert ti.same(got, hostio.join_distances_host(slots, lengths))
    assert (got[0] == n - 3).all() and not got[1].any() and not got[2].any()


def test_unrelated_trees_the_table_at_its_fullest(engines):
    eng = eng_of(engines)
    n, k = 130, 33
    slots = ti.random_tables(n, k, 131)
    lengths = np.random.default_rng(3).standard_normal(slots.shape)
    got = eng.join_distances(slots, lengths)
    assert ti.same(got, hostio.join_distances_host(slots, lengths))
    off = got[0][~np.eye(k, dtype=bool)]
    assert off.max() < (n - 3) // 4 and (got[1][~np.eye(k, dtype=bool)] > 0).all()


def test_three_sources_equal_three_calls_and_chunks_under_a_small_limit(engines):
    """``ws_limit_mb = 1``, N = 130, K = 33: a source's state (about 0.4 MB) fits twice, so three sources run in chunks of
    two and one; a source of 300 trees of 300 sequences is refused with the bytes in the message."""
    eng = eng_of(engines)
    n, k = 130, 33
    slots = np.stack([ti.mixed(n, k)[0], ti.random_tables(n, k, 7), np.repeat(ti.mixed(n, 1)[0], k, axis=0)])
    lengths = np.random.default_rng(4).standard_normal(slots.shape)
    flag = np.zeros((3, k), dtype=bool)
    flag[1, 0] = flag[1, 32] = True
    want = hostio.join_distances_host(slots, lengths, flag)
    whole = eng.join_distances(slots, lengths, flag)
    singles = [eng.join_distances(slots[b], lengths[b], flag[b]) for b in range(3)]
    assert 2 * treedist_state_bytes(n, k) <= 1 << 20 < 3 * treedist_state_bytes(n, k)
    eng.set_option("ws_limit_mb", 1)
    try:
        chunked = eng.join_distances(slots, lengths, flag)
        with pytest.raises(ValueError, match=r"tree distances of K=300 trees of N=300 sequences need \d+ bytes of state per source"):
            eng.join_distances(np.stack([bme.caterpillar_slots(300)] * 300))
    finally:
        eng.set_option("ws_limit_mb", 24 << 10)
    assert ti.same(whole, want) and ti.same(chunked, want)
    assert ti.same(tuple(np.stack([s[x] for s in singles]) for x in range(4)), want)
    assert (want[0][1, 0] == -1).all() and np.isnan(want[1][1, :, 32]).all()


def treedist_state_bytes(n: int, k: int) -> int:
    """``pftd::state_bytes`` restated: every array padded to 8 bytes."""
    s, w, e = n - 3, (n + 63) // 64, k * (n - 3)
    cap = 2
    while cap < 2 * e:
        cap *= 2
    up = lambda x: (x + 7) // 8 * 8
    return (8 * e * w + 8 * e + 2 * up(4 * k * n) + 6 * up(4 * e) + 2 * up(4 * cap) + 8)


def test_device_arrays_with_tables_that_are_none(engines):
    eng = eng_of(engines)
    n, k = 65, 5
    base, lens = ti.mixed(n, k)
    slots, lengths = np.stack([base] * 4), np.stack([lens] * 4)
    slots[1, 2, 7] = n
    slots[2, 4, 40] = -1
    flag = np.zeros((4, k), dtype=np.uint8)
    got = device_form(eng, slots, lengths, flag)
    want = hostio.join_distances_host(base, lens)
    assert got[3].tolist() == [0, 1, 1, 0]
    for b in (1, 2):
        assert not got[0][b].any() and not got[1][b].any() and not got[2][b].any()
    for b in (0, 3):
        assert ti.same(tuple(a[b] for a in got), want)
    assert ti.same(got, hostio.join_distances_host(slots, lengths, flag))


def test_every_refusal(engines):
    eng = eng_of(engines)
    slots, lengths = ti.mixed(9, 3)
    bad = slots.copy()
    bad[1, 3] = 9
    with pytest.raises(ValueError, match="not a join table"):
        eng.join_distances(bad, lengths)
    d = eng.malloc(1 << 12)
    try:
        for args, text in (((1, 3, 3), "N >= 4"), ((1, 3, 16385), "at most 16384"), ((0, 3, 9), "B=0"), ((1, 0, 9), "K >= 1"),
                           ((1, 4097, 9), "at most 4096 trees"), ((1, 4096, 16384), r"need \d+ bytes of state per source")):
            with pytest.raises(ValueError, match=text):
                eng.join_distances_device(d, d, d, *args, d, d, d, d)
        for nulls in ((0,), (3,), (6,), (4,), (5,)):
            ptrs = [0 if x in nulls else d for x in range(7)]
            with pytest.raises(ValueError, match="null buffer"):
                eng.join_distances_device(*ptrs[:3], 1, 3, 9, *ptrs[3:])
    finally:
        eng.free(d)


@pytest.mark.parametrize("stem", ["0_20_tips", "3_50_tips"])
def test_the_engines_own_tables_against_the_statement(engines, repo, stem):
    from phyloformer_amd import fasta
    eng = eng_of(engines)
    idx, ids = fasta.load_alignment(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"))
    preds = eng.forward(np.asarray(idx)[None])
    nj, nj_len, bad = eng.nj_joins(preds)
    bj, bj_len, bad2 = eng.bionj_joins(preds)
    assert not bad.any() and not bad2.any()
    nni = eng.bme_nni(preds, nj)
    spr = eng.bme_spr(preds, nj)
    slots = np.stack([nj[0], bj[0], nni[0][0], spr[0][0]])
    lengths = np.stack([nj_len[0], bj_len[0], nni[1][0], spr[1][0]])
    got = eng.join_distances(slots, lengths)
    want = treedist.join_distances_py(slots, lengths, None, len(ids))
    assert ti.same(got, (want.shared, want.kf, want.wrf, np.uint8(0)))


@pytest.mark.parametrize("lowered", [False, True])
def test_cli_treedist(repo, tmp_path, monkeypatch, lowered):
    """``-t --bme --bionj --treedist-ref data/testdata/trees --bootstrap 5 --tbe`` on three shipped files, as it is and with the
    device thresholds lowered to 4 (the GPU thread's calls): the bytes of the ``--python-io`` run, where the statement itself
    computes the distances; every file of a run without the flag keeps its bytes."""
    import shutil

    import infer_alns
    from phyloformer_amd import bionj, supports
    stems = ("0_20_tips", "1_30_tips", "2_40_tips")
    ind = tmp_path / "in"
    ind.mkdir()
    for stem in stems:
        shutil.copy(os.path.join(repo, "data/testdata/msas", f"{stem}.fa"), ind / f"{stem}.fa")
    base = [os.path.join(repo, "models/pf.ckpt"), str(ind), "-t", "--bme", "--bionj", "--bootstrap", "5", "--seed", "1", "--tbe",
            "--gpu-streams", "1"]
    flag = ["--treedist-ref", os.path.join(repo, "data/testdata/trees")]
    assert infer_alns.main(base + ["-o", str(tmp_path / "plain")]) == 0
    assert infer_alns.main(base + flag + ["--python-io", "-o", str(tmp_path / "python")]) == 0
    for mod, name in ((bme, "BME_DEVICE_MIN"), (bionj, "BIONJ_DEVICE_MIN"), (supports, "SUPPORT_DEVICE_MIN"),
                      (treedist, "TREEDIST_DEVICE_MIN"), (treedist, "TREEDIST_REPS_DEVICE_MIN")):
        if lowered:
            monkeypatch.setattr(mod, name, 4)
    eng_calls = []
    from phyloformer_amd.engine import Engine
    real = Engine.join_distances
    monkeypatch.setattr(Engine, "join_distances", lambda self, *a, _real=real, **kw: (eng_calls.append(1), _real(self, *a, **kw))[1])
    assert infer_alns.main(base + flag + ["-o", str(tmp_path / "new")]) == 0
    monkeypatch.undo()
    if lowered:
        assert len(eng_calls) == 6                                # (three shapes: the kinds' call and the replicates' call each)
    read = lambda d: {f: open(tmp_path / d / f, "rb").read() for f in sorted(os.listdir(tmp_path / d))}
    plain, python, new = read("plain"), read("python"), read("new")
    added = [f"{s}.treedist.{x}" for s in stems for x in ("tsv", "reps.tsv", "rf.phy")]
    assert sorted(new) == sorted(list(plain) + added)
    for f in plain:
        assert new[f] == plain[f], f
    for f in added:
        assert new[f] == python[f], f
    rows = new["0_20_tips.treedist.tsv"].decode().splitlines()
    assert len(rows) == 1 + 10 and all(r.split("\t")[2] != "NA" for r in rows[1:])
