"""-m gpu: query placement on the device - the bit-identity of forward_place's whole, backbone and query sets with
forward of the host-built alignments where the three take different routes, the reductions against their float64 twin,
batch and chunk invariance, refusals, and the CLI's --place on two 20-tip test MSAs."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers.profiled import Profiled as _Profiled
from phyloformer_amd import place as PL
from phyloformer_amd.engine import Engine
from phyloformer_amd.msa_sim import simulate_batch
from phyloformer_amd.taxa import pair_index

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# device statistics against the float64 twin: at most P_N <= 19,900 terms accumulated in double and rounded to float once
# (below 2^-23 relative before the square root); 1e-6 leaves room for sqrt and the twin's own order of summation
RTOL, ATOL = 1e-6, 1e-12
# (M, Q, L): 9 x 300 - the backbone (7 rows: 21 x 300 = 6,300 pair-site tokens) takes the float64 route, the sets (8 rows:
# 8,400) and the whole (10,800) the default kernels; 5 x 33 - everything float64, and L % 4 != 0: the gather's byte paths
SHAPES = [(9, 2, 300), (5, 2, 33)]
NAMES = ("out", "base", "place", "disturb", "shift", "joint", "sets")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def placed(engines):
    """forward_place of B = 3 alignments at both shapes, computed once and left unchanged."""
    e = engines("pf")
    out = {}
    for M, Q, L in SHAPES:
        idx = simulate_batch(3, M, L, seed=300 + M)
        with _Profiled(e):
            res = e.forward_place(idx, Q, keep_sets=True)
            counts = {k: e.profile_get(k)[0] for k in ("main", "precise", "gather_taxa", "place_stats")}
        out[M] = (idx, res, counts)
    return out


@pytest.mark.parametrize("M,Q,L", SHAPES)
def test_place_bitwise_against_forward_of_host_built_alignments(engines, placed, M, Q, L):
    e = engines("pf")
    idx, (out, base, place, disturb, shift, joint, sets), counts = placed[M]
    N, B = M - Q, idx.shape[0]
    assert out.shape == (B, M * (M - 1) // 2) and base.shape == (B, N * (N - 1) // 2) and sets.shape == (B, Q, (N + 1) * N // 2)
    assert place.shape == (B, Q, N) and disturb.shape == shift.shape == joint.shape == (B, Q)
    assert all(a.dtype == np.float32 for a in (out, base, place, disturb, shift, joint, sets))
    assert np.array_equal(_bits(out), _bits(e.forward(idx)))
    assert np.array_equal(_bits(base), _bits(e.forward(np.ascontiguousarray(idx[:, :N]))))
    for b in range(B):
        for q in range(Q):
            assert np.array_equal(_bits(sets[b, q]), _bits(e.forward(PL.join_query(idx[b], N, q)))), (b, q)
            assert np.array_equal(_bits(place[b, q]), _bits(sets[b, q][[pair_index(i, N, N + 1) for i in range(N)]]))
    print(f"{M} x {L}, Q = {Q}: launches {counts}")
    assert counts["precise"] > 0 and counts["gather_taxa"] >= 3 and counts["place_stats"] >= 1
    assert (counts["main"] > 0) == (M == 9)
    assert disturb.min() > 0 and joint.min() > 0                  # context dependence: a query moves the others


@pytest.mark.parametrize("M,Q,L", SHAPES)
def test_place_statistics_against_the_twin(placed, M, Q, L):
    _idx, (out, base, place, disturb, shift, joint, sets), _counts = placed[M]
    want = PL.place_stats(out, base, sets, M - Q, Q)
    assert np.array_equal(_bits(place), _bits(want[0]))
    for got, w, name in zip((disturb, shift, joint), want[1:], ("disturb", "shift", "joint")):
        err = float(np.abs(got.astype(np.float64) - w).max())
        print(f"{M} x {L} {name}: max |device - twin| {err:.3e}, largest value {float(np.abs(w).max()):.3e}")
        assert np.allclose(got, w, rtol=RTOL, atol=ATOL), name


def _stats_device(e, whole, base, sets, B, N, Q):
    outs = [np.empty((B, Q, N), np.float32)] + [np.empty((B, Q), np.float32) for _ in range(3)]
    bufs = [e.malloc(a.nbytes) for a in (whole, base, sets, *outs)]
    try:
        for p, a in zip(bufs[:3], (whole, base, sets)):
            e.h2d(p, a)
        e.place_stats_device(*bufs[:3], B, N, Q, *bufs[3:])
        for a, p in zip(outs, bufs[3:]):
            e.d2h(a, p)
        e.synchronize()
    finally:
        for p in bufs:
            e.free(p)
    return outs


@pytest.mark.parametrize("B,N,Q", [(1, 2, 1), (2, 13, 3)])
def test_place_stats_device_on_hand_made_arrays(engines, B, N, Q):
    """N = 2, Q = 1: one backbone pair, the smallest case; N = 13: P_N = 78 > 64, so lanes take a second term."""
    e = engines("pf")
    rng = np.random.default_rng(N)
    M = N + Q
    whole = rng.uniform(0.05, 2.0, size=(B, M * (M - 1) // 2)).astype(np.float32)
    base = rng.uniform(0.05, 2.0, size=(B, N * (N - 1) // 2)).astype(np.float32)
    sets = rng.uniform(0.05, 2.0, size=(B, Q, (N + 1) * N // 2)).astype(np.float32)
    got = _stats_device(e, whole, base, sets, B, N, Q)
    want = PL.place_stats(whole, base, sets, N, Q)
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    for a, w, name in zip(got[1:], want[1:], ("disturb", "shift", "joint")):
        print(f"N={N} Q={Q} {name}: max |device - twin| {float(np.abs(a.astype(np.float64) - w).max()):.3e}")
        assert np.allclose(a, w, rtol=RTOL, atol=ATOL), name
    again = _stats_device(e, whole, base, sets, B, N, Q)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))


def test_place_batch_and_chunk_invariance_and_null_sets(weights, placed):
    """Alignment 1 of B = 3 against the same alignment alone, alone again under a workspace budget of 1 MB (one derived
    alignment per chunk: the Q sets take one gather each), and without `sets`."""
    idx, whole, _counts = placed[9]
    with Engine(weights("pf"), 0) as e:
        e.set_option("profile", 1)
        e.profile_reset()
        alone = e.forward_place(idx[1], 2, keep_sets=True)
        n_default = e.profile_get("gather_taxa")[0]
        without = e.forward_place(idx[1], 2)
        e.set_option("ws_limit_mb", 1)
        e.profile_reset()
        chunked = e.forward_place(idx[1], 2, keep_sets=True)
        n_chunked = e.profile_get("gather_taxa")[0]
    print(f"gather launches: {n_default} by default, {n_chunked} under ws_limit_mb = 1")
    assert n_default >= 3 and n_chunked > n_default         # (whole, backbone, sets: one gather each by default)
    for name, a, c, w in zip(NAMES, alone, chunked, whole):
        assert np.array_equal(_bits(a), _bits(w[1])), name
        assert np.array_equal(_bits(c), _bits(w[1])), name
    assert len(without) == 6 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(without, alone))


def test_place_refusals_leave_outputs_untouched(weights):
    idx = simulate_batch(1, 5, 33, seed=305)
    with Engine(weights("pf"), 0) as e:
        e.set_option("profile", 1)
        e.profile_reset()
        lib, h = e._lib, e._h
        bufs = [np.full(64, -7.0, np.float32) for _ in range(7)]        # out, base, sets, place, disturb, shift, joint
        ptr = [a.ctypes.data for a in bufs]

        def refused(rc, text):
            assert rc == -1 and text.encode() in lib.pf_last_error(h), lib.pf_last_error(h)
            assert all((a == -7.0).all() for a in bufs)

        refused(lib.pf_forward_place(h, idx.ctypes.data, 1, 5, 33, 0, *ptr), "Q >= 1")
        refused(lib.pf_forward_place(h, idx.ctypes.data, 1, 5, 33, 4, *ptr), "M - Q >= 2")
        bad = idx.copy()
        bad[0, 4, 32] = 22
        refused(lib.pf_forward_place(h, bad.ctypes.data, 1, 5, 33, 2, *ptr), "residue index 22")
        refused(lib.pf_forward_place(h, idx.ctypes.data, 1, 5, 33, 2, *ptr[:3], None, *ptr[4:]), "null buffer")
        assert all(e.profile_get(k)[0] == 0 for k in ("gather_taxa", "place_stats", "precise", "main"))
        with pytest.raises(ValueError, match="Q >= 1"):
            e.forward_place(idx, 0)
        with pytest.raises(ValueError, match="M - Q >= 2"):
            e.forward_place(idx, 4, keep_sets=True)
        # the handle still works, and the profile counts the reduction
        out = e.forward_place(idx, 2)
        assert np.array_equal(_bits(out[0]), _bits(e.forward(idx)))
        assert e.profile_get("place_stats")[0] == 1 and e.profile_get("gather_taxa")[0] == 3
        e.set_option("profile", 0)
        e.profile_reset()
        e.forward_place(idx, 2)
        assert e.profile_get("place_stats")[0] == 0


# ---- CLI on two 20-tip test MSAs -----------------------------------------------------------------------------------

def _run(args):
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, timeout=900)


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_cli_place_on_20_tip_msas(tmp_path, engines):
    from phyloformer_amd.fasta import load_alignment
    msas = tmp_path / "msas"
    msas.mkdir()
    stems = ["0_20_tips", "1_20_tips"]
    for s in stems:
        shutil.copy(os.path.join(REPO, "data", "testdata", "msas", f"{s}.fa"), msas / f"{s}.fa")
    plain = _run([str(msas), "-o", str(tmp_path / "plain"), "-t"])
    placed_run = _run([str(msas), "-o", str(tmp_path / "place"), "-t", "--place", "3"])
    assert plain.returncode == 0 and placed_run.returncode == 0, plain.stderr[-2000:] + placed_run.stderr[-2000:]
    p, w = _files(tmp_path / "plain"), _files(tmp_path / "place")
    assert set(w) == set(p) | {f"{s}.{ext}" for s in stems for ext in ("place.dist.tsv", "place.tsv", "placed.nwk")}
    for name, data in p.items():
        assert w[name] == data, name                           # <stem>.phy and <stem>.nj.nwk unchanged
    e = engines("pf_base")
    for s in stems:
        idx, ids = load_alignment(os.path.join(msas, f"{s}.fa"))
        _out, _base, place, disturb, shift, joint = e.forward_place(idx, 3)
        assert w[f"{s}.place.dist.tsv"].decode() == PL.place_dist_tsv(ids[:17], ids[17:], place)
        rows = [r.split("\t") for r in w[f"{s}.place.tsv"].decode().splitlines()]
        assert rows[0] == list(PL.TSV_COLUMNS + PL.TREE_COLUMNS) and len(rows) == 4
        for q, row in enumerate(rows[1:]):
            assert row[:2] == [str(17 + q), ids[17 + q]] and row[2] == ids[int(np.argmin(place[q]))]
            assert row[4:7] == [f"{float(v[q]):.10f}" for v in (disturb, shift, joint)]
            assert set(row[7].split("|")) < set(ids[:17]) and float(row[10]) >= 0
