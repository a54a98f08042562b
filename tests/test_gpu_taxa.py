"""-m gpu: the taxon axis on the device - k_gather_taxa's bytes, the bit-identity of forward_taxa with forward of the
host-cut alignments on every path, leave-one-out (distances, cuts, statistics), parity with the reference's own
outputs, refusals, and the CLI's --leave-one-out on the 20-tip test MSAs."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers.profiled import Profiled as _Profiled
from phyloformer_amd import taxa as T
from phyloformer_amd.engine import Engine
from phyloformer_amd.msa_sim import simulate_batch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2.0 ** -23, 1e-9          # device statistics against the float64 twin: one float rounding


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_taxa(e, idx, taxa):
    """forward_taxa against forward of cut_taxa, bit for bit; idx [B][N][L]."""
    B, _N, L = idx.shape
    S, M = np.asarray(taxa).shape
    got = e.forward_taxa(idx, taxa)
    want = e.forward(T.cut_taxa(idx, taxa).reshape(B * S, M, L)).reshape(B, S, -1)
    assert got.shape == want.shape == (B, S, M * (M - 1) // 2) and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want))
    return got


def _subsets(N, S, M, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.sort(rng.choice(N, size=M, replace=False)) for _ in range(S)]).astype(np.int32)


# ---- the gather alone ----------------------------------------------------------------------------------------------

def _gather(e, src, taxa, dst_offset=0):
    B, N, L = src.shape
    tab = np.ascontiguousarray(taxa, dtype=np.int32)
    S, M = tab.shape
    d_src, d_tab, d_dst = e.malloc(src.nbytes), e.malloc(tab.nbytes), e.malloc(B * S * M * L + dst_offset + 3)
    try:
        e.h2d(d_src, src)
        e.h2d(d_tab, tab)
        guard = np.full(B * S * M * L + dst_offset + 3, 0xA5, np.uint8)
        e.h2d(d_dst, guard)
        e.gather_taxa_device(d_src, B, N, L, d_tab, S, M, d_dst + dst_offset)
        e.d2h(guard, d_dst)
        e.synchronize()
    finally:
        for p in (d_src, d_tab, d_dst):
            e.free(p)
    # nothing outside dst was written (heads and tails are byte stores)
    assert (guard[:dst_offset] == 0xA5).all() and (guard[dst_offset + B * S * M * L:] == 0xA5).all()
    return guard[dst_offset:dst_offset + B * S * M * L].reshape(B, S, M, L)


@pytest.mark.parametrize("dst_offset", [0, 1])
@pytest.mark.parametrize("L", [1, 3, 4, 6, 7, 1023, 1024, 1029])
def test_gather_bytes_match_host_twin(engines, L, dst_offset):
    """Every L % 4 and the tile edge of 1,024 sites; rows of 5 sources L bytes apart, so source and destination rows
    take every alignment modulo 4; dst aligned and odd; a reversed row, a row with repeats and the identity."""
    e = engines("pf")
    rng = np.random.default_rng(L)
    B, N = 2, 5
    src = rng.integers(0, 22, size=(B, N, L), dtype=np.uint8)
    for M in (2, 4, 7):
        taxa = np.stack([np.arange(N - 1, N - 1 - M, -1) % N, rng.integers(0, 2, size=M) * 3, np.arange(M) % N])
        got = _gather(e, src, taxa, dst_offset)
        bad = int((got != T.cut_taxa(src, taxa)).sum())
        print(f"L={L} M={M} dst+{dst_offset}: {bad} wrong bytes")
        assert bad == 0


def test_gather_leave_one_out_table_200(engines):
    e = engines("pf")
    src = np.random.default_rng(5).integers(0, 22, size=(1, 200, 5), dtype=np.uint8)
    taxa = T.leave_one_out_sets(200)
    assert np.array_equal(_gather(e, src, taxa), T.cut_taxa(src, taxa))


def test_gather_device_table_out_of_range_is_reported_not_dereferenced(weights):
    src = np.arange(2 * 3 * 8, dtype=np.uint8).reshape(2, 3, 8) % 22
    with Engine(weights("pf"), 0) as e:
        with pytest.raises(ValueError, match="taxon table"):
            _gather(e, src, np.array([[1, 3], [0, 2]]))           # entry == N
        e.synchronize()                                           # reported once
        ok = np.array([[1, 2], [0, 2]])
        assert np.array_equal(_gather(e, src, ok), T.cut_taxa(src, ok))


# ---- bit identity with forward of the host-cut alignments ----------------------------------------------------------

def test_taxa_bitwise_default_kernels_row_tiling(engines):
    with _Profiled(engines("pf")) as e:
        got = _check_taxa(e, simulate_batch(1, 60, 128, seed=81), _subsets(60, 3, 40, 81))
        assert got.shape == (1, 3, 780)
        assert e.profile_get("main")[0] > 0 and e.profile_get("precise")[0] == 0 and e.profile_get("gather_taxa")[0] >= 1


def test_taxa_bitwise_default_kernels_flat_tiling(engines):
    with _Profiled(engines("pf")) as e:
        idx = simulate_batch(1, 20, 200, seed=82)
        taxa = np.concatenate([_subsets(20, 3, 12, 82), np.arange(11, -1, -1, dtype=np.int32)[None], np.arange(12, dtype=np.int32)[None] // 2])
        got = _check_taxa(e, idx, taxa)
        assert e.profile_get("main")[0] > 0 and e.profile_get("precise")[0] == 0
        one = e.forward_taxa(idx[0], taxa)                         # 2-D input gives [S][P]; int64 tables are accepted
        assert one.shape == (5, 66) and np.array_equal(_bits(one), _bits(got[0]))
        assert np.array_equal(_bits(e.forward_taxa(idx, taxa.astype(np.int64))), _bits(got))


def test_taxa_bitwise_float64_route_by_token_count(engines):
    with _Profiled(engines("pf")) as e:
        _check_taxa(e, simulate_batch(2, 9, 100, seed=83), _subsets(9, 4, 8, 83))      # 28 pairs x 100 sites < 8,192 tokens
        assert e.profile_get("precise")[0] > 0 and e.profile_get("main")[0] == 0


def test_taxa_bitwise_float64_route_by_site_count(engines):
    with _Profiled(engines("pf")) as e:
        _check_taxa(e, simulate_batch(2, 12, 24, seed=84), _subsets(12, 3, 9, 84))
        assert e.profile_get("precise")[0] > 0 and e.profile_get("main")[0] == 0


def test_taxa_three_sources_in_one_call_against_one_by_one(engines):
    e = engines("pf")
    idx = simulate_batch(3, 20, 200, seed=85)
    taxa = _subsets(20, 4, 12, 85)
    got = _check_taxa(e, idx, taxa)
    for b in range(3):
        assert np.array_equal(_bits(e.forward_taxa(idx[b:b + 1], taxa)[0]), _bits(got[b]))


@pytest.mark.parametrize("ws_mb", [24, 64, 400])
def test_taxa_bitwise_across_chunks(weights, ws_mb):
    """A small workspace budget: the 9 subsets of one source span several chunks (runs of one source's sets)."""
    idx = simulate_batch(2, 24, 200, seed=86)
    taxa = _subsets(24, 9, 20, 86)
    with Engine(weights("pf"), 0) as e:
        e.set_option("ws_limit_mb", ws_mb)
        e.set_option("profile", 1)
        e.profile_reset()
        got = e.forward_taxa(idx, taxa)
        n_gather = e.profile_get("gather_taxa")[0]
        assert got.shape == (2, 9, 190)
        print(f"ws_limit_mb={ws_mb}: {n_gather} gather launches")
        if ws_mb <= 64:                    # (fewer than S = 9 alignments of 20 x 200 fit: several chunks per source)
            assert n_gather >= 4
        _check_taxa(e, idx, taxa)


def test_taxa_recheck_trips_in_the_random_source(weights):
    """Source 1 holds uniformly random residues: its subsets' distances saturate above the re-check threshold (default 8);
    they are rebuilt from the resident source and recomputed in float64, exactly as pf_forward recomputes the host cut."""
    idx = simulate_batch(2, 20, 200, seed=87).copy()
    idx[1] = np.random.default_rng(7).integers(0, 20, size=(20, 200), dtype=np.uint8)
    taxa = _subsets(20, 3, 12, 87)
    with Engine(weights("pf"), 0) as e:
        e.profile_reset()
        got = e.forward_taxa(idx, taxa)
        n_taxa = e.rechecked_count()
        e.profile_reset()
        want = e.forward(T.cut_taxa(idx, taxa).reshape(6, 12, 200)).reshape(2, 3, -1)
        print(f"rechecked: {n_taxa} through forward_taxa, {e.rechecked_count()} through forward; max distance {got[1].max():.3f}")
        assert n_taxa == e.rechecked_count() and n_taxa >= 1
        assert np.array_equal(_bits(got), _bits(want))
        assert got[0].max() < 8


# ---- leave-one-out -------------------------------------------------------------------------------------------------

def _check_loo(e, idx):
    """idx [2][N][L]: distances, cuts and statistics of one call, and of each source alone."""
    B, N, _L = idx.shape
    out, infl, shift, ctx, loo = e.forward_leave_one_out(idx, keep_loo=True)
    P, P1 = N * (N - 1) // 2, (N - 1) * (N - 2) // 2
    assert out.shape == ctx.shape == (B, P) and infl.shape == shift.shape == (B, N) and loo.shape == (B, N, P1)
    assert np.array_equal(_bits(out), _bits(e.forward(idx)))
    assert np.array_equal(_bits(loo), _bits(e.forward_taxa(idx, T.leave_one_out_sets(N))))
    for got, want, name in zip((infl, shift, ctx), T.loo_stats(out, loo), ("influence", "shift", "context")):
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"N={N} {name}: max |device - twin| {err:.3e}, largest value {float(np.abs(want).max()):.3e}")
        assert np.allclose(got, want, rtol=RTOL, atol=ATOL), name
    without = e.forward_leave_one_out(idx)
    assert len(without) == 4 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(without, (out, infl, shift, ctx)))
    for b in range(B):
        one = e.forward_leave_one_out(idx[b], keep_loo=True)
        for a, whole in zip(one, (out, infl, shift, ctx, loo)):
            assert np.array_equal(_bits(a), _bits(whole[b]))
    return out, infl, shift, ctx, loo


@pytest.mark.parametrize("N,L", [(3, 40), (4, 64), (20, 200)])
def test_leave_one_out(engines, N, L):
    _out, infl, _shift, ctx, _loo = _check_loo(engines("pf"), simulate_batch(2, N, L, seed=90 + N))
    assert infl.min() > 0 and ctx.min() > 0          # context dependence: removing a sequence moves the others


def test_leave_one_out_whole_on_default_kernels_cuts_in_float64(engines):
    """14 x 100: the whole alignment has 91 x 100 = 9,100 tokens (default kernels), a cut 78 x 100 = 7,800 (float64)."""
    with _Profiled(engines("pf")) as e:
        e.forward_leave_one_out(simulate_batch(1, 14, 100, seed=95))
        assert e.profile_get("main")[0] > 0 and e.profile_get("precise")[0] > 0
        assert e.profile_get("gather_taxa")[0] >= 1 and e.profile_get("loo_stats")[0] >= 1
    _check_loo(engines("pf"), simulate_batch(2, 14, 100, seed=95))


def test_loo_stats_device_n200_against_twin(engines):
    e = engines("pf")
    rng = np.random.default_rng(200)
    N = 200
    P, P1 = N * (N - 1) // 2, (N - 1) * (N - 2) // 2
    full = rng.uniform(0.05, 2.0, size=(1, P)).astype(np.float32)
    loo = (full[0][T._loo_map(N)] + rng.normal(0, 0.03, size=(N, P1))).astype(np.float32)[None]
    bufs = [e.malloc(a) for a in (full.nbytes, loo.nbytes, 4 * N, 4 * N, 4 * P)]
    try:
        e.h2d(bufs[0], full)
        e.h2d(bufs[1], loo)
        e.loo_stats_device(*bufs[:2], 1, N, *bufs[2:])
        got = [np.empty((1, N), np.float32), np.empty((1, N), np.float32), np.empty((1, P), np.float32)]
        for a, p in zip(got, bufs[2:]):
            e.d2h(a, p)
        e.synchronize()
    finally:
        for p in bufs:
            e.free(p)
    for a, want, name in zip(got, T.loo_stats(full, loo), ("influence", "shift", "context")):
        print(f"N=200 {name}: max |device - twin| {float(np.abs(a.astype(np.float64) - want).max()):.3e}")
        assert np.allclose(a, want, rtol=RTOL, atol=ATOL), name


# ---- against the reference's own outputs ---------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["0_20_tips", "1_30_tips_12"])
def test_leave_one_out_reference_parity(golden, engines, key):
    g = golden("loo.npz")
    out, infl, shift, ctx, loo = engines("pf").forward_leave_one_out(g[f"{key}/idx"], keep_loo=True)
    e_full = float(np.abs(out - g[f"{key}/full"]).max())
    e_loo = float(np.abs(loo - g[f"{key}/loo"]).max())
    print(f"{key}: distances max-abs error vs reference: whole {e_full:.3e}, cuts {e_loo:.3e}")
    assert e_full <= 1e-4 and e_loo <= 1e-4
    for got, name in ((infl, "influence"), (shift, "shift"), (ctx, "context")):
        err = float(np.abs(got - g[f"{key}/{name}"]).max())
        print(f"{key}: {name} max-abs error vs reference {err:.3e} (values up to {float(np.abs(g[f'{key}/{name}']).max()):.3e})")
        assert err <= 2e-4, name


# ---- validation ----------------------------------------------------------------------------------------------------

def test_refusals_leave_outputs_untouched_and_the_handle_usable(weights):
    idx = simulate_batch(1, 6, 30, seed=99)
    taxa = np.ascontiguousarray(_subsets(6, 3, 4, 99))
    with Engine(weights("pf"), 0) as e:
        e.set_option("profile", 1)
        e.profile_reset()
        lib, h = e._lib, e._h
        out = np.full((1, 6, 15), -7.0, np.float32)
        aux = [np.full(64, -7.0, np.float32) for _ in range(4)]             # loo, influence, shift, context
        p_idx, p_out, p_tab = idx.ctypes.data, out.ctypes.data, taxa.ctypes.data
        p_loo, p_inf, p_shift, p_ctx = (a.ctypes.data for a in aux)

        def refused(rc, text):
            assert rc == -1 and text.encode() in lib.pf_last_error(h), lib.pf_last_error(h)
            assert (out == -7.0).all() and all((a == -7.0).all() for a in aux)

        def table(entries, S=3, M=4):
            t = np.ascontiguousarray(entries, dtype=np.int32)
            return lib.pf_forward_taxa(h, p_idx, 1, 6, 30, t.ctypes.data, S, M, p_out)

        two = idx[:, :2].copy()
        refused(lib.pf_forward_leave_one_out(h, two.ctypes.data, 1, 2, 30, p_out, p_loo, p_inf, p_shift, p_ctx), "N >= 3")
        refused(lib.pf_forward_taxa(h, p_idx, 1, 6, 30, p_tab, 3, 1, p_out), "M >= 2")
        refused(lib.pf_forward_taxa(h, p_idx, 1, 6, 30, p_tab, 0, 4, p_out), "S >= 1")
        bad = taxa.copy()
        bad[2, 3] = 6
        refused(table(bad), "taxon 6 at set 2, position 3 is outside [0, 6)")
        bad[2, 3], bad[0, 1] = 5, -1
        refused(table(bad), "taxon -1 at set 0, position 1 is outside [0, 6)")
        refused(lib.pf_forward_leave_one_out(h, p_idx, 1, 6, 30, p_out, p_loo, None, p_shift, p_ctx), "null buffer")
        refused(lib.pf_forward_leave_one_out(h, p_idx, 1, 6, 30, p_out, p_loo, p_inf, None, p_ctx), "null buffer")
        refused(lib.pf_forward_leave_one_out(h, None, 1, 6, 30, p_out, p_loo, p_inf, p_shift, p_ctx), "null buffer")
        refused(lib.pf_forward_taxa(h, p_idx, 1, 6, 30, None, 3, 4, p_out), "null buffer")
        assert lib.pf_forward_taxa(h, p_idx, 1, 6, 30, p_tab, 3, 4, None) == -1
        refused(lib.pf_forward_taxa(h, p_idx, 0, 6, 30, p_tab, 3, 4, p_out), "bad dimensions")
        refused(lib.pf_forward_taxa(h, p_idx, 1, 6, 30, p_tab, 1, 201, p_out), "n_seqs must be smaller or equal to 200")
        refused(lib.pf_forward_taxa(h, p_idx, 1 << 30, 6, 30, p_tab, 1 << 30, 4, p_out), "overflow")
        res = idx.copy()
        res[0, 2, 5] = 22
        refused(lib.pf_forward_taxa(h, res.ctypes.data, 1, 6, 30, p_tab, 3, 4, p_out), "residue index 22")
        refused(lib.pf_forward_leave_one_out(h, res.ctypes.data, 1, 6, 30, p_out, p_loo, p_inf, p_shift, p_ctx), "residue index 22")
        # nothing of all that reached the device
        assert all(e.profile_get(k)[0] == 0 for k in ("gather_taxa", "loo_stats", "precise", "main"))
        # the Python surface raises ValueError, also for what ctypes could not carry
        with pytest.raises(ValueError, match="outside"):
            e.forward_taxa(idx, np.array([[0, 6]]))
        with pytest.raises(ValueError, match="outside"):
            e.forward_taxa(idx, np.array([[0, 2 ** 40]]))
        with pytest.raises(ValueError):
            e.forward_taxa(idx, np.array([[0.0, 1.0]]))
        with pytest.raises(ValueError, match="N >= 3"):
            e.forward_leave_one_out(two)
        assert e.profile_get("gather_taxa")[0] == 0
        # the handle still works; loo may be NULL
        assert lib.pf_forward_taxa(h, p_idx, 1, 6, 30, p_tab, 3, 4, p_out) == 0
        want = e.forward(T.cut_taxa(idx, taxa)[0])
        assert np.array_equal(_bits(out.reshape(-1)[:18]), _bits(want.reshape(-1))) and e.profile_get("gather_taxa")[0] >= 1
        assert lib.pf_forward_leave_one_out(h, p_idx, 1, 6, 30, p_out, None, p_inf, p_shift, p_ctx) == 0
        assert np.array_equal(_bits(out.reshape(-1)[:15]), _bits(e.forward(idx)[0]))


# ---- CLI on the 20-tip test MSAs -----------------------------------------------------------------------------------

def _run(args):
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, timeout=900)


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_cli_leave_one_out_on_20_tip_msas(tmp_path, engines):
    from phyloformer_amd.fasta import load_alignment
    msas = tmp_path / "msas"
    msas.mkdir()
    stems = [f"{k}_20_tips" for k in range(5)]
    for s in stems:
        shutil.copy(os.path.join(REPO, "data", "testdata", "msas", f"{s}.fa"), msas / f"{s}.fa")
    plain = _run([str(msas), "-o", str(tmp_path / "plain"), "-t"])
    loo = _run([str(msas), "-o", str(tmp_path / "loo"), "-t", "--leave-one-out"])
    assert plain.returncode == 0 and loo.returncode == 0, plain.stderr[-2000:] + loo.stderr[-2000:]
    p, w = _files(tmp_path / "plain"), _files(tmp_path / "loo")
    assert set(w) == set(p) | {f"{s}.{ext}" for s in stems for ext in ("taxa.tsv", "context.phy")}
    for name, data in p.items():
        assert w[name] == data, name                           # <stem>.phy and <stem>.nj.nwk unchanged
    e = engines("pf_base")
    for s in stems:
        idx, ids = load_alignment(os.path.join(msas, f"{s}.fa"))
        _out, infl, shift, ctx = e.forward_leave_one_out(idx)
        assert w[f"{s}.context.phy"] == e_phylip(ctx, ids)
        rows = [r.split("\t") for r in w[f"{s}.taxa.tsv"].decode().splitlines()]
        assert rows[0] == ["index", "id", "influence", "shift", "relative", "rf_pruned"] and len(rows) == 21
        for k, row in enumerate(rows[1:]):
            assert row[:4] == [str(k), ids[k], f"{float(infl[k]):.10f}", f"{float(shift[k]):.10f}"] and row[5].isdigit()


def e_phylip(vec, ids):
    from phyloformer_amd.taxa import context_phylip
    return context_phylip(vec, ids).encode()
