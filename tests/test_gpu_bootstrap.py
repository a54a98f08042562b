"""-m gpu: site bootstrap on the device - k_resample's bytes, pf_bootstrap's bit-identity with pf_forward on every path,
parity with the oracle, refusals, and the CLI's --bootstrap on the 20 test MSAs."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from phyloformer_amd import bootstrap as bs
from phyloformer_amd.engine import Engine
from phyloformer_amd.msa_sim import simulate_batch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = re.compile(r"\)(\d+)")


def _host_replicates(idx, R, seed):
    return bs.resample(idx, R, seed)          # [B][R][N][L]


@pytest.mark.parametrize("B,N,L,r_begin,R", [(1, 2, 1, 0, 3), (3, 20, 200, 5, 17), (1, 200, 500, 0, 4), (2, 7, 2001, 1000, 9)])
def test_resample_kernel_bytes_match_host_twin(engines, B, N, L, r_begin, R):
    e = engines("pf")
    rng = np.random.default_rng(B * 1000 + L)
    src = rng.integers(0, 22, size=(B, N, L), dtype=np.uint8)
    seed = 0x1234_5678_9ABC_DEF0 + L
    d_src, d_dst = e.malloc(src.nbytes), e.malloc(B * R * N * L)
    try:
        e.h2d(d_src, src)
        e.resample_sites_device(d_src, B, N, L, r_begin, R, seed, d_dst)
        got = np.empty((B, R, N, L), np.uint8)
        e.d2h(got, d_dst)
        e.synchronize()
    finally:
        e.free(d_src)
        e.free(d_dst)
    sites = bs.resample_sites(L, R, seed, first=r_begin)
    want = np.ascontiguousarray(np.moveaxis(src[..., sites], -2, -3))
    assert np.array_equal(got, want)


def _check_bitwise(e, idx, R, seed):
    got = e.bootstrap(idx, R, seed)
    reps = _host_replicates(idx, R, seed)
    B, N, L = idx.shape
    want = e.forward(reps.reshape(B * R, N, L)).reshape(B, R, -1)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return got


def test_bootstrap_bitwise_split_fp16_path(engines):
    e = engines("pf")
    idx = simulate_batch(3, 20, 200, seed=31)
    got = _check_bitwise(e, idx, 16, 3)
    # 2-D input gives [R][P]; a replicate's distances do not depend on its batch
    one = e.bootstrap(idx[1], 16, 3)
    assert one.shape == (16, 190) and np.array_equal(one, got[1])


def test_bootstrap_bitwise_precise_shape(engines):
    e = engines("pf")
    _check_bitwise(e, simulate_batch(2, 5, 20, seed=32), 6, 11)


def test_bootstrap_bitwise_precise_option(engines, weights):
    with Engine(weights("pf"), 0) as e:
        e.set_option("precise", 1)
        _check_bitwise(e, simulate_batch(2, 12, 64, seed=33), 5, 4)


def test_bootstrap_bitwise_generic_architecture():
    from phyloformer_amd.weights import random_weights
    with Engine(random_weights(3, n_blocks=2, n_heads=2, embed_dim=32), 0) as e:
        e.set_option("profile", 1)
        e.profile_reset()
        _check_bitwise(e, simulate_batch(2, 10, 80, seed=34), 4, 8)
        assert e.profile_get("generic")[0] > 0 and e.profile_get("main")[0] == 0


@pytest.mark.parametrize("ws_mb", [24, 64, 400])
def test_bootstrap_bitwise_across_chunks(weights, ws_mb):
    """A small workspace budget: one call spans several chunks (runs of one source's replicates, or several sources)."""
    with Engine(weights("pf"), 0) as e:
        e.set_option("ws_limit_mb", ws_mb)
        e.set_option("profile", 1)
        _check_bitwise(e, simulate_batch(3, 20, 200, seed=35), 7, 5)
        if ws_mb <= 64:                    # (fewer than R = 7 alignments of 20 x 200 fit: several chunks)
            assert e.profile_get("resample")[0] >= 2


def test_bootstrap_recheck_runs_per_replicate(weights):
    """Uniformly random residues predict distances above the re-check threshold: flagged replicates are recomputed in
    float64 from their device bytes, exactly like pf_forward recomputes them."""
    rng = np.random.default_rng(6)
    idx = rng.integers(0, 20, size=(2, 8, 300), dtype=np.uint8)
    with Engine(weights("pf"), 0) as e:
        e.set_option("ws_limit_mb", 64)
        e.profile_reset()
        got = e.bootstrap(idx, 5, 1)
        n_boot = e.rechecked_count()
        e.profile_reset()
        want = e.forward(_host_replicates(idx, 5, 1).reshape(10, 8, 300)).reshape(2, 5, -1)
        assert n_boot == e.rechecked_count() > 0
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_bootstrap_reference_parity(weights):
    from oracle import pf_oracle
    from phyloformer_amd.fasta import load_alignment
    idx, _ids = load_alignment(os.path.join(REPO, "data", "testdata", "msas", "0_20_tips.fa"))
    w = weights("pf")
    with Engine(w, 0) as e:
        got = e.bootstrap(idx, 2, 7)
    for r, rep in enumerate(_host_replicates(idx, 2, 7)):
        want = pf_oracle.forward(w.tensors, rep)
        assert np.abs(got[r] - want).max() <= 1e-4


def test_bootstrap_refusals_before_device_work(engines):
    import ctypes as C
    e = engines("pf")
    idx = simulate_batch(1, 6, 30, seed=36)
    with pytest.raises(ValueError, match="R >= 1"):
        e.bootstrap(idx, 0, 0)
    bad = idx.copy()
    bad[0, 2, 5] = 22
    with pytest.raises(ValueError, match="residue index 22"):
        e.bootstrap(bad, 3, 0)
    rc = e._lib.pf_bootstrap(e._h, idx.ctypes.data, 1, 6, 30, 3, 0, None)
    assert rc == -1 and b"null buffer" in e._lib.pf_last_error(e._h)
    big = simulate_batch(1, 201, 8, seed=37)
    with pytest.raises(ValueError, match="n_seqs must be smaller or equal to 200"):
        e.bootstrap(big, 2, 0)
    out = np.empty(1, np.float32)
    assert e._lib.pf_bootstrap(e._h, idx.ctypes.data, 1 << 30, 6, 30, 1 << 30, 0, out.ctypes.data) == -1
    assert b"overflow" in e._lib.pf_last_error(e._h)
    del C


# ---- CLI on the 20 test MSAs ---------------------------------------------------------------------------------------

def _run(args):
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf_base.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, timeout=900)


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_cli_bootstrap_on_test_msas(tmp_path):
    msas = os.path.join(REPO, "data", "testdata", "msas")
    flags = ["-t", "--bootstrap", "20", "--seed", "3"]
    plain = _run([msas, "-o", str(tmp_path / "plain"), "-t"])
    boot = _run([msas, "-o", str(tmp_path / "boot"), *flags])
    assert plain.returncode == 0 and boot.returncode == 0, plain.stderr[-2000:] + boot.stderr[-2000:]
    p, b = _files(tmp_path / "plain"), _files(tmp_path / "boot")
    stems = sorted(n[:-3] for n in os.listdir(msas) if n.endswith(".fa"))
    assert len(stems) == 20 and sorted(b) == sorted(list(p) + [f"{s}.sup.nwk" for s in stems])
    for name, data in p.items():
        assert b[name] == data, name                           # .phy and .nj.nwk unchanged
    for s in stems:
        sup = b[f"{s}.sup.nwk"].decode()
        assert LABEL.sub(")", sup).encode() == b[f"{s}.nj.nwk"]
        labels = [int(v) for v in LABEL.findall(sup)]
        n = int(b[f"{s}.phy"].split(b"\n", 1)[0])
        assert len(labels) == n - 3 and all(0 <= v <= 100 for v in labels)
    again = _run([msas, "-o", str(tmp_path / "again"), *flags])
    assert again.returncode == 0 and _files(tmp_path / "again") == b
    lone_in = tmp_path / "lone_in"
    lone_in.mkdir()
    shutil.copy(os.path.join(msas, "3_40_tips.fa"), lone_in)
    lone = _run([str(lone_in), "-o", str(tmp_path / "lone"), *flags])
    assert lone.returncode == 0 and _files(tmp_path / "lone")["3_40_tips.sup.nwk"] == b["3_40_tips.sup.nwk"]
    pyio = _run([msas, "-o", str(tmp_path / "pyio"), *flags, "--python-io"])
    assert pyio.returncode == 0 and _files(tmp_path / "pyio") == b, pyio.stderr[-2000:]
    one = _run([msas, "-o", str(tmp_path / "one"), *flags, "--batch", "1"])
    assert one.returncode == 0 and _files(tmp_path / "one") == b, one.stderr[-2000:]
