"""The head fold of the last block (pf_host_prep.h, fold_head) on the host: u = W2^T head_w in the lane order the
folded kernel reads, and c0 = head_w . b2 + head_b.  No GPU: the header is compiled with g++ into a test library."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, FF = 64, 256


def kmap(j, h):
    return 8 * (j >> 2) + 4 * h + (j & 3)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib = str(tmp_path_factory.mktemp("fold") / "libfold_head.so")
    cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
           os.path.join(REPO, "tests", "native", "fold_head_shim.cpp"), "-o", lib]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    so = ctypes.CDLL(lib)
    fp = ctypes.POINTER(ctypes.c_float)
    so.shim_fold_head.argtypes = [fp, fp, fp, ctypes.c_float, ctypes.c_double, fp, fp]
    so.shim_fold_head.restype = None
    return so


def fold(so, w2, b2, hw, hb, scale):
    fp = ctypes.POINTER(ctypes.c_float)
    u = np.zeros(FF, np.float32)
    c0 = np.zeros(1, np.float32)
    so.shim_fold_head(w2.ctypes.data_as(fp), b2.ctypes.data_as(fp), hw.ctypes.data_as(fp), float(hb), scale,
                      u.ctypes.data_as(fp), c0.ctypes.data_as(fp))
    return u, float(c0[0])


def test_fold_head_values_and_lane_order(shim):
    rng = np.random.default_rng(5)
    w2 = rng.standard_normal((E, FF)).astype(np.float32)
    b2 = rng.standard_normal(E).astype(np.float32)
    hw = rng.standard_normal(E).astype(np.float32)
    hb = np.float32(0.37)
    scale = 0.5 / np.sqrt(0.5 * np.log2(np.e))             # the image's W2 factor 1 / (2 a)
    u, c0 = fold(shim, w2, b2, hw, hb, scale)
    u_nat = (hw.astype(np.float64) @ w2.astype(np.float64)) * scale
    assert c0 == np.float32(float(hb) + hw.astype(np.float64) @ b2.astype(np.float64))
    # lane order: entry (T, h, r) is the hidden row GEMM1's accumulator register r holds in lane half h of tile T,
    # row(r, h) = (r & 3) + 8 (r >> 2) + 4 h
    for T in range(8):
        for h in range(2):
            for r in range(16):
                k = 32 * T + (r & 3) + 8 * (r >> 2) + 4 * h
                assert u[(T * 2 + h) * 16 + r] == np.float32(u_nat[k]), (T, h, r)
    # ... which is the K order GEMM2's B operand consumed: step s = 2 T + v takes registers 8 v .. 8 v + 7 of tile T
    # as K = kmap(8 s + i, h) (pack_frags)
    for T in range(8):
        for h in range(2):
            for v in range(2):
                for i in range(8):
                    assert u[(T * 2 + h) * 16 + 8 * v + i] == np.float32(u_nat[kmap(8 * (2 * T + v) + i, h)])
    assert sorted(int(32 * T + (r & 3) + 8 * (r >> 2) + 4 * h) for T in range(8) for h in range(2) for r in range(16)) \
        == list(range(FF))
