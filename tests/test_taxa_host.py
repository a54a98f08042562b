"""The taxon axis on the host (no GPU): the pair-index rules (Python twins and the native ones of csrc/pf_taxa_host.h),
cut_taxa, loo_stats, restrict_splits, and the ABI additions."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from phyloformer_amd import taxa as T
from phyloformer_amd import treecmp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(N):
    """pair -> index by walking the row-major upper triangle."""
    d = {}
    for i in range(N):
        for j in range(i + 1, N):
            d[(i, j)] = len(d)
    return d


# ---- pair indices --------------------------------------------------------------------------------------------------

def test_pair_index_literal():
    assert [T.pair_index(i, j, 3) for i, j in ((0, 1), (0, 2), (1, 2))] == [0, 1, 2]
    assert [T.pair_index(i, j, 4) for i, j in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))] == [0, 1, 2, 3, 4, 5]
    assert [T.pair_index(i, j, 5) for i, j in ((0, 4), (1, 2), (1, 4), (2, 3), (3, 4))] == [3, 4, 6, 7, 9]
    assert T.pair_of(0, 3) == (0, 1) and T.pair_of(2, 3) == (1, 2) and T.pair_of(5, 4) == (2, 3) and T.pair_of(6, 5) == (1, 4)


def test_loo_pair_index_literal():
    # N = 3: every cut keeps one pair
    assert T.loo_pair_index(1, 2, 0, 3) == T.loo_pair_index(0, 2, 1, 3) == T.loo_pair_index(0, 1, 2, 3) == 0
    # N = 4, t = 1: the rows 0, 2, 3 remain
    assert [T.loo_pair_index(i, j, 1, 4) for i, j in ((0, 2), (0, 3), (2, 3))] == [0, 1, 2]
    assert [T.loo_pair_index(i, j, 0, 4) for i, j in ((1, 2), (1, 3), (2, 3))] == [0, 1, 2]
    assert [T.loo_pair_index(i, j, 3, 4) for i, j in ((0, 1), (0, 2), (1, 2))] == [0, 1, 2]
    # N = 5, t = 2: the rows 0, 1, 3, 4 remain
    assert [T.loo_pair_index(i, j, 2, 5) for i, j in ((0, 1), (0, 3), (0, 4), (1, 3), (1, 4), (3, 4))] == [0, 1, 2, 3, 4, 5]
    assert T.leave_one_out_sets(4).tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    assert T.leave_one_out_sets(3).dtype == np.int32


def test_pair_rules_refusals():
    for bad in ((1, 1, 4), (2, 1, 4), (-1, 2, 4), (0, 4, 4)):
        with pytest.raises(ValueError):
            T.pair_index(*bad)
    for bad in ((0, 1, 0, 4), (0, 1, 1, 4), (0, 1, 4, 4), (0, 1, -1, 4)):
        with pytest.raises(ValueError):
            T.loo_pair_index(*bad)
    for bad in ((6, 4), (-1, 4), (0, 1)):
        with pytest.raises(ValueError):
            T.pair_of(*bad)
    with pytest.raises(ValueError):
        T.leave_one_out_sets(2)


@pytest.mark.parametrize("N", range(2, 13))
def test_pair_rules_against_brute_force(N):
    number = _brute(N)
    for (i, j), q in number.items():
        assert T.pair_index(i, j, N) == q and T.pair_of(q, N) == (i, j)
    if N < 3:
        return
    sets = T.leave_one_out_sets(N)
    for t in range(N):
        rows = [r for r in range(N) if r != t]
        assert sets[t].tolist() == rows
        inner = _brute(N - 1)
        for (a, b), q in inner.items():
            assert T.loo_pair_index(rows[a], rows[b], t, N) == q
    assert np.array_equal(T._loo_map(N), np.array([[number[(sets[t][a], sets[t][b])] for (a, b) in _brute(N - 1)]
                                                   for t in range(N)]))


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib = str(tmp_path_factory.mktemp("taxa_shim") / "libpf_taxa_shim.so")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                          os.path.join(REPO, "tests", "native", "pf_taxa_shim.cpp"), "-o", lib], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    so = C.CDLL(lib)
    so.t_first_bad_taxon.restype = so.t_pair_index.restype = so.t_loo_pair_index.restype = C.c_longlong
    so.t_first_bad_taxon.argtypes = [C.c_void_p, C.c_longlong, C.c_int]
    so.t_pair_index.argtypes = [C.c_int] * 3
    so.t_loo_pair_index.argtypes = [C.c_int] * 4
    so.t_pair_of.argtypes = [C.c_longlong, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return so


def test_native_twins_agree(native):
    for N in list(range(2, 13)) + [57, 200]:
        i, j = C.c_int(), C.c_int()
        for (a, b), q in _brute(N).items():
            assert native.t_pair_index(a, b, N) == q
            assert native.t_pair_of(q, N, C.byref(i), C.byref(j)) == 1 and (i.value, j.value) == (a, b)
            if N <= 12:
                for t in range(N):
                    want = -1 if t in (a, b) or N < 3 else T.loo_pair_index(a, b, t, N)
                    assert native.t_loo_pair_index(a, b, t, N) == want
        assert native.t_pair_of(N * (N - 1) // 2, N, C.byref(i), C.byref(j)) == 0 and (i.value, j.value) == (-1, -1)
        assert native.t_pair_index(1, 1, N) == -1 and native.t_pair_index(0, N, N) == -1
    tab = np.array([0, 4, 2, 5, -1], np.int32)
    assert native.t_first_bad_taxon(tab.ctypes.data, 3, 5) == -1
    assert native.t_first_bad_taxon(tab.ctypes.data, 4, 5) == 3 and native.t_first_bad_taxon(tab.ctypes.data, 5, 6) == 4
    assert native.t_first_bad_taxon(None, 0, 5) == -1


# ---- cut_taxa, loo_stats -------------------------------------------------------------------------------------------

def test_cut_taxa_layout_and_refusals():
    rng = np.random.default_rng(2)
    idx = rng.integers(0, 22, size=(2, 5, 9), dtype=np.uint8)
    taxa = np.array([[4, 3, 2, 1, 0, 0, 2], [0, 1, 2, 3, 4, 4, 4]])          # M = 7 > N = 5: repeats
    cut = T.cut_taxa(idx, taxa)
    assert cut.shape == (2, 2, 7, 9) and cut.dtype == np.uint8 and cut.flags["C_CONTIGUOUS"]
    for b in range(2):
        for s in range(2):
            assert np.array_equal(cut[b, s], idx[b][taxa[s]])
    assert np.array_equal(T.cut_taxa(idx[1], taxa), cut[1])
    loo = T.cut_taxa(idx, T.leave_one_out_sets(5))
    for t in range(5):
        assert np.array_equal(loo[:, t], np.delete(idx, t, axis=1))
    for bad in ([[5, 0]], [[-1, 0]], [[0.5, 1.0]]):
        with pytest.raises(ValueError):
            T.cut_taxa(idx, np.array(bad))


def test_loo_stats_hand_made_n3():
    """N = 3: full = (d01, d02, d12); the cut without t keeps the one pair that does not hold t."""
    full = np.array([1.0, 2.0, 3.0], np.float32)
    loo = np.array([[3.5], [2.5], [1.25]], np.float32)          # without 0: d12; without 1: d02; without 2: d01
    infl, shift, ctx = T.loo_stats(full, loo)
    assert infl.dtype == shift.dtype == ctx.dtype == np.float32
    assert infl.tolist() == [0.5, 0.5, 0.25] and shift.tolist() == [0.5, 0.5, 0.25]
    assert ctx.tolist() == [0.25, 0.5, 0.5]                     # (0,1) <- t = 2, (0,2) <- t = 1, (1,2) <- t = 0
    infl, shift, _ctx = T.loo_stats(full, np.array([[2.0], [2.5], [1.0]], np.float32))
    assert infl.tolist() == [1.0, 0.5, 0.0] and shift.tolist() == [-1.0, 0.5, 0.0]


def test_loo_stats_n4_and_batch():
    """N = 4 by hand: delta is nonzero in the cut without 1 only, for pairs (0,2) -> +3 and (2,3) -> -4."""
    full = np.arange(1.0, 7.0)
    loo = np.array([full[[3, 4, 5]], full[[1, 2, 5]], full[[0, 2, 4]], full[[0, 1, 3]]])
    loo[1] += [3.0, 0.0, -4.0]
    infl, shift, ctx = T.loo_stats(full, loo)
    assert np.allclose(infl, [0, np.sqrt(25 / 3), 0, 0]) and np.allclose(shift, [0, -1 / 3, 0, 0])
    assert np.allclose(ctx, [0, np.sqrt(9 / 2), 0, 0, 0, np.sqrt(16 / 2)])
    both = T.loo_stats(np.stack([full, full + 1]), np.stack([loo, loo + 1]))
    for got, one in zip(both, (infl, shift, ctx)):
        assert got.shape == (2,) + one.shape and np.array_equal(got[0], one) and np.allclose(got[1], one, atol=1e-6)
    with pytest.raises(ValueError):
        T.loo_stats(full, loo[:, :2])
    with pytest.raises(ValueError):
        T.loo_stats(full[:3], np.zeros((2, 0)))


# ---- restrict_splits -----------------------------------------------------------------------------------------------

def test_restrict_splits_on_a_five_leaf_tree():
    leaves = ["a", "b", "c", "d", "e"]
    tree = treecmp.parse_newick("((a:1,b:1):2,c:1,(d:1,e:1):3);")
    sp = treecmp.splits(tree)
    internal = {k for k in sp if 1 < len(k) < 4}
    assert internal == {frozenset("cde"), frozenset("de")}      # ab|cde stored as the side without 'a'
    # without c: ab|de survives (both splits become it: their lengths add)
    assert T.restrict_splits(sp, "c", leaves) == {frozenset("de"): 5.0}
    # without e: ab|cd survives, de|abc became trivial
    assert T.restrict_splits(sp, "e", leaves) == {frozenset("cd"): 2.0}
    # without a, the anchor: the new anchor is b; cde|b became trivial, de|bc is stored as the side without b
    assert T.restrict_splits(sp, "a", leaves) == {frozenset("de"): 3.0}
    for leaf in leaves:
        pruned = treecmp.parse_newick({"a": "(b:3,c:1,(d:1,e:1):3);", "b": "(a:3,c:1,(d:1,e:1):3);",
                                       "c": "((a:1,b:1):5,d:1,e:1);", "d": "((a:1,b:1):2,c:1,e:4);",
                                       "e": "((a:1,b:1):2,c:1,d:4);"}[leaf])
        want = {k: v for k, v in treecmp.splits(pruned).items() if 1 < len(k) < 3}
        assert T.restrict_splits(sp, leaf, leaves) == want, leaf
    with pytest.raises(ValueError):
        T.restrict_splits(sp, "z", leaves)
    # rf_pruned on index labels: a cut whose tree is the pruned tree has distance 0
    full = "((0:1,1:1):2,2:1,(3:1,(4:1,5:1):1):3);"
    cuts = ["(1:3,2:1,(3:1,(4:1,5:1):1):3);", "(0:3,2:1,(3:1,(4:1,5:1):1):3);", "((0:1,1:1):2,3:1,(4:1,5:1):1);",
            "((0:1,1:1):2,2:1,(4:1,5:1):1);", "((0:1,2:1):2,1:1,(3:1,5:1):1);", "((0:1,1:1):2,2:1,(3:1,4:1):1);"]
    assert T.rf_pruned(full, cuts, 6) == [0, 0, 0, 0, 2, 0]           # cut 4 has 02|135 where the pruned tree has 01|235
    assert T.rf_pruned("((0:1,1:1):1,2:1,3:1);", ["(1:1,2:1,3:1);"] * 4, 4) == ["NA"] * 4


def test_taxa_tsv_format():
    text = T.taxa_tsv(["x", "y y", "z"], np.array([0.5, 0.25, 0.75], np.float32), np.array([-0.5, 0.0, 0.125], np.float32))
    rows = text.splitlines()
    assert rows[0].split("\t") == ["index", "id", "influence", "shift", "relative"]
    assert rows[1] == "0\tx\t0.5000000000\t-0.5000000000\t1.000000000000000"
    assert rows[2].split("\t") == ["1", "y y", "0.2500000000", "0.0000000000", "0.500000000000000"]
    zero = T.taxa_tsv(["x", "y", "z"], np.zeros(3), np.zeros(3), rf_pruned=["NA", 2, 0]).splitlines()
    assert zero[0].endswith("\trf_pruned") and zero[1].split("\t")[4:] == ["NA", "NA"] and zero[2].split("\t")[5] == "2"


# ---- ABI -----------------------------------------------------------------------------------------------------------

def test_header_declares_taxon_entry_points():
    names = ("pf_gather_taxa_device", "pf_forward_taxa", "pf_forward_leave_one_out", "pf_loo_stats_device")
    h = open(os.path.join(REPO, "include", "phyloformer_amd.h")).read()
    for name in names:
        assert re.search(rf"^int {name}\(", h, re.M), name
    assert int(re.search(r"#define PF_ABI_VERSION (\d+)", h).group(1)) == 5
    from phyloformer_amd import build, engine
    new = {"pf_taxa.hip.h", "pf_taxa_host.h", "pf_bytes.hip.h"}
    assert new <= set(build.HEADERS) and not new & set(build.KERNEL_FILES)           # the kernel hash does not move
    assert set(names) <= set(engine.SIGNATURES) and set(names) <= engine.CALL_TIME_SYMBOLS and engine.ABI_VERSION == 5
    build.build()
    lib = engine.load_library()
    assert all(hasattr(lib, n) for n in names) and lib.pf_abi_version() == 5
    # load_run4 has one definition, shared by both gathers
    csrc = os.path.join(REPO, "phyloformer_amd", "csrc")
    defs = [f for f in os.listdir(csrc) if re.search(r"uint32_t load_run4\(", open(os.path.join(csrc, f)).read())]
    assert defs == ["pf_bytes.hip.h"]
