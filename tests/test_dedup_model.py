"""The numpy model of the column classes and of k_main_plan's record (``helpers/dedup_model.py``) on hand-worked cases.
``tests/test_gpu_dedup_routes.py`` holds the forward's debug taps against this model; here the model itself is held
against values worked out by hand from DESIGN.md section 4 and the text of ``csrc/pf_layout.h``.  No GPU."""
import numpy as np
import pytest

from helpers import dedup_model as M


def test_threshold_is_the_headers():
    assert M.threshold() == (17, 20)


def test_classes_are_first_occurrences():
    #            site   0  1  2  3  4  5  6
    a = np.array([[3, 3, 5, 3, 5, 3, 7],
                  [1, 1, 1, 2, 1, 1, 1]], np.uint8)        # columns: A A B C B A D
    srep, ulist, k = M.classes(a)
    assert srep.tolist() == [0, 0, 2, 3, 2, 0, 6] and ulist.tolist() == [0, 2, 3, 6] and k == 4
    assert srep.dtype == np.int32 and ulist.dtype == np.int32
    one = M.classes(np.zeros((5, 1), np.uint8))
    assert one[0].tolist() == [0] and one[1].tolist() == [0] and one[2] == 1
    # columns that differ in one sequence only are different columns, whichever sequence it is
    b = np.zeros((3, 4), np.uint8)
    b[0] = [0, 1, 0, 1]
    assert M.classes(b)[0].tolist() == [0, 1, 0, 1]
    b = np.zeros((3, 4), np.uint8)
    b[2] = [0, 1, 1, 2]
    assert M.classes(b)[0].tolist() == [0, 1, 1, 3]


def test_compact_tiles():
    assert M.compact_tiles(3, 33) == 4                      # 99 tokens: 32 + 32 + 32 + 3
    assert M.compact_tiles(3, 32) == 3 and M.compact_tiles(1, 32) == 1 and M.compact_tiles(1, 33) == 2
    assert M.compact_tiles(15, 200) == 94                   # 3,000 tokens: 93 tiles and 24 tokens
    for P in (1, 3, 15, 528):                               # fewer than 32 distinct columns: one ragged tile per row
        for K in (1, 2, 31):
            assert M.compact_tiles(P, K) == P


@pytest.mark.parametrize("K,L", [(34, 40), (170, 200), (28, 33)])
def test_split_at_the_threshold(K, L):
    assert K * 20 <= L * 17 < (K + 1) * 20                  # K is the largest count that still splits
    assert M.split(K, L, 1) and not M.split(K + 1, L, 1)
    assert M.split(1, L, 1) and not M.split(L, L, 1)


def test_mode_0_never_splits_and_mode_2_always():
    for L in (1, 33, 40, 200, 4097):
        for K in sorted({1, 28, min(L, 34), L}):
            assert not M.split(K, L, 0) and M.split(K, L, 2)


def test_plan_by_hand():
    # P = 3, L = 33: K = 1 -> 3 tiles, 20 -> 3 tiles, 28 -> 3 tiles (all split); 29 and 33 stay fused
    ucounts = [33, 1, 29, 20, 28, 33, 28]
    nf, ns, tiles, flist, slist, cpre = M.plan(ucounts, 3, 33, 1)
    assert (nf, ns, tiles) == (3, 4, 12) and flist == [0, 2, 5] and slist == [1, 3, 4, 6] and cpre == [0, 3, 6, 9, 12]
    nf, ns, tiles, flist, slist, cpre = M.plan(ucounts, 3, 33, 2)
    assert (nf, ns, tiles) == (0, 7, 23) and flist == [] and slist == list(range(7))
    assert cpre == [0, 4, 7, 10, 13, 16, 20, 23]            # K = 33: 99 tokens, 4 tiles; K = 29 < 32: 3 tiles
    nf, ns, tiles, flist, slist, cpre = M.plan(ucounts, 3, 33, 0)
    assert (nf, ns, tiles) == (7, 0, 0) and flist == list(range(7)) and slist == [] and cpre == [0]
    # the int record as the tap holds it: [nf, ns, tiles, 0 | flist B | slist B | cpre B + 1]
    tap = np.full(4 + 3 * 7 + 1, -7, np.int32)
    tap[:4] = [3, 4, 12, 0]
    tap[4:7], tap[11:15], tap[18:23] = [0, 2, 5], [1, 3, 4, 6], [0, 3, 6, 9, 12]
    assert M.read_plan(tap, 7) == M.plan(ucounts, 3, 33, 1)


def test_builders_give_the_counts_they_promise():
    for placement in M.PLACEMENTS:
        for k in (1, 2, 31, 39, 40):
            a = M.alignment(6, 40, k, placement)
            srep, ulist, count = M.classes(a)
            assert count == k and a.max() <= 21
            if placement == "behind":
                assert ulist.tolist() == list(range(k))
            elif k > 1:
                assert ulist[-1] == 39                       # the last site is a first occurrence
    pool = M.simulated_pool(8)
    assert pool.shape[0] == 8 and pool.shape[1] >= 200 and pool.max() <= 21 and M.classes(pool)[2] == pool.shape[1]
    a = M.alignment_simulated(8, 200, 33, "between")
    assert M.classes(a)[2] == 33 and {a[:, s].tobytes() for s in range(200)} <= {pool[:, s].tobytes() for s in range(33)}
    with pytest.raises(AssertionError, match="distinct simulated columns"):
        M.alignment_simulated(2, 600, 500, "front")          # two sequences: 22 x 22 = 484 columns at the most
