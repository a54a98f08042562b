"""-m gpu: neighbour joining on the device - pf_nj_joins against nj.nj_joins on the same float32-derived matrix, bit
for bit (slots equal, lengths equal as uint64); the sources of a call are independent; chunks under a workspace budget;
the entry point on device arrays and the call counter; the non-finite flag; refusals by their texts; and tiled distances
to Newick text end to end against hostio.nj_newick."""
import numpy as np
import pytest

from helpers.nj_table import assert_table, tie_cases
from phyloformer_amd import hostio
from phyloformer_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _preds(B, N, seed):
    return np.random.default_rng(seed).uniform(0.01, 3.0, size=(B, N * (N - 1) // 2)).astype(np.float32)


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(np.ascontiguousarray(a[1]).view(np.uint64), np.ascontiguousarray(b[1]).view(np.uint64))
            and np.array_equal(a[2], b[2]))


# no join; the under-8 sums; eight accumulators; the recursive split on the way down from 137; 300: more rows than one
# workgroup of the minimum has threads, and 256 partial minima for the join to reduce
@pytest.mark.parametrize("N", [3, 4, 9, 137, 300])
def test_joins_equal_nj_joins_bit_for_bit_and_sources_are_independent(engines, N):
    e = engines("pf")
    preds = _preds(2, N, seed=2000 + N)
    slots, lengths, flag = e.nj_joins(preds)
    assert slots.shape == lengths.shape == (2, 2 * (N - 3) + 3) and slots.dtype == np.int32 and lengths.dtype == np.float64
    assert flag.tolist() == [False, False]
    for b in range(2):
        assert_table(slots[b], lengths[b], preds[b], N)
    alone = e.nj_joins(preds[1])
    assert _same(alone, (slots[1], lengths[1], flag[1]))


def test_ties_and_zero_distances(engines):
    n = 23
    preds = tie_cases(n)
    slots, lengths, flag = engines("pf").nj_joins(preds)
    assert not flag.any()
    for b in range(len(preds)):
        assert_table(slots[b], lengths[b], preds[b], n)


def test_chunks_under_a_workspace_budget_give_the_same_bits(weights):
    """N = 300: 720 KB of matrix per source, so ws_limit_mb = 1 runs the three sources one after the other."""
    preds = _preds(3, 300, seed=2301)
    with Engine(weights("pf"), 0) as e:
        whole = e.nj_joins(preds)
        e.set_option("ws_limit_mb", 1)
        chunked = e.nj_joins(preds)
        assert _same(whole, chunked)
        with pytest.raises(ValueError, match=r"N=400 sequences needs \d+ bytes of state per source .*workspace limit of 1048576 bytes"):
            e.nj_joins(_preds(1, 400, seed=1))
    assert_table(whole[0][2], whole[1][2], preds[2], 300)


def test_device_entry_point_and_call_counter(weights):
    B, N = 2, 37
    T = 2 * (N - 3) + 3
    preds = _preds(B, N, seed=2037)
    with Engine(weights("pf"), 0) as e:
        e.profile_reset()
        want = e.nj_joins(preds)
        assert e.profile_get("nj_joins")[0] == 1
        slots, lengths, flag = np.empty((B, T), np.int32), np.empty((B, T), np.float64), np.full(B, 7, np.uint8)
        bufs = [e.malloc(a.nbytes) for a in (preds, slots, lengths, flag)]
        try:
            e.h2d(bufs[0], preds)
            e.nj_joins_device(bufs[0], B, N, bufs[1], bufs[2], bufs[3])
            e.nj_joins_device(bufs[0], B, N, bufs[1], bufs[2], bufs[3])
            for host, dev in zip((slots, lengths, flag), bufs[1:]):
                e.d2h(host, dev)
            e.synchronize()
        finally:
            for ptr in bufs:
                e.free(ptr)
        assert e.profile_get("nj_joins")[0] == 3
        assert _same((slots, lengths, flag.astype(bool)), want)
        e.profile_reset()
        assert e.profile_get("nj_joins")[0] == 0
    for b in range(B):
        assert_table(slots[b], lengths[b], preds[b], N)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_flags_that_source_only(engines, bad):
    N = 40
    preds = _preds(3, N, seed=2040)
    clean = engines("pf").nj_joins(preds)
    dirty = preds.copy()
    dirty[1, 333] = bad
    slots, lengths, flag = engines("pf").nj_joins(dirty)
    assert flag.tolist() == [False, True, False] and not clean[2].any()
    for b in (0, 2):
        assert_table(slots[b], lengths[b], preds[b], N)


def test_refusals(weights):
    preds = _preds(1, 9, seed=9)
    T = 2 * (9 - 3) + 3
    slots, lengths, flag = np.full(T, -7, np.int32), np.full(T, -7.0), np.full(1, 7, np.uint8)
    with Engine(weights("pf"), 0) as e:
        lib, h = e._lib, e._h
        p, s, l, f = preds.ctypes.data, slots.ctypes.data, lengths.ctypes.data, flag.ctypes.data

        def refused(rc, text):
            assert rc == -1 and text.encode() in lib.pf_last_error(h), (rc, lib.pf_last_error(h))
            assert (slots == -7).all() and (lengths == -7.0).all() and flag[0] == 7

        for fn in (lib.pf_nj_joins, lib.pf_nj_joins_device):
            refused(fn(h, p, 1, 2, s, l, f), "neighbour joining needs N >= 3 sequences (got 2)")
            refused(fn(h, p, 0, 9, s, l, f), "bad dimensions B=0 N=9")
            refused(fn(h, None, 1, 9, s, l, f), "null buffer")
            refused(fn(h, p, 1, 9, None, l, f), "null buffer")
            refused(fn(h, p, 1, 9, s, None, f), "null buffer")
            refused(fn(h, p, 1, 9, s, l, None), "null buffer")
            refused(fn(h, p, 1, 65537, s, l, f), "their 2147516416 pairs each overflow a distance vector")
            refused(fn(h, p, 1, 60000, s, l, f), "above the workspace limit of 25769803776 bytes (option ws_limit_mb)")
        assert e.profile_get("nj_joins")[0] == 0
        with pytest.raises(ValueError, match="not the pairs of any number of sequences"):
            e.nj_joins(np.zeros(7, np.float32))
        got = e.nj_joins(preds[0])                   # the handle still works
    assert_table(got[0], got[1], preds[0], 9)


def test_tiled_distances_to_newick_text_end_to_end(engines):
    """pf_forward_tiled at 13 x 600 with M = 8, the joins on the device, the text from the table: hostio.nj_newick's
    bytes for the same distances."""
    e = engines("pf")
    idx = np.random.default_rng(1919).integers(0, 22, size=(2, 13, 600), dtype=np.uint8)
    out, _spread = e.forward_tiled(idx, 8)
    slots, lengths, flag = e.nj_joins(out)
    assert not flag.any()
    ids = [f"s{k}" for k in range(12)] + ["s0"]
    for b in range(2):
        assert hostio.newick_of_joins(slots[b], lengths[b], ids) == hostio.nj_newick(out[b], ids)
        assert hostio.newick_of_joins_py(slots[b], lengths[b], ids).encode() == hostio.nj_newick(out[b], ids)


def test_cli_runner_joins_a_large_tiled_files_tree_on_the_device(tmp_path, engines):
    """257 x 8 with --tile 200 -t through the runner (N >= NJ_DEVICE_MIN): <stem>.nj.nwk is hostio.nj_newick of the tiled
    distances, the device joined it, and the small file beside it went the host's way."""
    from phyloformer_amd import analyses, scheduler
    assert analyses.NJ_DEVICE_MIN is not None and analyses.NJ_DEVICE_MIN <= 257
    alpha = "ARNDCQEGHILKMFPSTWYVX-"
    alns = {"wide": np.random.default_rng(257).integers(0, 20, size=(257, 8), dtype=np.uint8),
            "small": np.random.default_rng(5).integers(0, 20, size=(5, 8), dtype=np.uint8)}
    (tmp_path / "in").mkdir()
    (tmp_path / "out").mkdir()
    for stem, a in alns.items():
        with open(tmp_path / "in" / f"{stem}.fa", "w") as fh:
            for k, row in enumerate(a):
                fh.write(f">t{k}\n{''.join(alpha[int(v)] for v in row)}\n")
    e = engines("pf")
    e.profile_reset()
    runner = scheduler.DirectoryRunner(e, str(tmp_path / "out"), trees=True, modes=[analyses.Tile(200)])
    stats = runner.run(sorted(str(p) for p in (tmp_path / "in").iterdir()))
    assert stats["nj_device"] == 1 and stats["tiled"] == 1 and e.profile_get("nj_joins")[0] == 1
    out, _spread = e.forward_tiled(alns["wide"], 200)
    assert (tmp_path / "out" / "wide.nj.nwk").read_bytes() == hostio.nj_newick(out, [f"t{k}" for k in range(257)])
    assert (tmp_path / "out" / "small.nj.nwk").read_bytes() == hostio.nj_newick(e.forward(alns["small"]), [f"t{k}" for k in range(5)])
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["small.nj.nwk", "small.phy", "wide.nj.nwk", "wide.phy",
                                                                    "wide.spread.phy", "wide.tile.tsv"]
