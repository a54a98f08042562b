"""The description of the CLI's trees (``treekinds``) without a GPU: the kind table and what is derived from it, the
thresholds looked up at use, the one join-refine-flag procedure on a counting stand-in engine, and the two host sides
against each other."""
import numpy as np
import pytest

from helpers import bme_check as bc
from phyloformer_amd import analyses, bionj, bme, consensus, hostio, supports, treekinds
from phyloformer_amd.treekinds import KINDS, NativeHost, PythonHost, join_refine, reaches


def test_the_derived_names_are_todays():
    assert supports.SEARCHES == {"nj": None, "bme": "bme_nni", "spr": "bme_spr"}
    assert supports.SUFFIXES == {"nj": ("sup.nwk", "tbe.nwk"), "bme": ("bme.sup.nwk", "bme.tbe.nwk"), "spr": ("spr.sup.nwk", "spr.tbe.nwk")}
    assert supports.INSTABILITY_SUFFIXES == {"nj": ("instability.tsv", "branches.tsv", "branches.nwk"),
                                             "bme": ("bme.instability.tsv", "bme.branches.tsv", "bme.branches.nwk"),
                                             "spr": ("spr.instability.tsv", "spr.branches.tsv", "spr.branches.nwk")}
    assert consensus.SUFFIXES == {"nj": "con.nwk", "bme": "bme.con.nwk", "spr": "spr.con.nwk"}
    assert [list(d) for d in (supports.SEARCHES, supports.SUFFIXES, supports.INSTABILITY_SUFFIXES, consensus.SUFFIXES)] == [["nj", "bme", "spr"]] * 4


def test_the_six_kinds():
    assert [(k.name, k.start, k.search, k.flags, f"{k.name}.nwk", k.stats) for k in KINDS] == [
        ("nj", "nj", None, (), "nj.nwk", ()),
        ("bme", "nj", "bme_nni", ("--bme",), "bme.nwk", ("bme", "bme_steps", "bme_device", "bme_device_s")),
        ("spr", "nj", "bme_spr", ("--spr",), "spr.nwk", ("spr", "spr_steps", "spr_device", "spr_device_s")),
        ("bionj", "bionj", None, ("--bionj",), "bionj.nwk", ("bionj", "bionj_device", "bionj_device_s")),
        ("bionj.bme", "bionj", "bme_nni", ("--bionj", "--bme"), "bionj.bme.nwk", ()),
        ("bionj.spr", "bionj", "bme_spr", ("--bionj", "--spr"), "bionj.spr.nwk", ())]
    assert list(treekinds.FLAGS) == ["--bme", "--spr", "--bionj"]
    names = lambda flags: [[k.name for k in group] for group in treekinds.switched_on(flags)]      # noqa: E731
    assert names(()) == [] and names({"--spr"}) == [["spr"]] and names({"--bionj"}) == [["bionj"]]
    assert names({"--bme", "--spr", "--bionj"}) == [["bme"], ["spr"], ["bionj", "bionj.bme", "bionj.spr"]]
    assert next(treekinds.refusals(["--bionj", "--bme"], trees=False)) == "--bionj writes a tree beside that of --trees: give -t as well"
    assert list(treekinds.refusals(["--bme", "--bionj"], trees=False, shard_sites=True)) == [
        "--bme refines the tree of --trees: give -t as well",
        "--bme cannot be combined with --shard sites: the site-sharded runner writes NJ trees only",
        "--bionj writes a tree beside that of --trees: give -t as well",
        "--bionj cannot be combined with --shard sites: the site-sharded runner writes NJ trees only"]
    assert list(treekinds.refusals(["--bme", "--spr", "--bionj"], trees=True)) == []


def test_a_threshold_is_looked_up_when_it_is_used(monkeypatch):
    homes = {"nj": (analyses, "NJ_DEVICE_MIN"), "bme": (bme, "BME_DEVICE_MIN"), "spr": (bme, "SPR_DEVICE_MIN"),
             "bionj": (bionj, "BIONJ_DEVICE_MIN"), "bionj.bme": (bme, "BME_DEVICE_MIN"), "bionj.spr": (bme, "SPR_DEVICE_MIN")}
    for k in KINDS:
        module, name = homes[k.name]
        assert k.minimum() == getattr(module, name)
        monkeypatch.setattr(module, name, 7)
        assert k.minimum() == 7 and reaches(k.minimum(), 7) and not reaches(k.minimum(), 6) and not reaches(k.minimum(), 7, 8)
        monkeypatch.setattr(module, name, None)
        assert k.minimum() is None and not reaches(k.minimum(), 10 ** 6)
        monkeypatch.setattr(module, name, 2)
        assert reaches(k.minimum(), 3, 3) and not reaches(k.minimum(), 2, 3)      # (the floor: no table below three sequences)


class Engine:
    """Counts and keeps its calls; the joins and searches are the host twins'."""

    def __init__(self, capped=None):
        self.calls, self.capped = [], capped

    def _joins(self, name, preds):
        self.calls.append((name, preds))
        return getattr(hostio, name + "_host")(preds)

    def nj_joins(self, preds):
        return self._joins("nj_joins", preds)

    def bionj_joins(self, preds):
        return self._joins("bionj_joins", preds)

    def _search(self, name, preds, starts):
        self.calls.append((name, preds, starts))
        slots, lengths, steps, length, status = getattr(hostio, name + "_host")(preds, starts)
        if self.capped is not None:                                 # (a stub: that source stopped at the move cap)
            status[self.capped] = bme.CAPPED
        return slots, lengths, steps, length, status

    def bme_nni(self, preds, starts):
        return self._search("bme_nni", preds, starts)

    def bme_spr(self, preds, starts):
        return self._search("bme_spr", preds, starts)


def _native():
    from phyloformer_amd import build
    build.build()


def _sources(n, count, seed):
    base = bc.random_tree_distances(n, seed)
    noise = np.random.default_rng(seed).standard_normal((count,) + base.shape)
    return np.abs(base * (1 + 0.25 * noise)).astype(np.float32)


@pytest.mark.parametrize("kind", [k for k in KINDS if k.search is not None], ids=lambda k: k.name)
def test_join_refine_flags_and_stands_in(kind):
    """Three sources of N = 5, the second with a NaN: it is bad for the start tree and the search, the search saw the
    caterpillar for it and the join's table for the others; one join call and one search call."""
    _native()
    preds = _sources(5, 3, 17)
    preds[1, 3] = np.nan
    engine = Engine()
    made = join_refine(engine, kind.start, [kind.search], preds)
    assert [c[0] for c in engine.calls] == [f"{kind.start}_joins", kind.search] and set(made) == {None, kind.search}
    assert all(c[1] is preds for c in engine.calls)
    joined = getattr(hostio, f"{kind.start}_joins_host")(preds)[0]
    given = engine.calls[1][2]
    assert given[1].tolist() == bme.caterpillar_slots(5).tolist() == [0, 1, 0, 2, 0, 3, 4]
    assert np.array_equal(given[[0, 2]], joined[[0, 2]]) and given.dtype == np.int32
    for slots, lengths, steps, bad in made.values():
        assert bad.tolist() == [False, True, False] and bad.dtype == bool
        assert slots.shape == lengths.shape == (3, 7) and len(steps) == 3
    want = getattr(hostio, kind.search + "_host")(preds[[0, 2]], joined[[0, 2]])
    assert np.array_equal(made[kind.search][0][[0, 2]], want[0]) and made[kind.search][2][[0, 2]].tolist() == want[2].tolist()
    assert not made[None][2].any()                                  # the start tree has no moves


def test_a_source_stopped_at_the_move_cap_is_not_bad():
    _native()
    preds = _sources(5, 3, 17)
    made = join_refine(Engine(capped=2), "nj", ["bme_nni"], preds)
    assert made["bme_nni"][3].tolist() == [False, False, False]
    preds[0, 0] = np.inf
    assert join_refine(Engine(capped=2), "nj", ["bme_nni"], preds)["bme_nni"][3].tolist() == [True, False, False]


def test_the_two_host_sides_agree():
    """One file of 6 sequences with 4 replicates, one of them with a NaN: join tables (both starts, both searches), supports,
    transfers and consensus of the native and the Python side - integers equal, lengths bit for bit (as
    tests/test_consensus_host.py compares the consensus of the two sides)."""
    _native()
    native, python = NativeHost(), PythonHost()
    every = _sources(6, 5, 23)                                      # the file's own distances first
    every[3, 7] = np.nan
    for start in ("nj", "bionj"):
        a, b = (join_refine(side, start, ["bme_nni", "bme_spr"], every) for side in (native, python))
        assert list(a) == list(b) == [None, "bme_nni", "bme_spr"]
        for search in a:
            (slots, lengths, steps, bad), (pslots, plengths, psteps, pbad) = a[search], b[search]
            assert bad.tolist() == pbad.tolist() == [False, False, False, True, False], (start, search)
            ok = ~bad
            assert np.array_equal(slots[ok], pslots[ok]) and np.asarray(steps)[ok].tolist() == np.asarray(psteps)[ok].tolist(), (start, search)
            assert lengths[ok].astype(np.float64).tobytes() == np.asarray(plengths, dtype=np.float64)[ok].tobytes(), (start, search)
        if start == "nj":
            tables = a
    for search in tables:
        slots, lengths, _steps, bad = tables[search]
        ref, reps, rep_lengths, flag = slots[0], slots[1:], lengths[1:], bad[1:]
        got, want = native.join_supports(ref, reps, flag), python.join_supports(ref, reps, flag)
        assert len(got) == len(want) == 4 and [np.asarray(x).tolist() for x in got] == [np.asarray(x).tolist() for x in want]
        for cutoff in (30, 100):
            got, want = native.join_transfers(ref, reps, flag, cutoff), python.join_transfers(ref, reps, flag, cutoff)
            assert len(got) == len(want) == 8 and [np.asarray(x).tolist() for x in got] == [np.asarray(x).tolist() for x in want]
        got, want = native.join_consensus(reps, rep_lengths, flag, 60), python.join_consensus(reps, rep_lengths, flag, 60)
        assert int(got[0]) == want.n_splits and int(got[7]) == want.status == 0
        for k in (1, 2, 3, 5):
            assert got[k].tolist() == list(want[k]), (search, k)
        for k in (4, 6):
            assert got[k].tobytes() == np.asarray(want[k], dtype=np.float64).tobytes(), (search, k)
    # the texts: bytes from the native side, the same characters from the Python one
    ids = [f"t{i}" for i in range(6)]
    for kind in KINDS[1:]:
        (text, moves), (ptext, pmoves) = native.tree_text(kind, every[0], ids), python.tree_text(kind, every[0], ids)
        assert isinstance(text, bytes) and text.decode() == ptext and moves == pmoves, kind.name
    assert native.nj_support(every[0], every[1:], ids).decode() == python.nj_support(every[0], every[1:], ids)
    assert native.phylip(every[0], ids).decode() == python.phylip(every[0], ids)
