"""The inputs and the statement's results the tests of the per-taxon transfer counts share (tests/test_transfers_host.py,
tests/test_transfers_native.py, tests/test_gpu_transfers.py): computed once per shape and never changed."""
import functools

import numpy as np

from helpers import support_inputs as si
from phyloformer_amd import supports

CUTOFFS = (0, 30, 100)
# the order of the native entry points' results (branch_moves may be None)
NAMES = ("count", "transfer", "depth", "moves", "used", "capped", "branch_moves", "status")


@functools.lru_cache(maxsize=None)
def statement(n: int, r: int, b: int, cutoff: int) -> dict:
    """``supports.transfer_taxa`` of source ``b`` of ``support_inputs.sources(n, r)``."""
    ref, reps, flag = si.sources(n, r)
    return supports.transfer_taxa(ref[b], reps[b], n, flag[b], cutoff)


@functools.lru_cache(maxsize=None)
def mixed(n: int):
    """One source ``(ref int32 [T], reps int32 [5][T], flag bool [5])``: two unrelated random trees, the reference itself,
    a replicate passed with its flag (a table of zeros, never read) and a noisy copy of the reference."""
    ref, noisy = si.noisy_tables(n, 1)
    reps = np.stack([*si.unrelated_tables(n, 2), ref, np.zeros_like(ref), noisy[0]])
    flag = np.array([False, False, False, True, False])
    reps.setflags(write=False)
    flag.setflags(write=False)
    return ref, reps, flag


def as_lists(out) -> dict:
    """A native entry point's tuple of one source as the statement's dict (and ``status``)."""
    return {k: (None if v is None else np.asarray(v).tolist()) for k, v in zip(NAMES, out)}


def assert_same(got, want):
    """Two native results: the same shapes, types and integers."""
    for name, g, w in zip(NAMES, got, want):
        if g is None or w is None:
            assert g is None and w is None, name
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(g, w), name


def _table(children, root, n: int) -> np.ndarray:
    """The join table of a tree given by its children lists (``root``: three children, every other inner node two): the
    joins in post-order, a cluster staying in the slot of its first child."""
    slots, slot_of = [], {}

    def visit(v):
        if v < n:
            slot_of[v] = v
            return
        a, b = children[v]
        visit(a)
        visit(b)
        slots.extend((slot_of[a], slot_of[b]))
        slot_of[v] = slot_of[a]
    for c in children[root]:
        visit(c)
    table = np.array(slots + [slot_of[c] for c in children[root]], dtype=np.int32)
    assert table.size == 2 * (n - 3) + 3
    return table


def _graft(children, root, leaf: int, rng):
    """``leaf`` on a random edge of the tree: a new node between a random non-root node and its parent."""
    edges = [(p, i) for p, cs in children.items() for i in range(len(cs))]
    p, i = edges[int(rng.integers(len(edges)))]
    new = max(max(children), leaf) + 1
    children[new] = [children[p][i], leaf]
    children[p][i] = new


@functools.lru_cache(maxsize=None)
def planted_rogue(n: int, r: int = 10):
    """``(ref int32 [T], reps int32 [r][T])``: one random tree on the sequences ``0 .. n - 2`` (every sequence on a random
    edge of the tree so far), with sequence ``n - 1`` regrafted on a random edge in the reference and in each replicate."""
    rng = np.random.default_rng(n)
    root = n
    base = {root: [0, 1, 2]}
    for leaf in range(3, n - 1):
        _graft(base, root, leaf, rng)
    tables = []
    for _ in range(r + 1):
        tree = {k: list(v) for k, v in base.items()}
        _graft(tree, root, n - 1, rng)
        tables.append(_table(tree, root, n))
    out = np.stack(tables)
    out.setflags(write=False)
    return out[0], out[1:]
