"""The trees the CLI writes, each described ONCE (``KINDS``), the records their tables travel in (``JoinTable``,
``SupportTables``), the one procedure that joins and refines them (``join_refine``) and the two host sides that answer to
the engine's method names (``NativeHost``: ``hostio``; ``PythonHost``: the statements).  ``DirectoryRunner`` picks its host
side once (``runner.host``); device or host is a choice of object where ``n`` meets a threshold.  DESIGN.md section 28."""
from __future__ import annotations

import importlib
from functools import partial
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from . import bionj, bme, nj, phylip
from .bootstrap import support_newick_py


class Kind(NamedTuple):
    name: str                       # its tree is <stem>.<name>.nwk
    start: str                      # the tree the search starts from: "nj" | "bionj"
    search: Optional[str]           # the Engine's / bme.py's search, None: the start tree itself
    flags: Tuple[str, ...]          # the CLI flags (besides -t) that switch it on, all of them
    stats: Tuple[str, ...]          # its keys of the run's stats, in the order of the summary
    threshold: Tuple[str, str]      # (module, constant): from that many sequences on it runs on the GPU thread

    def files(self, *endings: str) -> Tuple[str, ...]:
        """The files that label this kind's tree: ``<name>.<ending>``, NJ's without a name."""
        return tuple(e if self.name == "nj" else f"{self.name}.{e}" for e in endings)

    def minimum(self) -> Optional[int]:
        """The threshold as it is NOW (looked up at every use: None = the device path is off)."""
        return getattr(importlib.import_module(f".{self.threshold[0]}", __package__), self.threshold[1])


def reaches(minimum: Optional[int], n: int, floor: int = 0) -> bool:
    """Do files of ``n`` sequences (``floor`` at the least) take the device path that starts at ``minimum`` (None: off)?"""
    return minimum is not None and n >= max(floor, minimum)


# the flags beside -t, and what each does to the tree of --trees (the text of the refusal without -t)
FLAGS = {"--bme": "refines the tree of --trees", "--spr": "refines the tree of --trees",
         "--bionj": "writes a tree beside that of --trees"}
KINDS = (Kind("nj", "nj", None, (), (), ("analyses", "NJ_DEVICE_MIN")),
         Kind("bme", "nj", "bme_nni", ("--bme",), ("bme", "bme_steps", "bme_device", "bme_device_s"), ("bme", "BME_DEVICE_MIN")),
         Kind("spr", "nj", "bme_spr", ("--spr",), ("spr", "spr_steps", "spr_device", "spr_device_s"), ("bme", "SPR_DEVICE_MIN")),
         Kind("bionj", "bionj", None, ("--bionj",), ("bionj", "bionj_device", "bionj_device_s"), ("bionj", "BIONJ_DEVICE_MIN")),
         Kind("bionj.bme", "bionj", "bme_nni", ("--bionj", "--bme"), (), ("bme", "BME_DEVICE_MIN")),
         Kind("bionj.spr", "bionj", "bme_spr", ("--bionj", "--spr"), (), ("bme", "SPR_DEVICE_MIN")))
NJ = KINDS[0]
NJ_STARTED = tuple(k for k in KINDS if k.start == "nj")      # the kinds whose trees get supports and a consensus


def switched_on(flags) -> List[List[Kind]]:
    """The kinds ``flags`` adds to the tree of ``--trees``, in the groups that share a start table and a timer on the
    GPU thread: a search from the NJ tree alone, the BIONJ tree with its searches; a group's first kind owns its stats."""
    on = [k for k in KINDS[1:] if set(k.flags) <= set(flags)]
    return [[k for k in on if (k.name if k.start == "nj" else k.start) == head.name] for head in on if head.stats]


def refusals(flags, trees: bool, shard_sites: bool = False):
    """The texts with which ``infer_alns.py`` and the runner turn the flags of ``flags`` down, in their order."""
    for flag in flags:
        if not trees:
            yield f"{flag} {FLAGS[flag]}: give -t as well"
        if shard_sites:
            yield f"{flag} cannot be combined with --shard sites: the site-sharded runner writes NJ trees only"


class JoinTable(NamedTuple):
    """One tree as a join table (``Engine.nj_joins``' layout) and the moves of the search behind it."""
    slots: np.ndarray
    lengths: np.ndarray
    steps: int


class SupportTables(NamedTuple):
    """One file's tables of one kind behind its supports: its own tree (``slots`` None: its distances are not finite),
    its replicates' trees, and what the GPU thread already made of them (None: the writer thread's host side does it)."""
    slots: Optional[np.ndarray]
    lengths: np.ndarray
    rep_slots: np.ndarray
    rep_flag: np.ndarray
    results: Optional[tuple]         # join_supports' (count, transfer, depth) or join_transfers' seven arrays
    rep_lengths: np.ndarray
    consensus: Optional[tuple]       # join_consensus' results
    distances: Optional[tuple] = None      # join_distances' results over [own tree, replicates] (--treedist)


def with_stand_ins(slots: np.ndarray, bad) -> np.ndarray:
    """``slots [M, T]`` with a caterpillar where ``bad [M]`` is set (its joins are unspecified; the result is not used)."""
    return np.where(np.asarray(bad, dtype=bool)[:, None], bme.caterpillar_slots((slots.shape[1] + 3) // 2)[None, :], slots)


def join_refine(who, start: str, searches, preds: np.ndarray) -> dict:
    """By ``who`` - an ``Engine`` or a host side -: join every source of ``preds [M, P]`` into its ``start`` tree, then refine
    the tables by each of ``searches`` (``Kind.search``): ``{search: (slots, lengths, steps, bad)}``, None for the start tree
    itself; ``bad`` = non-finite distances (a source stopped at the move cap is used as it stands)."""
    slots, lengths, nonfinite = (who.bionj_joins if start == "bionj" else who.nj_joins)(preds)
    bad = np.asarray(nonfinite, dtype=bool)
    made = {None: (slots, lengths, np.zeros(len(bad), dtype=np.int32), bad)}
    first = with_stand_ins(slots, bad) if searches else None
    for search in searches:
        slots, lengths, steps, _length, status = getattr(who, search)(preds, first)
        made[search] = (slots, lengths, steps, bad | (status == bme.NONFINITE))
    return made


class Host:
    """A host side answers to the ``Engine``'s names for the computations on join tables (``nj_joins``, ``bionj_joins``,
    ``bme_nni``, ``bme_spr``, ``join_supports``, ``join_transfers``, ``join_consensus``, ``tree_fit``, ``tree_ols``, ``join_distances``, ``tree_root``) with its arguments and results,
    so an engine serves wherever a side does.  A host side formats as well: ``tree_text`` is ``(text, moves)`` of a kind's
    tree of a distance vector (``texts``; the BIONJ-started searches do not count their moves)."""

    def tree_text(self, kind: Kind, vec, ids):
        return self.texts[kind.name](vec, ids)


class NativeHost(Host):
    """The library's host code: texts are bytes."""

    def __init__(self):
        from . import hostio as h, weights_sites
        self.load_alignment, self.compress_sites = h.load_alignment, weights_sites.native_compress_sites
        self.phylip, self.nj, self.newick_of_joins = h.format_phylip, h.nj_newick, h.newick_of_joins
        self.nj_joins, self.bionj_joins, self.bme_nni, self.bme_spr = h.nj_joins_host, h.bionj_joins_host, h.bme_nni_host, h.bme_spr_host
        self.join_supports, self.join_transfers, self.join_consensus = h.join_supports_host, h.join_transfers_host, h.join_consensus_host
        self.tree_fit, self.tree_ols, self.join_distances = h.tree_fit_host, h.tree_ols_host, h.join_distances_host
        self.tree_root = h.tree_root_host
        self.nj_support = lambda pred, reps, ids, threads=1: h.nj_support(pred, reps, ids, threads=threads)
        self.texts = {"bme": lambda vec, ids: h.bme_newick(vec, ids, with_steps=True),
                      "spr": lambda vec, ids: h.spr_newick(vec, ids, with_steps=True),
                      "bionj": lambda vec, ids: (h.bionj_newick(vec, ids), 0),
                      "bionj.bme": lambda vec, ids: (h.bionj_refined_newick("bme", vec, ids), 0),
                      "bionj.spr": lambda vec, ids: (h.bionj_refined_newick("spr", vec, ids), 0)}


class PythonHost(Host):
    """The readable statements (``--python-io``): texts are str; the adapters to the Engine's signatures live here."""

    def __init__(self):
        from . import fasta, hostio, supports, weights_sites
        self.load_alignment, self.compress_sites = fasta.load_alignment, weights_sites.compress_sites
        self.newick_of_joins = hostio.newick_of_joins_py
        self.nj_joins, self.bionj_joins = partial(supports.joins_py, "nj"), partial(supports.joins_py, "bionj")
        self.bme_nni, self.bme_spr = partial(supports.refine_py, "bme_nni"), partial(supports.refine_py, "bme_spr")
        self.texts = {"bme": bme.bme_tree_py,
                      "spr": bme.spr_tree_py,
                      "bionj": lambda vec, ids: (bionj.bionj_newick_py(vec, ids), 0),
                      "bionj.bme": lambda vec, ids: (bionj.bionj_bme_newick_py(vec, ids), 0),
                      "bionj.spr": lambda vec, ids: (bionj.bionj_spr_newick_py(vec, ids), 0)}

    def phylip(self, vec, ids):
        return phylip.vec_to_phylip(vec, ids)[1]

    def tree_fit(self, preds, slots, lengths, patristic: bool = True):
        from .fit import tree_fit_batch_py
        out = tree_fit_batch_py(preds, slots, lengths)
        return out if patristic else (None, *out[1:])

    def tree_ols(self, preds, slots):
        from .ols import tree_ols_batch_py
        return tree_ols_batch_py(preds, slots)

    def tree_root(self, slots, lengths):
        from .root import tree_root_batch_py
        return tree_root_batch_py(slots, lengths)

    def join_distances(self, slots, lengths=None, flag=None):
        from .treedist import join_distances_batch_py
        return join_distances_batch_py(slots, lengths, flag)

    def nj(self, vec, ids):
        return nj.neighbor_joining(phylip.vec_to_phylip(vec, ids)[0].astype("float64"), ids)

    def nj_support(self, pred, reps, ids, threads: int = 1):
        return support_newick_py(pred, reps, ids)

    # (one source each, the Engine's ``[T]`` / ``[R, T]`` form; the statements take N and have no status)
    def join_supports(self, ref_slots, rep_slots, rep_flag):
        from .supports import split_supports
        return (*split_supports(ref_slots, rep_slots, (len(ref_slots) + 3) // 2, rep_flag), 0)

    def join_transfers(self, ref_slots, rep_slots, rep_flag, cutoff):
        from .supports import transfer_taxa, transfer_tuple
        return (*transfer_tuple(transfer_taxa(ref_slots, rep_slots, (len(ref_slots) + 3) // 2, rep_flag, cutoff)), 0)

    def join_consensus(self, rep_slots, rep_lengths, rep_flag, percent):
        from .consensus import join_consensus
        return join_consensus(rep_slots, (len(rep_slots[0]) + 3) // 2, rep_lengths, rep_flag, percent)
