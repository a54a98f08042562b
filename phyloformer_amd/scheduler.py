"""Batched, shape-bucketed, I/O-overlapped inference over a directory of alignments.

The reference loop (/root/reference/infer_alns.py:95-123) is strictly serial:
parse one FASTA, run one forward, format and write one PHYLIP file.  On an
MI355X the forward of a 60 x 500 alignment takes 2.3 ms — less than CPython
needs for the parsing and formatting around it — so the CLI would be host-bound
by a wide margin.  This module keeps the GPU fed:

* loader threads parse FASTA files ahead of the GPU (native parser, GIL released);
* alignments are *bucketed by shape* ``(N, L)``; a bucket is launched when it
  holds ``batch`` alignments (or a token budget's worth), whatever order the
  files arrived in, and all partial buckets are flushed at the end;
* writer threads format and write the PHYLIP (and NJ) files of batch ``k`` while
  the GPU runs batch ``k + 1``;
* two engines on two host threads (``--gpu-streams``) keep the GPU busy across the
  host-side gaps of the synchronous ``pf_forward``;
* ``run_multi_device`` shards the *files* over several GPUs, one process per
  GPU, no collective (alignment-level data parallelism, SURVEY.md §8e way 1);
* ``--shard sites`` (``SiteShardedRunner``) spreads every alignment over the GPUs instead
  (SURVEY.md §8e way 2): each rank parses the file, keeps its block of sites and calls
  ``pf_forward_sharded`` - n_blocks + 1 RCCL all-reduces per launch - and rank 0 writes the
  outputs.  The ranks meet through ``rendezvous.TcpGroup`` and walk the files in ONE
  deterministic order (collectives must be issued in the same order everywhere).

Every alignment is computed independently inside a launch and no launch parameter
that affects the order of a sum depends on the batch size: an alignment's distances
are bit-identical whatever batch it travels in (tests/test_gpu_parity.py,
tests/test_cli_gpu.py).
"""
from __future__ import annotations

import itertools
import json
import os
import queue
import subprocess
import sys
import threading
import time
from collections import OrderedDict, deque
from concurrent.futures import Future, ThreadPoolExecutor
from contextlib import closing
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .analyses import Analysis, sub_batches
from .treekinds import KINDS, JoinTable, Kind, NativeHost, PythonHost, join_refine, reaches, refusals, switched_on

# one launch should carry about this many (pair, site) tokens: 16 alignments of 60 x 500
# (3.6 GB of residual stream), the size bench.py measures the headline number at
TOKEN_BUDGET = 16 * 1770 * 500


# files per native load call (FastaBatch): enough to amortise a thread-pool start over many small files, few enough
# that the first launch does not wait for the whole directory
FILES_PER_LOAD = 256
# a partial shape bucket is launched after this many further load calls (bounds what the native pipeline keeps parsed)
STALE_LOADS = 16


def auto_batch(n_seqs: int, n_sites: int, max_batch: int = 4096, token_budget: int = TOKEN_BUDGET) -> int:
    """Alignments per launch for shape ``(N, L)``: fill the token budget, at least 1."""
    tokens = max(1, n_seqs * (n_seqs - 1) // 2 * n_sites)
    return int(min(max_batch, max(1, token_budget // tokens)))


# the refusal of --delta with --shard sites, in the wording of treekinds.refusals
DELTA_SHARD_SITES = "--delta cannot be combined with --shard sites: the site-sharded runner writes distances and NJ trees only"
# the refusals of --fit, in the wording of treekinds.refusals
FIT_NEEDS_TREES = "--fit measures the trees of --trees: give -t as well"
FIT_SHARD_SITES = "--fit cannot be combined with --shard sites: the site-sharded runner writes NJ trees only"
# the refusals of --ols, in the same wording
OLS_NEEDS_TREES = "--ols re-estimates the branch lengths of the trees of --trees: give -t as well"
OLS_SHARD_SITES = "--ols cannot be combined with --shard sites: the site-sharded runner writes NJ trees only"
# the refusals of --root, in the same wording
ROOT_NEEDS_TREES = "--root roots the trees of --trees: give -t as well"
ROOT_SHARD_SITES = "--root cannot be combined with --shard sites: the site-sharded runner writes NJ trees only"
HEARTBEAT = "#pf-heartbeat"      # stderr line prefix of a site-sharded worker's sign of life (swallowed by the launcher)
MAX_SEQS = 200     # SEQ2PAIR = seq2pair(200), /root/reference/phyloformer/model.py:39


def single_sequence_error(batch: int = 1) -> RuntimeError:
    """An alignment of ONE sequence parses (data.py:11-31) but has no pair: the reference's forward fails on the empty
    tensor in attention.py:193 with this RuntimeError (tests/golden/cli_bad_entry.json, from the real CLI)."""
    return RuntimeError(f"cannot reshape tensor of 0 elements into shape [{batch}, -1, 0, 64] because the unspecified "
                        "dimension size -1 can be any value and is ambiguous")


def over_seq_cap(n_seqs, modes: Sequence[Analysis] = ()):
    """More than ``MAX_SEQS`` sequences, and none of the run's modes lifts the cap for such a file
    (``Analysis.lifts_seq_cap``)?  Elementwise: an int or the array of a FastaBatch."""
    over = np.asarray(n_seqs) > MAX_SEQS
    for m in modes:
        over = over & ~np.asarray(m.lifts_seq_cap(n_seqs), dtype=bool)
    return over


def too_many_seqs(n_seqs: int, modes: Sequence[Analysis] = ()) -> Optional[Exception]:
    """The reference's forward refuses more than 200 sequences (ValueError, adaptable_seq2pair, model.py:24-28) and fails
    on a single one (RuntimeError, attention.py:193) when the loop reaches that file; the runner raises the same error at
    the same place in the order - after the files in front of it.  The cap is a question to the run's ``modes``."""
    if over_seq_cap(n_seqs, modes):
        return ValueError(f"n_seqs must be smaller or equal to {MAX_SEQS} (or pre-compute a larger global_seq2pair)")
    if n_seqs == 1:
        return single_sequence_error()
    return None


def has_fasta_ext(alnpath: str) -> bool:
    """Checks if a path ends in .fa or .fasta (infer_alns.py:36-38)."""
    return alnpath.lower().endswith(".fa") or alnpath.lower().endswith(".fasta")


def non_fasta_entry(paths: Sequence[str]) -> Optional[Tuple[int, ValueError]]:
    """``(k, error)`` of the first entry without a FASTA extension - the reference's ``ValueError`` for it
    (infer_alns.py:100-103) - or None."""
    for k, p in enumerate(paths):
        if not has_fasta_ext(p):
            return k, ValueError("Input files must be fasta files (.fa or .fasta). Got " f"{p}")
    return None


def require_fasta_entries(paths: Sequence[str]):
    """The modes without a counterpart in the reference refuse such a directory up front."""
    bad = non_fasta_entry(paths)
    if bad is not None:
        raise bad[1]


def slice_paths(paths: Sequence[str], rank: int, world: int) -> List[str]:
    """Deterministic share of ``paths`` for worker ``rank`` of ``world``: files are sorted by
    (size, name) and dealt round-robin, so every worker sees the same mix of shapes."""
    if world <= 1:
        return list(paths)

    def key(p):
        try:
            return (os.path.getsize(p), p)
        except OSError:
            return (0, p)
    return sorted(paths, key=key)[rank::world]


class Entry:
    """One alignment of a launch group: its file, what the launch batches - the parsed residues (``np.stack``) or, on the
    native path, ``(FastaBatch, file)`` (``hostio.gather``; residues and ids stay in the library until the launch gathers
    them / the writer formats them) - and its ids."""
    __slots__ = ("path", "source", "_ids")

    def __init__(self, path: str, source, ids: Optional[List[str]] = None):
        self.path, self.source, self._ids = path, source, ids

    def ids(self) -> List[str]:
        return self.source[0].ids(self.source[1]) if self._ids is None else self._ids


class DirectoryRunner:
    """Runs every alignment of a file list through the engine(s) and writes the outputs.

    ``engine`` may be one engine or a list: each engine gets its own host thread (one HIP stream each),
    so the host-side gaps of one synchronous ``pf_forward`` (index copy, result copy, Python between
    calls) are filled by the other's kernels — measured 486 -> 501 alignments/s at 60 x 500 with two.

    ``modes`` are the per-alignment analyses of the run (``analyses.Analysis`` instances): at most one of them replaces
    the launch's forward, the others follow it."""

    def __init__(self, engine, out_dir: str, trees: bool = False, batch: int = 0,
                 io_threads: int = 4, native_io: bool = True, progress=None, modes: Sequence[Analysis] = (),
                 bme: bool = False, spr: bool = False, bionj: bool = False, delta: bool = False, fit: bool = False, ols: bool = False,
                 treedist: bool = False, treedist_ref: Optional[str] = None, root: Optional[str] = None):
        # with --trees: <stem>.bme.nwk / .spr.nwk / .bionj.nwk (and .bionj.bme.nwk / .bionj.spr.nwk) as well (treekinds.KINDS)
        self.flags = [flag for flag, on in (("--bionj", bionj), ("--bme", bme), ("--spr", spr)) if on]
        if not trees and self.flags:
            raise ValueError(next(refusals(self.flags, trees)))
        self.kind_groups = switched_on(self.flags)
        if fit and not trees:
            raise ValueError(FIT_NEEDS_TREES)
        self.delta = delta            # --delta: <stem>.delta.tsv / .delta.phy / .delta.hist.tsv of every launch's distances
        # --fit: <stem>.fit.tsv and, of every written kind, <stem>[.<kind>].fit.taxa.tsv / .patristic.phy (fit.py)
        self.fit = fit
        if ols and not trees:
            raise ValueError(OLS_NEEDS_TREES)
        # --ols: <stem>.ols.tsv and, of every written kind, <stem>[.<kind>].ols.nwk: its table with least-squares lengths (ols.py)
        self.ols = ols
        # --treedist: <stem>.treedist.tsv, every pair of the written kinds and the tree of --treedist-ref DIR (treedist.py)
        self.treedist, self.treedist_ref = bool(treedist or treedist_ref), treedist_ref
        if self.treedist:
            from . import treedist as TD
            from .analyses import Bootstrap
            boots = [m for m in modes if isinstance(m, Bootstrap)]
            if not trees:
                raise ValueError(TD.NEEDS_TREES)
            if not self.kind_groups and not treedist_ref and not boots:
                raise ValueError(TD.NOTHING_TO_COMPARE)
            for m in boots:
                m.treedist = True
        if root and not trees:
            raise ValueError(ROOT_NEEDS_TREES)
        if root:
            from .root import METHODS
            if root not in METHODS:
                raise ValueError(f"--root takes one of {', '.join(METHODS)} (got {root})")
        # --root mad|midpoint: <stem>.root.tsv and, of every written kind, <stem>[.<kind>].rooted.nwk: its table rooted (root.py)
        self.root = root
        self._made = threading.local()        # the tables device_tables made on this GPU thread for the launch in hand
        self.engines = list(engine) if isinstance(engine, (list, tuple)) else [engine]
        self.out_dir = out_dir
        self.trees = trees
        self.batch = batch            # 0 = auto per shape
        self.io_threads = max(1, io_threads)
        self.native_io = native_io
        self.host = NativeHost() if native_io else PythonHost()      # whoever computes on the loader and writer threads
        # (bytes from the native side, text from the Python one; the table of the distances ``nj`` joins gives ``nj``'s bytes)
        self._load, self.phylip, self.newick_of_joins = self.host.load_alignment, self.host.phylip, self.host.newick_of_joins
        self.progress = progress
        self.stats = {"alignments": 0, "launches": 0, "forward_s": 0.0, "load_wait_s": 0.0,
                      "write_wait_s": 0.0, "shapes": {}, "gpu_streams": len(self.engines)}
        for kinds in self.kind_groups:
            self.stats.update({key: 0.0 if key.endswith("_s") else 0 for key in kinds[0].stats})
        if delta:
            self.stats.update({"delta": 0, "delta_s": 0.0})
        if fit:
            self.stats.update({"fit": 0, "fit_s": 0.0})
        if ols:
            self.stats.update({"ols": 0, "ols_s": 0.0})
        if self.treedist:
            self.stats.update({"treedist": 0, "treedist_s": 0.0, "treedist_ref_missing": 0})
        if root:
            self.stats.update({"root": 0, "root_s": 0.0})
        self.modes = list(modes)
        for m in self.modes:
            m.bind(self.modes)
            self.stats.update(m.stats())
        self._forwarder = next((m for m in self.modes if m.forward is not None), None)
        self._followers = [m for m in self.modes if m.follow is not None]
        self._lock = threading.Lock()

    # -- stages -----------------------------------------------------------------------------
    def nj(self, vec: np.ndarray, ids: List[str]):
        """The neighbour-joining tree of a distance vector, from the same side as ``phylip`` (infer_alns.py:120-123)."""
        return self.host.nj(vec, ids)

    def device_tables(self, engine, n: int, preds: np.ndarray, kinds: Sequence[Kind]) -> dict:
        """On the GPU thread, from the threshold of ``kinds[0]`` on (3 sequences at the least), which books the device's
        files and seconds: every file's joins of the kinds' start tree and, for each kind from its own threshold on, their
        refinement.  ``{kind name: [JoinTable, None for a non-finite file]}``; None or missing keeps the host's path."""
        head = kinds[0]
        if not reaches(head.minimum(), n, 3):
            return {}
        t0 = time.perf_counter()
        run = [k for k in kinds if k.search is not None and reaches(k.minimum(), n)]
        made = join_refine(engine, head.start, [k.search for k in run], preds)
        out = {k.name: [None if bad else JoinTable(s, l, int(moves)) for s, l, moves, bad in zip(*made[k.search])]
               for k in kinds if k.search is None or k in run}
        self.book(**{f"{head.name}_device": sum(t is not None for t in out[head.name]), f"{head.name}_device_s": time.perf_counter() - t0})
        getattr(self._made, "tables", {}).update(out)
        return out

    def _write_trees(self, group: list, preds: np.ndarray, tables, kind: Kind):
        """``<stem>.<kind>.nwk`` of some files of a launch, on a writer thread: formatted from the device's table where
        there is one, joined and refined on the host where not."""
        moves = 0
        for k, (e, pred) in enumerate(zip(group, preds)):
            ids = e.ids()
            table = tables[k] if tables is not None else None
            text, steps = (self.host.tree_text(kind, pred, ids) if table is None else
                           (self.newick_of_joins(table.slots, table.lengths, ids), table.steps))
            self.put(e.path, f"{kind.name}.nwk", text)
            moves += steps
        if kind.stats:
            self.book(**{kind.name: len(group)}, **({f"{kind.name}_steps": moves} if kind.search else {}))

    def delta_arrays(self, engine, preds: np.ndarray):
        """``--delta`` on the GPU thread, behind the forward: ``Engine.delta`` of the launch's distances (None below four
        sequences, which have no quartet); books its seconds."""
        from .delta import BINS, MIN_SEQS, n_of_pairs
        if n_of_pairs(preds.shape[1]) < MIN_SEQS:
            return None
        t0 = time.perf_counter()
        arrays = engine.delta(preds, bins=BINS)
        self.book(delta_s=time.perf_counter() - t0)
        return arrays

    def _write_delta(self, group: list, arrays):
        """The three files of ``--delta`` of some files of a launch, on a writer thread: the means derived from the
        integers (``delta.delta_scores``); ``nan`` and 0 quartets counted for a file without a quartet or whose distances
        are not finite."""
        from . import delta as D
        for k, e in enumerate(group):
            ids = e.ids()
            if arrays is None or arrays[2][k]:
                scores, hist = D.no_scores(len(ids)), np.zeros(D.BINS, dtype=np.int64)
            else:
                scores, hist = D.delta_scores(arrays[0][k], arrays[1][k], len(ids)), arrays[1][k]
            self.put(e.path, "delta.tsv", D.delta_tsv(ids, scores))
            self.put(e.path, "delta.phy", self.phylip(D.pair_vector(scores), ids))
            self.put(e.path, "delta.hist.tsv", D.hist_tsv(hist))
        self.book(delta=len(group))

    def written_kinds(self) -> List[Kind]:
        """The kinds whose trees a run with ``--trees`` writes, in the order of ``KINDS``."""
        on = {k.name for kinds in self.kind_groups for k in kinds}
        return [k for k in KINDS if k is KINDS[0] or k.name in on]

    def table_of(self, kind: Kind, k: int, pred: np.ndarray, tables: dict) -> Optional[JoinTable]:
        """On a writer thread, the table behind the written tree of ``kind`` of file ``k`` of a group (three sequences at the
        least): the device's (``tables``) or, as the tree's text was, joined and refined on the host; None for distances that
        are not finite."""
        if tables.get(kind.name) is not None:
            return tables[kind.name][k]
        if kind.name in tables:
            return None
        search = [kind.search] if kind.search else []
        slots, lengths, _steps, bad = join_refine(self.host, kind.start, search, pred[None])[kind.search]
        return None if bad[0] else JoinTable(slots[0], lengths[0], 0)

    def fit_arrays(self, engine, n: int, preds: np.ndarray) -> dict:
        """``--fit`` on the GPU thread: ``Engine.tree_fit`` of the launch's distances on the tables that were made on this
        thread (``device_tables``), one call for all their kinds, from ``fit.FIT_DEVICE_MIN`` sequences on; a file without
        a table (distances that are not finite) gets a table of zeros, which is none (status 2).  ``{kind name:
        (patristic, rows, worst_j, status)}``; the other kinds are the writer thread's.  Books its seconds."""
        from . import fit as F
        made = {name: tables for name, tables in getattr(self._made, "tables", {}).items() if tables is not None}
        if not made or not reaches(F.FIT_DEVICE_MIN, n, F.MIN_SEQS):
            return {}
        t0 = time.perf_counter()
        width = F.table_len(n)
        slots = np.zeros((len(preds), len(made), width), dtype=np.int32)
        lengths = np.zeros((len(preds), len(made), width), dtype=np.float64)
        for m, tables in enumerate(made.values()):
            for b, table in enumerate(tables):
                if table is not None:
                    slots[b, m], lengths[b, m] = table.slots, table.lengths
        out = engine.tree_fit(preds, slots, lengths)
        self.book(fit_s=time.perf_counter() - t0)
        return {name: tuple(a[:, m] for a in out) for m, name in enumerate(made)}

    def _write_fit(self, group: list, preds: np.ndarray, tables: dict, fits: dict):
        """The files of ``--fit`` of some files of a launch, on a writer thread: of every written kind the GPU thread's
        arrays where it made them (``fits``), else the twin's on its table - the device's (``tables``) or, as the tree's
        text was, joined and refined on the host; ``nan`` for fewer than three sequences, distances or lengths that are
        not finite."""
        from . import fit as F
        t0 = time.perf_counter()
        for k, (e, pred) in enumerate(zip(group, preds)):
            ids = e.ids()
            n, lines = len(ids), []
            for kind in self.written_kinds():
                arrays = None
                if kind.name in fits:
                    arrays = tuple(a[k] for a in fits[kind.name])
                elif n >= F.MIN_SEQS:
                    table = self.table_of(kind, k, pred, tables)
                    if table is not None:
                        arrays = self.host.tree_fit(pred, table.slots, table.lengths)
                if arrays is None or arrays[3]:
                    scores, tree = F.no_scores(n), np.full(n * (n - 1) // 2, np.nan, dtype=np.float32)
                else:
                    scores, tree = F.fit_scores(pred, arrays[1], arrays[2], n), arrays[0].astype(np.float32)
                lines.append((kind.name, scores))
                self.put(e.path, kind.files("fit.taxa.tsv")[0], F.taxa_tsv(ids, scores))
                self.put(e.path, kind.files("patristic.phy")[0], self.phylip(tree, ids))
            self.put(e.path, "fit.tsv", F.fit_tsv(lines))
        self.book(fit=len(group), fit_s=time.perf_counter() - t0)

    def ols_arrays(self, engine, n: int, preds: np.ndarray) -> dict:
        """``--ols`` on the GPU thread: ``Engine.tree_ols`` of the launch's distances on the tables that were made on this
        thread (``device_tables``), one call for all their kinds, from ``ols.OLS_DEVICE_MIN`` sequences on, followed by one
        ``Engine.tree_fit`` of every table with its own and with the OLS lengths; a file without a table (distances that are
        not finite) gets a table of zeros, which is none (status 2).  ``{kind name: (ols, status, rows [.., 2, n, 6], worst_j
        [.., 2, n])}``; the other kinds are the writer thread's.  Books its seconds."""
        from . import fit as F, ols as O
        made = {name: tables for name, tables in getattr(self._made, "tables", {}).items() if tables is not None}
        if not made or not reaches(O.OLS_DEVICE_MIN, n, F.MIN_SEQS):
            return {}
        t0 = time.perf_counter()
        width, m = F.table_len(n), len(made)
        slots = np.zeros((len(preds), m, width), dtype=np.int32)
        lengths = np.zeros((len(preds), m, width), dtype=np.float64)
        for k, tables in enumerate(made.values()):
            for b, table in enumerate(tables):
                if table is not None:
                    slots[b, k], lengths[b, k] = table.slots, table.lengths
        best, status = engine.tree_ols(preds, slots)
        _tree, rows, worst_j, _status = engine.tree_fit(preds, np.concatenate([slots, slots], axis=1),
                                                        np.concatenate([lengths, best], axis=1), patristic=False)
        self.book(ols_s=time.perf_counter() - t0)
        return {name: (best[:, k], status[:, k], rows[:, [k, m + k]], worst_j[:, [k, m + k]]) for k, name in enumerate(made)}

    def _write_ols(self, group: list, preds: np.ndarray, tables: dict, made: dict):
        """The files of ``--ols`` of some files of a launch, on a writer thread: of every written kind the GPU thread's
        arrays where it made them (``made``), else the host side's on the kind's table (``table_of``).  ``<stem>[.<kind>].ols.nwk``
        is the table with the OLS lengths through the call that formats the kind's own tree; ``<stem>.ols.tsv`` has
        ``ols.ols_scores`` of the unclamped tables.  Fewer than three sequences or distances that are not finite: the kind's own
        text and ``nan``."""
        from . import fit as F, ols as O
        t0 = time.perf_counter()
        for k, (e, pred) in enumerate(zip(group, preds)):
            ids = e.ids()
            n, lines = len(ids), []
            for kind in self.written_kinds():
                table = self.table_of(kind, k, pred, tables) if n >= F.MIN_SEQS else None
                arrays = None
                if table is not None and kind.name in made:
                    arrays = tuple(a[k] for a in made[kind.name])
                elif table is not None:
                    best, status = self.host.tree_ols(pred, table.slots)
                    _tree, rows, worst_j, _status = self.host.tree_fit(pred, np.stack([table.slots, table.slots]),
                                                                       np.stack([table.lengths, best]), patristic=False)
                    arrays = (best, status, rows, worst_j)
                if arrays is None or arrays[1]:
                    scores = O.no_scores()
                    text = self.nj(pred, ids) if kind is KINDS[0] else self.host.tree_text(kind, pred, ids)[0]
                else:
                    scores = O.ols_scores(pred, table.lengths, arrays[0], arrays[2], arrays[3], n)
                    text = self.newick_of_joins(table.slots, arrays[0], ids)
                lines.append((kind.name, scores))
                self.put(e.path, kind.files("ols.nwk")[0], text)
            self.put(e.path, "ols.tsv", O.ols_tsv(lines))
        self.book(ols=len(group), ols_s=time.perf_counter() - t0)

    def root_arrays(self, engine, n: int, preds: np.ndarray) -> dict:
        """``--root`` on the GPU thread: ``Engine.tree_root`` of the tables that were made on this thread (``device_tables``), one
        call for all their kinds, from ``root.ROOT_DEVICE_MIN`` sequences on; a file without a table (distances that are not
        finite) gets a table of zeros, which is none (status 2).  ``{kind name: (ssq, pos, mid, status)}``; the other kinds are
        the writer thread's.  Books its seconds."""
        from . import fit as F, root as R
        made = {name: tables for name, tables in getattr(self._made, "tables", {}).items() if tables is not None}
        if not made or not reaches(R.ROOT_DEVICE_MIN, n, F.MIN_SEQS):
            return {}
        t0 = time.perf_counter()
        width, m = F.table_len(n), len(made)
        slots = np.zeros((len(preds), m, width), dtype=np.int32)
        lengths = np.zeros((len(preds), m, width), dtype=np.float64)
        for k, tables in enumerate(made.values()):
            for b, table in enumerate(tables):
                if table is not None:
                    slots[b, k], lengths[b, k] = table.slots, table.lengths
        out = engine.tree_root(slots, lengths)
        self.book(root_s=time.perf_counter() - t0)
        return {name: tuple(a[:, k] for a in out) for k, name in enumerate(made)}

    def _write_root(self, group: list, preds: np.ndarray, tables: dict, made: dict):
        """The files of ``--root`` of some files of a launch, on a writer thread: of every written kind the GPU thread's arrays
        where it made them (``made``), else the host side's on the kind's table (``table_of``).  ``<stem>[.<kind>].rooted.nwk`` is
        the table rooted by the chosen method; ``<stem>.root.tsv`` has ``root.root_scores`` of both rootings.  Fewer than three
        sequences or lengths that are not finite: the kind's own text and ``nan``."""
        from . import fit as F, root as R
        t0 = time.perf_counter()
        for k, (e, pred) in enumerate(zip(group, preds)):
            ids = e.ids()
            n, lines = len(ids), []
            for kind in self.written_kinds():
                table = self.table_of(kind, k, pred, tables) if n >= F.MIN_SEQS else None
                arrays = None
                if table is not None and kind.name in made:
                    arrays = tuple(a[k] for a in made[kind.name])
                elif table is not None:
                    arrays = self.host.tree_root(table.slots, table.lengths)
                if arrays is None or arrays[3]:
                    scores = R.no_scores()
                    text = self.nj(pred, ids) if kind is KINDS[0] else self.host.tree_text(kind, pred, ids)[0]
                else:
                    scores = R.root_scores(table.slots, table.lengths, arrays[0], arrays[1], arrays[2], n)
                    text = R.rooted_newick(ids, table.slots, table.lengths, *R.root_choice(scores, self.root))
                lines.append((kind.name, self.root, scores, ids))
                self.put(e.path, kind.files("rooted.nwk")[0], text)
            self.put(e.path, "root.tsv", R.root_tsv(lines))
        self.book(root=len(group), root_s=time.perf_counter() - t0)

    def compared(self) -> List[str]:
        """The trees of ``<stem>.treedist.tsv``: every written kind, then ``ref`` with ``--treedist-ref``."""
        return [k.name for k in self.written_kinds()] + (["ref"] if self.treedist_ref else [])

    def reference_table(self, path: str, ids: List[str]):
        """``(JoinTable, None)`` of ``DIR/<stem>.nwk``, or ``(None, the reason it has none)``: missing, unreadable, refused."""
        from . import treedist as TD
        try:
            with open(os.path.join(self.treedist_ref, f"{Path(path).stem}.nwk"), errors="replace") as fh:
                return JoinTable(*TD.table_of_newick(fh.read(), ids), 0), None
        except OSError as exc:
            reason = f"no reference tree ({exc.strerror or type(exc).__name__})"
        except ValueError as exc:
            reason = " ".join(str(exc).split())
        self.book(treedist_ref_missing=1)
        return None, reason

    @staticmethod
    def treedist_source(tables: list, reasons: list):
        """The trees of one file for ``join_distances``: a tree without a table is passed flagged, with a table of zeros."""
        width = next((len(t.slots) for t in tables if t is not None), 0)
        slots, lengths = np.zeros((len(tables), width), dtype=np.int32), np.zeros((len(tables), width), dtype=np.float64)
        for m, t in enumerate(tables):
            if t is not None:
                slots[m], lengths[m] = t.slots, t.lengths
        return slots, lengths, np.array([r is not None for r in reasons], dtype=bool)

    def treedist_arrays(self, engine, n: int, preds: np.ndarray, group: list):
        """``--treedist`` on the GPU thread, from ``treedist.TREEDIST_DEVICE_MIN`` sequences on and where every refined kind's
        table was made on this thread (``device_tables``): the NJ tables joined here, the reference trees read, one
        ``Engine.join_distances`` for the launch.  ``(distances [B, ...], reasons [B][K])`` or None: the writer thread's."""
        from . import treedist as TD
        made = getattr(self._made, "tables", {})
        kinds = self.written_kinds()
        if len(self.compared()) < 2 or not reaches(TD.TREEDIST_DEVICE_MIN, n, TD.MIN_SEQS) or any(made.get(k.name) is None for k in kinds[1:]):
            return None                  # (one tree has no pair: the header alone, the writer's)
        t0 = time.perf_counter()
        slots, lengths, bad = engine.nj_joins(preds)
        rows, reasons = [], []
        for b, e in enumerate(group):
            tables = [None if bad[b] else JoinTable(slots[b], lengths[b], 0)] + [made[k.name][b] for k in kinds[1:]]
            why = [None if t is not None else TD.NOT_FINITE for t in tables]
            if self.treedist_ref:
                ref, reason = self.reference_table(e.path, e.ids())
                tables.append(ref)
                why.append(reason)
            rows.append(self.treedist_source(tables, why))
            reasons.append(why)
        if not any(len(r[0][0]) for r in rows):
            return None
        width = max(r[0].shape[1] for r in rows)
        rows = [r if r[0].shape[1] else (np.zeros((len(r[2]), width), np.int32), np.zeros((len(r[2]), width)), r[2]) for r in rows]
        out = engine.join_distances(*(np.stack(x) for x in zip(*rows)))
        self.book(treedist_s=time.perf_counter() - t0)
        return out, reasons

    def _write_treedist(self, group: list, preds: np.ndarray, tables: dict, made):
        """``<stem>.treedist.tsv`` of some files of a launch, on a writer thread: the GPU thread's distances where it made
        them (``made``), else the host side's on every kind's table (``table_of``) and the reference tree; ``NA`` with a
        note for fewer than four sequences, a kind without a table and a reference tree that is missing or refused."""
        from . import treedist as TD
        t0 = time.perf_counter()
        names = self.compared()
        for k, (e, pred) in enumerate(zip(group, preds)):
            ids = e.ids()
            n = len(ids)
            if n < TD.MIN_SEQS or len(names) < 2:
                dist, reasons = None, [TD.FEW_SEQUENCES] * len(names)
            elif made is not None:
                dist, reasons = tuple(a[k] for a in made[0]), made[1][k]
            else:
                trees = [self.table_of(kind, k, pred, tables) for kind in self.written_kinds()]
                reasons = [None if t is not None else TD.NOT_FINITE for t in trees]
                if self.treedist_ref:
                    ref, reason = self.reference_table(e.path, ids)
                    trees.append(ref)
                    reasons.append(reason)
                dist = self.host.join_distances(*self.treedist_source(trees, reasons)) if any(t is not None for t in trees) else None
            self.put(e.path, "treedist.tsv", TD.treedist_tsv(names, n, dist, reasons))
        self.book(treedist=len(group), treedist_s=time.perf_counter() - t0)

    def book(self, **amounts):
        """Add to the run's stats from inside a mode's own engine call (takes the runner's lock)."""
        with self._lock:
            for key, value in amounts.items():
                self.stats[key] = self.stats.get(key, 0) + value

    def out_path(self, path: str, suffix: str) -> str:
        return os.path.join(self.out_dir, f"{Path(path).stem}.{suffix}")

    def put(self, path: str, suffix: str, data):
        """``<stem>.<suffix>`` of the input ``path``: bytes as they are, text through the locale's encoding."""
        with open(self.out_path(path, suffix), "wb" if isinstance(data, bytes) else "w") as fh:
            fh.write(data)

    def _write(self, path: str, pred: np.ndarray, ids: List[str], tree: bool = True):
        self.put(path, "phy", self.phylip(pred, ids))
        if self.trees and tree:
            self.put(path, "nj.nwk", self.nj(pred, ids))

    def writer_cap(self) -> int:
        # (at most 4 threads: creating files in ONE directory from 8 / 16 threads is a lock convoy on the directory -
        # 4,096 outputs took 0.98 / 1.19 s instead of 0.01 s, profiles/r05c_cli_bench.txt.  The neighbour joining of
        # --trees rides on the same threads: 64 us per 20-taxon tree, 18 ms at 200 taxa, against 90 us / 22 ms of GPU time
        # per alignment.  PF_WRITER_THREADS moves the cap for experiments, profiles/r06r_cli_bench_overlay_writer_threads.txt.)
        return max(1, min(self.io_threads, int(os.environ.get("PF_WRITER_THREADS", "4"))))

    def _write_native(self, n: int, group: list, preds: np.ndarray, tree: bool = True):
        """``<stem>.phy`` - and with ``--trees`` ``<stem>.nj.nwk``, unless a mode writes the tree of this shape itself
        (``tree`` = False) - of a whole launch: formatted (the trees: joined) and written on native threads
        (infer_alns.py:105-123)."""
        from .hostio import write_phylip
        trees = [self.out_path(e.path, "nj.nwk") for e in group] if self.trees and tree else None
        write_phylip([e.source for e in group], n, preds, [self.out_path(e.path, "phy") for e in group],
                     self.writer_cap(), trees)

    def _launch(self, engine, shape: Tuple[int, int], group: List[Entry], writers: ThreadPoolExecutor, pending: deque):
        def submit(jobs):
            pending.extend(writers.submit(*job) for job in jobs)
        self._made.tables = {}
        t0 = time.perf_counter()
        if self.native_io:
            from .hostio import gather
            batch = gather([e.source for e in group], shape[0], shape[1])
        else:
            batch = np.stack([e.source for e in group])
        mode = self._forwarder
        preds, payload = mode.forward(self, engine, shape, batch) if mode else (engine.forward(batch), ())
        dt = time.perf_counter() - t0
        tree = not (mode and self.trees and mode.writes_tree(shape))      # (False: the mode writes the tree itself)
        cap = self.writer_cap()
        for kinds in self.kind_groups:
            device = self.device_tables(engine, shape[0], preds, kinds)
            for kind in kinds:
                tables = device.get(kind.name)
                submit([(self._write_trees, group[k::cap], preds[k::cap], None if tables is None else tables[k::cap], kind)
                        for k in range(min(cap, len(group)))])
        if self.fit:
            made, fits = dict(self._made.tables), self.fit_arrays(engine, shape[0], preds)
            submit([(self._write_fit, group[k::cap], preds[k::cap], {name: None if t is None else t[k::cap] for name, t in made.items()},
                     {name: tuple(a[k::cap] for a in arrays) for name, arrays in fits.items()}) for k in range(min(cap, len(group)))])
        if self.ols:
            made, best = dict(self._made.tables), self.ols_arrays(engine, shape[0], preds)
            submit([(self._write_ols, group[k::cap], preds[k::cap], {name: None if t is None else t[k::cap] for name, t in made.items()},
                     {name: tuple(a[k::cap] for a in arrays) for name, arrays in best.items()}) for k in range(min(cap, len(group)))])
        if self.root:
            made, roots = dict(self._made.tables), self.root_arrays(engine, shape[0], preds)
            submit([(self._write_root, group[k::cap], preds[k::cap], {name: None if t is None else t[k::cap] for name, t in made.items()},
                     {name: tuple(a[k::cap] for a in arrays) for name, arrays in roots.items()}) for k in range(min(cap, len(group)))])
        if self.treedist:
            made, dists = dict(self._made.tables), self.treedist_arrays(engine, shape[0], preds, group)
            submit([(self._write_treedist, group[k::cap], preds[k::cap], {name: None if t is None else t[k::cap] for name, t in made.items()},
                     None if dists is None else (tuple(a[k::cap] for a in dists[0]), dists[1][k::cap])) for k in range(min(cap, len(group)))])
        if self.delta:
            arrays = self.delta_arrays(engine, preds)
            submit([(self._write_delta, group[k::cap], None if arrays is None else tuple(a[k::cap] for a in arrays))
                    for k in range(min(cap, len(group)))])
        with self._lock:
            self.stats["forward_s"] += dt
            self.stats["launches"] += 1
            self.stats["alignments"] += len(group)
            key = f"{shape[0]}x{shape[1]}"
            self.stats["shapes"][key] = self.stats["shapes"].get(key, 0) + len(group)
            if self.native_io:
                submit([(self._write_native, shape[0], group, preds, tree)])
            else:
                submit([(self._write, e.path, pred, e.ids(), tree) for e, pred in zip(group, preds)])
            if mode:
                mode.account(self.stats, len(group), shape, dt)
                if payload:
                    submit(mode.jobs(self, shape, group, preds, *payload))
            if self.progress is not None and not self._followers:
                self.progress(len(group))
        # the modes behind the forward, in sub-batches; their outputs are computed and written on the writer threads
        for mode in self._followers:
            for s in sub_batches(len(group), mode.floats(shape)):
                t0 = time.perf_counter()
                res = mode.follow(engine, batch[s])
                dt = time.perf_counter() - t0
                # (a mode's further device work on the results, booked by itself: Bootstrap's --tbe / --bootstrap-refined)
                cols = (res,) if mode.extend is None else mode.extend(self, engine, shape, preds[s], res)
                with self._lock:
                    mode.account(self.stats, len(group[s]), shape, dt)
                    submit(mode.jobs(self, shape, group[s], preds[s], *cols))
        if self.progress is not None and self._followers:
            self.progress(len(group))
        with self._lock:
            drain = []
            # bound the write queue so results do not pile up in memory
            room = (1 if self.native_io else len(group)) * (2 if any(m.write for m in self.modes) else 1)
            while len(pending) > 8 * self.io_threads + room:
                drain.append(pending.popleft())
        t0 = time.perf_counter()
        for f in drain:
            f.result()
        with self._lock:
            self.stats["write_wait_s"] += time.perf_counter() - t0

    def _gpu_worker(self, engine, jobs: "queue.Queue", writers, pending, errors: list):
        while True:
            job = jobs.get()
            if job is None:
                return
            if errors:
                continue                      # drain the queue after a failure
            try:
                self._launch(engine, job[0], job[1], writers, pending)
            except BaseException as exc:      # noqa: BLE001 - re-raised in run()
                errors.append(exc)

    # -- driver -----------------------------------------------------------------------------
    def run(self, paths: Sequence[str]) -> dict:
        """Process ``paths`` in the given order.  Side effects on a bad entry are the reference's
        (infer_alns.py:97-117 handles one file after the other): every alignment in front of the first entry
        without a FASTA extension (``ValueError``, :100-103), or of the first file that does not parse
        (``KeyError`` / ``ValueError`` / ... from ``load_alignment``, :108), is computed and written; nothing
        behind it is; then the exception is raised."""
        paths = list(paths)
        deferred: Optional[BaseException] = None
        bad_entry = non_fasta_entry(paths)
        if bad_entry is not None:
            paths, deferred = paths[:bad_entry[0]], bad_entry[1]
        t_start = time.perf_counter()
        pending: deque = deque()
        errors: list = []
        jobs: "queue.Queue" = queue.Queue(maxsize=2 * len(self.engines))
        with ThreadPoolExecutor(self.io_threads, thread_name_prefix="pf-load") as loaders, \
                ThreadPoolExecutor(self.io_threads, thread_name_prefix="pf-write") as writers:
            workers = [threading.Thread(target=self._gpu_worker, args=(e, jobs, writers, pending, errors),
                                        name=f"pf-gpu{k}", daemon=True) for k, e in enumerate(self.engines)]
            for w in workers:
                w.start()
            try:
                feed = self._feed_native if self.native_io else self._feed_python
                bad = feed(paths, loaders, jobs, errors)
                deferred = bad or deferred         # a file that fails to parse sits in front of a bad extension
            finally:
                for _ in workers:
                    jobs.put(None)
                for w in workers:
                    w.join()
            if errors:
                raise errors[0]
            t0 = time.perf_counter()
            while pending:
                pending.popleft().result()
            self.stats["write_wait_s"] += time.perf_counter() - t0
        self.stats["wall_s"] = time.perf_counter() - t_start
        if deferred is not None:
            raise deferred
        return self.stats

    def _file_error(self, path: str, n_seqs: int, n_sites: int) -> Optional[Exception]:
        """Why a parsed file cannot be run, if it cannot: the reference's own limits, then the modes' (``accepts``); an
        error for that file, raised where the loop reaches it."""
        bad = too_many_seqs(n_seqs, self.modes)
        for m in self.modes:
            if bad is None and not m.accepts(n_seqs, n_sites):
                bad = m.file_error(path, n_seqs, n_sites)
        return bad

    def _parse_ahead(self, paths, loaders, lookahead: int):
        """``(path, future of its parse)`` in the order of ``paths``, at most ``lookahead`` files submitted ahead of the
        consumer; closing the generator cancels what is still queued."""
        inflight: "deque[Tuple[str, Future]]" = deque()
        it = iter(paths)
        try:
            while True:
                inflight.extend((p, loaders.submit(self._load, p)) for p in itertools.islice(it, lookahead - len(inflight)))
                if not inflight:
                    return
                yield inflight.popleft()
        finally:
            for _p, f in inflight:
                f.cancel()

    def _feed_python(self, paths, loaders, jobs, errors) -> Optional[BaseException]:
        """One future per file (``--python-io``, ``-t``): parse ahead, bucket by shape, launch full buckets."""
        buckets: "OrderedDict[Tuple[int, int], list]" = OrderedDict()
        bad: Optional[BaseException] = None
        ahead = self._parse_ahead(paths, loaders, max(64, 4 * (self.batch or 64)))
        for path, fut in ahead:
            if errors:
                break
            t0 = time.perf_counter()
            try:
                idx, ids = fut.result()          # parser exceptions surface here, as in the reference
            except Exception as exc:             # noqa: BLE001 - raised by run() once the files in front are written
                bad = exc
                break
            finally:
                self.stats["load_wait_s"] += time.perf_counter() - t0
            shape = (int(idx.shape[0]), int(idx.shape[1]))
            bad = self._file_error(path, *shape)
            if bad is not None:
                break
            group = buckets.setdefault(shape, [])
            group.append(Entry(path, idx, ids))
            if len(group) >= (self.batch or auto_batch(*shape)):
                jobs.put((shape, group))
                buckets[shape] = []
        ahead.close()                                # (cancels what is still queued, whichever way the loop ended)
        for shape, group in sorted(buckets.items(), key=lambda kv: -len(kv[1])):
            if group and not errors:
                jobs.put((shape, group))
        return bad

    def _feed_native(self, paths, loaders, jobs, errors) -> Optional[BaseException]:
        """The fast path: ``FILES_PER_LOAD`` files per native call (read + parsed on ``io_threads`` std::threads,
        no GIL), two calls in flight ahead of the bucketing; a bucket entry points into its ``FastaBatch``."""
        from .hostio import FastaBatch
        buckets: "OrderedDict[Tuple[int, int], list]" = OrderedDict()
        born: Dict[Tuple[int, int], int] = {}          # load call that opened each partial bucket
        chunks = [paths[k:k + FILES_PER_LOAD] for k in range(0, len(paths), FILES_PER_LOAD)]
        inflight: "deque[Future]" = deque()
        nxt = 0
        done = 0
        bad: Optional[BaseException] = None
        while not errors and bad is None:
            while nxt < len(chunks) and len(inflight) < 2:
                inflight.append(loaders.submit(FastaBatch, chunks[nxt], self.io_threads))
                nxt += 1
            if not inflight:
                break
            t0 = time.perf_counter()
            fb = inflight.popleft().result()
            self.stats["load_wait_s"] += time.perf_counter() - t0
            ok = (fb.status == 0) & (fb.l > 0) & ~over_seq_cap(fb.n, self.modes) & (fb.n != 1)
            for m in self.modes:
                ok &= m.accepts(fb.n, fb.l)
            stop = len(fb) if ok.all() else int(np.argmin(ok))
            if stop < len(fb):
                bad = fb.error(stop) or self._file_error(fb.paths[stop], int(fb.n[stop]), int(fb.l[stop]))
            ns, ls = fb.n.tolist(), fb.l.tolist()
            for i in range(stop):
                shape = (ns[i], ls[i])
                group = buckets.get(shape)
                if not group:
                    group = buckets[shape] = []
                    born[shape] = done
                group.append(Entry(fb.paths[i], (fb, i)))
                if len(group) >= (self.batch or auto_batch(*shape)):
                    jobs.put((shape, group))
                    buckets[shape] = []
            done += 1
            # A partial bucket keeps its entries' batch objects - every parsed file of those load calls - alive: a rare
            # shape in a long directory would pin the whole directory in memory.  A bucket that has waited for
            # STALE_LOADS load calls is launched as it is (an alignment's bits do not depend on its batch).
            for shape in [sh for sh, g in buckets.items() if g and done - born[sh] >= STALE_LOADS]:
                jobs.put((shape, buckets[shape]))
                buckets[shape] = []
        for f in inflight:
            f.cancel()
        for shape, group in sorted(buckets.items(), key=lambda kv: -len(kv[1])):
            if group and not errors:
                jobs.put((shape, group))
        return bad


class SiteShardedRunner(DirectoryRunner):
    """``--shard sites``: every alignment is spread over the ``world`` ranks of one node.

    Rank ``r`` holds the sites ``dist.site_range(L, world, r)`` of every pair; the row-attention statistics
    (/root/reference/phyloformer/attention.py:183-190 reduced over sites, model.py:91) and the final site sums
    (model.py:185) are all-reduced inside ``pf_forward_sharded``, so every rank receives the full distance
    vector and rank 0 alone writes ``<stem>.phy`` / ``<stem>.nj.nwk`` (output contract: infer_alns.py:105-123).

    Collectives must be issued in the same order on every rank: all ranks sort the paths the same way, parse
    every file themselves (the parse is cheap beside a sharded forward of a long alignment), bucket by shape in
    that order on ONE host thread and flush the partial buckets in sorted shape order.  Before each launch the
    ranks compare (shape, batch, checksum of the file names) through the rendezvous: a directory that differs
    between ranks is an error on all of them, not a hang."""

    def __init__(self, engine, group, rank: int, world: int, out_dir: str, heartbeat_s: Optional[float] = None, **kw):
        if kw.get("delta"):
            raise ValueError(DELTA_SHARD_SITES)
        if kw.get("fit"):
            raise ValueError(FIT_SHARD_SITES)
        if kw.get("ols"):
            raise ValueError(OLS_SHARD_SITES)
        if kw.get("root"):
            raise ValueError(ROOT_SHARD_SITES)
        if kw.get("treedist") or kw.get("treedist_ref"):
            from .treedist import SHARD_SITES as TREEDIST_SHARD_SITES
            raise ValueError(TREEDIST_SHARD_SITES)
        super().__init__([engine], out_dir, **kw)
        self.group, self.rank, self.world = group, rank, world
        self.stats["site_sharded_over"] = world
        # A worker of `--devices ... --shard sites` prints nothing until its report (no progress bar): the launcher's
        # stall watchdog (run_multi_device) would take a long healthy run for a hang.  Every `heartbeat_s` seconds of
        # progress the rank says so on stderr; the launcher swallows these lines.
        self.heartbeat_s = heartbeat_s
        self._last_beat = time.monotonic()

    def _beat(self):
        if self.heartbeat_s is not None and time.monotonic() - self._last_beat >= self.heartbeat_s:
            self._last_beat = time.monotonic()
            print(f"{HEARTBEAT} rank {self.rank}: {self.stats['alignments']} alignments in {self.stats['launches']} launches",
                  file=sys.stderr, flush=True)

    def _launch_sharded(self, shape, group_items, writers, pending):
        import zlib
        from .dist import site_range
        engine = self.engines[0]
        N, L = shape
        lo, hi = site_range(L, self.world, self.rank)
        if self.group is not None:
            tag = [N, L, len(group_items), zlib.crc32("\n".join(os.path.basename(g[0]) for g in group_items).encode())]
            seen = self.group.allgather(tag)
            if any(list(t) != tag for t in seen):
                raise RuntimeError(f"site-sharded ranks disagree on the next launch: {seen} (do all ranks see the same files?)")
        local = np.ascontiguousarray(np.stack([g[1] for g in group_items])[:, :, lo:hi])
        t0 = time.perf_counter()
        preds = engine.forward_sharded(local, lo, hi, L)
        self.stats["forward_s"] += time.perf_counter() - t0
        self.stats["launches"] += 1
        self.stats["alignments"] += len(group_items)
        key = f"{N}x{L}"
        self.stats["shapes"][key] = self.stats["shapes"].get(key, 0) + len(group_items)
        if self.rank == 0:
            for (path, _idx, ids), pred in zip(group_items, preds):
                pending.append(writers.submit(self._write, path, pred, ids))
            while len(pending) > 8 * self.io_threads + len(group_items):
                pending.popleft().result()
        if self.progress is not None:
            self.progress(len(group_items))
        self._beat()

    def run(self, paths: Sequence[str]) -> dict:
        require_fasta_entries(paths)
        paths = sorted(paths)
        t_start = time.perf_counter()
        buckets: "OrderedDict[Tuple[int, int], list]" = OrderedDict()
        pending: deque = deque()
        with ThreadPoolExecutor(self.io_threads, thread_name_prefix="pf-load") as loaders, \
                ThreadPoolExecutor(self.io_threads, thread_name_prefix="pf-write") as writers, \
                closing(self._parse_ahead(paths, loaders, max(16, 2 * (self.batch or 16)))) as ahead:
            for path, fut in ahead:
                t0 = time.perf_counter()
                idx, ids = fut.result()
                self.stats["load_wait_s"] += time.perf_counter() - t0
                self._beat()                 # (parsing a long run of files that fill no bucket is progress too)
                shape = (int(idx.shape[0]), int(idx.shape[1]))
                bucket = buckets.setdefault(shape, [])
                bucket.append((path, idx, ids))
                if len(bucket) >= (self.batch or auto_batch(shape[0], shape[1], token_budget=TOKEN_BUDGET * self.world)):
                    self._launch_sharded(shape, bucket, writers, pending)
                    buckets[shape] = []
            for shape in sorted(buckets):
                if buckets[shape]:
                    self._launch_sharded(shape, buckets[shape], writers, pending)
            t0 = time.perf_counter()
            while pending:
                pending.popleft().result()
            self.stats["write_wait_s"] += time.perf_counter() - t0
        if self.group is not None:
            self.group.barrier()
        self.stats["wall_s"] = time.perf_counter() - t_start
        return self.stats


def cli_engine(weights, device: int):
    """The engine the CLI drives.  ``PF_CLI_ENGINE_FACTORY=module:function`` swaps in a stand-in with the Engine
    interface (``function(weights, device)``): the CPU tests of the multi-rank plumbing, which have no GPU."""
    hook = os.environ.get("PF_CLI_ENGINE_FACTORY")
    if hook:
        import importlib
        # a test hook, never set by the product: say so on every use, so that a run through a stand-in cannot pass
        # for a GPU run (there is no CPU fallback: without the hook a missing library or GPU is an error)
        print(f"infer_alns: PF_CLI_ENGINE_FACTORY={hook} REPLACES the GPU engine (test hook)", file=sys.stderr)
        mod_name, fn = hook.split(":")
        return getattr(importlib.import_module(mod_name), fn)(weights, device)
    from .engine import Engine
    return Engine(weights, device=device)


def summarize(stats: dict, load_s: float = 0.0) -> dict:
    n, wall = stats["alignments"], stats.get("wall_s", 0.0)
    return {"alignments": n, "launches": stats["launches"], "shapes": stats["shapes"],
            "model_load_s": round(load_s, 4), "wall_s": round(wall, 6),
            "gpu_streams": stats.get("gpu_streams", 1),
            "forward_s": round(stats["forward_s"], 6),      # summed over the streams' host threads
            "load_wait_s": round(stats["load_wait_s"], 6), "write_wait_s": round(stats["write_wait_s"], 6),
            "alignments_per_s": round(n / wall, 3) if wall > 0 else None,
            "alignments_per_s_forward_only": round(n * stats.get("gpu_streams", 1) / stats["forward_s"], 3)
            if stats["forward_s"] > 0 else None,
            "replicates": stats.get("replicates", 0), "bootstrap_s": round(stats.get("bootstrap_s", 0.0), 6),
            "windows": stats.get("windows", 0), "windows_s": round(stats.get("windows_s", 0.0), 6),
            **{key: round(stats[key], 6) for kind in KINDS if kind.name in stats for key in kind.stats},
            **({k: round(stats[k], 6) for k in ("tbe", "refined_supports", "supports_device", "supports_device_s")}
               if "tbe" in stats else {}),
            **({k: stats[k] for k in ("consensus", "consensus_device")} if "consensus" in stats else {}),
            **({k: stats[k] for k in ("instability", "transfers_device")} if "instability" in stats else {}),
            **({"delta": stats["delta"], "delta_s": round(stats["delta_s"], 6)} if "delta" in stats else {}),
            **({"fit": stats["fit"], "fit_s": round(stats["fit_s"], 6)} if "fit" in stats else {}),
            **({"ols": stats["ols"], "ols_s": round(stats["ols_s"], 6)} if "ols" in stats else {}),
            **({"root": stats["root"], "root_s": round(stats["root_s"], 6)} if "root" in stats else {}),
            **({"treedist": stats["treedist"], "treedist_s": round(stats["treedist_s"], 6),
                "treedist_ref_missing": stats["treedist_ref_missing"]} if "treedist" in stats else {})}


def run_multi_device(script: str, argv: List[str], devices: Sequence[int], shard: str = "files") -> Tuple[int, List[dict]]:
    """One child process per GPU (``--worker r/W``): each on its own share of the files, or - ``shard="sites"`` -
    all of them on every file, each with its block of sites; the ranks then meet through the rendezvous the
    environment set here names (127.0.0.1, a free port, a run id).
    Children are started before any of them touches a GPU; the parent never does."""
    procs = []
    env = dict(os.environ)
    if shard == "sites":
        import socket
        import uuid
        s = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        # (HSA_ENABLE_IPC_MODE_LEGACY=0: the pool's host driver only supports dmabuf IPC, which RCCL's intra-node
        # transports need; exported on the boxes already, pinned here for the children - DESIGN.md section 6)
        env.update({"WORLD_SIZE": str(len(devices)), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                    "PF_RUN_ID": uuid.uuid4().hex,
                    "HSA_ENABLE_IPC_MODE_LEGACY": env.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")})
    for r, d in enumerate(devices):
        cmd = [sys.executable, script, *argv, "--device", str(d), "--worker", f"{r}/{len(devices)}", "--bench"]
        if shard == "sites":
            cmd += ["--shard", "sites"]
        procs.append(subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True,
                                      env=dict(env, RANK=str(r), LOCAL_RANK=str(r)) if shard == "sites" else None))
    # One reader thread per child keeps its stderr drained (a rank blocked on a full 64 KB pipe while its peers wait
    # for it in a collective is a deadlock), the parent polls all children: in sites mode the ranks depend on each
    # other, so as soon as one exits non-zero - or no child has produced a line or exited for `stall_s` - the others,
    # parked in an all-reduce that will never complete, are terminated.
    lines: List[List[str]] = [[] for _ in procs]
    last_event = [time.monotonic()]

    def drain(k, pipe):
        for line in pipe:
            lines[k].append(line)
            last_event[0] = time.monotonic()
        pipe.close()
    readers = [threading.Thread(target=drain, args=(k, p.stderr), daemon=True) for k, p in enumerate(procs)]
    for t in readers:
        t.start()
    stall_s = float(os.environ.get("PF_CLI_STALL_TIMEOUT", "900"))
    failed, alive = None, set(range(len(procs)))
    while alive:
        for k in sorted(alive):
            code = procs[k].poll()
            if code is not None:
                alive.discard(k)
                last_event[0] = time.monotonic()
                if code != 0 and failed is None:
                    failed = (k, code)
        stalled = shard == "sites" and time.monotonic() - last_event[0] > stall_s
        if alive and shard == "sites" and (failed is not None or stalled):
            why = (f"rank {failed[0]} exited with code {failed[1]}" if failed is not None
                   else f"no rank made progress for {stall_s:.0f} s")
            print(f"infer_alns: {why}; terminating the other site-sharded ranks", file=sys.stderr)
            for k in alive:
                procs[k].terminate()
            deadline = time.monotonic() + 10
            for k in list(alive):
                try:
                    procs[k].wait(timeout=max(0.1, deadline - time.monotonic()))
                except subprocess.TimeoutExpired:
                    procs[k].kill()
                    procs[k].wait()
            if failed is None:
                failed = (-1, 124)
            alive.clear()
        if alive:
            time.sleep(0.05)
    for t in readers:
        t.join(timeout=5)
    # Exit code: the first rank that FAILED ON ITS OWN decides (or 124 for a stall) - not the -15 of a peer this
    # launcher terminated, which may have a lower rank number; a child ended by a signal counts as 128 + signal.
    def code_of(c):
        return 1 if c is None else (128 - c if c < 0 else c)
    rc, reports = (code_of(failed[1]) or 1) if failed is not None else 0, []
    for k, p in enumerate(procs):
        rc = rc or code_of(p.returncode)
        rep = None
        for line in "".join(lines[k]).splitlines():
            if line.startswith("{") and '"alignments"' in line:
                try:
                    rep = json.loads(line)
                    continue
                except ValueError:
                    pass
            if line.strip() and not line.startswith(HEARTBEAT):
                print(line, file=sys.stderr)
        if rep is not None:
            reports.append(rep)
    return rc, reports
