"""The CLI's per-alignment analyses (``--bootstrap``, ``--windows``, ``--site-profile``, ``--leave-one-out``,
``--compress-sites``, ``--place``, ``--tile``), each described ONCE: its flag and help, what it refuses to be combined with, the files it
cannot run on, the stats it reports, its call into the engine and its writer.  ``infer_alns.py`` builds its parser and
its refusals from ``MODES``; ``scheduler.DirectoryRunner`` drives whatever modes it is given and names none of them.

A mode plays one of two roles in a launch (``DirectoryRunner._launch``):

* it REPLACES the forward (``forward``): the launch's distances plus a payload, one row per alignment, for ``write``;
* it FOLLOWS the forward (``follow``) in sub-batches of at most ``FLOATS`` result floats, each written behind it.
"""
from __future__ import annotations

import time
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .treekinds import NJ, NJ_STARTED, Kind, SupportTables, join_refine, reaches, with_stand_ins

# Result floats of one engine call behind the launch's forward (16 MiB): the replicate distances of a pf_bootstrap call,
# the window distances of a pf_forward_windows call, the distances of the cuts (N x P1 floats per alignment) of a
# pf_forward_leave_one_out call, the distances of the query sets (Q x P_{N+1} floats per alignment) of a pf_forward_place
# call.  This bounds host memory, not GPU work: the results wait in the writer queue (up to
# 8 x io_threads entries) until their files are written, so the cap keeps that queue to a few hundred MB even at 200
# taxa (R = 100 x 19,900 floats = 8 MB per alignment).  The GPU stays fed: one alignment's R = 100 replicates at
# 60 x 500 are already 6 x TOKEN_BUDGET, and the library chunks every one of these calls itself.
FLOATS = 1 << 22

SHARD_SITES = "--shard sites"

# From this many sequences on, a file that ``--tile`` lifts over the cap gets its ``-t`` tree from the device
# (``Engine.nj_joins``) instead of from the writer thread's host neighbour joining.  A measured constant (DESIGN.md
# section 20, tools/nj_bench.py, profiles/nj_bench.txt): the smallest measured N at which the device side takes at most
# half the host's time - it occupies the GPU thread, where the host's overlaps the next launch.  Never below 201: no file
# that ran before the device path existed changes path.  None = the device path is off.
NJ_DEVICE_MIN = 256
assert NJ_DEVICE_MIN is None or NJ_DEVICE_MIN >= 201


def sub_batches(count: int, floats_each: int) -> List[slice]:
    """``count`` alignments in runs whose results stay within ``FLOATS`` (at least one alignment per run)."""
    sub = max(1, FLOATS // max(1, floats_each))
    return [slice(s0, s0 + sub) for s0 in range(0, count, sub)]


def _text(tree) -> str:
    return tree.decode("utf8") if isinstance(tree, bytes) else tree


class Analysis:
    """One mode.  The class is what the command line knows (``flag``, ``help``, ``option``, ``refuses``, ``from_args``);
    an instance is the mode switched on, with its parameters."""
    flag = ""
    help = ""
    option: dict = {"action": "store_true"}      # argparse keywords besides ``help``
    refuses: Tuple[Tuple[str, str], ...] = ()    # (other flag or SHARD_SITES, reason), in the order they are reported
    forward = None                               # forward(runner, engine, shape, batch) -> (preds, payload columns)
    follow = None                                # follow(engine, batch) -> results [B, ...]
    extend = None                                # extend(runner, engine, shape, preds, results) -> the columns of ``jobs``:
                                                 # further device work behind ``follow``, booked by the mode itself
    write = None                                 # write(runner, shape, entry, pred, *payload row): one file's outputs

    @classmethod
    def dest(cls) -> str:
        return cls.flag[2:].replace("-", "_")

    @classmethod
    def add_arguments(cls, parser):
        parser.add_argument(cls.flag, help=cls.help, **cls.option)

    @classmethod
    def from_args(cls, args) -> "Optional[Analysis]":
        """The mode as ``args`` asks for it, None if it is off; ``ValueError`` carries the text of a usage error."""
        return cls() if getattr(args, cls.dest()) else None

    @classmethod
    def refusal(cls, other: str, reason: str) -> str:
        return f"{cls.flag} is not supported with {other} ({reason})" + ("; use --shard files" if other == SHARD_SITES else "")

    def stats(self) -> dict:
        """The keys this mode adds to the run's stats."""
        return {}

    def bind(self, modes: "Sequence[Analysis]"):
        """Called once with all the modes of the run."""

    def accepts(self, n, l):
        """Can a file of ``n`` sequences and ``l`` sites be run?  Elementwise: ints or the arrays of a FastaBatch."""
        return True

    def file_error(self, path: str, n: int, l: int) -> Exception:
        """What a file that ``accepts`` turns down raises, where the loop reaches it."""
        raise NotImplementedError

    def lifts_seq_cap(self, n):
        """Does this mode run a file of ``n`` sequences that exceeds the reference's cap (``scheduler.MAX_SEQS``)?
        Elementwise, like ``accepts``."""
        return False

    def writes_tree(self, shape: Tuple[int, int]) -> bool:
        """With ``--trees``: does this mode write ``<stem>.nj.nwk`` of a file of this shape itself (``write``)?  The
        launch's default writer then leaves the tree to it - it is computed once."""
        return False

    def floats(self, shape: Tuple[int, int]) -> int:
        """Result floats of ``follow`` per alignment."""
        raise NotImplementedError

    def account(self, stats: dict, count: int, shape: Tuple[int, int], seconds: float):
        """Book one engine call over ``count`` alignments (under the runner's lock)."""

    def jobs(self, runner, shape, part, preds, *payload) -> list:
        """The writer jobs ``(callable, *args)`` of a (sub-)batch: one per file through the Python writers, one for all
        of them on the native path, where the ids come out of the ``FastaBatch`` on the writer thread."""
        rows = list(zip(part, preds, *payload))
        if runner.native_io:
            return [(lambda: [self.write(runner, shape, *row) for row in rows],)]
        return [(self.write, runner, shape, *row) for row in rows]


class Bootstrap(Analysis):
    flag = "--bootstrap"
    option = {"type": int, "default": 0, "metavar": "R"}
    help = ("site-bootstrap replicates per alignment, resampled and inferred on the GPU: writes "
            "<stem>.sup.nwk, the NJ tree of the alignment's distances with the percent of replicate "
            "trees that contain each internal branch's split (Felsenstein's proportion); with --tbe also "
            "<stem>.tbe.nwk, the same tree with the transfer bootstrap expectation; with --bootstrap-refined "
            "the trees of --bme / --spr get their supports too; with --consensus [F] also <stem>.con.nwk, the "
            "majority-rule consensus of the replicate trees; with --instability [C] also the per-sequence "
            "transfer counts that single out rogue sequences; 0 (default) = off")
    refuses = ((SHARD_SITES, "every replicate would need its own collectives"),)
    call = "bootstrap"
    treedist = False        # set by a runner with --treedist: <stem>.treedist.reps.tsv / .treedist.rf.phy (treedist.py)

    def __init__(self, replicates: int, seed: int = 0, tbe: bool = False, refined: bool = False, consensus: Optional[int] = None,
                 instability: Optional[int] = None):
        self.replicates, self.seed = int(replicates), int(seed)
        self.tbe, self.refined = bool(tbe), bool(refined)
        self.consensus = None if consensus is None else int(consensus)      # the threshold in percent
        self.instability = None if instability is None else int(instability)      # the cutoff in percent
        if self.tbe or self.refined or self.consensus is not None or self.instability is not None:
            self.extend = self._extend

    @classmethod
    def add_arguments(cls, parser):
        super().add_arguments(parser)
        parser.add_argument("--seed", type=int, default=0,
                            help="seed of the bootstrap replicate stream (default 0): a file's supports depend on the "
                                 "weights, the alignment, R and the seed only")
        parser.add_argument("--tbe", action="store_true",
                            help="with --bootstrap R: also write <stem>.tbe.nwk, the tree of <stem>.sup.nwk labelled with the "
                                 "transfer bootstrap expectation in percent (Lemoine et al. 2018): per branch and replicate, "
                                 "how many sequences would have to move for the branch's split to appear in the replicate "
                                 "tree, against the p - 1 of a split with p sequences on its smaller side; it does not "
                                 "collapse on deep branches of large trees as Felsenstein's all-or-nothing count does")
        parser.add_argument("--bootstrap-refined", action="store_true",
                            help="with --bootstrap R and --bme and / or --spr: also write <stem>.bme.sup.nwk / "
                                 "<stem>.spr.sup.nwk, the refined tree with the percent of replicate trees - each "
                                 "replicate's NJ tree refined by the same search - that contain each branch's split (with "
                                 "--tbe also <stem>.bme.tbe.nwk / <stem>.spr.tbe.nwk); R more searches per file")
        parser.add_argument("--consensus", nargs="?", type=int, const=50, default=None, metavar="F",
                            help="with --bootstrap R: also write <stem>.con.nwk, the majority-rule consensus of the R "
                                 "replicates' NJ trees: every split found in more than F percent of them (50 to 99, default "
                                 "50; exactly half is not enough), nested into a multifurcating tree, each internal node "
                                 "labelled with the percent of replicates that contain its split, branch lengths the means "
                                 "over the replicates that have the branch; with --bootstrap-refined and --bme / --spr also "
                                 "<stem>.bme.con.nwk / <stem>.spr.con.nwk, the consensus of the refined replicate trees")

        parser.add_argument("--instability", nargs="?", type=int, const=30, default=None, metavar="C",
                            help="with --bootstrap R: also write <stem>.instability.tsv, per sequence how often it is among "
                                 "those that have to move for a branch of the tree to appear in a replicate tree (the "
                                 "per-taxon companion of the transfer bootstrap, Lemoine et al. 2018: rogue sequences "
                                 "collect the moves) and that count per thousand used (branch, replicate) pairs; "
                                 "<stem>.branches.tsv, per branch its depth, supports, used and capped replicates and its "
                                 "five most-moved sequences; and <stem>.branches.nwk, the tree labelled with the branch "
                                 "numbers of that table.  A pair is used if its transfer distance is at most C percent "
                                 "of the branch's depth - 1 (0 to 100, default 30: a far-away closest split says nothing "
                                 "about single sequences); with --bootstrap-refined also <stem>.bme.* / <stem>.spr.*")

    @classmethod
    def from_args(cls, args):
        if args.bootstrap < 0:
            raise ValueError(f"--bootstrap must be >= 0 (got {args.bootstrap})")
        if args.tbe and not args.bootstrap:
            raise ValueError("--tbe labels the tree of --bootstrap: give --bootstrap R as well")
        if args.bootstrap_refined and not args.bootstrap:
            raise ValueError("--bootstrap-refined counts over the replicates of --bootstrap: give --bootstrap R as well")
        if args.bootstrap_refined and not (args.bme or args.spr):
            raise ValueError("--bootstrap-refined supports the trees of --bme / --spr: give at least one of them as well")
        if args.consensus is not None and not args.bootstrap:
            raise ValueError("--consensus is the consensus of the replicate trees of --bootstrap: give --bootstrap R as well")
        if args.consensus is not None and not 50 <= args.consensus <= 99:
            raise ValueError(f"--consensus takes a threshold of 50 to 99 percent (got {args.consensus})")
        if args.instability is not None and not args.bootstrap:
            raise ValueError("--instability counts over the replicates of --bootstrap: give --bootstrap R as well")
        if args.instability is not None and not 0 <= args.instability <= 100:
            raise ValueError(f"--instability takes a cutoff of 0 to 100 percent (got {args.instability})")
        return cls(args.bootstrap, args.seed, args.tbe, args.bootstrap_refined, args.consensus, args.instability) if args.bootstrap else None

    def stats(self):
        more = {"tbe": 0, "refined_supports": 0, "supports_device": 0, "supports_device_s": 0.0} if self.extend else {}
        if self.consensus is not None:
            more.update(consensus=0, consensus_device=0)
        if self.instability is not None:
            more.update(instability=0, transfers_device=0)
        return {"replicates": self.replicates, "bootstrap_s": 0.0, **more}

    def floats(self, shape):
        return self.replicates * (shape[0] * (shape[0] - 1) // 2)

    def follow(self, engine, batch):
        return getattr(engine, self.call)(batch, self.replicates, self.seed)

    def account(self, stats, count, shape, seconds):
        stats["bootstrap_s"] += seconds

    def write(self, runner, shape, entry, pred, reps):
        """``<stem>.sup.nwk``: the NJ tree of ``pred`` with the supports of ``reps``."""
        runner.put(entry.path, "sup.nwk", runner.host.nj_support(pred, reps, entry.ids(), runner.writer_cap()))

    # -- --tbe / --bootstrap-refined (supports.py) -----------------------------------------------
    def kinds(self, runner) -> List[Kind]:
        """The trees that get supports: NJ (``.sup.nwk``, from the same replicate NJ tables as every other output), and
        with ``--bootstrap-refined`` those of ``--bme`` / ``--spr``."""
        return [k for k in NJ_STARTED if k.search is None or (self.refined and set(k.flags) <= set(runner.flags))]

    def _match(self, who, ref_slots, rep_slots, rep_flag) -> tuple:
        """The supports by ``who``, without the status; with ``--instability`` the transfers, whose first three arrays they are."""
        if self.instability is not None:
            return who.join_transfers(ref_slots, rep_slots, rep_flag, self.instability)[:-1]
        return who.join_supports(ref_slots, rep_slots, rep_flag)[:-1]

    def _extend(self, runner, engine, shape, preds, reps):
        """On the GPU thread, behind ``follow``: from a kind's threshold on the NJ tables of all ``B (R + 1)`` trees of the
        sub-batch and their refinement, from ``SUPPORT_DEVICE_MIN`` (``--instability``: ``TRANSFER_DEVICE_MIN``) on the matching
        of every kind whose tables are the device's (NJ's: joined there for it), from ``CONSENSUS_DEVICE_MIN`` on their consensus.
        Returns the columns ``(reps, tables)``: ``tables[b][kind name]`` is a ``SupportTables``, or absent (the writer's work)."""
        from . import consensus, supports, treedist
        B, R, n = len(preds), self.replicates, shape[0]
        tables = [{} for _ in range(B)]
        refine = [k for k in self.kinds(runner) if k.search is not None and reaches(k.minimum(), n, 4)]
        moves = self.instability is not None
        match = reaches(supports.TRANSFER_DEVICE_MIN if moves else supports.SUPPORT_DEVICE_MIN, n, 4)
        agree = self.consensus is not None and reaches(consensus.CONSENSUS_DEVICE_MIN, n, 4)
        far = self.treedist and reaches(treedist.reps_minimum(R + 1), n, 4)
        if not refine and not match and not agree and not far:
            return reps, tables
        t0 = time.perf_counter()
        every = np.concatenate([preds[:, None, :], reps], axis=1).reshape(B * (R + 1), -1)       # own tree first
        made = join_refine(engine, "nj", [k.search for k in refine], every)      # (joined once: they serve every output)
        matched = agreed = 0
        for kind in [NJ] + refine:
            slots, lengths, _steps, flag = (x.reshape(B, R + 1, *x.shape[1:]) for x in made[kind.search])
            res = con = dist = None
            if far and kind is NJ:          # (a flagged tree - the file's own too - is never read)
                dist = engine.join_distances(slots, lengths, flag)
            if match:
                res = self._match(engine, with_stand_ins(slots[:, 0], flag[:, 0]), slots[:, 1:], flag[:, 1:])
            if agree:
                con = engine.join_consensus(slots[:, 1:], lengths[:, 1:], flag[:, 1:], self.consensus)
            for b in range(B):
                if flag[b, 0]:
                    continue                                     # no tree of its own: the writer's plain text
                tables[b][kind.name] = SupportTables(
                    slots[b, 0], lengths[b, 0], slots[b, 1:], flag[b, 1:], None if res is None else tuple(x[b] for x in res),
                    lengths[b, 1:], None if con is None else tuple(x[b] for x in con), None if dist is None else tuple(x[b] for x in dist))
                matched += res is not None
                agreed += con is not None
        runner.book(supports_device=matched, supports_device_s=time.perf_counter() - t0, **({"consensus_device": agreed} if agree else {}),
                    **({"transfers_device": matched} if moves else {}))
        return reps, tables

    def _host_tables(self, runner, kind, pred, reps) -> SupportTables:
        """One file's tables of one kind on a writer thread, by the runner's host side."""
        every = np.concatenate([np.asarray(pred, dtype=np.float32).reshape(1, -1), reps])
        slots, lengths, _steps, bad = join_refine(runner.host, "nj", [s for s in (kind.search,) if s], every)[kind.search]
        return SupportTables(None if bad[0] else slots[0], lengths[0], slots[1:], bad[1:], None, lengths[1:], None)

    def write_supports(self, runner, shape, rows):
        """Some files of a sub-batch on a writer thread: per kind of tree ``<stem>[.<kind>].sup.nwk`` and, with ``--tbe``,
        ``<stem>[.<kind>].tbe.nwk``.  Tables and results the GPU thread left are formatted; the others come from the
        runner's host side first.  With ``--consensus`` also ``<stem>[.<kind>].con.nwk``, from the same replicate tables;
        with ``--instability`` the transfers' other results give the three files of ``supports.instability_texts``."""
        from . import supports
        from .consensus import newick_of_consensus, star
        n, R, host, cap = shape[0], self.replicates, runner.host, runner.writer_cap()
        kinds = self.kinds(runner)
        for entry, pred, reps, given in rows:
            ids = entry.ids()
            for kind in kinds:
                table = None                                 # (fewer than four sequences: no split)
                if n >= 4:
                    table = given[kind.name] if kind.name in given else self._host_tables(runner, kind, pred, reps)
                if table is None or table.slots is None:    # no split, or no tree of its own: the plain text
                    text = host.nj_support(pred, reps, ids, cap) if kind.search is None else host.tree_text(kind, pred, ids)[0]
                    texts, slots, lengths, res = (text, text), None, None, None
                else:
                    slots, lengths = table.slots, table.lengths
                    res = table.results
                    if res is None:
                        res = self._match(host, slots, table.rep_slots, table.rep_flag)
                    texts = supports.support_texts(slots, lengths, ids, *res[:3], R)
                if self.instability is not None:
                    moved = supports.instability_texts(slots, lengths, ids, res, R, _text(texts[0]))
                    for suffix, text in zip(kind.files("instability.tsv", "branches.tsv", "branches.nwk"), moved):
                        runner.put(entry.path, suffix, text)
                for suffix, text in zip(kind.files("sup.nwk", "tbe.nwk"), texts[:1 + self.tbe]):
                    runner.put(entry.path, suffix, text)
                if self.consensus is not None:
                    # (no table: fewer than four sequences - the star; else the GPU thread's results where it left them)
                    con = star(n) if table is None else table.consensus
                    if con is None:
                        con = host.join_consensus(table.rep_slots, table.rep_lengths, table.rep_flag, self.consensus)
                    runner.put(entry.path, kind.files("con.nwk")[0], newick_of_consensus(ids, con, R))
        runner.book(tbe=len(rows) * len(kinds) if self.tbe else 0, refined_supports=len(rows) * (len(kinds) - 1),
                    **({"consensus": len(rows) * len(kinds)} if self.consensus is not None else {}),
                    **({"instability": len(rows) * len(kinds)} if self.instability is not None else {}))

    def write_treedist(self, runner, shape, rows):
        """Some files of a sub-batch on a writer thread, with ``--treedist``: ``<stem>.treedist.reps.tsv`` and
        ``<stem>.treedist.rf.phy`` over ``[nj tree, replicate 1 .. R]`` - the GPU thread's distances where it left them,
        else the host side's on the NJ tables; ``NA`` throughout for fewer than four sequences."""
        from . import treedist
        n, R = shape[0], self.replicates
        for entry, pred, reps, given in rows:
            dist = treedist.no_distances(R + 1)
            if n >= treedist.MIN_SEQS:
                table = given["nj"] if "nj" in given else self._host_tables(runner, NJ, pred, reps)
                dist = table.distances
                if dist is None:
                    own = table.slots is None
                    slots = np.concatenate([(np.zeros_like(table.rep_slots[0]) if own else table.slots)[None], table.rep_slots])
                    dist = runner.host.join_distances(slots, np.concatenate([np.asarray(table.lengths)[None], table.rep_lengths]),
                                                      np.concatenate([[own], np.asarray(table.rep_flag, dtype=bool)]))
            runner.put(entry.path, "treedist.reps.tsv", treedist.reps_tsv(n, dist))
            runner.put(entry.path, "treedist.rf.phy", treedist.rf_phylip(n, dist))

    def jobs(self, runner, shape, part, preds, reps, tables=None):
        cap = runner.writer_cap()       # (the host twins of R searches per file: spread over the writers, as _write_trees)
        if tables is None:
            out = super().jobs(runner, shape, part, preds, reps)
        else:
            rows = list(zip(part, preds, reps, tables))
            out = [(self.write_supports, runner, shape, rows[k::cap]) for k in range(min(cap, len(rows)))]
        if self.treedist:
            rows = list(zip(part, preds, reps, tables if tables is not None else [{}] * len(part)))
            out += [(self.write_treedist, runner, shape, rows[k::cap]) for k in range(min(cap, len(rows)))]
        return out


class Windows(Analysis):
    flag = "--windows"
    option = {"default": None, "metavar": "W[:STEP]"}
    help = ("scan along every alignment: the distances (with -t the NJ tree) of every window of W sites, "
            "STEP sites apart (default STEP = W: non-overlapping; a last window is anchored at L - W so that "
            "every site is covered), cut and inferred on the GPU: writes <stem>.w<first>-<last>.phy per "
            "window (1-based inclusive sites) and <stem>.windows.tsv (first, last, mean_distance, and the "
            "Robinson-Foulds distances of the window's NJ tree to the previous window's and to the whole "
            "alignment's); <stem>.phy is unchanged; a file with fewer than W sites is an error")
    refuses = (("--bootstrap", "replicates of windows are out of scope"),
               (SHARD_SITES, "every window would need its own collectives"))

    def __init__(self, width: int, step: int):
        self.width, self.step = int(width), int(step)

    @classmethod
    def from_args(cls, args):
        if args.windows is None:
            return None
        from .windows import parse_windows_arg
        try:
            return cls(*parse_windows_arg(args.windows))
        except ValueError as exc:
            raise ValueError(f"--windows: {exc}") from None

    def stats(self):
        return {"windows": 0, "windows_s": 0.0}

    def accepts(self, n, l):
        return l >= self.width

    def file_error(self, path, n, l):
        return ValueError(f"--windows: {path} has L = {l} sites, fewer than the window width W = {self.width}")

    def starts(self, n_sites: int) -> List[int]:
        from .windows import window_starts
        return window_starts(n_sites, self.width, self.step)

    def floats(self, shape):
        return len(self.starts(shape[1])) * (shape[0] * (shape[0] - 1) // 2)

    def follow(self, engine, batch):
        """(``pf_forward_windows``: the sources go up once, the windows are cut on the device)"""
        return engine.forward_windows(batch, self.width, self.step)

    def account(self, stats, count, shape, seconds):
        stats["windows_s"] += seconds
        stats["windows"] += count * len(self.starts(shape[1]))

    def suffixes(self, n_sites: int, ext: str) -> List[str]:
        from .windows import window_label
        return [f"{window_label(n_sites, st, self.width)}.{ext}" for st in self.starts(n_sites)]

    def write(self, runner, shape, entry, pred, wpred, files: bool = True):
        """One file's window outputs: ``<stem>.w<first>-<last>.phy`` (``.nj.nwk`` with ``--trees``) per window - unless
        ``write_native`` has written them - and ``<stem>.windows.tsv``."""
        from .windows import summary_tsv
        ids = entry.ids()
        wtrees = [runner.nj(w, ids) for w in wpred]
        if files:
            for phy, nwk, w, tree in zip(self.suffixes(shape[1], "phy"), self.suffixes(shape[1], "nj.nwk"), wpred, wtrees):
                runner.put(entry.path, phy, runner.phylip(w, ids))
                if runner.trees:
                    runner.put(entry.path, nwk, tree)
        runner.put(entry.path, "windows.tsv", summary_tsv(self.starts(shape[1]), self.width, wpred,
                                                           [_text(t) for t in wtrees], _text(runner.nj(pred, ids))))

    def write_native(self, runner, shape, part, preds, wpreds):
        """The same files for a sub-batch: the window matrices (and trees) of all its files in one native call, then
        the tables."""
        from .hostio import write_phylip
        entries = [e.source for e in part for _ in self.starts(shape[1])]
        outs = [runner.out_path(e.path, s) for e in part for s in self.suffixes(shape[1], "phy")]
        trees = [runner.out_path(e.path, s) for e in part for s in self.suffixes(shape[1], "nj.nwk")] if runner.trees else None
        write_phylip(entries, shape[0], wpreds.reshape(len(entries), -1), outs, runner.writer_cap(), trees)
        for entry, pred, wp in zip(part, preds, wpreds):
            self.write(runner, shape, entry, pred, wp, files=False)

    def jobs(self, runner, shape, part, preds, wpreds):
        if runner.native_io:
            return [(self.write_native, runner, shape, part, preds, wpreds)]
        return super().jobs(runner, shape, part, preds, wpreds)


class SiteProfile(Analysis):
    flag = "--site-profile"
    help = ("site-resolved distances from the same forward: writes <stem>.sites.tsv (site, profile = the "
            "mean over pairs of the site's term of the distances, relative = profile / its mean over sites) "
            "and <stem>.se.phy, the standard error of every distance's mean over sites as a PHYLIP matrix (a "
            "descriptive statistic of the model's own per-site terms, not a calibrated confidence interval); "
            "<stem>.phy is unchanged")
    refuses = (("--bootstrap", "site maps of replicates are out of scope"),
               ("--windows", "site maps of windows are out of scope"),
               (SHARD_SITES, "a rank would hold a slice of the site map"))

    def forward(self, runner, engine, shape, batch):
        # the same forward (its distances are forward's, bit for bit) also leaves se and the site profile
        preds, ses, profiles = engine.forward_site_profile(batch)
        return preds, (ses, profiles)

    def write(self, runner, shape, entry, pred, se, profile):
        """``<stem>.sites.tsv`` and ``<stem>.se.phy`` of one file (ids and number format of ``<stem>.phy``)."""
        from .siteprofile import sites_tsv
        runner.put(entry.path, "sites.tsv", sites_tsv(profile))
        runner.put(entry.path, "se.phy", runner.phylip(se, entry.ids()))


class LeaveOneOut(Analysis):
    flag = "--leave-one-out"
    help = ("taxon influence: every alignment is inferred again without each of its sequences in turn (cut and "
            "inferred on the GPU): writes <stem>.taxa.tsv (index, id, influence = RMS move of the other "
            "distances when the sequence leaves, shift = their mean move, relative = influence / its mean; with "
            "-t rf_pruned = Robinson-Foulds distance of the cut's NJ tree to the whole alignment's NJ tree "
            "without that leaf) and <stem>.context.phy, how much each distance depends on the other sequences, "
            "as a PHYLIP matrix (descriptive statistics, not a test); <stem>.phy is unchanged; a file with "
            "fewer than 3 sequences is an error")
    refuses = (("--bootstrap", "replicates of taxon subsets are out of scope"),
               ("--windows", "taxon subsets of windows are out of scope"),
               ("--site-profile", "site maps of taxon subsets are out of scope"),
               (SHARD_SITES, "every cut would need its own collectives"))

    def stats(self):
        return {"loo_sets": 0}

    def accepts(self, n, l):
        return n >= 3

    def file_error(self, path, n, l):
        """(a file with fewer than 3 sequences has no leave-one-out cut with a pair)"""
        return ValueError(f"--leave-one-out: {path} has N = {n} sequences, fewer than the 3 a cut with one pair needs")

    def forward(self, runner, engine, shape, batch):
        """The same distances (forward's, bit for bit), then the N cuts of every alignment and their statistics, in
        sub-batches; the cuts' distances are kept only for the trees of ``rf_pruned`` (``--trees``)."""
        N = shape[0]
        parts = [engine.forward_leave_one_out(batch[s], keep_loo=runner.trees)
                 for s in sub_batches(len(batch), N * (N - 1) * (N - 2) // 2)]
        preds, infls, shifts, ctxs, *loos = [np.concatenate([p[k] for p in parts]) for k in range(len(parts[0]))]
        return preds, (infls, shifts, ctxs, loos[0] if loos else [None] * len(batch))

    def account(self, stats, count, shape, seconds):
        stats["loo_sets"] += count * shape[0]

    def write(self, runner, shape, entry, pred, infl, shift, ctx, loo):
        """``<stem>.taxa.tsv`` and ``<stem>.context.phy`` of one file (ids and number format of ``<stem>.phy``); with
        ``--trees`` the column ``rf_pruned`` from NJ trees on index labels."""
        from .taxa import rf_pruned, taxa_tsv
        ids = entry.ids()
        N = len(ids)
        rf = None
        if runner.trees:
            labels = [str(k) for k in range(N)]
            rf = ["NA"] * N if N - 1 < 4 else rf_pruned(
                _text(runner.nj(pred, labels)), [_text(runner.nj(loo[t], labels[:t] + labels[t + 1:])) for t in range(N)], N)
        runner.put(entry.path, "taxa.tsv", taxa_tsv(ids, infl, shift, rf))
        runner.put(entry.path, "context.phy", runner.phylip(ctx, ids))


class CompressSites(Analysis):
    flag = "--compress-sites"
    help = ("site-pattern compression: every alignment is inferred on its distinct columns with their "
            "counts as site weights (the same distances to rounding, fewer tokens where columns repeat); "
            "with --bootstrap R it is the R replicates that run on their distinct sites with their "
            "multiplicities (about a third fewer tokens per replicate; the alignment itself is inferred "
            "as without the flag, so only the support values of <stem>.sup.nwk can differ)")
    refuses = (("--windows", "a window is a run of sites, not of patterns"),
               ("--site-profile", "the profile is per site, not per pattern"),
               ("--leave-one-out", "weighted taxon subsets are out of scope"),
               (SHARD_SITES, "weighted forwards are not site-sharded"))

    def bind(self, modes):
        boot = next((m for m in modes if isinstance(m, Bootstrap)), None)
        if boot is not None:
            # (with --bootstrap the whole alignment keeps forward's bits - <stem>.phy, the tree and its branch lengths in
            # <stem>.sup.nwk are those of a run without the flag - and the R replicates, the cost, run compressed)
            boot.call = "bootstrap_weighted"
            self.forward = None

    def forward(self, runner, engine, shape, batch):
        """Every alignment as its distinct columns with their counts as weights, padded to ``padded_sites`` of its own
        count (site 0, weight 0).  Alignments of one padded size share a launch; a file's distances depend on the file
        alone."""
        from . import weights_sites as ws
        B, N, L = batch.shape
        tables = [ws.pad_table(f, c, ws.padded_sites(len(f), L)) for f, c in (runner.host.compress_sites(a) for a in batch)]
        preds = np.empty((B, N * (N - 1) // 2), dtype=np.float32)
        for kp in sorted({len(s) for s, _w in tables}):
            who = [b for b in range(B) if len(tables[b][0]) == kp]
            cut = np.stack([batch[b][:, tables[b][0]] for b in who])
            preds[who] = engine.forward_weighted(cut, np.stack([tables[b][1] for b in who]))
        return preds, ()


class Place(Analysis):
    flag = "--place"
    option = {"type": int, "default": 0, "metavar": "Q"}
    help = ("query placement: the last Q sequences of every file are queries, the sequences before them the "
            "backbone (where `mafft --add` puts added sequences); every query is inferred alone with the backbone "
            "(cut and inferred on the GPU): writes <stem>.place.dist.tsv (the distances of every query to every "
            "backbone sequence) and <stem>.place.tsv (index, id, nearest = backbone id of the smallest distance, "
            "nearest_distance, disturb = RMS move of the backbone's own distances when the query joins, shift = "
            "their mean move, joint = RMS move of the query's distances when the other queries join too; with -t "
            "edge, x, pendant, residual = the least-squares placement on the backbone's NJ tree, the edge named "
            "by the leaves of its smaller side) and with -t <stem>.placed.nwk, that tree with all queries "
            "attached (descriptive statistics, not a test); <stem>.phy is unchanged; a file with fewer than Q + 2 "
            "sequences is an error; 0 (default) = off")
    refuses = (("--bootstrap", "replicates of query sets are out of scope"),
               ("--windows", "query sets of windows are out of scope"),
               ("--site-profile", "site maps of query sets are out of scope"),
               ("--leave-one-out", "cuts of query sets are out of scope"),
               ("--compress-sites", "weighted query sets are out of scope"),
               (SHARD_SITES, "every query set would need its own collectives"))

    def __init__(self, queries: int):
        self.queries = int(queries)

    @classmethod
    def from_args(cls, args):
        if args.place < 0:
            raise ValueError(f"--place must be >= 0 (got {args.place})")
        return cls(args.place) if args.place else None

    def stats(self):
        return {"place_sets": 0}

    def accepts(self, n, l):
        return n >= self.queries + 2

    def file_error(self, path, n, l):
        """(a backbone needs two sequences: one pair)"""
        return ValueError(f"--place: {path} has n = {n} sequences, fewer than the Q + 2 = {self.queries + 2} that "
                          f"Q = {self.queries} queries and a backbone of 2 need")

    def forward(self, runner, engine, shape, batch):
        """The same distances (forward's, bit for bit), then the backbone's and the Q query sets of every alignment and
        their statistics, in sub-batches; the sets' distances themselves are not kept."""
        Q, N = self.queries, shape[0] - self.queries
        parts = [engine.forward_place(batch[s], Q) for s in sub_batches(len(batch), Q * (N + 1) * N // 2)]
        preds, *rest = [np.concatenate([p[k] for p in parts]) for k in range(len(parts[0]))]
        return preds, tuple(rest)

    def account(self, stats, count, shape, seconds):
        stats["place_sets"] += count * self.queries

    def write(self, runner, shape, entry, pred, base, place, disturb, shift, joint):
        """``<stem>.place.dist.tsv`` and ``<stem>.place.tsv`` of one file; with ``--trees`` the placement columns and
        ``<stem>.placed.nwk``, from the backbone's NJ tree on index labels (duplicate ids do not matter)."""
        from .place import Backbone, graft, ls_place, place_dist_tsv, place_tsv
        ids = entry.ids()
        N = len(ids) - self.queries
        back, queries = ids[:N], ids[N:]
        cols = None
        if runner.trees:
            labels = [str(k) for k in range(N)]
            bb = Backbone(_text(runner.nj(base, labels)), labels)
            found = [ls_place(bb, d) for d in place]
            cols = [("NA",) * 4 if N == 2 else (bb.edge_label(p.edge, back), p.x, p.pendant, p.residual) for p in found]
            runner.put(entry.path, "placed.nwk", graft(bb, found, queries, back))
        runner.put(entry.path, "place.dist.tsv", place_dist_tsv(back, queries, place))
        runner.put(entry.path, "place.tsv", place_tsv(back, queries, place, disturb, shift, joint, cols))


class Tile(Analysis):
    flag = "--tile"
    option = {"type": int, "default": 0, "metavar": "M"}
    help = ("tiled inference for files with more than M sequences, the model's sequence cap included: the sequences "
            "are cut, in file order, into groups of at most M / 2, every pair of groups is inferred as one alignment of "
            "at most M sequences (cut and inferred on the GPU, about twice the tokens of one forward, the memory of "
            "one context) and the results are combined on the GPU: <stem>.phy holds, for two sequences of different "
            "groups, the distance of the one context they share and, for two of one group, the mean over all the "
            "contexts of that group (with -t <stem>.nj.nwk is the NJ tree of these distances; a file of " + str(NJ_DEVICE_MIN) + " "
            "sequences or more has it joined on the GPU, the same bytes); writes <stem>.spread.phy, the standard deviation of "
            "every within-group distance over its contexts (0 across groups: one context, nothing measured; "
            "descriptive, not a test) and <stem>.tile.tsv (index, id, group); a file with at most M sequences runs "
            "exactly as without the flag; M must be between 2 and the model's cap of 200; 0 (default) = off")
    refuses = (("--bootstrap", "replicates of tile sets are out of scope"),
               ("--windows", "tile sets of windows are out of scope"),
               ("--site-profile", "site maps of tile sets are out of scope"),
               ("--leave-one-out", "cuts of tile sets are out of scope"),
               ("--compress-sites", "weighted tile sets are out of scope"),
               ("--place", "query sets of tile sets are out of scope"),
               (SHARD_SITES, "every tile set would need its own collectives"))

    def __init__(self, context: int):
        self.context = int(context)

    @classmethod
    def from_args(cls, args):
        from .scheduler import MAX_SEQS
        if args.tile and not 2 <= args.tile <= MAX_SEQS:
            raise ValueError(f"--tile must be 0 (off) or a context of 2 to {MAX_SEQS} sequences (got {args.tile})")
        return cls(args.tile) if args.tile else None

    def stats(self):
        return {"tiled": 0, "tile_sets": 0, "nj_device": 0, "nj_device_s": 0.0}

    def lifts_seq_cap(self, n):
        return n > self.context

    def forward(self, runner, engine, shape, batch):
        """A launch of files with at most M sequences is the plain forward and has no payload: nothing but ``<stem>.phy``
        (and the tree) is written for them.  Larger files: the tiled distances in place of forward's, and the spread."""
        if shape[0] <= self.context:
            return engine.forward(batch), ()
        out, spread = engine.forward_tiled(batch, self.context)
        tables = [None] * len(out)
        if runner.trees and self.writes_tree(shape):
            # the joins of every file's tree on the device; a file with a non-finite distance keeps the host's
            tables = runner.device_tables(engine, shape[0], out, [NJ]).get("nj", tables)
        return out, (spread, tables)

    def account(self, stats, count, shape, seconds):
        if shape[0] > self.context:
            from .tile import groups
            G = groups(shape[0], self.context)
            stats["tiled"] += count
            stats["tile_sets"] += count * G * (G - 1) // 2

    def writes_tree(self, shape):
        return NJ_DEVICE_MIN is not None and shape[0] > self.context and shape[0] >= NJ_DEVICE_MIN

    def write(self, runner, shape, entry, pred, spread, table):
        """``<stem>.spread.phy`` (ids and number format of ``<stem>.phy``) and ``<stem>.tile.tsv`` of one file; where the
        tree is this mode's (``writes_tree``), ``<stem>.nj.nwk`` from the device's join table - the bytes of the host's
        neighbour joining, which a file without a table (non-finite distances) falls back to."""
        from .tile import tile_tsv
        ids = entry.ids()
        runner.put(entry.path, "spread.phy", runner.phylip(spread, ids))
        runner.put(entry.path, "tile.tsv", tile_tsv(ids, self.context))
        if runner.trees and self.writes_tree(shape):
            runner.put(entry.path, "nj.nwk", runner.nj(pred, ids) if table is None else runner.newick_of_joins(table.slots, table.lengths, ids))


MODES = (Bootstrap, Windows, SiteProfile, LeaveOneOut, CompressSites, Place, Tile)


def modes_from_args(args, error) -> List[Analysis]:
    """The modes ``args`` switches on.  A bad value or a refused combination goes to ``error(text)`` (``parser.error``,
    which does not return): modes in the order of ``MODES``, each its own value first, then its ``refuses`` in order."""
    on = {}
    for cls in MODES:
        try:
            mode = cls.from_args(args)
        except ValueError as exc:
            error(str(exc))
        if mode is None:
            continue
        for other, reason in cls.refuses:
            if other in on or (other == SHARD_SITES and args.shard == "sites"):
                error(cls.refusal(other, reason))
        on[cls.flag] = mode
    return list(on.values())
