"""Identity and speed of the host side of the tree calls between two trees of this repository (no GPU).

    python tools/host_tree_calls_identity.py PARENT_TREE [NEW_TREE] [--speed REPEATS]

Both trees must hold a built library.  One child process per tree runs the same cases - every text call and every table
call of ``hostio``, every text symbol through ctypes directly, and the host forms of ``Engine`` against a recording stub
in place of the library - and writes one record per case: the bytes returned, every array (``tobytes()``), the return
code, or the type and text of the exception.  The parent process compares the records and prints one line per family
and every mismatch in full.  ``--speed``: also times ``nj_newick`` / ``bme_newick`` / ``spr_newick`` / ``bionj_newick``
over the distances of ``tests/golden/e2e_testdata.npz`` (the ``pf/`` keys), one child per tree and repeat, alternating.
"""
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 2, 3, 4, 5, 8, 33, 65, 130)          # 65, 130: across the 64-bit words of the split sets
EDGE_IDS = ("", "nul\0in", "é", "日本", "a b", "(x:1)", "x" * 40)


def digest(x):
    if x is None or isinstance(x, (int, float, str, bool)):
        return x
    if isinstance(x, (bytes, bytearray)):
        return ["bytes", len(x), hashlib.sha256(bytes(x)).hexdigest()[:24]]
    if isinstance(x, np.ndarray):
        return ["array", str(x.dtype), list(x.shape), hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:24]]
    if isinstance(x, np.generic):
        return ["scalar", str(x.dtype), x.tobytes().hex()]
    if isinstance(x, (tuple, list)):
        return [digest(y) for y in x]
    raise TypeError(type(x))


def attempt(fn, *args, **kw):
    try:
        return digest(fn(*args, **kw))
    except Exception as exc:                      # the type and the text are part of the record
        return ["raised", type(exc).__name__, str(exc)]


def ids_of(n, kind):
    if kind == "plain":
        return [f"taxon{i}" for i in range(n)]
    return [EDGE_IDS[i % len(EDGE_IDS)] + ("" if i < len(EDGE_IDS) else str(i)) for i in range(n)]


def vector(n, kind, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    v = rng.uniform(0.05, 3.0, size=n * (n - 1) // 2).astype(np.float32)
    if kind == "negative" and v.size > 2:         # far from additive: negative branch lengths for the clamp
        v[::3] *= 0.01
    if kind == "nan" and v.size:
        v[v.size // 2] = np.nan
    if kind == "inf" and v.size:
        v[-1] = np.inf
    return v


def text_cases(h, rec):
    for n in SIZES:
        for kind in ("plain", "negative", "nan", "inf"):
            for clamp in (True, False):
                for idk in ("plain", "edge"):
                    if idk == "edge" and kind not in ("plain", "negative"):
                        continue
                    v, ids, key = vector(n, kind), ids_of(n, idk), f"text N={n} {kind} clamp={clamp} ids={idk}"
                    rec[key + " nj_newick"] = attempt(h.nj_newick, v, ids, clamp)
                    rec[key + " bionj_newick"] = attempt(h.bionj_newick, v, ids, clamp)
                    rec[key + " format_phylip"] = attempt(h.format_phylip, v, ids)
                    for search in ("bme", "spr"):
                        rec[key + " bionj_refined " + search] = attempt(h.bionj_refined_newick, search, v, ids, clamp)
                    for steps in (False, True):
                        rec[key + f" bme_newick steps={steps}"] = attempt(h.bme_newick, v, ids, clamp, steps)
                        rec[key + f" spr_newick steps={steps}"] = attempt(h.spr_newick, v, ids, clamp, steps)
                    reps = np.stack([vector(n, "plain", s) for s in (1, 2, 3)]) if n > 1 else np.zeros((3, 0), np.float32)
                    for threads in (1, 3):
                        rec[key + f" nj_support threads={threads}"] = attempt(h.nj_support, v, reps, ids, clamp, threads)
                    if n >= 3 and kind in ("plain", "negative"):
                        slots, lengths, _ = h.nj_joins_host(v[None, :])
                        rec[key + " newick_of_joins"] = attempt(h.newick_of_joins, slots[0], lengths[0], ids, clamp)
        ids = ids_of(n, "plain")
        for name, v in (("short", vector(n + 1, "plain")[:max(0, n * (n - 1) // 2 - 1)]), ("long", vector(n + 1, "plain"))):
            key = f"text N={n} wrong count ({name})"
            for fn in ("nj_newick", "bionj_newick", "format_phylip", "bme_newick", "spr_newick"):
                rec[f"{key} {fn}"] = attempt(getattr(h, fn), v, ids)
            rec[key + " bionj_refined"] = attempt(h.bionj_refined_newick, "bme", v, ids)
            rec[key + " nj_support"] = attempt(h.nj_support, v, v[None, :], ids)
            rec[key + " nj_support reps"] = attempt(h.nj_support, vector(n, "plain"), v[None, :], ids)
        rec[f"text N={n} newick_of_joins short table"] = attempt(h.newick_of_joins, np.zeros(2, np.int32), np.zeros(2), ids)
        rec[f"text N={n} newick_of_joins slot out of range"] = attempt(
            h.newick_of_joins, np.full(max(0, 2 * (n - 3) + 3), n, np.int32), np.zeros(max(0, 2 * (n - 3) + 3)), ids)
    rec["text no ids format_phylip"] = attempt(h.format_phylip, np.zeros(0, np.float32), [])
    rec["text no ids nj_newick"] = attempt(h.nj_newick, np.zeros(0, np.float32), [])
    rec["text no ids bme_newick"] = attempt(h.bme_newick, np.zeros(0, np.float32), [], True, True)


def ctypes_cases(h, rec):
    """Every text symbol directly: capacities, a negative id length, each null argument, n out of range, a bad slot."""
    lib = h._lib()
    max_n = 16384                                 # pfbme::MAX_N
    for n in (3, 4, 9, 65):
        v = vector(n, "negative")
        enc = [s.encode("utf8") for s in ids_of(n, "edge")]
        arr = (C.c_char_p * n)(*enc)
        lens = np.array([len(e) for e in enc], dtype=np.int64)
        reps = np.stack([vector(n, "plain", s) for s in (1, 2)])
        slots, lengths, _ = h.nj_joins_host(v[None, :])
        slots, lengths = np.ascontiguousarray(slots[0]), np.ascontiguousarray(lengths[0])
        steps = C.c_int32(-7)
        # symbol -> (arguments with "out" / "cap" in place, positions of the pointers that may be nulled, of n, least n,
        # whether n above MAX_N is refused)
        def calls(ids=arr, id_lens=lens, sl=slots):
            d, il = v.ctypes.data, id_lens.ctypes.data
            table = {
                "pf_nj_newick_n": ([d, n, ids, il, 1, "out", "cap"], (0, 2, 3), 1, 1, False),
                "pf_bionj_newick_n": ([d, n, ids, il, 1, "out", "cap"], (0, 2, 3), 1, 1, False),
                "pf_bme_newick_n": ([d, n, ids, il, 0, "out", "cap"], (0, 2, 3), 1, 1, True),
                "pf_bme_spr_newick_n": ([d, n, ids, il, 1, "out", "cap"], (0, 2, 3), 1, 1, True),
                "pf_bme_newick_steps_n": ([d, n, ids, il, 1, "out", "cap", C.byref(steps)], (0, 2, 3, 7), 1, 1, True),
                "pf_bme_spr_newick_steps_n": ([d, n, ids, il, 0, "out", "cap", C.byref(steps)], (0, 2, 3, 7), 1, 1, True),
                "pf_format_phylip_n": ([d, n, ids, il, "out", "cap"], (0, 2, 3), 1, 1, False),
                "pf_nj_format_joins_n": ([sl.ctypes.data, lengths.ctypes.data, n, ids, il, 1, "out", "cap"], (0, 1, 3, 4), 2, 3, False),
                "pf_nj_support_n": ([d, reps.ctypes.data, 2, n, ids, il, 1, 2, "out", "cap"], (0, 1, 4, 5), 3, 1, False),
            }
            return table

        def run(symbol, args, cap, with_out=True):
            buf = C.create_string_buffer(max(cap, 1)) if with_out else None
            steps.value = -7
            rc = getattr(lib, symbol)(*[buf if a == "out" else cap if a == "cap" else a for a in args])
            text = buf.raw[:rc] if with_out and 0 <= rc <= cap else None
            return digest([rc, text, steps.value])

        for symbol, (args, pointers, n_at, least, bounded) in calls().items():
            key = f"ctypes N={n} {symbol}"
            need = getattr(lib, symbol)(*[None if a == "out" else 0 if a == "cap" else a for a in args])
            rec[key + " query"] = digest([need, steps.value])
            for cap in (need - 1, need, need + 5):
                rec[key + f" cap=need{cap - need:+d}"] = run(symbol, args, cap)
            rec[key + " null out, cap > 0"] = run(symbol, args, need, with_out=False)
            for at in pointers:
                rec[key + f" null argument {at}"] = run(symbol, [None if i == at else a for i, a in enumerate(args)], need)
            bad_lens = lens.copy()
            bad_lens[n // 2] = -1
            rec[key + " negative id length"] = run(symbol, calls(id_lens=bad_lens)[symbol][0], need)
            rec[key + " n below the least"] = run(symbol, [least - 1 if i == n_at else a for i, a in enumerate(args)], need)
            if bounded:                           # refused before anything is read
                rec[key + " n above MAX_N"] = run(symbol, [max_n + 1 if i == n_at else a for i, a in enumerate(args)], need)
            if symbol == "pf_nj_support_n":
                rec[key + " R = 0"] = run(symbol, [0 if i == 2 else a for i, a in enumerate(args)], need)
            if symbol == "pf_nj_format_joins_n":
                for where, value in ((0, -1), (len(slots) - 1, n), (len(slots) // 2, 2 ** 31 - 1)):
                    bad = slots.copy()
                    bad[where] = value
                    rec[key + f" slot {where} = {value}"] = run(symbol, calls(sl=bad)[symbol][0], need)
                rec[key + " equals pf_nj_newick_n"] = run(symbol, args, need) == run("pf_nj_newick_n", calls()["pf_nj_newick_n"][0], need)


def table_cases(h, rec):
    for n in (3, 4, 5, 9, 65):
        for b in (1, 3):
            p = np.stack([vector(n, "negative" if s % 2 else "plain", s) for s in range(b)])
            key = f"table N={n} B={b}"
            for threads in (1, 4):
                rec[key + f" nj_joins_host threads={threads}"] = attempt(h.nj_joins_host, p, threads)
            rec[key + " bionj_joins_host"] = attempt(h.bionj_joins_host, p)
            bad = p.copy()
            bad[b - 1, 1] = np.nan
            rec[key + " nj_joins_host nan"] = attempt(h.nj_joins_host, bad, 4)
            rec[key + " bionj_joins_host nan"] = attempt(h.bionj_joins_host, bad)
            nj_start, bionj_start = h.nj_joins_host(p)[0], h.bionj_joins_host(p)[0]
            for name, fn in (("bme_nni_host", h.bme_nni_host), ("bme_spr_host", h.bme_spr_host)):
                rec[f"{key} {name} nj start"] = attempt(fn, p, nj_start)
                rec[f"{key} {name} bionj start"] = attempt(fn, p, bionj_start)
                rec[f"{key} {name} nan"] = attempt(fn, bad, nj_start)
                rec[f"{key} {name} no join table"] = attempt(fn, p, np.zeros_like(nj_start))
                rec[f"{key} {name} start of another shape"] = attempt(fn, p, nj_start[:, :-1])
                rec[f"{key} {name} start without B"] = attempt(fn, p, nj_start[0])
                rec[f"{key} {name} distances without B"] = attempt(fn, p[0], nj_start)
            if n < 4:
                continue
            for r in (1, 2, 7):
                reps = np.stack([np.stack([vector(n, "plain", 10 * s + k) for k in range(r)]) for s in range(b)])
                rep_slots, rep_lengths, _ = h.nj_joins_host(reps.reshape(b * r, -1))
                rep_slots, rep_lengths = rep_slots.reshape(b, r, -1), rep_lengths.reshape(b, r, -1)
                flag = np.zeros((b, r), bool)
                flag[b - 1, r - 1] = True
                for fname, fl in (("no flags", None), ("flags", flag)):
                    k2 = f"{key} R={r} {fname}"
                    rec[k2 + " join_supports_host"] = attempt(h.join_supports_host, nj_start, rep_slots, fl)
                    for moves in (True, False):
                        for cutoff in (100, 50, 0, -1, 101):
                            rec[k2 + f" join_transfers_host branch_moves={moves} cutoff={cutoff}"] = attempt(
                                h.join_transfers_host, nj_start, rep_slots, fl, cutoff, moves)
                    for percent in (50, 75, 99, 49, 100):
                        for ln in (None, rep_lengths):
                            rec[k2 + f" join_consensus_host percent={percent} lengths={ln is not None}"] = attempt(
                                h.join_consensus_host, rep_slots, ln, fl, percent)
                    if b == 1:                    # the shapes without B
                        f1 = None if fl is None else fl[0]
                        rec[k2 + " join_supports_host single"] = attempt(h.join_supports_host, nj_start[0], rep_slots[0], f1)
                        rec[k2 + " join_transfers_host single"] = attempt(h.join_transfers_host, nj_start[0], rep_slots[0], f1)
                        rec[k2 + " join_consensus_host single"] = attempt(h.join_consensus_host, rep_slots[0], rep_lengths[0], f1)
                broken = rep_slots.copy()
                broken[0, 0, :] = 0
                k2 = f"{key} R={r} a table that is none"
                rec[k2 + " join_supports_host"] = attempt(h.join_supports_host, nj_start, broken)
                rec[k2 + " join_transfers_host"] = attempt(h.join_transfers_host, nj_start, broken)
                rec[k2 + " join_consensus_host"] = attempt(h.join_consensus_host, broken, rep_lengths)
                rec[k2 + " join_supports_host reference"] = attempt(h.join_supports_host, np.zeros_like(nj_start), rep_slots)
                rec[k2 + " join_supports_host shapes"] = attempt(h.join_supports_host, nj_start[:, :-1], rep_slots)
    for shape in ((4,), (1, 4), (0, 3), (2, 2, 3), (1, 1), (1, 0)):
        p = np.full(shape, 0.5, np.float32)
        for fn in ("nj_joins_host", "bionj_joins_host"):
            rec[f"table distances {shape} {fn}"] = attempt(getattr(h, fn), p)
        rec[f"table distances {shape} bme_nni_host"] = attempt(h.bme_nni_host, p, np.zeros((1, 3), np.int32))


class Recorder:
    """In the library's place under an Engine without a device: every call is recorded - null or not for an address,
    the value for a dimension - and answers `rc`."""

    def __init__(self, rc):
        self.rc, self.calls = rc, []

    def pf_last_error(self, _h):
        return b"the library's message"

    def __getattr__(self, name):
        if not name.startswith("pf_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append([name] + [None if a is None else "address" if isinstance(a, int) and a > 1 << 20 else a for a in args[1:]])
            return self.rc
        return call


def engine_cases(tree, rec):
    from phyloformer_amd.engine import Engine
    for rc in (0, -1, -4):
        e = object.__new__(Engine)
        e._lib, e._h = Recorder(rc), None

        def through(key, fn, *args):
            e._lib.calls.clear()
            got = attempt(fn, *args)
            rec[f"engine rc={rc} {key}"] = [got, digest(e._lib.calls)]

        for n in (2, 3, 4, 9):
            t = max(0, 2 * (n - 3) + 3)
            for b in (1, 3):
                p = np.stack([vector(n, "plain", s) for s in range(b)])
                st = np.tile(np.arange(t, dtype=np.int64) % n, (b, 1))
                for symbol in ("pf_nj_joins", "pf_bionj_joins"):
                    through(f"_joins {symbol} N={n} [{b}, P]", e._joins, symbol, p)
                    through(f"_joins {symbol} N={n} [P]", e._joins, symbol, p[0])
                for symbol in ("pf_bme_nni", "pf_bme_spr"):
                    through(f"_refine {symbol} N={n} [{b}, P]", e._refine, symbol, p, st)
                    through(f"_refine {symbol} N={n} [P] [T]", e._refine, symbol, p[0], st[0])
                    through(f"_refine {symbol} N={n} [P] [1, T]", e._refine, symbol, p[0], st[:1])
                    through(f"_refine {symbol} N={n} start one short", e._refine, symbol, p, st[:, :-1] if t else np.zeros((b, 1), np.int32))
                    through(f"_refine {symbol} N={n} start without B", e._refine, symbol, p, st[0])
                if n >= 4:
                    rep = np.tile(st[:, None, :], (1, 2, 1))
                    through(f"join_supports N={n} B={b}", e.join_supports, st, rep)
                    through(f"join_supports N={n} B={b} flags", e.join_supports, st, rep, np.eye(b, 2, dtype=bool))
                    through(f"join_supports N={n} single", e.join_supports, st[0], rep[0])
                    through(f"join_supports N={n} shapes", e.join_supports, st, rep[:, :, :-1])
                    through(f"join_transfers N={n} B={b}", e.join_transfers, st, rep, None, 70, False)
                    through(f"join_consensus N={n} B={b}", e.join_consensus, rep, rep.astype(np.float64))
        for shape in ((4,), (1, 4), (0, 3), (2, 2, 3), (0,), (1, 0), ()):
            p = np.full(shape, 0.5, np.float32)
            through(f"_joins distances {shape}", e._joins, "pf_nj_joins", p)
            through(f"_refine distances {shape}", e._refine, "pf_bme_nni", p, np.zeros((1, 3), np.int32))


def record(tree, out):
    sys.path.insert(0, tree)
    from phyloformer_amd import hostio as h
    rec = {}
    text_cases(h, rec)
    ctypes_cases(h, rec)
    table_cases(h, rec)
    engine_cases(tree, rec)
    with open(out, "w") as fh:
        json.dump(rec, fh)


def speed(tree):
    sys.path.insert(0, tree)
    from phyloformer_amd import hostio as h
    z = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "e2e_testdata.npz"))
    vecs = [z[k] for k in sorted(z.keys()) if k.startswith("pf/")]
    ids = {v.size: [f"taxon{i}" for i in range((1 + int(round((1 + 8 * v.size) ** 0.5))) // 2)] for v in vecs}
    out = {}
    for name in ("nj_newick", "bme_newick", "spr_newick", "bionj_newick"):
        fn = getattr(h, name)
        fn(vecs[0], ids[vecs[0].size])
        t0 = time.perf_counter()
        for v in vecs:
            fn(v, ids[v.size])
        out[name] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


def child(mode, tree, *more):
    env = dict(os.environ, PYTHONPATH=tree, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PHYLOFORMER_AMD_LIB", None)
    return subprocess.run([sys.executable, os.path.abspath(__file__), mode, tree, *more], env=env, check=True, capture_output=True,
                          text=True, cwd=tree).stdout


def main(argv):
    if argv and argv[0] == "--record":
        return record(argv[1], argv[2])
    if argv and argv[0] == "--time":
        return speed(argv[1])
    repeats = int(argv[argv.index("--speed") + 1]) if "--speed" in argv else 0
    trees = [os.path.abspath(a) for a in argv if not a.startswith("--") and not a.isdigit()]
    parent, new = trees[0], trees[1] if len(trees) > 1 else os.path.dirname(HERE)
    recs = []
    for i, tree in enumerate((parent, new)):
        out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"host_tree_calls_{os.getpid()}_{i}.json")
        child("--record", tree, out)
        with open(out) as fh:
            recs.append(json.load(fh))
        os.remove(out)
    old, cur = recs
    families, different = {}, []
    for key in sorted(set(old) | set(cur)):
        fam = key.split(" ")[0]
        same = key in old and key in cur and old[key] == cur[key]
        raised = isinstance(cur.get(key), list) and cur[key][:1] == ["raised"]
        f = families.setdefault(fam, [0, 0, 0])
        f[0] += 1
        f[1] += same
        f[2] += raised
        if not same:
            different.append(f"DIFFERENT {key}\n  parent: {old.get(key)}\n  new   : {cur.get(key)}")
    for fam, (total, same, raised) in families.items():
        print(f"{fam}: {total} cases, {same} identical, {total - same} different ({raised} of them end in an exception)")
    print("\n".join(different) if different else "no mismatch")
    if repeats:
        times = {"parent": [], "new": []}
        for _ in range(repeats):
            for name, tree in (("parent", parent), ("new", new)):
                times[name].append(json.loads(child("--time", tree)))
        for fn in times["parent"][0]:
            a, b = [t[fn] for t in times["parent"]], [t[fn] for t in times["new"]]
            inside = min(a) <= statistics.median(b) <= max(a)
            print(f"{fn}: ms per pass over the distances, parent {' '.join(f'{x:.2f}' for x in a)} (min {min(a):.2f}, max {max(a):.2f}); "
                  f"new {' '.join(f'{x:.2f}' for x in b)} (median {statistics.median(b):.2f}): "
                  f"{'inside' if inside else 'below' if statistics.median(b) < min(a) else 'ABOVE'} the parent's min-max")
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
