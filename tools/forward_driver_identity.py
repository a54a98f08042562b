"""Identity of the default forward's host driver between two trees of this repository (needs a GPU).

    python tools/forward_driver_identity.py PARENT_TREE [NEW_TREE]

Both trees must hold a built library.  One fresh child process per tree, one after the other and each under its own
``timeout -k 10``, runs the same forwards on the default kernels (option ``precise`` 0) and writes one record per case:
sha256 digests of every output and - under ``debug_keep`` 1 - of every debug tap (of ``ulist`` and ``plan``, the part the
kernels write), the ``main``, ``site_classes``, ``embed``, ``rowfin``, ``colstats`` and ``colfin`` profile counts, or the
type and text of a refusal.  The parent process compares the records and prints one line per family and every mismatch
in full.

Cases: the shapes (B, N, L) below, their alignments built by ``tests/helpers/dedup_model.py`` with repeated columns so
that ``main_dedup`` 1 sends some alignments down each route; ``main_dedup`` {0, 1, 2} x ``head_fold`` {0, 1} x
``debug_keep`` {0, 1} x ``two_streams`` {0, 1} over the plain, weighted, site-map and emulated-shard forwards (1, 3 and
more shards than sites: empty shards); and once each ``embed_mfma`` 1, ``materialize_x0`` 1, ``colstats_ring`` 0 / 1,
``colstats_fine`` 0 / 1 and a ``ws_limit_mb`` that cuts (5, 3, 70) into chunks of one alignment.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((1, 2, 1), (3, 4, 7), (3, 4, 32), (3, 4, 40), (2, 5, 33), (5, 3, 70))
COUNTS = ("main", "site_classes", "embed", "rowfin", "colstats", "colfin")
CROSS = (("main_dedup", (0, 1, 2)), ("head_fold", (0, 1)), ("debug_keep", (0, 1)), ("two_streams", (0, 1)))
DEFAULTS = {"main_dedup": 1, "head_fold": 1, "debug_keep": 0, "two_streams": 1, "embed_mfma": 0, "materialize_x0": 0,
            "colstats_ring": 1, "colstats_fine": -1, "ws_limit_mb": 24 << 10}
SINGLES = (("embed_mfma", 1), ("materialize_x0", 1), ("colstats_ring", 0), ("colstats_ring", 1), ("colstats_fine", 0),
           ("colstats_fine", 1), ("ws_limit_mb", 0))
CHILD_SECONDS = 600


def sha(x):
    x = np.ascontiguousarray(x)
    return [str(x.dtype), list(x.shape), hashlib.sha256(x.tobytes()).hexdigest()[:24]]


def batch(M, B, N, L):
    """B alignments of N x L: every other one with half its columns distinct (the split route under main_dedup 1), the
    rest with no repeated column (fused)."""
    ks = [max(1, L // 2) if b % 2 == 0 else L for b in range(B)]
    return np.stack([M.alignment(N, L, k, M.PLACEMENTS[b % 3], seed=b) for b, k in enumerate(ks)])


def tap_names(n_blocks):
    names = ["srep", "ulist", "ucount", "plan", "x0"]
    for k in range(n_blocks):
        names += [f"srow{k}", f"ctx{k}", f"mrow{k}", f"x{k + 1}"]
    return names


def written(M, raw):
    """The taps of the (last) run cut down to what its kernels write: a row of ``ulist`` holds ucount[b] entries, the
    rest of the row is whatever the workspace held; likewise the plan's lists (``dedup_model.read_plan``)."""
    if isinstance(raw["ucount"], str):
        return
    ucount = raw["ucount"]
    rows = raw["ulist"].reshape(len(ucount), -1)
    raw["ulist"] = np.concatenate([row[:k] for row, k in zip(rows, ucount)])
    if not isinstance(raw["plan"], str):
        raw["plan"] = [list(map(int, v)) if isinstance(v, list) else int(v) for v in M.read_plan(raw["plan"], len(ucount))]


def record(tree, out):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    from helpers import dedup_model as M
    from phyloformer_amd.engine import Engine, EngineError
    from phyloformer_amd.weights import load_weights
    e = Engine(load_weights(os.path.join(tree, "models", "pf.ckpt")), device=0)
    e.set_option("precise", 0)
    e.set_option("profile", 1)
    names = tap_names(e.architecture[0])
    rec = {}

    def run(key, call, taps):
        e.profile_reset()
        try:
            got = call()
            r = {"out": [sha(g) for g in (got if isinstance(got, tuple) else (got,))]}
        except (EngineError, ValueError) as exc:          # the type and the text are part of the record
            r = {"refused": [type(exc).__name__, str(exc)]}
        r["counts"] = {name: e.profile_get(name)[0] for name in COUNTS}
        if taps:
            raw = {}
            for name in names:
                try:
                    raw[name] = e.debug_read(name).view(np.int32)
                except EngineError as exc:
                    raw[name] = str(exc)
            written(M, raw)
            r["taps"] = {name: t if isinstance(t, (str, list)) else sha(t) for name, t in raw.items()}
        rec[key] = r

    def calls(tag, idx, keep):
        B, _, L = idx.shape
        rng = np.random.default_rng(L)
        w = rng.integers(0, 4, (B, L)).astype(np.float32)
        w[:, 0] = 1.0
        run(f"plain {tag}", lambda: e.forward(idx), keep)
        run(f"weighted {tag}", lambda: e.forward_weighted(idx, w), keep)
        run(f"sitemap {tag}", lambda: e.forward_site_map(idx), keep)
        for nshards in (1, 3, min(L + 1, 64)):
            run(f"shards {tag} nshards={nshards}", lambda: e.forward_shards_emulated(idx, nshards), False)

    def setting(options):
        for key, value in {**DEFAULTS, **options}.items():
            e.set_option(key, value)

    for B, N, L in SHAPES:
        idx = batch(M, B, N, L)
        shape = f"B={B} N={N} L={L}"
        print(f"{tree}: {shape}", file=sys.stderr, flush=True)
        for md in CROSS[0][1]:
            for hf in CROSS[1][1]:
                for dk in CROSS[2][1]:
                    for ts in CROSS[3][1]:
                        setting({"main_dedup": md, "head_fold": hf, "debug_keep": dk, "two_streams": ts})
                        calls(f"{shape} main_dedup={md} head_fold={hf} debug_keep={dk} two_streams={ts}", idx, bool(dk))
        for key, value in SINGLES:
            setting({key: value})
            run(f"single {shape} {key}={value}", lambda: e.forward(idx), False)
            setting({key: value, "debug_keep": 1})
            run(f"single {shape} {key}={value} debug_keep=1", lambda: e.forward(idx), True)
    setting({})
    e.close()
    with open(out, "w") as fh:
        json.dump(rec, fh)


def child(tree, out):
    env = dict(os.environ, PYTHONPATH=tree, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PHYLOFORMER_AMD_LIB", None)
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--record", tree, out]
    res = subprocess.run(cmd, env=env, cwd=tree)          # (its progress lines, one per shape, go to stderr)
    if res.returncode != 0:                   # a fault, an abort or the time limit: nothing more is started
        sys.exit(f"the child for {tree} ended with status {res.returncode}")


def main(argv):
    if argv and argv[0] == "--record":
        return record(argv[1], argv[2])
    trees = [os.path.abspath(a) for a in argv if not a.startswith("--")]
    parent, new = trees[0], trees[1] if len(trees) > 1 else os.path.dirname(HERE)
    recs = []
    for i, tree in enumerate((parent, new)):
        out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"forward_driver_{os.getpid()}_{i}.json")
        child(tree, out)
        with open(out) as fh:
            recs.append(json.load(fh))
        os.remove(out)
    old, cur = recs
    families, different = {}, []
    for key in sorted(set(old) | set(cur)):
        same = key in old and key in cur and old[key] == cur[key]
        f = families.setdefault(key.split(" ")[0], [0, 0, 0, 0])
        f[0] += 1
        f[1] += same
        f[2] += "refused" in cur.get(key, {})
        f[3] += len(cur.get(key, {}).get("taps", {}))
        if not same:
            different.append(f"DIFFERENT {key}\n  parent: {old.get(key)}\n  new   : {cur.get(key)}")
    for fam, (total, same, refused, taps) in families.items():
        print(f"{fam}: {total} cases, {same} identical, {total - same} different ({refused} refused, {taps} taps read)")
    print("\n".join(different) if different else "no mismatch")
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
