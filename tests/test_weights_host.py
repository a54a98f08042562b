"""Site weights, host side (no GPU): ``csrc/pf_weights_host.h`` behind ``pf_compress_sites`` / ``pf_boot_counts`` /
``pf_padded_sites``, their Python twins in ``phyloformer_amd/weights_sites.py``, and the premise of DESIGN.md section 16
on the reference's own arithmetic (the float64 oracle): the network does not know a site's position, so a repeated
column carries identical tokens and an alignment with repeated columns is a permutation away from its expansion."""
import os

import numpy as np
import pytest

from oracle import pf_oracle as O
from phyloformer_amd import weights_sites as ws
from phyloformer_amd.bootstrap import resample_sites

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- pinned literally ------------------------------------------------------------------------------------------------

def test_padded_sites_literals():
    cases = {(1, 1): 1, (1, 500): 32, (32, 500): 32, (33, 500): 64, (316, 500): 320, (481, 500): 500, (500, 500): 500,
             (20, 20): 20, (5, 31): 31, (64, 64): 64, (65, 96): 96, (65, 97): 96}
    for (K, L), want in cases.items():
        assert ws.padded_sites(K, L) == want == ws.native_padded_sites(K, L), (K, L)
    for K, L in [(0, 5), (6, 5), (-1, 5), (1, 0)]:
        with pytest.raises(ValueError):
            ws.padded_sites(K, L)
        with pytest.raises(ValueError):
            ws.native_padded_sites(K, L)


def test_compress_sites_literals():
    #               site 0  1  2  3  4  5  6
    idx = np.array([[0, 1, 0, 2, 1, 0, 2],
                    [3, 3, 3, 4, 3, 3, 5]], np.uint8)
    # columns: (0,3) (1,3) (0,3) (2,4) (1,3) (0,3) (2,5)
    for fn in (ws.compress_sites, ws.native_compress_sites):
        first, count = fn(idx)
        assert first.tolist() == [0, 1, 3, 6] and count.tolist() == [3, 2, 1, 1] and first.dtype == count.dtype == np.int32
        first, count = fn(np.array([[7, 7, 7, 7]], np.uint8))                 # all identical
        assert first.tolist() == [0] and count.tolist() == [4]
        first, count = fn(np.array([[1, 2, 3], [1, 1, 1]], np.uint8))         # no repeats
        assert first.tolist() == [0, 1, 2] and count.tolist() == [1, 1, 1]
        first, count = fn(np.array([[9], [4]], np.uint8))                     # L = 1
        assert first.tolist() == [0] and count.tolist() == [1]
    sites, w = ws.compressed_table(idx)
    assert sites.tolist() == [0, 1, 3, 6, 0, 0, 0] and w.tolist() == [3, 2, 1, 1, 0, 0, 0] and w.dtype == np.float32


def test_boot_counts_literals():
    # replicate 0 of seed 0 over 8 sites, by the stream's definition (pf_boot.hip.h), worked out here in Python ints
    M = (1 << 64) - 1

    def mix(z):
        z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 & M
        z ^= z >> 27; z = z * 0x94D049BB133111EB & M
        return z ^ (z >> 31)
    for L, seed, r in [(8, 0, 0), (5, 123, 2), (1, 9, 0)]:
        key = mix((seed + 0x9E3779B97F4A7C15) & M)
        draws = [((mix(key ^ ((r << 32) | l)) >> 32) * L) >> 32 for l in range(L)]
        want_sites = sorted(set(draws))
        want_counts = [draws.count(s) for s in want_sites]
        for fn in (ws.boot_counts, ws.native_boot_counts):
            sites, counts = fn(L, r + 1, seed, r)
            assert sites.tolist() == want_sites and counts.tolist() == want_counts, (L, seed, r)
    for fn in (ws.boot_counts, ws.native_boot_counts):
        for L, R, r in [(0, 1, 0), (5, 1, 1), (5, 1, -1), (5, 0, 0)]:
            with pytest.raises(ValueError):
                fn(L, R, 0, r)


# ---- native and Python twins on random cases -------------------------------------------------------------------------

def test_native_and_python_twins_agree():
    rng = np.random.default_rng(20260)
    shapes = [(3, 1), (2, 32), (4, 33), (3, 64), (5, 96), (2, 250)]
    ncases = 0
    for t in range(300):
        N, L = shapes[t % len(shapes)] if t % 2 else (int(rng.integers(1, 7)), int(rng.integers(1, 130)))
        kind = t % 5
        if kind == 0:
            idx = np.repeat(rng.integers(0, 22, (N, 1)), L, axis=1)                          # all-identical columns
        elif kind == 1:
            idx = np.stack([np.arange(L) % 22, np.arange(L) // 22 % 22] + [np.zeros(L, int)] * max(N - 2, 0))[:max(N, 2)]   # no repeats
        else:
            idx = rng.integers(0, int(rng.integers(1, 5)), (N, L))                           # many repeats
        idx = idx.astype(np.uint8)
        a, b = ws.compress_sites(idx), ws.native_compress_sites(idx)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        first, count = a
        assert count.sum() == idx.shape[1] and (np.diff(first) > 0).all() and first[0] == 0
        cols = [idx[:, l].tobytes() for l in range(idx.shape[1])]
        assert len(set(cols)) == len(first) and all(cols.count(cols[f]) == c for f, c in zip(first, count))
        if kind == 0:
            assert len(first) == 1
        if kind == 1:
            assert len(first) == idx.shape[1]
        L = idx.shape[1]
        R = int(rng.integers(1, 5)); r = int(rng.integers(0, R)); seed = int(rng.integers(0, 2 ** 63)) * 2 + t % 2
        p, q = ws.boot_counts(L, R, seed, r), ws.native_boot_counts(L, R, seed, r)
        assert np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1])
        assert ws.padded_sites(len(p[0]), L) == ws.native_padded_sites(len(p[0]), L)
        ncases += 1
    assert ncases == 300


@pytest.mark.parametrize("L,R,seed", [(1, 3, 0), (31, 4, 1), (32, 4, 2 ** 64 - 1), (100, 8, 5), (250, 8, 77), (500, 3, 12345)])
def test_expanded_boot_counts_are_the_sorted_replicate(L, R, seed):
    reps = resample_sites(L, R, seed)
    for r in range(R):
        sites, counts = ws.native_boot_counts(L, R, seed, r)
        assert (np.diff(sites) > 0).all() and (counts > 0).all()
        assert np.array_equal(np.repeat(sites, counts), np.sort(reps[r]))
    tab, w = ws.boot_tables(L, R, seed)
    K = ws.padded_sites(max(len(ws.boot_counts(L, R, seed, r)[0]) for r in range(R)), L)
    assert tab.shape == w.shape == (R, K) and (w.sum(axis=1) == L).all()
    assert ((w > 0) | (tab == 0)).all()                       # padding: site 0, weight 0


def test_expand_and_pad_table():
    idx = np.arange(12, dtype=np.uint8).reshape(2, 6)
    assert ws.expand(idx, [2, 0, 1, 0, 0, 3]).tolist() == [[0, 0, 2, 5, 5, 5], [6, 6, 8, 11, 11, 11]]
    with pytest.raises(ValueError):
        ws.expand(idx, [0.5, 1, 1, 1, 1, 1])
    with pytest.raises(ValueError):
        ws.pad_table([1, 2, 3], [1, 1, 1], 2)


# ---- the premise, on the reference's arithmetic (float64 oracle, no GPU) ---------------------------------------------

@pytest.fixture(scope="module")
def tips(weights):
    from phyloformer_amd.fasta import load_alignment
    idx = load_alignment(os.path.join(REPO, "data", "testdata", "msas", "0_20_tips.fa"))[0]
    w = weights("pf")
    return w, np.ascontiguousarray(idx)


def _oracle(w, idx, tap=None):
    return O.forward(w.tensors, idx, n_blocks=w.n_blocks, n_heads=w.n_heads, dtype=np.float64, tap=tap)


def test_oracle_does_not_know_a_sites_position(tips):
    """Columns repeated in place against the same multiset of columns in another order: equal to float64 rounding."""
    w, idx = tips
    rng = np.random.default_rng(4)
    counts = rng.integers(0, 3, idx.shape[1]); counts[0] = 2; counts[1] = 0
    rep = ws.expand(idx, counts)                               # site l repeated counts[l] times, in order
    perm = rng.permutation(rep.shape[1])
    a, b = _oracle(w, rep), _oracle(w, rep[:, perm])
    diff = float(np.abs(a - b).max())
    print(f"oracle, {rep.shape[0]} x {rep.shape[1]}: repeated in place vs permuted, max |diff| {diff:.3e} (distances up to {a.max():.3f})")
    assert diff <= 64 * np.finfo(np.float64).eps * max(1.0, float(a.max()))


def test_oracle_gives_duplicated_sites_equal_logits(tips):
    """A constant column appended twice: the per-site logits of the two copies are equal."""
    w, idx = tips
    const = np.full((idx.shape[0], 1), 3, np.uint8)
    both = np.concatenate([idx[:, :20], const, idx[:, 20:], const], axis=1)
    taps = {}
    _oracle(w, both, tap=lambda k, v: taps.__setitem__(k, np.array(v)))
    logits = taps["logits"]                                    # [P][L]
    diff = float(np.abs(logits[:, 20] - logits[:, -1]).max())
    print(f"oracle: logits of the two copies of a constant column differ by {diff:.3e} (|logit| up to {np.abs(logits).max():.2f})")
    assert diff <= 64 * np.finfo(np.float64).eps * max(1.0, float(np.abs(logits).max()))


# ---- infer_alns.py --compress-sites through the oracle engine (no GPU) -----------------------------------------------

@pytest.fixture(scope="module")
def repeated_alns():
    """Three small alignments whose columns repeat: 20 and 36 distinct columns among 40 sites (padded tables of 32 and
    of L = 40 entries in ONE shape bucket) and 12 among 33."""
    from phyloformer_amd.msa_sim import simulate_batch
    rng = np.random.default_rng(16)
    out, padded = {}, {}
    for stem, (n, sites, distinct, seed) in {"r0": (6, 40, 20, 161), "r1": (6, 40, 36, 175), "r2": (8, 33, 12, 163)}.items():
        cols = simulate_batch(1, n, distinct, seed=seed)[0]
        pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, sites - distinct)])
        out[stem] = np.ascontiguousarray(cols[:, rng.permutation(pick)])
        padded[stem] = ws.padded_sites(len(ws.compress_sites(out[stem])[0]), sites)
    assert padded == {"r0": 32, "r1": 40, "r2": 32}
    return out


def _cli(args, tmp_path):
    import subprocess
    import sys
    env = dict(os.environ, PF_CLI_ENGINE_FACTORY="helpers.oracle_weights_engine:make", TMPDIR=str(tmp_path))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "tests"), REPO, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(REPO, "infer_alns.py"), os.path.join(REPO, "models", "pf.ckpt"),
                           *args], capture_output=True, text=True, cwd=REPO, env=env, timeout=900)


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def _upper(data, N):
    m = np.array([[float(v) for v in row.split()[-N:]] for row in data.decode().splitlines()[1:]])
    return m[np.triu_indices(N, k=1)]


def test_cli_compress_sites_files(repeated_alns, tmp_path, weights):
    """``--compress-sites`` writes the files of a plain run; native and Python I/O agree byte for byte; the distances
    are the plain run's to the oracle's own float32 rounding.  The bound: the compressed run forwards the columns in
    another order (distinct columns in order of first occurrence, each repeated by its count), which the float64 oracle
    does not notice beyond 64 eps (test_oracle_does_not_know_a_sites_position), so the two float32 results differ by no
    more than their own distances to the float64 oracle, plus the two files' 10 decimals."""
    from phyloformer_amd.msa_sim import to_fasta
    src = tmp_path / "in"
    src.mkdir()
    for stem, a in repeated_alns.items():
        (src / f"{stem}.fa").write_text(to_fasta(a))
    plain = _cli([str(src), "-o", str(tmp_path / "plain"), "-t"], tmp_path)
    comp = _cli([str(src), "-o", str(tmp_path / "comp"), "-t", "--compress-sites"], tmp_path)
    assert plain.returncode == 0 and comp.returncode == 0, plain.stderr[-2000:] + comp.stderr[-3000:]
    base, files = _files(tmp_path / "plain"), _files(tmp_path / "comp")
    assert set(files) == set(base) == {f"{s}.{x}" for s in repeated_alns for x in ("phy", "nj.nwk")}
    w = weights("pf").tensors
    for stem, a in repeated_alns.items():
        first, count = ws.compress_sites(a)
        c = ws.expand(a[:, first], count)                  # what the compressed forward stands for
        assert c.shape == a.shape
        a32, a64, c32, c64 = (O.forward(w, x, dtype=dt) for x in (a, c) for dt in (np.float32, np.float64))
        bound = (float(np.abs(a32 - a64).max()) + float(np.abs(c32 - c64).max())
                 + 64 * np.finfo(np.float64).eps * max(1.0, float(a64.max())) + 1e-10)
        diff = float(np.abs(_upper(files[f"{stem}.phy"], len(a)) - _upper(base[f"{stem}.phy"], len(a))).max())
        print(f"{stem}: --compress-sites vs plain {diff:.3e}, the oracle's float32 rounding allows {bound:.3e}")
        assert diff <= bound, (stem, diff, bound)
    p = _cli([str(src), "-o", str(tmp_path / "pyio"), "-t", "--compress-sites", "--python-io"], tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _files(tmp_path / "pyio") == files
    # with --bootstrap the alignment itself is forwarded as without the flag; one support tree per input
    b = _cli([str(src), "-o", str(tmp_path / "boot"), "--bootstrap", "4", "--compress-sites"], tmp_path)
    assert b.returncode == 0, b.stderr[-3000:]
    boot = _files(tmp_path / "boot")
    assert set(boot) == {f"{s}.{x}" for s in repeated_alns for x in ("phy", "sup.nwk")}
    for stem in repeated_alns:
        assert boot[f"{stem}.phy"] == base[f"{stem}.phy"], stem
        assert boot[f"{stem}.sup.nwk"].strip().endswith(b";")
