"""ctypes binding of ``libphyloformer_amd.so`` (C ABI in ``include/phyloformer_amd.h``).

This is the only way the Python host code reaches the device: plain pointers
and sizes, no torch op dispatch.  If the shared library is missing or no
gfx950 device is present the calls raise — there is deliberately no CPU
fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import numpy as np

from . import cabi
from .treearrays import (JOINS, REFINE, consensus_arrays, consensus_outputs, distance_arrays, distance_outputs, ptr, support_arrays, support_outputs, transfer_outputs,
                         tree_call, unbatched)
from .weights import ModelWeights

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libphyloformer_amd.so")
ABI_VERSION = cabi.CONSTANTS["PF_ABI_VERSION"]          # of the include/phyloformer_amd.h this tree holds
UNIQUE_ID_BYTES = cabi.CONSTANTS["PF_UNIQUE_ID_BYTES"]  # two ncclUniqueIds, one per communicator / stream

PF_OK, PF_EINVAL, PF_EHIP, PF_ERCCL, PF_ENOMEM, PF_ESTATE = (
    cabi.CONSTANTS[k] for k in ("PF_OK", "PF_EINVAL", "PF_EHIP", "PF_ERCCL", "PF_ENOMEM", "PF_ESTATE"))


def _refuse_single_sequence(B: int, N: int):
    """One sequence = no pair: the reference's forward raises RuntimeError there (attention.py:193 cannot view the empty
    tensor; pinned by tests/golden/cli_bad_entry.json), the C ABI answers PF_EINVAL for any N < 2 - the host mirror
    raises what the reference raises."""
    if N == 1 and B >= 1:
        raise RuntimeError(f"cannot reshape tensor of 0 elements into shape [{B}, -1, 0, 64] because the unspecified "
                           "dimension size -1 can be any value and is ambiguous")


class EngineError(RuntimeError):
    """A HIP / RCCL / allocation failure reported by the native library."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"[pf status {code}] {msg}")
        self.code = code


class pf_weights_t(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_heads", C.c_int32), ("embed_dim", C.c_int32),
                ("n_alphabet", C.c_int32), ("blob", C.POINTER(C.c_float)), ("blob_len", C.c_uint64)]


# name -> (restype, argtypes) of every symbol declared in include/phyloformer_amd.h, and the additions to ABI 5 that a
# library built before them lacks (the header's banners say which): bound when present; a call through a missing one
# raises EngineError at call time (loading such a library stays possible).  Both are read from the header (cabi.py).
_H = C.c_void_p
SIGNATURES = {name: (p.restype, p.argtypes) for name, p in cabi.PROTOTYPES.items()}
CALL_TIME_SYMBOLS = frozenset(name for name, p in cabi.PROTOTYPES.items() if p.call_time)

_lib: Optional[C.CDLL] = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen the native library and attach the prototypes.  Raises if it is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("PHYLOFORMER_AMD_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise EngineError(PF_EHIP, f"native library not found at {p}; run "
                          "`python -m phyloformer_amd.build` (there is no CPU fallback)")
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        if name in CALL_TIME_SYMBOLS and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.pf_abi_version() != ABI_VERSION:
        raise EngineError(PF_ESTATE, f"{p} has ABI version {lib.pf_abi_version()}, this binding expects "
                          f"{ABI_VERSION}; rebuild with `python -m phyloformer_amd.build --force`")
    if path is None:
        _lib = lib
    return lib


def symbol(lib, name: str):
    """The function ``name`` of a loaded library.  One it lacks (of a library that loaded, only a ``CALL_TIME_SYMBOLS``
    one can be missing) raises here, when it is called."""
    fn = getattr(lib, name, None)
    if fn is None:
        raise EngineError(PF_ESTATE, f"the loaded native library does not export {name} (it was built before that "
                          "entry point was added); rebuild with `python -m phyloformer_amd.build --force`")
    return fn


def build_info(path: Optional[str] = None) -> Dict[str, object]:
    """What the loaded library was built from (``pf_build_info``, ABI 4): compiler, flags, the scheduling
    strategy that really compiled the kernels, source and kernel hashes.  Needs no device."""
    import json
    return json.loads(load_library(path).pf_build_info().decode())


class Engine:
    """One handle = one GPU + one stream + one set of prepared weights."""

    def __init__(self, weights: ModelWeights, device: int = 0):
        self._lib = load_library()
        self._h = _H()
        blob = weights.blob()
        expect = self._optional("pf_blob_len")(weights.n_blocks, weights.n_heads, weights.embed_dim)
        if blob.size != expect:
            raise ValueError(f"weight blob has {blob.size} floats, library expects {expect}")
        w = pf_weights_t(weights.n_blocks, weights.n_heads, weights.embed_dim, 22,
                         blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size)
        rc = self._optional("pf_create")(C.byref(w), device, C.byref(self._h))
        if rc != PF_OK:
            msg = (self._optional("pf_last_error")(None) or b"").decode()
            self._h = _H()
            if rc == PF_EINVAL:
                raise ValueError(msg)
            raise EngineError(rc, msg)
        self.device = device
        self.world = 1
        self.rank = 0
        self._arch = (int(weights.n_blocks), int(weights.n_heads), int(weights.embed_dim))

    @property
    def architecture(self) -> Tuple[int, int, int]:
        """``(n_blocks, n_heads, embed_dim)`` of the weights this handle was created with.  Anything but
        ``(n, 4, 64)`` runs on the generic float64 kernels (option "generic" in include/phyloformer_amd.h)."""
        return self._arch

    # -- plumbing ---------------------------------------------------------------------------
    def _optional(self, name: str):
        """The one way every method reaches a function of the library (``symbol``)."""
        return symbol(self._lib, name)

    def _check(self, rc: int):
        if rc >= 0:
            return rc
        msg = (self._optional("pf_last_error")(self._h) or b"").decode()
        if rc == PF_EINVAL:
            raise ValueError(msg)   # the reference raises ValueError for N > 200 (model.py:24-28)
        raise EngineError(rc, msg)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._optional("pf_destroy")(self._h)
            self._h = _H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, key: str, value: int):
        self._check(self._optional("pf_set_option")(self._h, key.encode(), int(value)))

    def device_info(self) -> Dict[str, object]:
        name = C.create_string_buffer(256)
        cu = C.c_int32()
        mem = C.c_uint64()
        self._check(self._optional("pf_device_info")(self._h, name, 256, C.byref(cu), C.byref(mem)))
        return {"name": name.value.decode(), "cu_count": cu.value, "hbm_bytes": mem.value}

    def build_info(self) -> Dict[str, object]:
        """What the library behind this engine was built from (``pf_build_info``)."""
        import json
        return json.loads(self._optional("pf_build_info")().decode())

    def device_pci(self) -> Tuple[int, int, int]:
        """(domain, bus, device) of this engine's GPU - the key rocm_smi finds it by (phyloformer_amd/smi.py)."""
        d, b, v = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._optional("pf_device_pci")(self._h, C.byref(d), C.byref(b), C.byref(v)))
        return d.value, b.value, v.value

    # -- forward ----------------------------------------------------------------------------
    @staticmethod
    def _sources(idx: np.ndarray, refuse_single: bool = True):
        """``uint8[B, N, L]`` (or ``[N, L]``) as contiguous ``[B, N, L]`` bytes, and whether to drop ``B`` again."""
        idx = np.ascontiguousarray(idx, dtype=np.uint8)
        single = idx.ndim == 2
        if single:
            idx = idx[None]
        if idx.ndim != 3:
            raise ValueError(f"idx must be [B, N, L] or [N, L], got shape {idx.shape}")
        if refuse_single:
            _refuse_single_sequence(idx.shape[0], idx.shape[1])
        return idx, single

    @staticmethod
    def _table(tab, what: str, entry: str, bound: int) -> np.ndarray:
        """An integer table (``what``: its name and shape) as contiguous int32; an ``entry`` that int32 cannot hold is
        outside ``[0, bound)`` before the library sees it."""
        tab = np.asarray(tab)
        if tab.ndim != 2 or tab.dtype.kind not in "iu":
            raise ValueError(f"{what}, got {tab.dtype} {tab.shape}")
        if tab.size and (tab.min() < -2 ** 31 or tab.max() >= 2 ** 31):
            raise ValueError(f"{entry} {int(tab.max() if tab.max() >= 2 ** 31 else tab.min())} is outside [0, {bound})")
        return np.ascontiguousarray(tab, dtype=np.int32)

    @staticmethod
    def _seed(seed: int) -> int:
        """Any Python int as the ``uint64_t`` seed of the replicate stream."""
        return int(seed) & 0xFFFFFFFFFFFFFFFF

    def forward(self, idx: np.ndarray) -> np.ndarray:
        """``uint8[B, N, L]`` (or ``[N, L]``) → ``float32[B, P]`` (or ``[P]``)."""
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        out = np.empty((B, N * (N - 1) // 2), dtype=np.float32)
        self._check(self._optional("pf_forward")(self._h, idx.ctypes.data, B, N, L, out.ctypes.data))
        return out[0] if single else out

    def bootstrap(self, idx: np.ndarray, replicates: int, seed: int = 0) -> np.ndarray:
        """Distances of ``replicates`` site-bootstrap replicates (``pf_bootstrap``): ``uint8[B, N, L]`` →
        ``float32[B, R, P]`` (``[N, L]`` → ``[R, P]``).  Replicate ``r`` of an alignment is
        ``idx[..., bootstrap.resample_sites(L, R, seed)[r]]``; its distances are ``forward`` of those bytes, bit for bit."""
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        R = int(replicates)
        out = np.empty((B, max(R, 0), N * (N - 1) // 2), dtype=np.float32)
        self._check(self._optional("pf_bootstrap")(self._h, idx.ctypes.data, B, N, L, R, self._seed(seed),
                                                   out.ctypes.data if out.size else None))
        return out[0] if single else out

    def resample_sites_device(self, d_src: int, B: int, N: int, L: int, r_begin: int, R: int, seed: int, d_dst: int):
        """``pf_resample_sites_device``: replicates ``r_begin .. r_begin + R - 1`` of ``d_src [B][N][L]`` into
        ``d_dst [B][R][N][L]`` (device buffers, asynchronous on the handle's stream)."""
        self._check(self._optional("pf_resample_sites_device")(self._h, d_src, B, N, L, r_begin, R, self._seed(seed), d_dst))

    def forward_sites(self, idx: np.ndarray, sites: np.ndarray) -> np.ndarray:
        """Distances of the alignments cut out of ``idx`` by a site table (``pf_forward_sites``): ``uint8[B, N, L]``,
        ``int[S, K]`` → ``float32[B, S, P]`` (``[N, L]`` → ``[S, P]``).  ``out[b, s]`` is ``forward`` of
        ``idx[b][:, sites[s]]`` (``windows.cut_sites``), bit for bit; entries outside ``[0, L)`` raise ``ValueError``."""
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        tab = self._table(sites, "sites must be an integer array [S, K]", "site", L)
        S, K = tab.shape
        out = np.empty((B, S, N * (N - 1) // 2), dtype=np.float32)
        self._check(self._optional("pf_forward_sites")(self._h, idx.ctypes.data, B, N, L, tab.ctypes.data if tab.size else None,
                                                       S, K, out.ctypes.data if out.size else None))
        return out[0] if single else out

    def forward_windows(self, idx: np.ndarray, W: int, step: "int | None" = None) -> np.ndarray:
        """Distances of every window of ``W`` sites, ``step`` apart (default ``W``: non-overlapping), of ``idx``
        (``pf_forward_windows``): ``uint8[B, N, L]`` → ``float32[B, S, P]`` (``[N, L]`` → ``[S, P]``), window ``s``
        starting at ``windows.window_starts(L, W, step)[s]``; bit for bit ``forward`` of the host-cut window."""
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        W, step = int(W), int(W if step is None else step)
        S = max(0, self._optional("pf_window_count")(L, W, step))
        out = np.empty((B, S, N * (N - 1) // 2), dtype=np.float32)
        self._check(self._optional("pf_forward_windows")(self._h, idx.ctypes.data, B, N, L, W, step,
                                                         out.ctypes.data if out.size else None, S))
        return out[0] if single else out

    # -- site-resolved distances ------------------------------------------------------------
    def forward_site_map(self, idx: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """Distances and their decomposition over sites (``pf_forward_site_map``): ``uint8[B, N, L]`` →
        ``(float32[B, P], float32[B, P, L])`` (``[N, L]`` → ``([P], [P, L])``).  ``map[b, p, l]`` is the softplus of the
        head's logit of pair ``p`` at site ``l``; ``dist[b, p]``, their mean over ``l``, is ``forward``'s, bit for bit."""
        fn = self._optional("pf_forward_site_map")
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        P = N * (N - 1) // 2
        out = np.empty((B, P), dtype=np.float32)
        smap = np.empty((B, P, L), dtype=np.float32)
        self._check(fn(self._h, idx.ctypes.data, B, N, L, out.ctypes.data, smap.ctypes.data if smap.size else None))
        return (out[0], smap[0]) if single else (out, smap)

    def forward_site_profile(self, idx: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Distances, their standard errors over sites and the site profile (``pf_forward_site_profile``):
        ``uint8[B, N, L]`` → ``(dist float32[B, P], se float32[B, P], profile float32[B, L])``: the moments
        (``siteprofile.site_moments``) of ``forward_site_map``'s map, reduced on the GPU."""
        fn = self._optional("pf_forward_site_profile")
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        P = N * (N - 1) // 2
        out = np.empty((B, P), dtype=np.float32)
        se = np.empty((B, P), dtype=np.float32)
        prof = np.empty((B, L), dtype=np.float32)
        self._check(fn(self._h, idx.ctypes.data, B, N, L, out.ctypes.data, se.ctypes.data,
                       prof.ctypes.data if prof.size else None))
        return (out[0], se[0], prof[0]) if single else (out, se, prof)

    # -- the taxon axis ---------------------------------------------------------------------
    def forward_taxa(self, idx: np.ndarray, taxa: np.ndarray) -> np.ndarray:
        """Distances of the alignments cut out of ``idx`` by a taxon table (``pf_forward_taxa``): ``uint8[B, N, L]``,
        ``int[S, M]`` → ``float32[B, S, M (M - 1) / 2]`` (``[N, L]`` → ``[S, ...]``).  ``out[b, s]`` is ``forward`` of
        ``idx[b][taxa[s], :]`` (``taxa.cut_taxa``), bit for bit; entries outside ``[0, N)`` raise ``ValueError``."""
        fn = self._optional("pf_forward_taxa")
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        tab = self._table(taxa, "taxa must be an integer array [S, M]", "taxon", N)
        S, M = tab.shape
        out = np.empty((B, S, max(M, 0) * max(M - 1, 0) // 2), dtype=np.float32)
        self._check(fn(self._h, idx.ctypes.data, B, N, L, tab.ctypes.data if tab.size else None, S, M,
                       out.ctypes.data if out.size else None))
        return out[0] if single else out

    def forward_leave_one_out(self, idx: np.ndarray, keep_loo: bool = False):
        """Leave-one-out taxon influence (``pf_forward_leave_one_out``): ``uint8[B, N, L]``, ``N >= 3`` →
        ``(dist float32[B, P], influence float32[B, N], shift float32[B, N], context float32[B, P])``, with
        ``keep_loo`` a fifth array ``loo float32[B, N, P1]`` (``[N, L]`` drops ``B`` everywhere).  ``dist`` is
        ``forward``'s, ``loo[b, t]`` is ``forward_taxa`` of ``taxa.leave_one_out_sets(N)[t]``, both bit for bit; the
        statistics are ``taxa.loo_stats(dist, loo)``, reduced on the GPU."""
        fn = self._optional("pf_forward_leave_one_out")
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        P, P1 = N * (N - 1) // 2, max(N - 1, 0) * max(N - 2, 0) // 2
        out = np.empty((B, P), dtype=np.float32)
        loo = np.empty((B, N, P1), dtype=np.float32) if keep_loo else None
        infl = np.empty((B, N), dtype=np.float32)
        shift = np.empty((B, N), dtype=np.float32)
        ctx = np.empty((B, P), dtype=np.float32)
        self._check(fn(self._h, idx.ctypes.data, B, N, L, out.ctypes.data, loo.ctypes.data if keep_loo and loo.size else None,
                       infl.ctypes.data, shift.ctypes.data, ctx.ctypes.data))
        res = (out, infl, shift, ctx) + ((loo,) if keep_loo else ())
        return tuple(r[0] for r in res) if single else res

    # -- query placement --------------------------------------------------------------------
    def forward_place(self, idx: np.ndarray, queries: int, keep_sets: bool = False):
        """Query placement (``pf_forward_place``): ``uint8[B, M, L]`` whose last ``queries`` rows are the queries, the
        first ``N = M - queries >= 2`` the backbone → ``(dist float32[B, P_M], base float32[B, P_N], place
        float32[B, Q, N], disturb float32[B, Q], shift float32[B, Q], joint float32[B, Q])``, with ``keep_sets`` a
        seventh array ``sets float32[B, Q, P_{N+1}]`` (``[M, L]`` drops ``B`` everywhere).  ``dist`` is ``forward``'s,
        ``base`` is ``forward(idx[:, :N])``, ``sets[b, q]`` is ``forward(place.join_query(idx[b], N, q))``, all bit for
        bit; the rest is ``place.place_stats(dist, base, sets, N, Q)``, reduced on the GPU."""
        fn = self._optional("pf_forward_place")
        idx, single = self._sources(idx)
        B, M, L = idx.shape
        Q = int(queries)
        N = M - Q
        ok = Q >= 1 and N >= 2                                    # (otherwise the library refuses; nothing is read)
        pairs = lambda n: n * (n - 1) // 2
        out = np.empty((B, pairs(M)), dtype=np.float32)
        base = np.empty((B, pairs(N) if ok else 1), dtype=np.float32)
        sets = np.empty((B, Q, pairs(N + 1)), dtype=np.float32) if keep_sets and ok else None
        place = np.empty((B, Q, N) if ok else (B, 1, 1), dtype=np.float32)
        dis, sh, jt = (np.empty((B, Q if ok else 1), dtype=np.float32) for _ in range(3))
        self._check(fn(self._h, idx.ctypes.data, B, M, L, Q, out.ctypes.data, base.ctypes.data,
                       sets.ctypes.data if sets is not None else None, place.ctypes.data, dis.ctypes.data, sh.ctypes.data,
                       jt.ctypes.data))
        res = (out, base, place, dis, sh, jt) + ((sets,) if keep_sets else ())
        return tuple(r[0] for r in res) if single else res

    # -- tiled inference -------------------------------------------------------------------
    def forward_tiled(self, idx: np.ndarray, M: int) -> Tuple[np.ndarray, np.ndarray]:
        """Tiled inference (``pf_forward_tiled``): ``uint8[B, N, L]`` with ``N > M >= 2`` → ``(out float32[B, P_N],
        spread float32[B, P_N])`` (``[N, L]`` drops ``B``): the sets of ``tile.plan(N, M)`` are cut and forwarded on the
        GPU, each on the path of its own shape, and combined there; bit for bit ``tile.combine`` of ``forward_taxa`` of
        every set.  The sequence cap applies to ``M``, not to ``N``; ``N <= M`` raises ``ValueError`` (use ``forward``)."""
        fn = self._optional("pf_forward_tiled")
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        out = np.empty((B, N * (N - 1) // 2), dtype=np.float32)
        spread = np.empty_like(out)
        self._check(fn(self._h, idx.ctypes.data, B, N, L, int(M), out.ctypes.data, spread.ctypes.data))
        return (out[0], spread[0]) if single else (out, spread)

    # -- neighbour joining -------------------------------------------------------------------
    def nj_joins(self, preds: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Neighbour joining on the GPU (``pf_nj_joins``): distances ``float32[B, P_N]`` → ``(slots int32[B, T], lengths
        float64[B, T], nonfinite bool[B])``, ``T = 2 (N - 3) + 3`` (``[P_N]`` drops ``B``): the joins ``a, b`` / ``la, lb``
        of ``nj.nj_joins`` on the symmetric matrix of every source, then the trifurcation ``i, j, k`` / ``li, lj, lk`` - bit
        for bit.  A source with a NaN or an infinity is flagged and its table unspecified (use ``hostio.nj_newick``)."""
        return self._joins("pf_nj_joins", preds)

    @staticmethod
    def _refuse_distances(p, st, N, T):
        """What the device forms refuse themselves (``treearrays.tree_call``); two sequences go to the library."""
        if p.ndim != 2:
            raise ValueError(f"expected distances [B, P] or [P], got {p.shape}")
        if N < 2:
            raise ValueError(f"{p.shape[1]} distances are not the pairs of any number of sequences")
        if st is not None and st.shape != (p.shape[0], T):
            raise ValueError(f"expected start tables {[p.shape[0], T]}, got {list(st.shape)}")

    def _joins(self, symbol: str, preds: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        fn = self._optional(symbol)
        p, _, (B, N, _T), single, out = tree_call(preds, JOINS, self._refuse_distances, single_ok=True)
        self._check(fn(self._h, ptr(p), B, N, *map(ptr, out)))
        return unbatched((out[0], out[1], out[2].astype(bool)), single)

    # -- BIONJ ------------------------------------------------------------------------------
    def bionj_joins(self, preds: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """BIONJ on the GPU (``pf_bionj_joins``): arguments and results as ``nj_joins``'; the table is that of
        ``bionj.bionj_joins`` on the symmetric matrix of every source - FastME's default start tree - bit for bit that of
        ``hostio.bionj_joins_host``, and a start table for ``bme_nni`` / ``bme_spr``.  A source with a NaN or an infinity
        is flagged and its table unspecified (use ``hostio.bionj_newick``)."""
        return self._joins("pf_bionj_joins", preds)

    # -- delta scores -----------------------------------------------------------------------
    def delta(self, preds: np.ndarray, bins: int = 20) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Delta scores on the GPU (``pf_delta``): distances ``float32[B, P_N]`` → ``(pair_sum int64[B, P_N], hist
        int64[B, bins], nonfinite uint8[B])`` (``[P_N]`` drops ``B``), ``4 <= N <= 2,048``: for every pair the sum of ``q =
        rint(delta 2^30)`` over the quartets that hold it, and the quartets per bin of ``q`` - bit for bit
        ``delta.delta_py`` of every source and ``hostio.delta_host``; ``delta.delta_scores`` derives the means.  A source
        with a NaN or an infinity is flagged and its arrays are zeros.  ``ValueError`` for what the library refuses."""
        from .delta import delta_arrays
        fn = self._optional("pf_delta")
        p, (B, N), single, out = delta_arrays(preds, bins)
        self._check(fn(self._h, ptr(p), B, N, int(bins), *map(ptr, out)))
        return unbatched(out, single)

    # -- tree fit ----------------------------------------------------------------------------
    def tree_fit(self, preds: np.ndarray, slots: np.ndarray, lengths: np.ndarray, patristic: bool = True):
        """Tree fit on the GPU (``pf_tree_fit``): distances ``float32[B, P_N]`` and join tables ``int32 / float64 [B, M, T]``
        (``[B, T]``: one tree per source, the results drop ``M``; ``[P_N]`` with ``[M, T]`` or ``[T]`` drops ``B``), ``3 <= N <=
        8,192`` → ``(patristic float64[B, M, P_N], rows float64[B, M, N, 6], worst_j int32[B, M, N], status uint8[B, M])`` - bit
        for bit ``fit.tree_fit_py`` of every tree and ``hostio.tree_fit_host``; ``fit.fit_scores`` derives what is reported.
        ``patristic`` = False: None in its place, the tree's distances stay on the device.  A tree with a status (1: not
        finite, 2: no join table) has zeros.  ``ValueError`` for what the library refuses."""
        from .fit import fit_arrays, squeezed
        fn = self._optional("pf_tree_fit")
        p, s, l, (B, M, N), flags, out = fit_arrays(preds, slots, lengths, patristic)
        self._check(fn(self._h, ptr(p), ptr(s), ptr(l), B, M, N, *map(ptr, out)))
        return squeezed(out, flags)

    # -- least-squares branch lengths ---------------------------------------------------------
    def tree_ols(self, preds: np.ndarray, slots: np.ndarray):
        """Least-squares branch lengths on the GPU (``pf_tree_ols``): distances ``float32[B, P_N]`` and the slots of join tables
        ``int32[B, M, T]`` (``[B, T]``: one tree per source, the results drop ``M``; ``[P_N]`` with ``[M, T]`` or ``[T]`` drops ``B``), ``3
        <= N <= 8,192`` → ``(ols float64[B, M, T], status uint8[B, M])``: the lengths that fit the distances best on each
        table's topology, in the positions of its own lengths, unclamped - bit for bit ``ols.tree_ols_py`` of every tree and
        ``hostio.tree_ols_host``; ``ols.ols_scores`` derives what is reported.  A tree with a status (1: not finite, 2: no join
        table) has zeros.  ``ValueError`` for what the library refuses."""
        from .ols import ols_arrays, squeezed
        fn = self._optional("pf_tree_ols")
        p, s, (B, M, N), flags, out = ols_arrays(preds, slots)
        self._check(fn(self._h, ptr(p), ptr(s), B, M, N, *map(ptr, out)))
        return squeezed(out, flags)

    # -- tree rooting -------------------------------------------------------------------------
    def tree_root(self, slots: np.ndarray, lengths: np.ndarray):
        """MAD and midpoint rooting on the GPU (``pf_tree_root``): join tables ``slots int32`` / ``lengths float64 [B, M, T]`` (``[B, T]``:
        one tree per source, the results drop ``M``; ``[T]`` drops ``B`` too), ``3 <= N <= 8,192`` → ``(ssq float64[B, M, T], pos
        float64[B, M, T], mid float64[B, M, 5], status uint8[B, M])``: per branch the sum of squared ancestor deviations at its best
        root position and that position above the branch's lower node, and the midpoint ``(entry, position, b, c, diameter)`` -
        bit for bit ``root.tree_root_py`` of every tree and ``hostio.tree_root_host``; ``root.root_scores`` derives what is
        reported.  A tree with a status (1: not finite, 2: no join table) has zeros.  ``ValueError`` for what the library
        refuses."""
        from .root import root_arrays, squeezed
        fn = self._optional("pf_tree_root")
        s, l, (B, M, N), flags, out = root_arrays(slots, lengths)
        self._check(fn(self._h, ptr(s), ptr(l), B, M, N, *map(ptr, out)))
        return squeezed(out, flags)

    # -- balanced NNI refinement -------------------------------------------------------------
    def bme_nni(self, preds: np.ndarray, start_slots: np.ndarray):
        """Balanced minimum-evolution NNI refinement on the GPU (``pf_bme_nni``): distances ``float32[B, P_N]`` and start
        join tables ``int32[B, T]`` (``Engine.nj_joins``' slots, or any valid join table) → ``(slots int32[B, T], lengths
        float64[B, T], steps int32[B], tree_length float64[B], status uint8[B])`` (``[P_N]`` / ``[T]`` drop ``B``): the
        tree of ``bme.bme_nni`` - a local optimum of the balanced tree length - as a join table with balanced branch
        lengths, bit for bit that of ``hostio.bme_nni_host``.  ``status`` 0 = ok, 1 = a NaN or an infinity in the source
        (its results are zeros: use ``hostio.bme_newick``), 2 = stopped at the cap of ``16 N`` moves."""
        return self._refine("pf_bme_nni", preds, start_slots)

    def _refine(self, symbol: str, preds: np.ndarray, start_slots: np.ndarray):
        fn = self._optional(symbol)
        p, st, (B, N, _T), single, out = tree_call(preds, REFINE, self._refuse_distances, start_slots, single_ok=True)
        self._check(fn(self._h, ptr(p), ptr(st), B, N, *map(ptr, out)))
        return unbatched(out, single)

    # -- balanced SPR refinement -------------------------------------------------------------
    def bme_spr(self, preds: np.ndarray, start_slots: np.ndarray):
        """Balanced subtree pruning and regrafting on the GPU (``pf_bme_spr``): arguments and results as ``bme_nni``'s; the
        tree is that of ``bme.bme_spr``, bit for bit that of ``hostio.bme_spr_host``.  ``status`` 1: use
        ``hostio.spr_newick`` for that source."""
        return self._refine("pf_bme_spr", preds, start_slots)

    # -- split supports of join tables -------------------------------------------------------
    def join_supports(self, ref_slots: np.ndarray, rep_slots: np.ndarray, rep_flag: Optional[np.ndarray] = None):
        """Split supports on the GPU (``pf_join_supports``): reference join tables ``int32[B, T]`` and replicate join tables
        ``int32[B, R, T]`` (``[T]`` / ``[R, T]`` drop ``B``), ``rep_flag bool[B, R]`` or None → ``(count int32[B, N - 3],
        transfer int64[B, N - 3], depth int32[B, N - 3], status uint8[B])``: per split of the reference the replicates that
        contain it, the sum of its transfer distances and its depth - ``supports.split_supports``, the same integers as
        ``hostio.join_supports_host``.  ``ValueError``-like refusals come as ``EngineError`` (a table that is no join
        table, ``N < 4``)."""
        fn = self._optional("pf_join_supports")
        ref, rep, flag, (B, R, N), single = support_arrays(ref_slots, rep_slots, rep_flag)
        out, ptrs = support_outputs(B, N)
        self._check(fn(self._h, ref.ctypes.data, rep.ctypes.data, ptr(flag), B, R, N, *ptrs))
        return unbatched(out, single)

    # -- per-taxon transfer counts ------------------------------------------------------------
    def join_transfers(self, ref_slots: np.ndarray, rep_slots: np.ndarray, rep_flag: Optional[np.ndarray] = None, cutoff: int = 100,
                       branch_moves: bool = True):
        """Per-taxon transfer counts on the GPU (``pf_join_transfers``): ``join_supports``' arguments and the cutoff in
        percent (0 .. 100) → ``(count, transfer, depth, moves int64[B, N], used int32[B, N - 3], capped int32[B, N - 3],
        branch_moves int32[B, N - 3, N] or None, status uint8[B])`` - ``supports.transfer_taxa``, the same integers as
        ``hostio.join_transfers_host``; the first three are ``join_supports``'.  Refusals as ``join_supports``."""
        fn = self._optional("pf_join_transfers")
        ref, rep, flag, (B, R, N), single = support_arrays(ref_slots, rep_slots, rep_flag)
        out, ptrs = transfer_outputs(B, N, branch_moves)
        self._check(fn(self._h, ref.ctypes.data, rep.ctypes.data, ptr(flag), B, R, N, int(cutoff), *ptrs))
        return unbatched(out, single)

    # -- majority-rule consensus of replicate join tables -----------------------------------
    def join_consensus(self, rep_slots: np.ndarray, rep_lengths: Optional[np.ndarray] = None,
                       rep_flag: Optional[np.ndarray] = None, percent: int = 50):
        """Majority-rule consensus on the GPU (``pf_join_consensus``): replicate join tables ``int32[B, R, T]``, their
        lengths ``float64[B, R, T]`` or None, ``rep_flag bool[B, R]`` or None (``[R, T]`` / ``[R]`` drop ``B``) and the
        threshold in percent (50 .. 99) → ``(n_splits int32[B], count, size, parent int32[B, N - 3], split_length
        float64[B, N - 3] or None, leaf_parent int32[B, N], leaf_length float64[B, N] or None, status uint8[B])`` -
        ``consensus.join_consensus``, the same integers and the same doubles, bit for bit, as
        ``hostio.join_consensus_host``.  A table that is no join table is refused (``ValueError``)."""
        fn = self._optional("pf_join_consensus")
        rep, lengths, flag, (B, R, N), single = consensus_arrays(rep_slots, rep_lengths, rep_flag)
        out, ptrs = consensus_outputs(B, N, lengths is not None)
        self._check(fn(self._h, rep.ctypes.data, ptr(lengths), ptr(flag), B, R, N, int(percent), *ptrs))
        return unbatched(out, single)

    # -- distances between join tables -------------------------------------------------------
    def join_distances(self, slots: np.ndarray, lengths: Optional[np.ndarray] = None, flag: Optional[np.ndarray] = None):
        """Tree distances on the GPU (``pf_join_distances``): join tables ``int32[B, K, T]``, their lengths ``float64[B, K,
        T]`` or None, ``flag bool[B, K]`` or None (``[K, T]`` / ``[K]`` drop ``B``) → ``(shared int32[B, K, K], kf float64[B,
        K, K] or None, wrf float64[B, K, K] or None, status uint8[B])``: per pair of a source's trees the splits both hold
        (``RF = 2 (N - 3) - 2 shared``), the Kuhner-Felsenstein branch score and weighted RF - ``treedist.join_distances_py``,
        the same integers and the same doubles, bit for bit, as ``hostio.join_distances_host``.  A table that is no join
        table is refused (``ValueError``)."""
        fn = self._optional("pf_join_distances")
        s, l, f, (B, K, N), single = distance_arrays(slots, lengths, flag)
        out, ptrs = distance_outputs(B, K, l is not None)
        self._check(fn(self._h, s.ctypes.data, ptr(l), ptr(f), B, K, N, *ptrs))
        return unbatched(out, single)

    # -- site weights -----------------------------------------------------------------------
    @staticmethod
    def _weights(w, shape, what: str) -> np.ndarray:
        arr = np.asarray(w)
        if arr.shape != shape or arr.dtype.kind not in "fiu":
            raise ValueError(f"{what} must be a real array of shape {list(shape)}, got {arr.dtype} {list(arr.shape)}")
        return np.ascontiguousarray(arr, dtype=np.float32)

    def site_classes(self, idx: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """The classes of equal alignment columns as the forward's own kernel finds them (``pf_site_classes``):
        ``uint8[B, N, L]`` → ``(srep int32[B, L], ucount int32[B])`` (``[N, L]`` → ``([L], int)``).  ``srep[b, l]`` is the
        smallest site whose column equals column ``l``; ``ucount[b]`` counts the distinct columns, the sites whose
        column statistics the forward computes (option ``site_dedup``; with 0 the identity)."""
        fn = self._optional("pf_site_classes")
        idx, single = self._sources(idx, refuse_single=False)
        B, N, L = idx.shape
        srep = np.empty((B, L), dtype=np.int32)
        ucount = np.empty(B, dtype=np.int32)
        self._check(fn(self._h, idx.ctypes.data, B, N, L, srep.ctypes.data, ucount.ctypes.data))
        return (srep[0], int(ucount[0])) if single else (srep, ucount)

    def forward_weighted(self, idx: np.ndarray, weights: np.ndarray) -> np.ndarray:
        """Distances of alignments whose site ``l`` counts ``weights[..., l]`` times (``pf_forward_weighted``):
        ``uint8[B, N, L]``, ``float[B, L]`` → ``float32[B, P]`` (``[N, L]``, ``[L]`` → ``[P]``).  Integer weights give
        the distances of the alignment with every site repeated that often (to rounding); unit weights give ``forward``'s
        bits.  Weights must be finite and >= 0 and not all zero, else ``ValueError``."""
        fn = self._optional("pf_forward_weighted")
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        w = self._weights(np.asarray(weights)[None] if single else weights, (B, L), "weights")
        out = np.empty((B, N * (N - 1) // 2), dtype=np.float32)
        self._check(fn(self._h, idx.ctypes.data, B, N, L, w.ctypes.data if w.size else None, out.ctypes.data))
        return out[0] if single else out

    def forward_sites_weighted(self, idx: np.ndarray, sites: np.ndarray, weights: np.ndarray) -> np.ndarray:
        """``forward_sites`` with a weight per table entry (``pf_forward_sites_weighted``): ``uint8[B, N, L]``,
        ``int[S, K]``, ``float[S, K]`` → ``float32[B, S, P]``; ``out[b, s]`` is ``forward_weighted`` of
        ``idx[b][:, sites[s]]`` with ``weights[s]``, bit for bit."""
        fn = self._optional("pf_forward_sites_weighted")
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        tab = self._table(sites, "sites must be an integer array [S, K]", "site", L)
        S, K = tab.shape
        w = self._weights(weights, (S, K), "weights")
        out = np.empty((B, S, N * (N - 1) // 2), dtype=np.float32)
        self._check(fn(self._h, idx.ctypes.data, B, N, L, tab.ctypes.data if tab.size else None,
                       w.ctypes.data if w.size else None, S, K, out.ctypes.data if out.size else None))
        return out[0] if single else out

    def bootstrap_weighted(self, idx: np.ndarray, replicates: int, seed: int = 0) -> np.ndarray:
        """``bootstrap`` computed on each replicate's DISTINCT sites with their multiplicities as weights
        (``pf_bootstrap_weighted``): the same replicates of the same stream, about a third fewer tokens; equal to
        ``bootstrap`` to rounding, not bit for bit.  ``uint8[B, N, L]`` → ``float32[B, R, P]``."""
        fn = self._optional("pf_bootstrap_weighted")
        idx, single = self._sources(idx)
        B, N, L = idx.shape
        R = int(replicates)
        out = np.empty((B, max(R, 0), N * (N - 1) // 2), dtype=np.float32)
        self._check(fn(self._h, idx.ctypes.data, B, N, L, R, self._seed(seed),
                       out.ctypes.data if out.size else None))
        return out[0] if single else out

    def forward_sharded(self, idx_local: np.ndarray, l_begin: int, l_end: int, L_total: int) -> np.ndarray:
        """This rank's sites ``[l_begin, l_end)`` of ``uint8[B, N, L_total]`` alignments."""
        idx, single = self._sources(idx_local)
        B, N, Ll = idx.shape
        if Ll != l_end - l_begin:
            raise ValueError(f"idx has {Ll} sites, expected {l_end - l_begin}")
        out = np.empty((B, N * (N - 1) // 2), dtype=np.float32)
        self._check(self._optional("pf_forward_sharded")(self._h, idx.ctypes.data, B, N, l_begin, l_end, L_total, out.ctypes.data))
        return out[0] if single else out

    def forward_shards_emulated(self, idx: np.ndarray, nshards: int) -> np.ndarray:
        """Site-sharded algorithm over ``nshards`` emulated ranks on this one GPU (tests)."""
        idx, single = self._sources(idx, refuse_single=False)      # (N = 1 is the library's PF_EINVAL here)
        B, N, L = idx.shape
        out = np.empty((B, N * (N - 1) // 2), dtype=np.float32)
        self._check(self._optional("pf_forward_shards_emulated")(self._h, idx.ctypes.data, B, N, L, nshards, out.ctypes.data))
        return out[0] if single else out

    # -- device-resident variant (benchmark) ------------------------------------------------
    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self._optional("pf_device_malloc")(self._h, nbytes, C.byref(p)))
        return p.value

    def free(self, ptr: int):
        self._check(self._optional("pf_device_free")(self._h, C.c_void_p(ptr)))

    def h2d(self, dst: int, src: np.ndarray):
        src = np.ascontiguousarray(src)
        self._check(self._optional("pf_memcpy_h2d")(self._h, C.c_void_p(dst), src.ctypes.data, src.nbytes))

    def d2h(self, dst: np.ndarray, src: int):
        assert dst.flags["C_CONTIGUOUS"]
        self._check(self._optional("pf_memcpy_d2h")(self._h, dst.ctypes.data, C.c_void_p(src), dst.nbytes))

    def synchronize(self):
        self._check(self._optional("pf_synchronize")(self._h))

    # -- RCCL -------------------------------------------------------------------------------
    def unique_id(self) -> bytes:
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        rc = self._optional("pf_comm_unique_id")(buf)
        if rc != PF_OK:
            raise EngineError(rc, (self._optional("pf_last_error")(None) or b"").decode())
        return buf.raw

    def comm_init(self, unique_id: Optional[bytes], rank: int, world: int):
        buf = C.create_string_buffer(unique_id, UNIQUE_ID_BYTES) if unique_id else None
        self._check(self._optional("pf_comm_init")(self._h, buf, rank, world))
        self.rank, self.world = rank, world

    def comm_destroy(self):
        self._check(self._optional("pf_comm_destroy")(self._h))
        self.rank, self.world = 0, 1

    def collective_count(self) -> int:
        """All-reduces issued by this handle since the last ``profile_reset`` (always counted)."""
        return self.profile_get("collectives")[0]

    def rechecked_count(self) -> int:
        """Alignments the range re-check (option "recheck_above") recomputed in float64 since ``profile_reset``."""
        return self.profile_get("rechecked")[0]

    def comm_info(self) -> dict:
        """Path and version of the librccl the native library resolved (loads it if necessary)."""
        buf = C.create_string_buffer(512)
        ver = C.c_int32()
        rc = self._optional("pf_comm_info")(buf, 512, C.byref(ver))
        if rc != PF_OK:
            raise EngineError(rc, (self._optional("pf_last_error")(None) or b"").decode())
        return {"library": buf.value.decode(), "version": int(ver.value)}

    # -- profiling / debugging --------------------------------------------------------------
    def profile_reset(self):
        self._check(self._optional("pf_profile_reset")(self._h))

    def profile_get(self, kernel: str) -> Tuple[int, float]:
        n = C.c_int64()
        ms = C.c_double()
        self._check(self._optional("pf_profile_get")(self._h, kernel.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def debug_read(self, name: str) -> np.ndarray:
        n = self._check(self._optional("pf_debug_read")(self._h, name.encode(), None, 0))
        out = np.empty(n, dtype=np.float32)
        self._check(self._optional("pf_debug_read")(self._h, name.encode(), out.ctypes.data, n))
        return out

    def selftest(self) -> np.ndarray:
        out = np.empty(2304, dtype=np.float32)
        self._check(self._optional("pf_selftest")(self._h, out.ctypes.data))
        return out


def _pass_through(symbol: str):
    """A method that only forwards: its arguments positionally in the header's order behind the handle, device addresses
    as plain ints (0 or None: NULL), the status through ``_check``.  ctypes refuses a wrong count with ``TypeError``."""
    def method(self, *args):
        return self._check(self._optional(symbol)(self._h, *args))
    method.__name__, method.__qualname__ = symbol[3:], "Engine." + symbol[3:]
    method.__doc__ = cabi.PROTOTYPES[symbol].text
    return method


# the ``*_device`` forms (device arrays in, device arrays out; include/phyloformer_amd.h has their contracts) - method: symbol
PASS_THROUGHS = {name: "pf_" + name for name in (
    "forward_device", "forward_sharded_device", "gather_sites_device", "forward_site_map_device", "site_moments_device",
    "gather_taxa_device", "loo_stats_device", "place_stats_device", "tile_combine_device", "nj_joins_device", "bionj_joins_device",
    "delta_device", "tree_fit_device", "bme_nni_device", "bme_spr_device", "join_supports_device", "join_transfers_device",
    "join_consensus_device", "forward_weighted_device")}
for _name, _symbol in PASS_THROUGHS.items():
    setattr(Engine, _name, _pass_through(_symbol))
Engine.tree_root_device = _pass_through("pf_tree_root_device")
Engine.tree_ols_device = _pass_through("pf_tree_ols_device")      # (beside the list: a later addition to the header)
Engine.join_distances_device = _pass_through("pf_join_distances_device")
