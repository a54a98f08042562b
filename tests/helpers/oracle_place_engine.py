"""``OracleEngine`` (real numerics through oracle/pf_oracle.py, no GPU) with ``forward_place``: the backbone and the
query sets are built by the host twin of the device gather (phyloformer_amd/place.py::join_query), go through the
oracle's forward, and are reduced by ``place.place_stats``.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_place_engine:make
"""
import numpy as np

from helpers.oracle_engine import OracleEngine
from phyloformer_amd.place import join_query, place_stats


class OraclePlaceEngine(OracleEngine):
    def forward_place(self, idx, queries, keep_sets=False):
        idx = np.asarray(idx, np.uint8)
        one = idx.ndim == 2
        src = idx[None] if one else idx
        Q = int(queries)
        N = src.shape[1] - Q
        if Q < 1 or N < 2:
            raise ValueError(f"placement needs Q >= 1 queries and a backbone of M - Q >= 2 sequences (got M={src.shape[1]}, Q={Q})")
        dist = self.forward(src).astype(np.float32)
        base = self.forward(src[:, :N]).astype(np.float32)
        sets = np.stack([self.forward(np.stack([join_query(a, N, q) for q in range(Q)])) for a in src]).astype(np.float32)
        res = (dist, base) + place_stats(dist, base, sets, N, Q) + ((sets,) if keep_sets else ())
        return tuple(r[0] for r in res) if one else res


def make(weights, device):
    return OraclePlaceEngine(weights, device)
