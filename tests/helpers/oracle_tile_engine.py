"""``OracleEngine`` (real numerics through oracle/pf_oracle.py, no GPU) with ``forward_tiled``: the sets are cut on the
host by the twin of the device gather (phyloformer_amd/tile.py::cut_sets), go through the oracle's forward, and are
combined by ``tile.combine``.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_tile_engine:make
"""
import numpy as np

from helpers.oracle_engine import OracleEngine
from phyloformer_amd.tile import combine, cut_sets


class OracleTileEngine(OracleEngine):
    def forward_tiled(self, idx, M):
        idx = np.asarray(idx, np.uint8)
        one = idx.ndim == 2
        src = idx[None] if one else idx
        sets = [self.forward(s).astype(np.float32) for s in cut_sets(src, M)]      # (ValueError for M < 2 or N <= M)
        out, spread = combine(sets, src.shape[1], M)
        return (out[0], spread[0]) if one else (out, spread)


def make(weights, device):
    return OracleTileEngine(weights, device)
