"""``OracleEngine`` (real numerics through oracle/pf_oracle.py, no GPU) with ``forward_sites`` / ``forward_windows``: the
derived alignments are cut by the host twin of the device gather (phyloformer_amd/windows.py::cut_sites) and go through
the oracle's forward.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_windows_engine:make
"""
import numpy as np

from helpers.oracle_engine import OracleEngine
from phyloformer_amd.windows import cut_sites, window_sites


class OracleWindowsEngine(OracleEngine):
    def forward_sites(self, idx, sites):
        idx = np.asarray(idx, np.uint8)
        one = idx.ndim == 2
        cut = cut_sites(idx[None] if one else idx, sites)                      # [B][S][N][K]
        out = np.stack([self.forward(c) for c in cut])
        return out[0] if one else out

    def forward_windows(self, idx, W, step=None):
        return self.forward_sites(idx, window_sites(np.asarray(idx).shape[-1], W, step))


def make(weights, device):
    return OracleWindowsEngine(weights, device)
