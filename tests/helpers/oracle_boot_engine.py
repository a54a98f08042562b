"""``OracleEngine`` (real numerics through oracle/pf_oracle.py, no GPU) with ``bootstrap``: the replicates are built by
the host twin of the device stream (phyloformer_amd/bootstrap.py::resample) and go through the oracle's forward.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_boot_engine:make
"""
import numpy as np

from helpers.oracle_engine import OracleEngine
from phyloformer_amd.bootstrap import resample


class OracleBootEngine(OracleEngine):
    def bootstrap(self, idx, replicates, seed=0):
        idx = np.asarray(idx, np.uint8)
        one = idx.ndim == 2
        reps = resample(idx[None] if one else idx, replicates, seed)          # [B][R][N][L]
        out = np.stack([self.forward(r) for r in reps])
        return out[0] if one else out


def make(weights, device):
    return OracleBootEngine(weights, device)
