"""``OracleBootEngine`` (real numerics through oracle/pf_oracle.py, no GPU) with ``forward_weighted`` /
``bootstrap_weighted``: integer site weights stand for repeated columns (``weights_sites.expand``), so the weighted
forward is the oracle's forward of the alignment with every column repeated by its weight, and a weighted replicate is
the oracle's forward of its ``weights_sites.boot_counts`` table expanded the same way.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_weights_engine:make
"""
import numpy as np

from helpers.oracle_boot_engine import OracleBootEngine
from phyloformer_amd.weights_sites import boot_counts, expand


class OracleWeightsEngine(OracleBootEngine):
    def forward_weighted(self, idx, weights):
        idx, w = np.asarray(idx, np.uint8), np.asarray(weights)
        one = idx.ndim == 2
        out = np.stack([self.forward(expand(a, wa)) for a, wa in zip(idx[None] if one else idx, w[None] if one else w)])
        return out[0] if one else out

    def bootstrap_weighted(self, idx, replicates, seed=0):
        idx = np.asarray(idx, np.uint8)
        one = idx.ndim == 2
        tables = [boot_counts(idx.shape[-1], replicates, seed, r) for r in range(replicates)]
        out = np.stack([np.stack([self.forward(expand(a[:, sites], counts)) for sites, counts in tables])
                        for a in (idx[None] if one else idx)])
        return out[0] if one else out


def make(weights, device):
    return OracleWeightsEngine(weights, device)
