"""``OracleEngine`` (real numerics through oracle/pf_oracle.py, no GPU) with ``forward_taxa`` /
``forward_leave_one_out``: the derived alignments are cut by the host twin of the device gather
(phyloformer_amd/taxa.py::cut_taxa), go through the oracle's forward, and are reduced by ``taxa.loo_stats``.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_taxa_engine:make
"""
import numpy as np

from helpers.oracle_engine import OracleEngine
from phyloformer_amd.taxa import cut_taxa, leave_one_out_sets, loo_stats


class OracleTaxaEngine(OracleEngine):
    def forward_taxa(self, idx, taxa):
        idx = np.asarray(idx, np.uint8)
        one = idx.ndim == 2
        cut = cut_taxa(idx[None] if one else idx, taxa)                        # [B][S][M][L]
        out = np.stack([self.forward(c) for c in cut])
        return out[0] if one else out

    def forward_leave_one_out(self, idx, keep_loo=False):
        idx = np.asarray(idx, np.uint8)
        one = idx.ndim == 2
        src = idx[None] if one else idx
        dist = self.forward(src).astype(np.float32)
        loo = self.forward_taxa(src, leave_one_out_sets(src.shape[1])).astype(np.float32)
        res = (dist,) + loo_stats(dist, loo) + ((loo,) if keep_loo else ())
        return tuple(r[0] for r in res) if one else res


def make(weights, device):
    return OracleTaxaEngine(weights, device)
