"""``OracleEngine`` (real numerics through oracle/pf_oracle.py, no GPU) with ``forward_site_map`` /
``forward_site_profile``: the oracle's ``logits`` tap -> softplus -> the numpy twins of phyloformer_amd/siteprofile.py.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_sitemap_engine:make
"""
import numpy as np

from helpers.oracle_engine import OracleEngine
from oracle import pf_oracle as O
from phyloformer_amd.siteprofile import site_moments, softplus


class OracleSiteMapEngine(OracleEngine):
    dtype = np.float32

    def _one(self, a):
        taps = {}
        dist = O.forward(self.w, a, dtype=self.dtype, tap=lambda k, v: taps.__setitem__(k, np.array(v)))
        return dist, softplus(taps["logits"])

    def forward_site_map(self, idx):
        idx = np.asarray(idx, np.uint8)
        one = idx.ndim == 2
        res = [self._one(a) for a in (idx[None] if one else idx)]
        dist = np.stack([r[0] for r in res]).astype(np.float32)
        smap = np.stack([r[1] for r in res]).astype(np.float32)
        return (dist[0], smap[0]) if one else (dist, smap)

    def forward_site_profile(self, idx):
        idx = np.asarray(idx, np.uint8)
        one = idx.ndim == 2
        dist, smap = self.forward_site_map(idx[None] if one else idx)
        se, prof = site_moments(smap)
        se, prof = se.astype(np.float32), prof.astype(np.float32)
        return (dist[0], se[0], prof[0]) if one else (dist, se, prof)


class OracleSiteMapEngine64(OracleSiteMapEngine):
    dtype = np.float64


def make(weights, device):
    return OracleSiteMapEngine(weights, device)
