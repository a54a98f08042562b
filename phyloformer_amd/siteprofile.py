"""Site-resolved distances on the host: the numpy twins of ``csrc/pf_sitemap.hip.h`` and the writers of
``infer_alns.py --site-profile``.

The head computes one value per (pair, site), ``d[p][l] = softplus(w . x[p][l] + b)``, and a distance is their mean
over sites.  From the map ``d [P][L]`` (``Engine.forward_site_map``):

    se[p]      = sqrt( sum_l (d[p][l] - m[p])^2 / (L (L - 1)) ),  m[p] = mean_l d[p][l]      (0 for L = 1)
    profile[l] = mean_p d[p][l]

``se`` is the spread of the site mean: a descriptive statistic of the model's own terms, not a calibrated confidence
interval (sites are not independent after column attention).
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np


def softplus(z: np.ndarray) -> np.ndarray:
    """``nn.Softplus(beta=1, threshold=20)`` in float64: the head's activation on its logits."""
    z = np.asarray(z, np.float64)
    return np.where(z > 20.0, z, np.log1p(np.exp(np.minimum(z, 20.0))))


def site_moments(smap: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``map [..., P, L]`` → ``(se [..., P], profile [..., L])`` in float64, the literal definitions."""
    m = np.asarray(smap, np.float64)
    if m.ndim < 2:
        raise ValueError(f"a site map is [..., P, L], got shape {m.shape}")
    L = m.shape[-1]
    mean = m.mean(axis=-1, keepdims=True)
    if L > 1:
        se = np.sqrt(((m - mean) ** 2).sum(axis=-1) / (L * (L - 1)))
    else:
        se = np.zeros(m.shape[:-1], np.float64)
    return se, m.mean(axis=-2)


def sites_tsv(profile: np.ndarray) -> str:
    """``<stem>.sites.tsv``: header ``site profile relative``, one row per site (1-based);
    ``relative = profile / mean(profile)``, ``NA`` when the mean is 0.  ``profile`` has the number format of
    ``<stem>.phy``; ``relative`` is written with 15 decimals, so that the column read back still averages to 1 to 1e-12."""
    p = np.asarray(profile, np.float64).reshape(-1)
    mean = float(p.mean()) if p.size else 0.0
    rows = ["site\tprofile\trelative\n"]
    for k, v in enumerate(p):
        rel = "NA" if mean == 0.0 else f"{float(v) / mean:.15f}"
        rows.append(f"{k + 1}\t{float(v):.10f}\t{rel}\n")
    return "".join(rows)


def se_phylip(se: np.ndarray, ids: Sequence[str]) -> str:
    """``<stem>.se.phy``: the standard errors as a PHYLIP matrix, ids and number format of ``<stem>.phy``."""
    from .phylip import vec_to_phylip
    return vec_to_phylip(np.asarray(se), ids)[1]
