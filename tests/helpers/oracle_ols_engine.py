"""``OracleFitEngine`` (real numerics through oracle/pf_oracle.py, no GPU; ``tree_fit`` and the join tables by the serial native
twins) with ``tree_ols`` by its twin as well, and a counter of its calls.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_ols_engine:make
"""
from helpers.oracle_fit_engine import OracleFitEngine
from phyloformer_amd import hostio


class OracleOlsEngine(OracleFitEngine):
    ols_calls = 0

    def tree_ols(self, preds, slots):
        type(self).ols_calls += 1
        return hostio.tree_ols_host(preds, slots)


def make(weights, device):
    return OracleOlsEngine(weights, device)
