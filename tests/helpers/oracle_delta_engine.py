"""``OracleEngine`` (real numerics through oracle/pf_oracle.py, no GPU) with ``delta``: the serial native twin
(``hostio.delta_host``) stands in for the device, with ``Engine.delta``'s arguments and results.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_delta_engine:make
"""
from helpers.oracle_engine import OracleEngine
from phyloformer_amd import hostio


class OracleDeltaEngine(OracleEngine):
    def delta(self, preds, bins=20):
        return hostio.delta_host(preds, bins=bins)


def make(weights, device):
    return OracleDeltaEngine(weights, device)
