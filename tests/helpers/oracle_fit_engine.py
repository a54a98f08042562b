"""``OracleEngine`` (real numerics through oracle/pf_oracle.py, no GPU) with ``tree_fit`` and the calls that make join
tables: the serial native twins (``hostio``) stand in for the device, with the ``Engine``'s arguments and results.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_fit_engine:make
"""
from helpers.oracle_engine import OracleEngine
from phyloformer_amd import hostio


class OracleFitEngine(OracleEngine):
    calls = 0

    def tree_fit(self, preds, slots, lengths, patristic=True):
        type(self).calls += 1
        return hostio.tree_fit_host(preds, slots, lengths, patristic)

    def nj_joins(self, preds):
        return hostio.nj_joins_host(preds)

    def bionj_joins(self, preds):
        return hostio.bionj_joins_host(preds)

    def bme_nni(self, preds, start):
        return hostio.bme_nni_host(preds, start)

    def bme_spr(self, preds, start):
        return hostio.bme_spr_host(preds, start)


def make(weights, device):
    return OracleFitEngine(weights, device)
