"""``OracleFitEngine`` (real numerics through oracle/pf_oracle.py, no GPU; the join tables by the serial native twins) with
``bootstrap`` by the host twin of the device stream, ``join_supports`` / ``join_distances`` by their twins, and a counter of the
distance calls.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_treedist_engine:make
"""
from helpers.oracle_boot_engine import OracleBootEngine
from helpers.oracle_fit_engine import OracleFitEngine
from phyloformer_amd import hostio


class OracleTreedistEngine(OracleFitEngine, OracleBootEngine):
    distance_calls = 0

    def join_distances(self, slots, lengths=None, flag=None):
        type(self).distance_calls += 1
        return hostio.join_distances_host(slots, lengths, flag)

    def join_supports(self, ref_slots, rep_slots, rep_flag=None):
        return hostio.join_supports_host(ref_slots, rep_slots, rep_flag)

    def tree_ols(self, preds, slots):
        return hostio.tree_ols_host(preds, slots)


def make(weights, device):
    return OracleTreedistEngine(weights, device)
