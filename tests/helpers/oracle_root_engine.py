"""``OracleTreedistEngine`` (real numerics through oracle/pf_oracle.py, no GPU; ``tree_fit``, ``tree_ols``, ``join_distances`` and the join
tables by the serial native twins) with ``tree_root`` by its twin as well, and a counter of its calls.

    PF_CLI_ENGINE_FACTORY=helpers.oracle_root_engine:make
"""
from helpers.oracle_treedist_engine import OracleTreedistEngine
from phyloformer_amd import hostio


class OracleRootEngine(OracleTreedistEngine):
    root_calls = 0

    def tree_root(self, slots, lengths):
        type(self).root_calls += 1
        return hostio.tree_root_host(slots, lengths)


def make(weights, device):
    return OracleRootEngine(weights, device)
