"""-m gpu: one engine runs every host entry point that carves a grow-only device buffer of the handle at a small shape,
at a larger one and at the small one again (``helpers/handle_cases.py``); every output array equals, as bytes, that of
an engine that has made only that call.  A stale capacity, a stale pair table or a span carved for the wrong count
shows as a difference.  Once with default options and once with ``ws_limit_mb = 1``, where chunks reuse a buffer."""
import numpy as np
import pytest

from helpers import handle_cases as hc

pytestmark = pytest.mark.gpu


def fresh(weights, ws_limit_mb):
    from phyloformer_amd import build
    from phyloformer_amd.engine import Engine
    build.build()
    eng = Engine(weights("pf"), device=0)
    if ws_limit_mb:
        eng.set_option("ws_limit_mb", ws_limit_mb)
    return eng


@pytest.mark.parametrize("ws_limit_mb", [0, 1], ids=["default", "ws_limit_mb=1"])
def test_a_shared_handle_gives_the_bytes_of_a_fresh_one(weights, ws_limit_mb):
    want = {}
    for visit in (0, 1):                            # (visit 2 repeats visit 0's shapes and inputs)
        for name, call in hc.calls(visit).items():
            with fresh(weights, ws_limit_mb) as lone:
                want[visit, name] = call(lone)
    assert sorted({name for _, name in want}) == sorted(hc.NAMES)
    differ = []
    with fresh(weights, ws_limit_mb) as eng:
        for visit in (0, 1, 2):
            for name, call in hc.calls(visit).items():
                got = call(eng)
                assert all(np.asarray(g).size for g in got), (visit, name)
                if not hc.same_bytes(got, want[visit % 2, name]):
                    differ.append((visit, name))
    assert not differ, differ
