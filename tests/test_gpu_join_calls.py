"""-m gpu: the pointers of the join-table entry points through the raw symbols - ``pf_join_supports``, ``pf_join_transfers``
and ``pf_join_consensus``, each with the caller's arrays on the host and on the device, at B = 1, R = 2, N = 5.  Every
required pointer passed as null in turn is refused with "null buffer" and nothing is written; every optional one
(``rep_flag``; ``branch_moves``; ``rep_lengths`` with both length results) may be null, and the remaining results are
then, as bytes, those of the call that passes it; ``rep_lengths`` without one of its two results is a null buffer."""
import numpy as np
import pytest

from helpers.handle_cases import random_tables
from phyloformer_amd.engine import Engine

pytestmark = pytest.mark.gpu

B, R, N = 1, 2, 5
T, S = 2 * (N - 3) + 3, N - 3
DIMS = "dims"          # where B, R, N and the call's percent stand among the arguments

# per call: its percent, and its arguments in the header's order as (name, dtype, shape, is it an input?)
CALLS = {
    "pf_join_supports": (None, [
        ("ref_slots", np.int32, (B, T), True), ("rep_slots", np.int32, (B, R, T), True), ("rep_flag", np.uint8, (B, R), True), DIMS,
        ("count", np.int32, (B, S), False), ("transfer", np.int64, (B, S), False), ("depth", np.int32, (B, S), False),
        ("status", np.uint8, (B,), False)]),
    "pf_join_transfers": (100, [
        ("ref_slots", np.int32, (B, T), True), ("rep_slots", np.int32, (B, R, T), True), ("rep_flag", np.uint8, (B, R), True), DIMS,
        ("count", np.int32, (B, S), False), ("transfer", np.int64, (B, S), False), ("depth", np.int32, (B, S), False),
        ("moves", np.int64, (B, N), False), ("used", np.int32, (B, S), False), ("capped", np.int32, (B, S), False),
        ("branch_moves", np.int32, (B, S, N), False), ("status", np.uint8, (B,), False)]),
    "pf_join_consensus": (50, [
        ("rep_slots", np.int32, (B, R, T), True), ("rep_lengths", np.float64, (B, R, T), True), ("rep_flag", np.uint8, (B, R), True), DIMS,
        ("n_splits", np.int32, (B,), False), ("count", np.int32, (B, S), False), ("size", np.int32, (B, S), False),
        ("parent", np.int32, (B, S), False), ("split_length", np.float64, (B, S), False), ("leaf_parent", np.int32, (B, N), False),
        ("leaf_length", np.float64, (B, N), False), ("status", np.uint8, (B,), False)]),
}
# what may be null together, and what else is then not compared
OPTIONAL = {
    "pf_join_supports": [("rep_flag",)],
    "pf_join_transfers": [("rep_flag",), ("branch_moves",)],
    "pf_join_consensus": [("rep_flag",), ("rep_lengths", "split_length", "leaf_length")],
}
# null alone, these are refused too: rep_lengths is there
HALVES = {"pf_join_consensus": ["split_length", "leaf_length"]}


def inputs(name):
    rng = np.random.default_rng(55)
    values = {"ref_slots": random_tables(rng, (B,), N), "rep_slots": random_tables(rng, (B, R), N),
              "rep_lengths": rng.uniform(0.01, 1.0, size=(B, R, T)), "rep_flag": np.zeros((B, R), np.uint8)}      # (flags nothing)
    return {arg[0]: np.ascontiguousarray(values[arg[0]], dtype=arg[1]) for arg in CALLS[name][1] if arg != DIMS and arg[3]}


def call(e, name, device, null=()):
    """``(rc, last error, {result: array})`` of one call with the arguments in ``null`` passed as null; the results start
    as 0x77 bytes."""
    percent, args = CALLS[name]
    fn = e._optional(name + ("_device" if device else ""))
    given = inputs(name)
    blank = lambda dtype, shape: np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x77, np.uint8).view(dtype).reshape(shape)
    host = {a[0]: given[a[0]] if a[3] else blank(a[1], a[2]) for a in args if a != DIMS}
    dev = {}
    try:
        if device:
            for k, v in host.items():
                dev[k] = e.malloc(v.nbytes)
                e.h2d(dev[k], v)
        ptrs = []
        for a in args:
            if a == DIMS:
                ptrs += [B, R, N] + ([] if percent is None else [percent])
            else:
                ptrs.append(None if a[0] in null else dev[a[0]] if device else host[a[0]].ctypes.data)
        rc = fn(e._h, *ptrs)
        err = e._lib.pf_last_error(e._h)
        if device:
            for k, v in host.items():
                e.d2h(v, dev[k])
            e.synchronize()
    finally:
        for ptr in dev.values():
            e.free(ptr)
    return rc, err, {a[0]: host[a[0]] for a in args if a != DIMS and not a[3]}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(CALLS))
def test_null_pointers(weights, name, device):
    names = [a[0] for a in CALLS[name][1] if a != DIMS]
    optional = {k for group in OPTIONAL[name] for k in group}
    with Engine(weights("pf"), 0) as e:
        rc, err, want = call(e, name, device)
        assert rc == 0, err
        assert all(v.tobytes() != b"\x77" * v.nbytes for v in want.values())
        for k in [k for k in names if k not in optional] + HALVES.get(name, []):
            rc, err, got = call(e, name, device, null=(k,))
            assert rc == -1 and b"null buffer" in err, (k, rc, err)
            assert all(v.tobytes() == b"\x77" * v.nbytes for v in got.values()), k
        for group in OPTIONAL[name]:
            rc, err, got = call(e, name, device, null=group)
            assert rc == 0, (group, err)
            for k, v in got.items():
                assert v.tobytes() == (b"\x77" * v.nbytes if k in group else want[k].tobytes()), (group, k)
