"""Which combinations of the mode flags ``infer_alns.py`` refuses, with which exit code and message: a replay of
``tests/golden/cli_flag_refusals.json`` (tools/gen_golden_cli_flag_refusals.py: every subset of the five mode flags
crossed with ``--shard files`` / ``--shard sites``, ``--bootstrap -1`` and malformed ``--windows``).  No engine, no GPU:
a case runs ``main`` in-process without ``-o``, so a combination that is not refused ends in the ``TypeError`` of
``os.path.abspath(None)`` right behind the flag checks."""
import contextlib
import io
import itertools
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (["--bootstrap", "5"], ["--windows", "16"], ["--site-profile"], ["--leave-one-out"], ["--compress-sites"])


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(REPO, "tests", "golden", "cli_flag_refusals.json")) as fh:
        return json.load(fh)


def test_golden_covers_every_subset_of_the_mode_flags(recorded):
    have = {tuple(r["flags"]) for r in recorded}
    for k in range(len(MODES) + 1):
        for combo in itertools.combinations(MODES, k):
            for shard in ("files", "sites"):
                assert tuple(a for flag in combo for a in flag) + ("--shard", shard) in have
    assert any(r["flags"][:2] == ["--bootstrap", "-1"] for r in recorded)
    assert any(r["flags"][:2] == ["--windows", "abc"] for r in recorded)
    accepted = [r["flags"] for r in recorded if r["code"] is None]
    assert all(any(f == mode + ["--shard", "files"] for f in accepted) for mode in MODES)     # every mode alone runs


def test_every_flag_combination_is_refused_or_accepted_as_recorded(recorded, monkeypatch):
    import infer_alns
    monkeypatch.setattr(sys, "argv", ["infer_alns.py"])             # argparse's prog, the first word of the message
    for r in recorded:
        err = io.StringIO()
        code, reached_error = None, False
        try:
            with contextlib.redirect_stderr(err):
                infer_alns.main(["W", "D", *r["flags"]])
            pytest.fail(f"{r['flags']}: main returned without an output directory")
        except SystemExit as exc:
            code, reached_error = exc.code, True
        except TypeError:
            pass                                                    # every flag check passed; nothing was started
        if r["code"] is None:
            assert not reached_error, (r["flags"], err.getvalue().splitlines()[-1:])
        else:
            assert code == r["code"], (r["flags"], code)
            assert err.getvalue().splitlines()[-1] == r["error"], r["flags"]
