#!/usr/bin/env python3
"""Record which combinations of the per-alignment mode flags ``infer_alns.py`` refuses, and with which message:
``tests/golden/cli_flag_refusals.json``, replayed by ``tests/test_cli_flag_refusals.py``.

Every case runs ``infer_alns.main(argv)`` in this process WITHOUT ``-o``: a refused combination leaves through
``parser.error`` (``SystemExit(2)``, the message is the last stderr line); one that is not refused reaches the
``os.path.abspath(None)`` behind the flag checks and raises ``TypeError`` before any engine exists (``code`` null).
The committed file was recorded at the commit before the refusals became data; regenerate it only to add cases.
"""
import contextlib
import io
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (["--bootstrap", "5"], ["--windows", "16"], ["--site-profile"], ["--leave-one-out"], ["--compress-sites"])
BAD_WINDOWS = ("0", "abc", "16:0", "1:2:3", "")


def cases():
    out = []
    for k in range(len(MODES) + 1):
        for combo in itertools.combinations(MODES, k):
            for shard in ("files", "sites"):
                out.append([a for flag in combo for a in flag] + ["--shard", shard])
    everything = [a for flag in MODES[1:] for a in flag]
    for rest in ([], ["--shard", "sites"], ["--windows", "16"], everything, everything + ["--shard", "sites"]):
        out.append(["--bootstrap", "-1"] + rest)
    for bad in BAD_WINDOWS:
        for rest in ([], ["--bootstrap", "5"], ["--shard", "sites"], ["--site-profile"], ["--leave-one-out", "--compress-sites"]):
            out.append(["--windows", bad] + rest)
    return out


def outcome(main, flags):
    """``(exit code or None, last stderr line or None)`` of ``main(["W", "D", *flags])``."""
    err = io.StringIO()
    argv0, sys.argv[0] = sys.argv[0], "infer_alns.py"          # argparse's prog
    try:
        with contextlib.redirect_stderr(err):
            main(["W", "D", *flags])
    except SystemExit as exc:
        return exc.code, err.getvalue().splitlines()[-1]
    except TypeError:                                          # abspath(None): every flag check passed
        return None, None
    finally:
        sys.argv[0] = argv0
    raise AssertionError(f"{flags}: main returned without an output directory")


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    import infer_alns
    rows = []
    for flags in cases():
        code, error = outcome(infer_alns.main, flags)
        rows.append({"flags": flags, "code": code, "error": error})
    with open(os.path.join(REPO, "tests", "golden", "cli_flag_refusals.json"), "w") as fh:
        json.dump(rows, fh, indent=0)
        fh.write("\n")
    print(f"{len(rows)} cases, {sum(r['code'] is not None for r in rows)} refused")
