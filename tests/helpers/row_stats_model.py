"""A plain-Python model of the row layout of option ``stats_dedup``, written from the definitions
of k_main's two tilings and without a call into the library:

  * ``part_lines``: the parts of every pair row of a (P, L) alignment - which tile of the alignment, which site the
    tile's lane 0 stands for (negative where a flat tile starts in the row in front), which partial slot;
  * ``ctile_lines``: the compact tiles of a row with K distinct columns;
  * ``kmax``: ROW_STATS_KMAX, read out of ``csrc/pf_layout.h``'s text.

The lines are those ``tests/native/pf_row_stats_layout_main.cpp`` prints.
"""
import re

from helpers.dedup_model import LAYOUT_H

_KMAX = []


def kmax():
    if not _KMAX:
        with open(LAYOUT_H) as fh:
            found = re.findall(r"^constexpr int ROW_STATS_KMAX\s*=\s*(\d+);", fh.read(), re.M)
        assert len(found) == 1, found
        _KMAX.append(int(found[0]))
    return _KMAX[0]


def row_parts(flat, P, L):
    """{p: [(tile, l0, slot), ...]} by enumerating every token of the alignment in its tile and lane."""
    ntiles = -(-L // 32)
    parts = {p: {} for p in range(P)}
    for p in range(P):
        for l in range(L):
            if flat:                       # 32 consecutive tokens of the alignment per tile; slot = tile + row
                tile, lane = divmod(p * L + l, 32)
                slot = tile + p
            else:                          # every row has its own ceil(L / 32) tiles; slot = tile
                tile, lane = p * ntiles + l // 32, l % 32
                slot = tile
            l0 = l - lane                  # the site lane 0 stands for
            assert parts[p].setdefault(tile, (tile, l0, slot)) == (tile, l0, slot)
    return {p: [parts[p][k] for k in sorted(parts[p])] for p in range(P)}


def part_lines(flat, P, L):
    rows = row_parts(flat, P, L)
    return [f"part {flat} {P} {L} {p} {j} {tile} {l0} {slot}" for p in range(P) for j, (tile, l0, slot) in enumerate(rows[p])]


def ctile_lines(K):
    return [f"ctile {K} {ct} {min(32, K - 32 * ct)}" for ct in range(-(-K // 32))]
