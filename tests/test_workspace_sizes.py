"""CPU: every workspace / scratch / state size query of the C ABI returns the recorded number.

tests/golden/workspace_sizes.json was recorded once from the library built at commit 3b6b88f (before the size
queries were derived from the entry points' workspace plans), over a grid that crosses the path boundaries:
channel counts 1..46 (fixed / wide / matrix-core / tile paths), lengths 2..1100 (one and several column
blocks, the matrix-core carries past 160 points, the global slabs past 509), 1..33 sequences, 1..8 levels,
orders 1, 2, 6, the three pair modes, dyadic orders 0..4, both difference flags.  Each row is the argument
list followed by the value.  A query may only ever grow against this table, and only where the old value
was smaller than a workspace the entry point can ask for; there is no such row so far.
"""
import ctypes
import json
import os

import pytest

from conftest import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
KNOBS = ["GPSIG_FO_FIXED_MAX", "GPSIG_WIDE_MF", "GPSIG_VJP_FIXED_MAX", "GPSIG_BWD_PK", "GPSIG_HO_SPLIT",
         "GPSIG_TVS_TILE_BYTES", "GPSIG_PDE_LP", "GPSIG_MF_PARTS", "GPSIG_MF_NW"]
TABLE = json.load(open(FIXTURE))


def test_fixture_covers_every_size_query_of_the_header():
    import re
    txt = open(os.path.join(ROOT, "include", "gpsig_amd.h")).read()
    assert sorted(TABLE) == sorted(set(re.findall(r"\bsize_t\s+(gpsig_[a-z_]+)\s*\(", txt)))
    assert sum(len(v) for v in TABLE.values()) >= 300


@pytest.mark.parametrize("name", sorted(TABLE))
def test_size_query_matches_recorded_values(name):
    for k in KNOBS:
        assert k not in os.environ, f"{k} is set: the table holds the defaults"
    import gpsig_amd._lib as L
    fn = getattr(L.load(), name)
    assert fn.restype is ctypes.c_size_t
    bad = [(row[:-1], row[-1], int(fn(*row[:-1]))) for row in TABLE[name] if int(fn(*row[:-1])) != row[-1]]
    assert not bad, f"{name}: (args, recorded, now) {bad[:8]}"
