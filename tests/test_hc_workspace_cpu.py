"""The workspace sizes of the HC pipelines are part of the ABI: a caller allocates what the _workspace function says and
the call refuses anything smaller.  tests/golden/hc_workspaces.json records them over the grid of tests/hcwsgrid.py (from
the library of the commit before the three pipelines shared one chunk rule, see tests/golden/gen_hc_workspaces.py); every
later library answers the same."""
import json
import os

import pytest

import hcwsgrid

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hc_workspaces.json")


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_table_has_the_whole_grid(table):
    assert [len(hcwsgrid.rows(k)) for k in hcwsgrid.KINDS] == [132, 792, 88]
    for kind in hcwsgrid.KINDS:
        assert len(table[kind]) == len(hcwsgrid.rows(kind)), kind
    # the rule bends inside the grid: sizes that grow with nblocks, stop at 8192 blocks, and stop earlier at 6 GiB
    plain = dict(zip(hcwsgrid.rows("plain"), table["plain"]))
    assert plain[8191, 200] < plain[8192, 200] == plain[8193, 200] == plain[100000, 200]
    assert plain[3, (1 << 24) + 1] < plain[4096, (1 << 24) + 1] == plain[100000, (1 << 24) + 1] <= 6 << 30
    assert plain[1, 0xFFFFFFFF] == plain[100000, 0xFFFFFFFF] > 6 << 30          # one block per chunk, whatever it takes


@pytest.mark.parametrize("kind", hcwsgrid.KINDS)
def test_workspace_sizes_match_the_recorded_table(zl, table, kind):
    L = zl.lib()
    wrong = [(row, got, want) for row, want in zip(hcwsgrid.rows(kind), table[kind])
             for got in [hcwsgrid.call(zl, L, kind, row)] if got != want]
    assert not wrong, "%d rows differ, the first (row, size, recorded): %r" % (len(wrong), wrong[0])
