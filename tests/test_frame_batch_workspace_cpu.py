"""The workspace sizes of the batch frame calls are part of the ABI: a caller allocates what the _workspace function says
and the call refuses anything smaller.  tests/golden/frame_batch_workspaces.json records them (from the library of the commit
before the layouts were given names, see tests/golden/gen_frame_batch_workspaces.py); every later library answers the same."""
import json
import os

import wsgrid

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_batch_workspaces.json")


def _rows():
    with open(TABLE) as f:
        return json.load(f)["rows"]


def test_table_covers_every_function_and_axis_value():
    rows = _rows()
    assert 200 <= len(rows) <= 900
    for fn in wsgrid.FUNCS:
        mine = [r for r in rows if r["fn"] == fn]
        assert mine, fn
        assert not wsgrid.missing(fn, mine), (fn, wsgrid.missing(fn, mine))
        for r in mine:                                   # a row of the grid, nothing else
            assert set(r) == {"fn", "bytes"} | set(wsgrid.FUNCS[fn]), r
            assert all(wsgrid._get(r, key) in want for key, want in wsgrid.axis_values(fn).items()), r
        if "max_src_len" in wsgrid.FUNCS[fn]:            # 0, 100, the block size and one byte more
            bs = wsgrid.BLOCK_SIZES
            kinds = {("bs" if r["max_src_len"] == bs[r["prefs"]["block_size_id"]] else
                      "bs+1" if r["max_src_len"] == bs[r["prefs"]["block_size_id"]] + 1 else r["max_src_len"]) for r in mine}
            assert kinds == {0, 100, "bs", "bs+1"}, kinds


def test_workspace_sizes_match_the_recorded_table(zl):
    L = zl.lib()
    wrong = [(r, got) for r in _rows() for got in [wsgrid.call(zl, L, r["fn"], r)] if got != r["bytes"]]
    assert not wrong, "%d rows differ, the first: %r" % (len(wrong), wrong[0])
