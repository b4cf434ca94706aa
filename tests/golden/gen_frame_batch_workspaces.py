#!/usr/bin/env python3
"""Writes tests/golden/frame_batch_workspaces.json: what the workspace-size functions of the batch frame calls answer for
the rows of tests/wsgrid.py (pure host arithmetic, no GPU needed).

The table pins the sizes across a change of how the layouts are written down, so it is recorded from a library built from
the PARENT of such a change, never from the changed tree itself: the committed table comes from the library of commit
8fdd6cf, the last one whose layouts were numbered slots.  Name the library to record from:

  python tests/golden/gen_frame_batch_workspaces.py path/to/parent/libzlz4_amd.so
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import wsgrid  # noqa: E402
import zig_lz4_amd as zl  # noqa: E402

OUT = os.path.join(HERE, "frame_batch_workspaces.json")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    L = C.CDLL(os.path.abspath(sys.argv[1]))
    rows = []
    for fn in wsgrid.FUNCS:
        f = getattr(L, fn)
        f.restype, f.argtypes = zl.SYMBOLS[fn]
        picked = wsgrid.sample(fn)
        assert not wsgrid.missing(fn, picked), fn
        rows.extend(dict(fn=fn, **row, bytes=wsgrid.call(zl, L, fn, row)) for row in picked)
        print("%s: %d of %d rows" % (fn, len(picked), len(wsgrid.product(fn))))
    with open(OUT, "w") as f:
        f.write('{"source": "libzlz4_amd.so of commit 8fdd6cf (the parent of the named layouts)", "rows": [\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")
    print("%d rows -> %s" % (len(rows), OUT))


if __name__ == "__main__":
    main()
