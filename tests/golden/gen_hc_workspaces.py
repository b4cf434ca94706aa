#!/usr/bin/env python3
"""Writes tests/golden/hc_workspaces.json: what the workspace-size functions of the HC pipelines (plain, dictionary, linked
frame blocks) answer for every row of tests/hcwsgrid.py (pure host arithmetic, no GPU needed).

The table pins the sizes across a change of how the chunk rule and the plans are written down, so it is recorded from a
library built from the PARENT of such a change, never from the changed tree itself: the committed table comes from the
library of commit 6994f37, the last one with a chunk rule per pipeline.  Name the library to record from:

  python tests/golden/gen_hc_workspaces.py path/to/parent/libzlz4_amd.so
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import hcwsgrid  # noqa: E402
import zig_lz4_amd as zl  # noqa: E402

OUT = os.path.join(HERE, "hc_workspaces.json")
FUNCS = ("zlz4_batch_compress_hc_workspace", "zlz4_batch_compress_hc_using_dict_workspace",
         "zlz4f_batch_compress_frame_workspace_ex")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    L = C.CDLL(os.path.abspath(sys.argv[1]))
    for fn in FUNCS:
        f = getattr(L, fn)
        f.restype, f.argtypes = zl.SYMBOLS[fn]
    with open(OUT, "w") as f:
        f.write('{"source": "libzlz4_amd.so of commit 6994f37 (the parent of the shared chunk rule)"')
        for kind in hcwsgrid.KINDS:
            sizes = [hcwsgrid.call(zl, L, kind, row) for row in hcwsgrid.rows(kind)]
            f.write(',\n"%s": %s' % (kind, json.dumps(sizes, separators=(",", ":"))))
            print("%s: %d rows" % (kind, len(sizes)))
        f.write("\n}\n")


if __name__ == "__main__":
    main()
