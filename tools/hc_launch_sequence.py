#!/usr/bin/env python3
"""What the HC launchers enqueue, as a kernel trace can see it: evidence for a change of their host code.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/hc_launch_sequence.py run
      one plain level-9 call of 5 blocks, one level-11 call of 5 blocks, one dictionary level-9 call of 5 records and one
      linked level-9 frame batch of 5 table entries (three rounds each: both halves, half 0 twice), on the library
      ZLZ4_AMD_LIB names (default: the tree's)
  python tools/hc_launch_sequence.py list TRACE.csv
      the ordered list of (kernel, grid, workgroup, LDS bytes, queue) of that run; queues are numbered in order of
      appearance, names are cut at the argument list
  python tools/hc_launch_sequence.py compare A.csv B.csv
      both lists side by side where they differ; exit status 1 if they do
"""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run():
    import torch
    import datagen as dg
    import gpu_harness as gh
    import hcdictcgen as hg
    import hcrounds
    import test_gpu_linked_frame_hc as tlf
    import zig_lz4_amd as zl
    dev = torch.device("cuda:0")
    items = hcrounds.boundary_blocks(5, 2, 4105)
    for level in (9, 11):
        got = gh.compress_hc(zl, items, dev, level)
        print("plain level %d:" % level, [n for n, _ in got])
    dicts = [bytes(dg.reptext_bytes(300, 4300 + i)) + r[:len(r) // 2] + b"xyz" for i, r in enumerate(items)]

    class NoRef:                                      # run_batch wants a restatement; the bytes are the tests' business
        def batch(self, buf, offs, lens, caps, *a):
            return 0, [0] * len(lens), [b""] * len(lens)
    got, _ = hg.run_batch(zl, NoRef(), items, [hg.bound(len(r)) for r in items], dicts, list(range(5)), dev, 9)
    print("dictionary level 9:", [n for n, _ in got])
    frames = hcrounds.boundary_blocks(5, 2, 4405, empty=False)
    text = bytes(dg.text_bytes(65536, 4505))
    frames[3:] = [text + text[1000:1000 + len(frames[4])]]
    rc, res, _, _ = tlf._compress_ex(zl, dev, frames, tlf._prefs(zl.Prefs, compression_level=9), zl.lz4f.BATCH_LINK_BLOCKS,
                                     max_blocks=5)
    print("linked level 9:", rc, res)


def launches(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    queues, out = {}, []
    for r in rows:
        q = queues.setdefault(r["Queue_Id"], len(queues))
        name = r["Kernel_Name"].split("(")[0].replace(" [clone .kd]", "").replace(".kd", "")
        grid = "x".join(r["Grid_Size_" + a] for a in "XYZ")
        wg = "x".join(r["Workgroup_Size_" + a] for a in "XYZ")
        out.append((name, grid, wg, r.get("LDS_Block_Size", r.get("LDS_Block_Size_v", "?")), "q%d" % q))
    return out


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "run":
        run()
    elif mode == "list" and len(sys.argv) == 3:
        for t in launches(sys.argv[2]):
            print("  ".join(t))
    elif mode == "compare" and len(sys.argv) == 4:
        a, b = launches(sys.argv[2]), launches(sys.argv[3])
        diff = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
        print("%d launches in the first list, %d in the second, %d positions differ" % (len(a), len(b), len(diff)))
        for i, x, y in diff[:40]:
            print("  #%d: %s | %s" % (i, "  ".join(x), "  ".join(y)))
        sys.exit(1 if diff or len(a) != len(b) else 0)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
