#!/usr/bin/env python3
"""Check the model of the wave decoder's grouping (tests/seqgen.py model()) against the kernel, once per build.

Runs the -DZLZ4_STAMPS library (`make stamps`) on a corpus in ONE batch call per build of k_decompress_safe -- the
tuning knobs pick the build, each in a child process since the launcher reads them once -- and prints the kernel's
event counters (g_zlz4_dstamps slots 8, 9, 11, 12, 13, 14) beside the model's totals for the same streams.

  python tools/decoder_census.py [crafted|old]

crafted = tests/seqgen.py corpus(); old = the 7000-block batch of tests/test_gpu_shipped_paths.py (streams of this
project's compressors, damaged and capacity-cut), to show what one of the earlier decode tests reached.  Exit status 1
when a counter differs from the model.
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seqgen as sg  # noqa: E402

STAMPS = os.path.join(ROOT, "zig-lz4_amd", "libzlz4_amd_stamps.so")
# (label, tuning knobs, model parameters)
BUILDS = [
    ("<true,true> lane copy + phases", dict(ZLZ4_DECOMP_SHORT="32"), dict(lane_copy=True, phases=True)),
    ("<true,false> sequence lane", dict(ZLZ4_DECOMP_SHORT="0"), dict(lane_copy=False, phases=False)),
    ("<true,true,false> PHASES=0", dict(ZLZ4_DECOMP_SHORT="32", ZLZ4_DECOMP_PHASES="0"), dict(lane_copy=True, phases=False)),
    ("<true,true> PHASE_MIN=1", dict(ZLZ4_DECOMP_SHORT="32", ZLZ4_DECOMP_PHASE_MIN="1"),
     dict(lane_copy=True, phases=True, min_phase_tokens=1)),
]
SLOTS = [(8, "batches"), (9, "batch_seqs"), (11, "single_seqs"), (12, "later_phases"), (13, "cap_cuts"), (14, "phase_limit")]


def streams(which):
    if which == "crafted":
        return [(it.src, it.cap) for it in sg.corpus()]
    from oracle import binding
    from test_gpu_shipped_paths import large_batch_blocks
    binding.lib()
    _, comp, caps = large_batch_blocks(binding)
    return list(zip(comp, caps))


def child(which):
    """one batch call of the stamps library (the build chosen by the environment) -> the 16 counters as JSON"""
    import torch
    import zig_lz4_amd as zl
    import gpu_harness as gh
    items = streams(which)
    dev = torch.device("cuda:0")
    L = zl.lib()
    L.zlz4_debug_read_dstamps.argtypes = [C.c_void_p, C.c_int]
    buf = (C.c_ulonglong * 16)()
    assert L.zlz4_debug_read_dstamps(buf, 1) == 0
    got = gh.decompress(zl, [s for s, _ in items], [c for _, c in items], dev)
    assert L.zlz4_debug_read_dstamps(buf, 0) == 0
    print(json.dumps({"n": len(items), "slots": list(buf), "results": [n for n, _ in got]}))


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "crafted"
    if len(sys.argv) > 2 and sys.argv[2] == "--child":
        return child(which)
    assert os.path.exists(STAMPS), "make stamps"
    items = streams(which)
    print("corpus %s: %d streams, %d bytes" % (which, len(items), sum(len(s) for s, _ in items)))
    ok = True
    for label, knobs, kw in BUILDS:
        env = dict(os.environ, ZLZ4_AMD_LIB=STAMPS, **knobs)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), which, "--child"], env=env, capture_output=True,
                           text=True, timeout=600)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:])
            return 2
        k = json.loads(r.stdout.strip().splitlines()[-1])
        tot, results = sg.Counts(), []
        for src, cap in items:
            res, c = sg.model(src, cap, **kw)
            tot.add(c)
            results.append(res)
        same_results = results == k["results"]
        print("\n%s  (%s)  results equal the model's: %s" % (label, " ".join("%s=%s" % kv for kv in knobs.items()),
                                                             same_results))
        print("  %-4s %-14s %12s %12s" % ("slot", "counter", "kernel", "model"))
        for slot, f in SLOTS:
            kv, mv = k["slots"][slot], getattr(tot, f)
            print("  %-4d %-14s %12d %12d%s" % (slot, f, kv, mv, "" if kv == mv else "   <-- differs"))
            ok = ok and kv == mv
        print("  (model only: room-cut walks %d, batches with >= 3 phases %d)" % (tot.room_cuts, tot.phases3))
        ok = ok and same_results
    print("\nall counters equal: %s" % ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
