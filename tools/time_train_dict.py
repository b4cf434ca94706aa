#!/usr/bin/env python3
"""Time dictionary training (zlz4_batch_train_dict) with HIP events and write
profiles/r38_train_dict.md.

  one    one dictionary: 16 384 x 4 KiB D-text records (64 MiB) in one group, C = 64 KiB, d = 8, k = 256, f = 20: the whole
         call, the steps that ran, and beside it the fast dictionary compress of the same records with the result
  many   1 024 groups of 256 KiB (64 records each), C = 16 KiB, in one call, against one such group alone: what batching
         buys over the serial steps
  sizes  compressed sizes of held-out records without a dictionary, with the last C bytes of the samples and with the trained
         dictionary, at the fast level and at HC 9 (device streams), and the small set-up of tests/test_train_dict_cpu.py
         through the CPU model

The time per phase (pack, count, reach, steps, finish) comes from a kernel trace of one call, taken in a run of its own and
handed to a second invocation, which writes the profile:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/time_train_dict.py --once one
  python tools/time_train_dict.py --stats one=DIR [--stats many=DIR2] --out profiles/r38_train_dict.md

  python tools/time_train_dict.py [--once one|many] [--stats NAME=DIR ...] [--scale K] [--out FILE]
"""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import numpy as np
import torch

import datagen as dg
import zig_lz4_amd as zl
import zig_lz4_dict_compress as zc
import zig_lz4_train_dict as zt

dev = torch.device("cuda:0")
REC = 4096
PHASES = (("pack", ("k_train_sum", "k_train_plan", "k_train_pack")), ("count", ("k_train_count",)),
          ("reach", ("k_train_reach",)), ("steps: score", ("k_train_score",)), ("steps: commit", ("k_train_commit",)),
          ("finish", ("k_train_finish",)))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def spread(ts):
    t = sorted(ts)
    return "best %.2f ms, median %.2f ms (%s)" % (t[0], t[len(t) // 2], " ".join("%.2f" % x for x in ts))


class Job:
    """ngroups groups of `per` records of REC bytes from `data` (a device tensor), one capacity for all"""

    def __init__(self, data, ngroups, per, cap, d=8, k=256, f=20):
        n = ngroups * per
        self.data, self.ngroups, self.cap, self.p = data, ngroups, cap, (d, k, f)
        self.off = torch.arange(n, dtype=torch.int64, device=dev) * REC
        self.len = torch.full((n,), REC, dtype=torch.int32, device=dev)
        self.first = (torch.arange(ngroups + 1, dtype=torch.int64, device=dev) * per).to(torch.int32)
        self.dict = torch.empty(ngroups * cap, dtype=torch.uint8, device=dev)
        self.dict_off = torch.arange(ngroups, dtype=torch.int64, device=dev) * cap
        self.dict_cap = torch.full((ngroups,), cap, dtype=torch.int32, device=dev)
        self.res = torch.empty(ngroups, dtype=torch.int64, device=dev)
        self.ws = torch.empty(zl.batch_train_dict_workspace(ngroups, n * REC, cap, d, k, f), dtype=torch.uint8, device=dev)
        self.steps = 2 * ((cap + k - 1) // k)

    def run(self):
        zl.batch_train_dict(self.data, self.off, self.len, self.first, self.dict, self.dict_off, self.dict_cap, self.res,
                            self.cap, self.ws, *self.p)

    def steps_run(self):
        """steps that ran per group: the launch count less the steps_left word of the group records at the front of the
        workspace (csrc/zlz4_train_dict.hip, TrainGroup: 64 bytes, steps_left at byte 36)"""
        g = self.ws[:64 * self.ngroups].cpu().numpy().view(np.uint32).reshape(self.ngroups, 16)
        return self.steps - g[:, 9].astype(np.int64)

    def dicts(self):
        r = self.res.cpu().tolist()
        h = self.dict.cpu().numpy()
        return [bytes(h[i * self.cap: i * self.cap + max(n, 0)]) for i, n in enumerate(r)]


def text(nbytes, seed):
    return torch.from_numpy(dg.text_bytes(nbytes, seed)).to(dev)


def compress_sizes(records, dicts):
    """{name: (fast total, HC 9 total)} with the device's streams"""
    out = {}
    for name, d in dicts:
        fast = zl.compressBlocksUsingDict(records, [d], [0] * len(records), device=dev)
        hc = zl.compressBlocksHCUsingDict(records, [d], [0] * len(records), level=9, device=dev)
        out[name] = (sum(map(len, fast)), sum(map(len, hc)))
    return out


def fast_dict_compress_time(data, nrec, d, rounds):
    dt = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).to(dev)
    doff = torch.zeros(1, dtype=torch.int64, device=dev)
    dlen = torch.tensor([len(d)], dtype=torch.int32, device=dev)
    tabs = torch.empty(4096, dtype=torch.int32, device=dev)
    lres = torch.empty(1, dtype=torch.int64, device=dev)
    slot = (zl.compressBound(REC) + 15) // 16 * 16
    ar = torch.arange(nrec, dtype=torch.int64, device=dev)
    out = torch.empty(nrec * slot, dtype=torch.uint8, device=dev)
    cap = torch.full((nrec,), slot, dtype=torch.int32, device=dev)
    res = torch.empty(nrec, dtype=torch.int64, device=dev)
    ln = torch.full((nrec,), REC, dtype=torch.int32, device=dev)
    idx = torch.zeros(nrec, dtype=torch.int32, device=dev)
    zeros = torch.zeros(nrec, dtype=torch.int64, device=dev)
    dl = dlen.expand(nrec).contiguous()

    def call():
        zl.batch_load_dict(dt, doff, dlen, tabs, lres)
        zl.batch_compress_fast_using_dict(data, ar * REC, ln, out, ar * slot, cap, dt, zeros, dl, tabs, idx, res, REC, len(d), 1)
    call()
    torch.cuda.synchronize()
    ts = [timed(call) for _ in range(rounds)]
    assert int((res <= 0).sum()) == 0
    return ts, int(res.sum())


def kernel_phases(directory):
    """{phase: (launches, total ms)} from the kernel_stats CSV of a rocprofv3 run under `directory`"""
    f = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    out = []
    for phase, names in PHASES:
        hit = [r for r in rows if any(n + "(" in r["Name"] for n in names)]
        out.append((phase, sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit) / 1e6))
    memset = [r for r in rows if "fill" in r["Name"].lower() or "memset" in r["Name"].lower()]
    out.append(("(table clear, where it shows as a kernel)", sum(int(r["Calls"]) for r in memset),
                sum(float(r["TotalDurationNs"]) for r in memset) / 1e6))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", default="", help="one|many: one training call and nothing else (for a kernel trace)")
    ap.add_argument("--stats", action="append", default=[], help="NAME=DIR of a rocprofv3 --kernel-trace --stats run of --once NAME")
    ap.add_argument("--scale", type=int, default=1, help="divide the number of records by this")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r38_train_dict.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available() and zl.device_available(), "needs a gfx950 device"
    n_one = 16384 // a.scale
    n_groups, per = 1024 // a.scale, 64
    pool = text(n_one * REC, 11)                       # 64 MiB of distinct D-text

    if a.once:
        if a.once == "one":
            job = Job(pool, 1, n_one, 65536)
        else:
            reps = (n_groups * per + n_one - 1) // n_one
            job = Job(pool.repeat(reps)[:n_groups * per * REC].contiguous(), n_groups, per, 16384)
        job.run()
        torch.cuda.synchronize()
        return

    L = []
    say = lambda s="": (L.append(s), print(s))
    say("# Dictionary training on the device (zlz4_batch_train_dict): times and sizes")
    say()
    say("Written by `tools/time_train_dict.py` on %s.  Every time and every size in sections 1 to 3 is from the device (HIP"
        % torch.cuda.get_device_name(0))
    say("events around whole calls, %d rounds after a warm-up call; per-kernel times from a rocprofv3 kernel trace of one call in"
        % a.rounds)
    say("a run of its own).  Section 4 is from the CPU model (`tools/pyref/zig_lz4_train_dict.py`,")
    say("`tools/pyref/zig_lz4_dict_compress.py`) and says so.  Nothing here is compared against a threshold: there is no")
    say("earlier trainer to compare a time with.")
    say()

    # ---- 1. one dictionary
    job = Job(pool, 1, n_one, 65536)
    job.run()
    torch.cuda.synchronize()
    ts = [timed(job.run) for _ in range(a.rounds)]
    ran = int(job.steps_run()[0])
    trained = job.dicts()[0]
    mib = n_one * REC / 2**20
    say("## 1. One dictionary: %d x 4 KiB D-text records (%.0f MiB), C = 64 KiB, d = 8, k = 256, f = 20" % (n_one, mib))
    say()
    say("- whole call: %s; %.2f GiB/s of samples" % (spread(ts), mib / 1024 / min(ts) * 1e3))
    say("- dictionary: %d bytes; %d of the %d step pairs launched did work (the rest returned at once)" % (len(trained), ran, job.steps))
    say("- workspace: %.2f GiB" % (job.ws.numel() / 2**30))
    fts, ftotal = fast_dict_compress_time(pool, n_one, trained, a.rounds)
    say("- beside it, loadDict + compressFastUsingDict of the same %d records against the trained dictionary: %s; ratio %.3f"
        % (n_one, spread(fts), n_one * REC / ftotal))
    say("- training costs %.1f x one fast dictionary compress of its own samples" % (min(ts) / min(fts)))
    say()
    one_time = min(ts)
    del job
    torch.cuda.empty_cache()

    # ---- 2. many dictionaries
    reps = (n_groups * per + n_one - 1) // n_one
    data = pool.repeat(reps)[:n_groups * per * REC].contiguous()
    many = Job(data, n_groups, per, 16384)
    many.run()
    torch.cuda.synchronize()
    tm = [timed(many.run) for _ in range(a.rounds)]
    single = Job(data, 1, per, 16384)
    single.run()
    torch.cuda.synchronize()
    tsg = [timed(single.run) for _ in range(a.rounds)]
    assert many.dicts()[0] == single.dicts()[0], "a group's answer alone differs from its answer in the batch"
    ran_many = many.steps_run()
    say("## 2. Many dictionaries: %d groups of 256 KiB (64 records each), C = 16 KiB, one call" % n_groups)
    say()
    say("- the batch: %s; %.3f ms per dictionary; %.2f GiB/s of samples" % (spread(tm), min(tm) / n_groups,
                                                                          n_groups * per * REC / 2**30 / min(tm) * 1e3))
    say("- one such group alone: %s" % spread(tsg))
    say("- batching: %d dictionaries in %.1f x the time of one (%.0f x faster than one call per group)"
        % (n_groups, min(tm) / min(tsg), n_groups * min(tsg) / min(tm)))
    say("- step pairs that did work per group: min %d, max %d of %d launched" % (ran_many.min(), ran_many.max(), many.steps))
    say("- workspace: %.2f GiB (%.1f MiB of it per group for the 2^20 counters)" % (many.ws.numel() / 2**30, 4.0))
    fts2, ftotal2 = fast_dict_compress_time(data, n_groups * per, many.dicts()[0], a.rounds)
    say("- beside it, loadDict + compressFastUsingDict of the same %d records against one dictionary: %s"
        % (n_groups * per, spread(fts2)))
    say("- training all groups costs %.1f x one fast dictionary compress of the same bytes" % (min(tm) / min(fts2)))
    say()
    del many, single, data
    torch.cuda.empty_cache()

    # ---- per-kernel times
    for item in a.stats:
        name, directory = item.split("=", 1)
        say("### Time per phase of one call (%s), rocprofv3 kernel trace" % name)
        say()
        say("| phase | launches | total ms |")
        say("|---|---|---|")
        tot = 0.0
        for phase, calls, ms in kernel_phases(directory):
            say("| %s | %d | %.3f |" % (phase, calls, ms))
            tot += ms
        say("| sum of kernel time | | %.3f |" % tot)
        say()

    # ---- 3. sizes on the device
    held_np = dg.text_bytes(1024 * REC, 12)
    held = [bytes(held_np[i:i + REC]) for i in range(0, len(held_np), REC)]
    samples_host = pool.cpu().numpy()
    say("## 3. Compressed sizes of 1 024 held-out 4 KiB D-text records (4 MiB), device streams")
    say()
    say("| dictionary | fast | HC 9 |")
    say("|---|---|---|")
    naive = bytes(samples_host[-65536:])
    for name, (fs, hs) in compress_sizes(held, [("none", b""), ("naive: the last 64 KiB of the samples", naive),
                                                 ("trained: 64 KiB, d 8, k 256 (section 1)", trained)]).items():
        say("| %s | %d | %d |" % (name, fs, hs))
    say()
    small = [bytes(samples_host[i:i + REC]) for i in range(0, 256 << 10, REC)]
    held1k = [bytes(held_np[i:i + 1024]) for i in range(0, 64 << 10, 1024)]
    say("The set-up of the tests (256 KiB of samples, 64 held-out 1 KiB records), trained on the device:")
    say()
    say("| dictionary | d | k | fast: none | naive | trained | HC 9: none | naive | trained |")
    say("|---|---|---|---|---|---|---|---|---|")
    for cap, d, k in ((4096, 6, 64), (16384, 6, 64), (65536, 8, 256)):
        t = zl.trainDicts([small], cap, d, k, 20, device=dev)[0]
        nv = bytes(samples_host[(256 << 10) - cap:256 << 10])
        s = compress_sizes(held1k, [("none", b""), ("naive", nv), ("trained", t)])
        say("| %d KiB | %d | %d | %d | %d | %d | %d | %d | %d |" % (cap // 1024, d, k, s["none"][0], s["naive"][0], s["trained"][0],
                                                                   s["none"][1], s["naive"][1], s["trained"][1]))
    say()

    # ---- 4. the CPU model
    t = zt.train(small, 4096, 6, 64, 20)
    tot = lambda d: sum(zc.compress_fast_using_dict(r, d)[0] for r in held1k)
    say("## 4. From the CPU model, not from the device")
    say()
    say("The 4 KiB row above through `zig_lz4_train_dict.train` and the pyref model of compressFastUsingDict: none %d, naive %d,"
        % (tot(b""), tot(bytes(samples_host[(256 << 10) - 4096:256 << 10]))))
    say("trained %d.  The device's dictionary equals the model's: %s." % (tot(t), zl.trainDicts([small], 4096, 6, 64, 20, device=dev)[0] == t))
    say()

    # ---- reading (the figures are those of the run that profiles/r38_train_dict.md records)
    say("## Reading")
    say()
    say('One dictionary is bound by its serial steps.  Of the 43.1 ms of kernel time of one call, 29.1 ms are the 512 `k_train_score`')
    say('launches and 2.0 ms the commits; pack, count and reach, the three streaming passes over the 64 MiB, take 12.0 ms together.')
    say('Half of the step pairs find the group done and return at once (the dictionary is full after 256 picks; T = 2 * nseg leaves')
    say('room for zero-score steps).  A score launch that works holds one epoch, 256 Ki window starts here: 256 workgroups of 256')
    say('lanes, four waves per CU, each lane summing four windows of 249 terms one after the other, about 110 us.  The epoch is too')
    say('small to fill the device, so the follow-up is more lanes per step (one lane per window start, in larger workgroups) and')
    say('fewer, larger steps (several epochs scored per launch: the epochs of one round are independent until a pick zeroes a hash')
    say('value that another epoch holds).  Neither is done here, and neither is graph capture or a persistent kernel.')
    say('Many dictionaries hide the serial part: every launch carries all groups, 1 024 dictionaries take 14.2 x the time of one,')
    say('and the score launches (65.6 of 105.8 ms) run with 4 096 workgroups each.  There reach (28.1 ms: brute force, up to 248')
    say('look-backs per position) and count (10.3 ms: one integer atomic add per position, no combining of equal hash values inside a')
    say('wave) are the next third of the time.')
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
