"""Test-side corpus and second statement of dictionary training (tests/test_train_dict_cpu.py, tests/test_gpu_train_dict.py;
include/zlz4_amd.h; the model: tools/pyref/zig_lz4_train_dict.py).

corpus() -> cases, each a Case(name, samples, C, d, k, f): the smallest shapes at which each kernel can go wrong.

A note on two shapes one might ask for.  Frequencies are never negative, so a window that contains another scores at
least as much, and ties go to the lowest start.  Every window clipped by its epoch's end is contained in the unclipped
window at e - m (where the epoch has one), so a clipped window -- one that starts at the last position of an epoch, or a
segment with S - s < k -- can win only in an epoch shorter than m.  The corpus holds those (nd = 1, 2, m - 1: the epoch is
the whole buffer), and, for the clipping itself, epochs whose richest d-mers lie just behind their end: a score that
looked past e would pick a start there.

train_vec() states the algorithm a third way (the model slides a window, the kernels look up reach flags per window):
reach distances from a sort, then per step every position adds its frequency to the range of window starts that count it,
through a difference array and one cumulative sum."""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import datagen as dg  # noqa: E402
import zig_lz4_train_dict as zt  # noqa: E402

Case = collections.namedtuple("Case", "name samples C d k f")


def split(B, seed, lo=0, hi=300):
    """B cut into samples of lo..hi bytes (empty ones included when lo == 0)"""
    rng = np.random.default_rng(seed)
    out, pos = [], 0
    while pos < len(B):
        n = int(rng.integers(lo, hi + 1))
        out.append(B[pos:pos + n])
        pos += n
    return out


def periodic(period, n, seed):
    unit = bytes(dg.random_bytes(period, seed)) if period > 200 else bytes(range(40, 40 + period))
    return (unit * (n // period + 1))[:n]


def corpus():
    text = bytes(dg.text_bytes(256 << 10, 31))
    cases = []
    add = lambda name, samples, C, d=4, k=16, f=12: cases.append(Case(name, [bytes(s) for s in samples], C, d, k, f))
    for d in (4, 6, 8):                                # S around d: nd = 0, 0, 1, 2
        for S in (0, d - 1, d, d + 1):
            add("S%d_d%d" % (S, d), [text[100:100 + S]], 64, d=d)
    add("no_samples", [], 64)
    add("empty_samples", [b"", b"", b""], 64)
    add("tiny_samples_d8", split(text[:900], 1, 1, 7), 64, d=8)
    add("tiny_samples_d4", split(text[1000:1600], 2, 1, 7), 100)
    add("one_epoch", split(text[2000:2100], 3, 0, 40), 64)                     # nd < 8k
    add("nd_mod_E", split(text[3000:3000 + 8 * 16 * 3 + 7 + 3], 4), 48)        # nd = 391, E = 3, size = 130
    add("epoch_shorter_than_m", [text[4000:4010]], 64)                         # nd = 7 < m: s = 0, seg = S = 10 < k
    add("nd_m_minus_1", [text[4100:4100 + 15]], 64)                            # nd = 12 = m - 1
    add("nd_m", [text[4200:4200 + 16]], 64)
    add("nd_m_plus_1", [text[4300:4300 + 17]], 64)
    # epochs whose richest content lies just behind their end: 4 epochs of 256 positions, in each the 12 positions in
    # front of the next epoch's start are plain, the first 12 of every epoch are the same frequent run
    hot = b"QRSTUVWXYZAB" * 2
    body = bytearray(dg.random_bytes(1027, 5))
    for e in range(1, 4):
        body[256 * e:256 * e + len(hot)] = hot
    add("rich_behind_epoch_end", split(bytes(body), 6), 64)
    base = text[5000:7200]
    for C in (0, 3, 15, 16, 17, 100, 1000):            # C in {0, d - 1, k - 1, k, k + 1, not a multiple of k}
        add("C%d" % C, split(base, 7 + C), C)
    add("C_above_S", [text[7300:7400]], 4096)
    add("all_equal", [b"a" * 400, b"a" * 600], 64)     # every score ties; then E zero steps; L == k
    for d, k in ((4, 16), (6, 64), (8, 1024)):         # the edge of reach: period m - 2 .. m + 1
        m = k - d + 1
        for per in (m - 2, m - 1, m, m + 1):
            add("period%d_d%d_k%d" % (per, d, k), split(periodic(per, 5 * per + 37, per), per, 0, 500), 3 * k + 5, d=d, k=k)
    add("f10_collisions", split(text[8192:8192 + 65536], 8, 0, 3000), 4096, d=6, k=64, f=10)
    # one rich epoch (2) among epochs that the first pick zeroes: 4 epochs of 256, T = 8 steps end the run with tail > 0
    poor = bytearray(periodic(13, 1027, 0))
    poor[520:760] = text[9000:9240]
    add("step_limit", split(bytes(poor), 9), 64)
    for d in (4, 6, 8):
        for k in (16, 64, 1024):
            for j, C in enumerate((2500, k)):
                add("grid_d%d_k%d_C%d" % (d, k, C), split(text[20000 * j + 1000 * d:20000 * j + 1000 * d + 20000], d * k + j, 0, 2000),
                    C, d=d, k=k, f=16)
    add("big_defaults", split(text, 10, 0, 8000), 8192, d=8, k=256, f=20)      # 256 KiB: many tiles, many workgroups
    return cases


def by_params(cases):
    """the cases of one call: d, k and f hold for a whole batch"""
    out = collections.OrderedDict()
    for c in cases:
        out.setdefault((c.d, c.k, c.f), []).append(c)
    return out


_model_cache = {}


def model(case):
    """the model's answer for a corpus case (computed once per process)"""
    if case.name not in _model_cache:
        _model_cache[case.name] = zt.train(case.samples, case.C, case.d, case.k, case.f)
    return _model_cache[case.name]


def reach(h, m):
    """dist[p] = distance to the nearest q < p with h[q] == h[p] where that is <= m - 1, else 0"""
    h = np.asarray(h, dtype=np.int64)
    n = len(h)
    order = np.argsort(h, kind="stable")
    prev = np.full(n, -1, dtype=np.int64)
    same = h[order[1:]] == h[order[:-1]]
    prev[order[1:][same]] = order[:-1][same]
    dist = np.arange(n, dtype=np.int64) - prev
    dist[(prev < 0) | (dist > m - 1)] = 0
    return dist


def train_vec(samples, C, d=8, k=256, f=20):
    if not zt.params_ok(d, k, f):
        return zt.INVALID_STATE
    B = b"".join(bytes(s) for s in samples)
    S = len(B)
    if C > zt.MAX_DICT or S > zt.MAX_GROUP:
        return zt.INVALID_STATE
    nd = S - d + 1
    if nd <= 0 or C == 0:
        return b""
    m = k - d + 1
    h = np.asarray(zt.hashes(B, d, f), dtype=np.int64)
    freq = np.bincount(h, minlength=1 << f).astype(np.int64)
    dist = reach(h, m)
    pos = np.arange(nd, dtype=np.int64)
    nseg, E, size = zt.epochs(nd, C, k)
    out = bytearray(C)
    tail, ep, zero = C, 0, 0
    for _ in range(2 * nseg):
        b = ep * size
        e = nd if ep == E - 1 else b + size
        p = pos[b:e]
        dj = dist[b:e]
        first = np.maximum(np.maximum(p - (m - 1), b), np.where(dj > 0, p - dj + 1, b))    # the starts that count p
        w = freq[h[b:e]]
        diff = np.zeros(e - b + 1, dtype=np.int64)
        np.add.at(diff, first - b, w)
        np.add.at(diff, p - b + 1, -w)
        score = np.cumsum(diff)[:e - b]
        s = b + int(np.argmax(score))
        best = int(score[s - b])
        ep = (ep + 1) % E
        if best == 0:
            zero += 1
            if zero == E:
                break
            continue
        zero = 0
        seg = min(k, tail, S - s)
        tail -= seg
        out[tail:tail + seg] = B[s:s + seg]
        freq[h[s:min(s + m, e)]] = 0
        if tail == 0:
            break
    return bytes(out[tail:C])
