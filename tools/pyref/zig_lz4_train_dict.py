"""Model of zlz4_train_dict / zlz4_batch_train_dict (include/zlz4_amd.h): the fastCover-style
dictionary selection, written the other way from the kernels.  The kernels decide "each distinct hash value counts once per
window" with reach flags computed once (csrc/zlz4_train_dict.hip); this model slides a literal window with a count per
hash value: the entering d-mer is added, the leaving one is dropped, and a value's frequency is part of the score while
its count is positive.  Integers only, so the two agree byte for byte.

train(samples, C, d, k, f) -> the dictionary (bytes), or a negative code.  `trace`, when given a list, receives one tuple
per step: (epoch, b, e, score, s, seg, tail after the step)."""
import numpy as np

INVALID_STATE = -5
PRIME = 0xCF1BBCDCB7A56463
MAX_DICT = 65536
MAX_GROUP = 1 << 27


def params_ok(d, k, f):
    return d in (4, 6, 8) and 16 <= k <= 1024 and k >= d and 10 <= f <= 24


def hashes(B, d, f):
    """h(p) for every p in [0, len(B) - d + 1) as a list of ints"""
    nd = len(B) - d + 1
    if nd <= 0:
        return []
    a = np.frombuffer(bytes(B), dtype=np.uint8).astype(np.uint64)
    v = np.zeros(nd, dtype=np.uint64)
    for j in range(d):
        v |= a[j:j + nd] << np.uint64(8 * j)
    with np.errstate(over="ignore"):
        h = ((v << np.uint64(64 - 8 * d)) * np.uint64(PRIME)) >> np.uint64(64 - f)
    return h.tolist()


def epochs(nd, C, k):
    """-> (nseg, E, size)"""
    nseg = (C + k - 1) // k
    E = max(1, min(nseg, nd // (8 * k)))
    return nseg, E, nd // E


def train(samples, C, d=8, k=256, f=20, trace=None):
    if not params_ok(d, k, f):
        return INVALID_STATE
    B = b"".join(bytes(s) for s in samples)
    S = len(B)
    if C > MAX_DICT or S > MAX_GROUP:
        return INVALID_STATE
    nd = S - d + 1
    if nd <= 0 or C == 0:
        return b""
    m = k - d + 1
    h = hashes(B, d, f)
    freq = {}
    for x in h:
        freq[x] = freq.get(x, 0) + 1
    nseg, E, size = epochs(nd, C, k)
    out = bytearray(C)
    tail, ep, zero = C, 0, 0
    for _ in range(2 * nseg):
        b = ep * size
        e = nd if ep == E - 1 else b + size
        cnt = {}
        score = 0
        for p in range(b, min(b + m, e)):             # the window at s = b
            x = h[p]
            c = cnt.get(x, 0)
            if c == 0:
                score += freq[x]
            cnt[x] = c + 1
        best, best_s = -1, b
        for s in range(b, e):
            if score > best:                          # ties go to the lowest s
                best, best_s = score, s
            x = h[s]                                  # s leaves
            c = cnt[x] - 1
            cnt[x] = c
            if c == 0:
                score -= freq[x]
            p = s + m                                 # s + m enters
            if p < e:
                x = h[p]
                c = cnt.get(x, 0)
                if c == 0:
                    score += freq[x]
                cnt[x] = c + 1
        this_ep = ep
        ep = (ep + 1) % E
        if best == 0:
            zero += 1
            if trace is not None:
                trace.append((this_ep, b, e, 0, best_s, 0, tail))
            if zero == E:
                break
            continue
        zero = 0
        s = best_s
        seg = min(k, tail, S - s)
        tail -= seg
        out[tail:tail + seg] = B[s:s + seg]
        for p in range(s, min(s + m, e)):
            freq[h[p]] = 0
        if trace is not None:
            trace.append((this_ep, b, e, best, s, seg, tail))
        if tail == 0:
            break
    return bytes(out[tail:C])
