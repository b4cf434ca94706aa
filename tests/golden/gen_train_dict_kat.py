"""Writes tests/golden/train_dict_kat.json: known answers of zlz4_train_dict, computed with
tools/pyref/zig_lz4_train_dict.py.  Run from anywhere: python tests/golden/gen_train_dict_kat.py

Vectors are literal (the samples as hex, the dictionary as hex) or taken from the corpus of tests/traingen.py by name (the
dictionary as its length and SHA-256).  tests/test_train_dict_cpu.py checks the model and the vectorised statement against
the file; the tests on the GPU check the kernels against the model.

The hand trace ("traced": d = 4, k = 16, f = 10, C = 24; the shortest k the parameters allow is 16, so the trace uses it).
B = "abcdefgh" "abcdefgh" "0123" "abcdefgh" "4567" "abcdefgh", S = 40, nd = 37, m = 13, nseg = 2, E = max(1, min(2, 37 /
128)) = 1: one epoch [0, 37), T = 4 steps.  The 4-grams abcd, bcde, cdef, defg, efgh occur 4 times each (at 0, 8, 20, 32 +
0..4); every other 4-gram occurs once; no two different 4-grams of B share a hash value at f = 10 (the file lists h(p) and
the initial freq per position, the test checks this claim).
  step 1  window 0 = positions 0..12: abcd .. efgh once each (5 x 4 = 20; their second occurrences at 8..12 do not count),
          fgha, ghab, habc (1 each): 23.  Window 1 loses abcd at 0 but still holds it at 8, and gains fgh0 at 13: 24.
          Windows 2, 3, 4 gain gh01, h012, 0123: 25, 26, 27.  Window 5 = 5..17 loses efgh at 4, holds it at 12, and gains
          123a: 28, the largest score (windows 6, 7 swap fgha, ghab for 23ab, 3abc: 28 again; window 8 loses habc and
          gains only the repeat abcd at 20: 27).  Ties go to the lowest start: s = 5.  seg = min(16, 24, 35) = 16,
          tail = 8, out[8..24) = B[5..21) = "fghabcdefgh0123a"; the values of positions 5..17 are zeroed: fgha ghab habc
          abcd bcde cdef defg efgh fgh0 gh01 h012 0123 123a.
  step 2  nine values of 1 are left: 23ab, 3abc (18, 19) and fgh4 gh45 h456 4567 567a 67ab 7abc (25..31).  Window 18 =
          18..30 holds 23ab, 3abc and 25..30: 8; window 19 = 19..31 holds 3abc and 25..31: 8; no window holds all nine
          (18..31 are 14 positions).  s = 18.  seg = min(16, 8, 22) = 8, tail = 0, out[0..8) = B[18..26) = "23abcdef": the
          run stops with L = 24.
The dictionary is "23abcdef" ++ "fghabcdefgh0123a".  "traced_C40" is the same buffer with C = 40: after s = 18 has
zeroed positions 18..30 its third step finds only 7abc (31) left and picks the lowest window that holds it, s = 19, with a
score of 1."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import traingen as tg  # noqa: E402
import zig_lz4_train_dict as zt  # noqa: E402

TRACED = [b"abcdefgh", b"abcdefgh0123", b"abcdefgh4567abcd", b"efgh"]     # d-mers straddle the samples
LITERAL = [
    ("traced", TRACED, 24, 4, 16, 10),
    ("traced_C40", TRACED, 40, 4, 16, 10),
    ("shorter_than_d", [b"ab", b"c"], 64, 4, 16, 10),
    ("exactly_d", [b"ab", b"", b"cd"], 64, 4, 16, 10),
    ("all_equal", [b"a" * 300], 64, 4, 16, 10),
    ("C_zero", TRACED, 0, 4, 16, 10),
    ("refused_d", TRACED, 24, 5, 16, 10),
    ("refused_k", TRACED, 24, 4, 8, 10),
    ("refused_f", TRACED, 24, 4, 16, 25),
    ("refused_C", TRACED, 65537, 4, 16, 10),
]
FROM_CORPUS = ["tiny_samples_d8", "nd_mod_E", "rich_behind_epoch_end", "period13_d4_k16", "period59_d6_k64", "step_limit",
               "f10_collisions", "grid_d6_k1024_C2500", "big_defaults"]


def scores(B, d, k, f, freq, b, e):
    """score(s) for every s in [b, e), by the definition (a set per window)"""
    h = zt.hashes(B, d, f)
    m = k - d + 1
    return [sum(freq[x] for x in set(h[s:min(s + m, e)])) for s in range(b, e)]


def traced_vector(name, samples, C, d, k, f):
    B = b"".join(samples)
    h = zt.hashes(B, d, f)
    freq = {}
    for x in h:
        freq[x] = freq.get(x, 0) + 1
    trace = []
    out = zt.train(samples, C, d, k, f, trace=trace)
    steps = []
    m = k - d + 1
    for ep, b, e, score, s, seg, tail in trace:
        steps.append({"epoch": ep, "b": b, "e": e, "scores": scores(B, d, k, f, freq, b, e), "score": score, "s": s,
                      "seg": seg, "tail": tail})
        if score:
            for p in range(s, min(s + m, e)):
                freq[h[p]] = 0
    first = {}
    for x in h:
        first[x] = first.get(x, 0) + 1
    return {"dmers": [B[p:p + d].decode() for p in range(len(h))], "hash": h, "freq": [first[x] for x in h], "steps": steps}


def main():
    vectors = []
    for name, samples, C, d, k, f in LITERAL:
        out = zt.train(samples, C, d, k, f)
        v = {"name": name, "samples": [s.hex() for s in samples], "C": C, "d": d, "k": k, "f": f}
        if isinstance(out, int):
            v["result"] = out
        else:
            v["result"] = len(out)
            v["out"] = out.hex()
        if name.startswith("traced"):
            v["trace"] = traced_vector(name, samples, C, d, k, f)
        vectors.append(v)
    by = {c.name: c for c in tg.corpus()}
    for name in FROM_CORPUS:
        c = by[name]
        out = zt.train(c.samples, c.C, c.d, c.k, c.f)
        vectors.append({"name": name, "corpus": name, "C": c.C, "d": c.d, "k": c.k, "f": c.f, "result": len(out),
                        "samples_sha256": hashlib.sha256(b"\0".join(c.samples)).hexdigest(),
                        "sha256": hashlib.sha256(out).hexdigest()})
    with open(os.path.join(HERE, "train_dict_kat.json"), "w") as fh:
        json.dump({"vectors": vectors}, fh, indent=1)
        fh.write("\n")
    print("%d vectors" % len(vectors))


if __name__ == "__main__":
    main()
