"""Writes tests/golden/hc_dict_kat.json: known answers of zlz4_compress_hc_using_dict, computed
with tools/pyref/zig_lz4_hc_dict.py.  Run from anywhere: python tests/golden/gen_hc_dict_kat.py

Vectors are either literal (dict / src as hex, the whole output as hex) or generated (tests/datagen.py generator, seed,
lengths; the output as its length and SHA-256).  tests/test_hc_dict_cpu.py checks both restatements against the file,
tests on the GPU check the kernels against the C restatement.

Hand traces against the specification (positions are positions in V = dict ++ src, D = len(dict), N = D + n; mflimit =
N - 12, matchlimit = N - 5; a search at ip first inserts every position below ip; chain[q] = q - previous position with
q's hash, = q when there is none (the empty table reads 0); a level L has A = 1 << (L - 1) attempts):

 thirteen_bytes    dict "0123456789ABCDEF", src "3456789ABCDEF" (n = 13, the shortest record that is parsed): D = 16,
                   N = 29, mflimit = 17, matchlimit = 24.  ip 16: positions 0 .. 15 go in (the 4-grams at 13, 14, 15 read
                   into the record).  "3456": the table holds 3.  Candidate 3: distance 13, four bytes equal, lz4Count
                   from 20 / 7: "789A" equal, then ip + 8 = matchlimit: mlt = 8 > 3: best (8, offset 13); level 3 leaves
                   here (8 > 4, :613), level 9 follows chain[3] = 3: m = 0, the walk ends.  Sequence: 0 literals,
                   ml code 4: token 04, offset 0d 00.  ip = 24 > mflimit.  Last literals V[24..29) = "BCDEF": token 50.
                   -> 04 0d00 50 4243444546 (9 bytes against 14 without the dictionary), at every level.
 v_pos_0           dict "WXYZ0123456789AB", src "qrsWXYZtuvwxyz!?": the only earlier "WXYZ" is at position 0 of V.
                   ip 19 "WXYZ": the table holds 0, which reads as empty (:566): no match anywhere, 16 literals:
                   token f0, 01, the record -> 18 bytes.
 v_pos_1           dict "_WXYZ0123456789A", the same record: the table holds 1.  ip 19: candidate 1, distance 18, four
                   bytes equal, V[23] = 't' != V[5] = '0': mlt = 4; chain[1] = 1: m = 0.  Sequence: 3 literals "qrs",
                   ml code 0: token 30, "qrs", 12 00.  ip = 23 > mflimit = 20.  Last literals "tuvwxyz!?" (9): token 90.
                   -> 30 717273 1200 90 7475767778797a213f (16 bytes).
 attempt_budget    tests/hcdictcgen.py traced(): D = 67, "QRST" at 7 (followed by the long string), at 60 (the dictionary's
                   end) and in the record at D + 0, 7, 14, 21, each followed by other bytes, then "QRSTlong-match-in-dict!"
                   at D + 28.  The first four record occurrences each find the nearest earlier one: 4 bytes, offset 7.
                   ip D + 28: the chain is D + 21, D + 14, D + 7, D + 0, 60, 7.  Level 3: four attempts, four candidates
                   of 4 bytes (4 > 4 is false: no early exit), the walk stops with (4, offset 7) before it reaches 60 and
                   7; the parse goes on at D + 32 "long", finds 11 in the dictionary: 19 bytes, offset 88 -> 48 bytes.
                   Level 4 and up: the sixth candidate, 7, matches all 23 bytes: (23, offset 88) -> 45 bytes.
 pattern_into_tail tests/hcdictcgen.py traced(): the level-9 pattern step whose reverse count runs from the record down
                   through the tail and puts a 350-byte match at offset 351, 50 bytes inside the tail; level 8 stops at
                   129 bytes, offset 130.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import datagen as dg  # noqa: E402
import hcdictcgen as hg  # noqa: E402
import zig_lz4_hc_dict as zh  # noqa: E402

DICT = b"0123456789ABCDEF"
REC = b"qrsWXYZtuvwxyz!?"
TRACED = {name: (d, r) for name, d, r, _ in hg.traced()}
LITERAL = [
    ("thirteen_bytes", DICT, b"3456789ABCDEF", 3, None),
    ("thirteen_bytes_l9", DICT, b"3456789ABCDEF", 9, None),
    ("v_pos_0", b"WXYZ0123456789AB", REC, 9, None),
    ("v_pos_1", b"_WXYZ0123456789A", REC, 9, None),
    ("attempt_budget_l3", *TRACED["attempt_budget"], 3, None),
    ("attempt_budget_l4", *TRACED["attempt_budget"], 4, None),
    ("pattern_into_tail_l9", *TRACED["pattern_into_tail"], 9, None),
    ("pattern_into_tail_l8", *TRACED["pattern_into_tail"], 8, None),
    ("twelve_bytes", DICT, b"456789ABCDEF", 9, None),
    ("empty_record", DICT, b"", 9, None),
    ("empty_dict", b"", b"abcdabcdabcdabcdabcd", 9, None),
    ("level_1_is_9", DICT, b"3456789ABCDEF", 1, None),
    ("level_2_unsupported", DICT, b"3456789ABCDEF", 2, None),
    ("level_10_unsupported", DICT, b"3456789ABCDEF", 10, None),
    ("level_13_is_12_unsupported", DICT, b"", 13, None),
    ("cap_exact", DICT, b"3456789ABCDEF", 9, 9),
    ("cap_one_short", DICT, b"3456789ABCDEF", 9, 8),
    ("cap_zero", DICT, b"3456789ABCDEF", 9, 0),
    ("cap_sequence_check", b"_WXYZ0123456789A", REC, 9, 10),
    ("spans_dict_end", DICT, b"BCDEFBCDEFBCDEFqrstuvwx", 6, None),
    ("one_byte_dict", b"a" * 9, b"a" * 40 + b"qrstuvwx", 9, None),
]
GENERATED = [(g, seed, dl, n, lv) for g, seed in (("text", 1), ("reptext", 2), ("mixed", 3), ("random", 4))
             for dl, n, lv in ((0, 1000, 9), (100, 37, 3), (4096, 4096, 6), (65536, 4096, 9), (70000, 1000, 4))]


def generated(gen, seed, dl, n):
    """dictionary = the dl bytes in front of position 70000 of the generator's stream, record = the n bytes after it"""
    s = bytes(getattr(dg, gen + "_bytes")(70000 + n, seed))
    return s[70000 - dl:70000], s[70000:]


def _result(out):
    return (out, b"") if isinstance(out, int) else (len(out), out)


def main():
    vectors = []
    for name, d, src, level, cap in LITERAL:
        r, out = _result(zh.compress_hc_using_dict(src, d, level, cap))
        vectors.append({"name": name, "dict": d.hex(), "src": src.hex(), "level": level, "dst_cap": cap, "result": r,
                        "out": out.hex()})
    for gen, seed, dl, n, level in GENERATED:
        d, src = generated(gen, seed, dl, n)
        r, out = _result(zh.compress_hc_using_dict(src, d, level))
        vectors.append({"name": "%s_d%d_n%d_l%d" % (gen, dl, n, level), "gen": gen, "seed": seed, "dict_len": dl, "n": n,
                        "level": level, "dst_cap": None, "result": r, "sha256": hashlib.sha256(out).hexdigest()})
    with open(os.path.join(HERE, "hc_dict_kat.json"), "w") as f:
        json.dump({"what": "zlz4_compress_hc_using_dict known answers (gen_hc_dict_kat.py)", "vectors": vectors}, f, indent=1)
        f.write("\n")
    print("%d vectors" % len(vectors))


if __name__ == "__main__":
    main()
