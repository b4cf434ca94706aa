"""Writes tests/golden/dict_compress_kat.json: known answers of zlz4_compress_fast_using_dict,
computed with tools/pyref/zig_lz4_dict_compress.py.  Run from anywhere: python tests/golden/gen_dict_compress_kat.py

Vectors are either literal (dict / src as hex, the whole output as hex) or generated (tests/datagen.py generator, seed,
lengths; the output as its length and SHA-256).  tests/test_dict_compress_cpu.py checks both restatements against the
file, tests on the GPU check the kernel against the C restatement.

Four of the literal vectors, traced by hand against the specification (positions are positions in V = dict ++ src,
D = len(dict); with DICT = "0123456789ABCDEF", D = 16, Stream.loadDict hashes the 4-grams at 0 .. D - 5 = 11: "0123" is
stored as position 0 = empty, "1234" -> 1, ..., "BCDE" -> 11; the 4-grams at 12 .. 15 are not in the table):

 empty_dict        dict "", src "abcdabcdabcdabcdabcd" (n = 20): D = 0, anchor = 0, ip = 1, L = 8, matchLimit = 15.
                   ip 1 "bcda", 2 "cdab", 3 "dabc", 4 "abcd": empty slots (position 0 was never put), each put.
                   ip 5 "bcda": match = 1, 1 < 5, same bytes -> sequence: 5 literals "abcda", offset 5 - 1 = 4,
                   extension from ip 9 / match 5: V[9..14] == V[5..10], stops at matchLimit 15: ml = 6.
                   token 0x56, "abcda", 04 00.  anchor = 15 >= L: no put, loop ends.  Last literals V[15..20) = "dabcd":
                   token 0x50.  -> 56 6162636461 0400 50 6461626364 (14 bytes) = compressFast(src).
 wholly_in_dict    dict DICT, src "xy3456789qrstuvwxyz" (n = 19): anchor = 16, ip = 16, L = 23, matchLimit = 30.
                   ip 16 "xy34", 17 "y345": empty.  ip 18 "3456": match = 3 (> 0, < 18, 3 + 65535 >= 18, same bytes):
                   2 literals "xy", offset 18 - 3 = 15, extension ip 22 / match 7: "789" equal, V[25] = 'q' != V[10] = 'A':
                   ml = 3.  token 0x23, "xy", 0f 00.  anchor = 25 >= L: ends.  Last literals "qrstuvwxyz" (10): token 0xa0.
                   -> 23 7879 0f00 a0 7172737475767778797a (16 bytes); the match lies wholly inside the dictionary.
 spans_dict_end    dict DICT, src "BCDEFBCDEFBCDEFqrstuvwx" (n = 23): anchor = 16, ip = 16, L = 27, matchLimit = 34.
                   ip 16 "BCDE": match = 11: 0 literals, offset 5, extension ip 20 / match 15: V[20] = 'F' == V[15] = 'F'
                   (the dictionary's last byte), then match = 16 .. 25 runs over the record itself (period 5) while ip =
                   21 .. 30; V[31] = 'q' != V[26] = 'B': ml = 11.  token 0x0b, 05 00.  anchor = 31 >= L: ends.  Last literals
                   "qrstuvwx" (8): token 0x80.  -> 0b 0500 80 7172737475767778 (12 bytes); 15 match bytes, 5 of them
                   dictionary bytes (positions 11 .. 15), 10 the record's own.
 first_byte_match  dict DICT, src "456789qrstuvwxyz!?" (n = 18): anchor = 16, ip = 16, L = 22, matchLimit = 29.
                   ip 16 "4567": match = 4: 0 literals (the record's first byte starts the match), offset 12, extension
                   ip 20 / match 8: "89" equal, V[22] = 'q' != V[10] = 'A': ml = 2.  token 0x02, 0c 00.  anchor = 22 >= L:
                   ends.  Last literals "qrstuvwxyz!?" (12): token 0xc0.  -> 02 0c00 c0 71..3f (16 bytes).

 dict_pos_0        dict DICT, src "0123qrstuvwxyz!?#": ip 16 "0123" reads table value 0 (the 4-gram at position 0 of V):
                   0 = empty, no match -- the record is 17 literals.
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
import zig_lz4_dict_compress as zc  # noqa: E402

DICT = b"0123456789ABCDEF"
LITERAL = [
    ("empty_dict", b"", b"abcdabcdabcdabcdabcd", 1, None),
    ("wholly_in_dict", DICT, b"xy3456789qrstuvwxyz", 1, None),
    ("spans_dict_end", DICT, b"BCDEFBCDEFBCDEFqrstuvwx", 1, None),
    ("first_byte_match", DICT, b"456789qrstuvwxyz!?", 1, None),
    ("dict_pos_0", DICT, b"0123qrstuvwxyz!?#", 1, None),
    ("twelve_bytes", DICT, b"456789ABCDEF", 1, None),
    ("empty_record", DICT, b"", 1, None),
    ("cap_exact", DICT, b"xy3456789qrstuvwxyz", 1, 16),
    ("cap_one_short", DICT, b"xy3456789qrstuvwxyz", 1, 15),
    ("cap_zero", DICT, b"xy3456789qrstuvwxyz", 1, 0),
    ("accel_8", DICT * 8, (DICT * 8)[5:90] + b"qrstuvwxyz!?#", 8, None),
    ("accel_65537", DICT * 8, (DICT * 8)[5:90] + b"qrstuvwxyz!?#", 65537, None),
    ("one_byte_dict", b"a" * 9, b"a" * 40 + b"qrstuvwx", 1, None),
    ("dict_of_four", b"abcd", b"abcdabcdabcdabcdqrst", 1, None),
    ("dict_of_five", b"abcde", b"abcdeabcdeabcdeqrstu", 1, None),
]
GENERATED = [(g, seed, dl, n, a) for g, seed in (("text", 1), ("reptext", 2), ("mixed", 3), ("random", 4))
             for dl, n, a in ((0, 1000, 1), (100, 37, 1), (4096, 4096, 1), (65536, 4096, 1), (70000, 1000, 8))]


def generated(gen, seed, dl, n):
    """dictionary = the dl bytes in front of position 70000 of the generator's stream, record = the n bytes after it"""
    s = bytes(getattr(dg, gen + "_bytes")(70000 + n, seed))
    return s[70000 - dl:70000], s[70000:]


def main():
    vectors = []
    for name, d, src, accel, cap in LITERAL:
        r, out = zc.compress_fast_using_dict(src, d, accel, cap)
        vectors.append({"name": name, "dict": d.hex(), "src": src.hex(), "acceleration": accel, "dst_cap": cap, "result": r,
                        "out": out.hex()})
    for gen, seed, dl, n, accel in GENERATED:
        d, src = generated(gen, seed, dl, n)
        r, out = zc.compress_fast_using_dict(src, d, accel)
        vectors.append({"name": "%s_d%d_n%d_a%d" % (gen, dl, n, accel), "gen": gen, "seed": seed, "dict_len": dl, "n": n,
                        "acceleration": accel, "dst_cap": None, "result": r, "sha256": hashlib.sha256(out).hexdigest()})
    with open(os.path.join(HERE, "dict_compress_kat.json"), "w") as f:
        json.dump({"what": "zlz4_compress_fast_using_dict known answers (gen_dict_compress_kat.py)", "vectors": vectors}, f, indent=1)
        f.write("\n")
    print("%d vectors" % len(vectors))


if __name__ == "__main__":
    main()
