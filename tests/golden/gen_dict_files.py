#!/usr/bin/env python3
"""Writes tests/golden/dict_files.json: .lz4 files written by the `lz4` command line tool (1.9.3) with `-D dict`, for the
dictionary file calls (tests/test_file_dict_cpu.py, tests/test_gpu_file_dict.py).

    python tests/golden/gen_dict_files.py [path to lz4]      (default: `lz4` on PATH, or $LZ4)

The inputs are synthetic text: long sentences drawn from a pool of 4 (generated here, seeded), so that the files stay small;
the dictionary is 70 000 bytes of the same sentences, so only its last 64 KiB can be reached.  Cases: one small record
(300 bytes) with and without -BD (linked blocks) and --content-size, 200 000 bytes (four 64 KiB blocks with -B4) plain,
with -BD and with --content-size (not both: nothing new), and two of the 200 000-byte files with a legacy file
(`lz4 -l`, no dictionary) between them.  NOT IN THE FIXTURE: a linked one-block member that uses the dictionary -- the tool
forces independent blocks for a one-block input, so `small_BD` is byte-identical to `small`; only the hand-built `DL1` of
tests/filedictgen.py covers that case.  Byte strings are stored as base64 of zlib (the content, the dictionary) or
base64 (the files), each content with its SHA-256.  A case names its file, or the parts that are concatenated.
"""
import base64
import hashlib
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))


def vocabulary(seed=11, words=120):
    r = random.Random(seed)
    return ["".join(r.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(r.randint(2, 9))) for _ in range(words)]


def sentences(vocab, seed=12, count=4):
    r = random.Random(seed)
    return [" ".join(r.choice(vocab) for _ in range(r.randint(140, 160))) + ".\n" for _ in range(count)]


def text(n, seed, pool):
    r = random.Random(seed)
    out = []
    size = 0
    while size < n:
        out.append(r.choice(pool))
        size += len(out[-1])
    return "".join(out)[:n].encode()


def run(tool, args, data, dict_path=None):
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out.lz4")
        open(src, "wb").write(data)
        cmd = [tool, "-f", "-q"] + list(args) + (["-D", dict_path] if dict_path else []) + [src, dst]
        subprocess.check_call(cmd)
        return open(dst, "rb").read()


def main():
    tool = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LZ4") or shutil.which("lz4")
    if not tool:
        sys.exit("no lz4 tool: pass its path")
    version = subprocess.run([tool, "--version"], capture_output=True, text=True).stdout.strip()
    vocab = sentences(vocabulary())
    dictionary = text(70000, 1, vocab)
    small, big_a, leg = text(300, 2, vocab), text(200000, 3, vocab), text(3000, 5, vocab)
    z = lambda b: base64.b64encode(zlib.compress(b, 9)).decode()          # noqa: E731
    files, contents, cases = {}, {}, []
    with tempfile.TemporaryDirectory() as tmp:
        dpath = os.path.join(tmp, "dict")
        open(dpath, "wb").write(dictionary)
        for cname, data in (("small", small), ("big_a", big_a)):
            contents[cname] = data
            for bd in (False, True):
                for cs in (False, True):
                    if cname == "big_a" and bd and cs:
                        continue
                    name = cname + ("_BD" if bd else "") + ("_cs" if cs else "")
                    args = ["-B4"] + (["-BD"] if bd else []) + (["--content-size"] if cs else [])
                    files[name] = run(tool, args, data, dpath)
                    blocks = -(-len(data) // 65536)
                    cases.append(dict(name=name, parts=[name], contents=[cname], args=args,
                                      linked_multiblock=bool(bd and blocks > 1)))
        contents["legacy"] = leg
        files["legacy"] = run(tool, ["-l"], leg)
    cases.append(dict(name="big_legacy_big", parts=["big_a", "legacy", "big_a_cs"], contents=["big_a", "legacy", "big_a"],
                      args=["cat"], linked_multiblock=False))
    out = dict(tool=version, dictionary=z(dictionary), dictionary_sha256=hashlib.sha256(dictionary).hexdigest(),
               contents={k: dict(zlib=z(v), sha256=hashlib.sha256(v).hexdigest(), size=len(v)) for k, v in contents.items()},
               files={k: base64.b64encode(v).decode() for k, v in files.items()}, cases=cases)
    path = os.path.join(HERE, "dict_files.json")
    json.dump(out, open(path, "w"), indent=0, sort_keys=True)
    print(path, os.path.getsize(path), {k: len(v) for k, v in files.items()})


if __name__ == "__main__":
    main()
