#!/usr/bin/env python3
"""Writes tests/golden/dict_frames.json: dictionary frames made by the system liblz4 (LZ4F_compressFrame_usingCDict), the
data no call of this library could read before the _using_dict frame calls.  Each entry records the recipe of its
dictionary and input (tests/dictframegen.py: recipe_dict, recipe_input), their sha256 and the frame.  The dictionaries are
longer than 64 KiB, so only their tail counts.

  python tests/golden/gen_dict_frames.py        (needs liblz4.so.1 with the CDict calls; written with liblz4 1.9.3)
"""
import base64
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dictframegen as dfg  # noqa: E402


def main():
    z = dfg.liblz4fd()
    assert z is not None, "liblz4.so.1 with LZ4F_compressFrame_usingCDict does not load"
    frames = []
    for r in dfg.RECIPES:
        d, data = dfg.recipe_dict(r), dfg.recipe_input(r)
        frame = z.compress(data, d, r["level"], bool(r["linked"]), r["block_size_id"], r["block_checksum"],
                           r["content_checksum"], r["dict_id"])
        # (liblz4 declares a frame of one block independent whatever the preferences say)
        assert bool(frame[4] & 0x20) == (not r["linked"] or len(data) <= 65536) and z.decompress(frame, len(data), d) == data
        assert z.decompress(frame, len(data), b"") != data, "the frame does not need its dictionary"
        frames.append(dict(name=r["name"], recipe=r, dict_sha256=hashlib.sha256(d).hexdigest(), input_len=len(data),
                           input_sha256=hashlib.sha256(data).hexdigest(), frame_len=len(frame),
                           frame_sha256=hashlib.sha256(frame).hexdigest(), frame_b64=base64.b64encode(frame).decode()))
        print("%s: %d -> %d bytes, FLG 0x%02x" % (r["name"], len(data), len(frame), frame[4]))
    with open(dfg.FIXTURES, "w") as f:
        json.dump(dict(source="liblz4 LZ4F_compressFrame_usingCDict", frames=frames), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
