#!/usr/bin/env python3
"""Writes tests/golden/linked_frames.json: linked-block frames made by the system liblz4 (LZ4F_compressFrame, blockMode
linked), the data no call of this library's reference-compatible surface can read.  Each entry records the recipe of its
input (tests/linkedgen.py: recipe_input), the input's sha256 and the frame; the frames are kept under 64 KiB.

  python tests/golden/gen_linked_frame_fixtures.py        (needs liblz4.so.1; written with liblz4 1.9.3)
"""
import base64
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import linkedgen as lg  # noqa: E402


def main():
    z = lg.liblz4f()
    assert z is not None, "liblz4.so.1 does not load"
    frames = []
    for r in lg.RECIPES:
        data = lg.recipe_input(r)
        frame = z.compress(data, r["block_size_id"], r["block_checksum"], r["content_checksum"], linked=True)
        assert len(frame) < 65536 and not frame[4] & 0x20 and z.decompress(frame, len(data)) == data
        frames.append(dict(name=r["name"], recipe=r, input_len=len(data), input_sha256=hashlib.sha256(data).hexdigest(),
                           frame_len=len(frame), frame_sha256=hashlib.sha256(frame).hexdigest(),
                           frame_b64=base64.b64encode(frame).decode()))
        print("%s: %d -> %d bytes, FLG 0x%02x" % (r["name"], len(data), len(frame), frame[4]))
    with open(lg.FIXTURES, "w") as f:
        json.dump(dict(source="liblz4 LZ4F_compressFrame, blockMode linked", frames=frames), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
