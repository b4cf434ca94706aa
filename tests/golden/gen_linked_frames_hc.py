#!/usr/bin/env python3
"""Writes tests/golden/linked_frames_hc.json: size and sha256 of the linked-block frames of the HC levels 3, 6 and 9
(zlz4f_batch_compress_frame_ex with ZLZ4F_BATCH_LINK_BLOCKS) for the recipes of tests/linkedgen.py.
A vector is recorded only where the two restatements agree byte for byte: the Python model
(tools/pyref/zig_lz4_linked_frame_hc.py) and the same frame composed from the C restatement of the block compressor
(tests/hc_dict_ref.c), and where the model's own decoder gives the input back.

  python tests/golden/gen_linked_frames_hc.py        (needs cc)
"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hcdictcgen as hg  # noqa: E402
import linkedgen as lg  # noqa: E402
import zig_lz4_linked_frame as lf  # noqa: E402
import zig_lz4_linked_frame_hc as lh  # noqa: E402

OUT = os.path.join(HERE, "linked_frames_hc.json")
LEVELS = (3, 6, 9)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        cref = hg.ref(tmp)
        frames = []
        for r in lg.RECIPES:
            data = lg.recipe_input(r)
            for level in LEVELS:
                frame = lh.compress_frame_linked_hc(data, level, r)
                by_c = lh.compress_frame_linked_hc(data, level, r, lambda b, d, lv: cref.compress(b, d, lv)[1])
                if frame != by_c:
                    print("%s level %d: the restatements differ, not recorded" % (r["name"], level))
                    continue
                assert not frame[4] & 0x20 and lf.decompress_frame_linked(frame, len(data)) == (len(data), data)
                frames.append(dict(name=r["name"], recipe=r, level=level, input_sha256=hashlib.sha256(data).hexdigest(),
                                   frame_len=len(frame), frame_sha256=hashlib.sha256(frame).hexdigest()))
                print("%s level %d: %d -> %d bytes" % (r["name"], level, len(data), len(frame)))
    with open(OUT, "w") as f:
        json.dump(dict(source="tools/pyref/zig_lz4_linked_frame_hc.py == tests/hc_dict_ref.c per block", frames=frames), f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
