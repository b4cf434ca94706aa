#!/usr/bin/env python3
"""Writes tests/golden/dict_frames_hc.json: size and sha256 of dictionary frames at the HC levels 3, 6 and 9
(zlz4f_batch_compress_frame_using_dict_ex) for the recipes of tests/dictframehcgen.py, both block
modes.  A vector is recorded only where the two restatements agree byte for byte: the Python model
(tools/pyref/zig_lz4_dict_frame_hc.py) and the same frame composed from the C restatement of the block compressor
(tests/hc_dict_ref.c), and where the model's own decoder gives the input back with the dictionary.

  python tests/golden/gen_dict_frames_hc.py        (needs cc; the three-block recipe takes the Python model a minute)
"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dictframehcgen as hcg  # noqa: E402
import hcdictcgen as hg  # noqa: E402
import zig_lz4_dict_frame as df  # noqa: E402
import zig_lz4_dict_frame_hc as dh  # noqa: E402

OUT = os.path.join(HERE, "dict_frames_hc.json")
KW = dict(block_checksum=1, content_checksum=1, dict_id=0x0D1C7)       # the three-block frames carry all of it


def main():
    with tempfile.TemporaryDirectory() as tmp:
        by_c = hcg.model(hg.ref(tmp))
        frames = []
        for name, level, mode in hcg.CASES:
            d, data = hcg.data_of(name)
            prefs = hcg.prefs_of(name, mode, **(KW if name == "three_blocks" else {}))
            frame = dh.compress_frame_using_dict_hc(data, d, level, prefs)
            if frame != by_c(data, d, level, prefs):
                print("%s level %d mode %d: the restatements differ, not recorded" % (name, level, mode))
                continue
            assert bool(frame[4] & 0x20) == (mode == 1)
            assert df.decompress_frame_using_dict(frame, len(data), d) == (len(data), data)
            frames.append(dict(name=name, recipe=hcg.recipe(name), level=level, prefs=prefs,
                               dict_sha256=hashlib.sha256(d).hexdigest(), input_sha256=hashlib.sha256(data).hexdigest(),
                               frame_len=len(frame), frame_sha256=hashlib.sha256(frame).hexdigest()))
            print("%s level %d mode %d: %d -> %d bytes" % (name, level, mode, len(data), len(frame)))
    with open(OUT, "w") as f:
        json.dump(dict(source="tools/pyref/zig_lz4_dict_frame_hc.py == tests/hc_dict_ref.c per block", frames=frames), f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
