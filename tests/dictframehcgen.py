"""Test-side helpers for lz4f dictionary frames at the HC levels 3..9 (tests/test_dict_frame_hc_cpu.py,
tests/test_gpu_dict_frame_hc.py, tests/golden/gen_dict_frames_hc.py, tools/time_dict_frames_hc.py).

* `RECIPES`: dictframegen's record recipe (1000 bytes), the same at 4096 bytes, and its three-block input (150 000 bytes
  against a 100 000-byte dictionary, block_size_id 4); `CASES`: every recipe at the levels 3, 6 and 9 in both block modes.
* `c_block(cref)`: the C restatement of the block compressor (tests/hc_dict_ref.c through hcdictcgen.ref) in the shape
  compress_frame_using_dict_hc takes as `compress_block`.
* `model(cref)`: memoised compress_frame_using_dict_hc over the C restatement -- one frame is computed once per process.
* `table_records()`: the six 4 KiB D-text records of DESIGN.md section 4.3c and the 64 KiB in front of them.
* `fixtures()`: tests/golden/dict_frames_hc.json.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools", "pyref"))
import datagen as dg  # noqa: E402
import dictframegen as dfg  # noqa: E402
import zig_lz4_dict_frame_hc as dh  # noqa: E402

FIXTURES = os.path.join(HERE, "golden", "dict_frames_hc.json")
LEVELS = (3, 6, 9)
_REC = {k: v for k, v in dfg.RECIPES[4].items() if k in ("dict_len", "dict_seed", "period", "input_len", "flip_every",
                                                         "block_size_id")}
RECIPES = (
    dict(_REC, name="record_1000"),
    dict(_REC, name="record_4096", input_len=4096),
    dict(dfg._BIG, name="three_blocks"),
)
SMALL = ("record_1000", "record_4096")                                 # what the Python block compressor does in seconds
CASES = tuple((r["name"], level, mode) for r in RECIPES for level in LEVELS for mode in (0, 1))


def recipe(name):
    return [r for r in RECIPES if r["name"] == name][0]


_DATA = {}


def data_of(name):
    """-> (dictionary, input) of a recipe; built once"""
    if name not in _DATA:
        r = recipe(name)
        _DATA[name] = (dfg.recipe_dict(r), dfg.recipe_input(r))
    return _DATA[name]


def prefs_of(name, mode, **kw):
    return dict(kw, block_size_id=recipe(name)["block_size_id"], block_mode=mode)


def c_block(cref):
    def compress(block, dictionary, level):
        n, out = cref.compress(block, dictionary, level)
        assert n == len(out) and n > 0
        return out
    return compress


def model(cref):
    """-> f(data, dict_bytes, level, prefs) = compress_frame_using_dict_hc with the C block compressor, memoised"""
    memo, block = {}, c_block(cref)

    def frame(data, dict_bytes, level, prefs=None):
        key = (bytes(data), bytes(dict_bytes or b"")[-65536:], level, tuple(sorted((prefs or {}).items())))
        if key not in memo:
            memo[key] = dh.compress_frame_using_dict_hc(data, dict_bytes, level, prefs, block)
        return memo[key]
    return frame


def table_records():
    """-> (dictionary of 65 536 bytes, six records of 4096 bytes): tests/test_hc_dict_cpu.py::test_the_dictionary_is_used"""
    s = bytes(dg.text_bytes(65536 + 6 * 4096, 77))
    return s[:65536], [s[65536 + i * 4096:65536 + (i + 1) * 4096] for i in range(6)]


def fixtures():
    return json.load(open(FIXTURES))["frames"]
