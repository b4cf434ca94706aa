"""The workspace-size functions of the batch frame calls as rows of arguments: the grid tests/golden/frame_batch_workspaces.json
is sampled from, and how one row is asked of a loaded library.  Pure host arithmetic: no device is touched.

The ten zlz4f_batch_*_workspace* functions of include/zlz4_amd.h, and the two HC workspace functions their layouts embed
(zlz4_batch_compress_hc_workspace, zlz4_batch_compress_hc_using_dict_workspace)."""
import ctypes as C
import itertools

NFRAMES = (0, 1, 3, 1000)
MAX_BLOCKS = (0, 1, 7, 4096)
BLOCK_SIZES = {4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}
LEVELS = (0, 1, 2, 3, 9, 10, 12)
BATCH_FLAGS = (0, 1, 4, 5)              # 0, ZLZ4F_BATCH_CONTENT_SIZE, ZLZ4F_BATCH_LINK_BLOCKS, both
DECODE_FLAGS = (0, 1)                   # 0, ZLZ4F_DECODE_LINKED
NDICTS = (0, 1, 5)
MAX_DICT_LEN = (0, 100, 65536)
BLOCK_MODES = (0, 1)

# fn -> (the keys of a row, in argument order; "prefs" stands for block_size_id / block_mode / compression_level)
FUNCS = {
    "zlz4f_batch_compress_frame_workspace": ("nframes", "max_blocks", "prefs"),
    "zlz4f_batch_compress_frame_workspace_ex": ("nframes", "max_blocks", "prefs", "batch_flags"),
    "zlz4f_batch_decompress_frame_workspace": ("nframes", "max_blocks"),
    "zlz4f_batch_decompress_frame_workspace_ex": ("nframes", "max_blocks", "decode_flags"),
    "zlz4f_batch_frame_decompressed_size_workspace": ("nframes", "max_blocks"),
    "zlz4f_batch_frame_decompressed_size_workspace_ex": ("nframes", "max_blocks", "decode_flags"),
    "zlz4f_batch_compress_frame_using_dict_workspace": ("nframes", "max_blocks", "prefs", "batch_flags", "ndicts",
                                                        "max_src_len", "max_dict_len"),
    "zlz4f_batch_compress_frame_using_dict_workspace_ex": ("nframes", "max_blocks", "prefs", "batch_flags", "ndicts",
                                                           "max_src_len", "max_dict_len"),
    "zlz4f_batch_decompress_frame_using_dict_workspace": ("nframes", "max_blocks"),
    "zlz4f_batch_frame_decompressed_size_using_dict_workspace": ("nframes", "max_blocks"),
    "zlz4_batch_compress_hc_workspace": ("max_blocks", "max_in_len"),
    "zlz4_batch_compress_hc_using_dict_workspace": ("max_blocks", "max_in_len", "max_dict_len"),
}

# how many rows of a function's full product the table keeps (None: all of them)
KEEP = {
    "zlz4f_batch_compress_frame_workspace": 48,
    "zlz4f_batch_compress_frame_workspace_ex": 80,
    "zlz4f_batch_compress_frame_using_dict_workspace": 96,
    "zlz4f_batch_compress_frame_using_dict_workspace_ex": 96,
    "zlz4_batch_compress_hc_using_dict_workspace": 24,
}


def _axis(key):
    return {"nframes": NFRAMES, "max_blocks": MAX_BLOCKS, "batch_flags": BATCH_FLAGS, "decode_flags": DECODE_FLAGS,
            "ndicts": NDICTS, "max_dict_len": MAX_DICT_LEN, "max_in_len": tuple(BLOCK_SIZES.values()),
            "prefs": tuple(dict(block_size_id=b, block_mode=m, compression_level=lv)
                           for b in BLOCK_SIZES for m in BLOCK_MODES for lv in LEVELS)}[key]


def product(fn):
    """Every row of the grid for one function, in a fixed order; max_src_len follows the row's block size."""
    keys = FUNCS[fn]
    rows = []
    for combo in itertools.product(*(_axis(k) for k in keys if k != "max_src_len")):
        row = dict(zip((k for k in keys if k != "max_src_len"), combo))
        if "max_src_len" in keys:
            bs = BLOCK_SIZES[row["prefs"]["block_size_id"]]
            rows.extend(dict(row, max_src_len=n) for n in (0, 100, bs, bs + 1))
        else:
            rows.append(row)
    return rows


def sample(fn):
    """The rows the table records: a fixed pseudo-random choice (a 31-bit LCG, no library generator), then one row more
    for every axis value the choice happened to miss."""
    rows = product(fn)
    keep = KEEP.get(fn)
    if keep is None or keep >= len(rows):
        return rows
    x, chosen = 0x2545F491, set()
    while len(chosen) < keep:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        chosen.add((x >> 8) % len(rows))
    picked = [rows[i] for i in sorted(chosen)]
    for key, value in missing(fn, picked):
        picked.append(next(r for r in rows if _get(r, key) == value))
    return picked


def _get(row, key):
    return row["prefs"][key] if key in ("block_size_id", "block_mode", "compression_level") else row[key]


def axis_values(fn):
    """axis -> the values the grid gives it (the preferences by field; max_src_len is relative to the block size)."""
    out = {}
    for k in FUNCS[fn]:
        if k == "prefs":
            out.update(block_size_id=set(BLOCK_SIZES), block_mode=set(BLOCK_MODES), compression_level=set(LEVELS))
        elif k != "max_src_len":
            out[k] = set(_axis(k))
    return out


def missing(fn, rows):
    """(axis, value) pairs of the grid that no row of `rows` has."""
    return [(key, v) for key, want in axis_values(fn).items() for v in sorted(want - {_get(r, key) for r in rows})]


def call(zl, L, fn, row):
    """The function's answer for one row; `L` is a ctypes library bound like zig_lz4_amd.lib()."""
    args = []
    for k in FUNCS[fn]:
        if k == "prefs":
            p = zl.Prefs()
            for name, v in row["prefs"].items():
                setattr(p, name, v)
            args.append(C.byref(p))
        else:
            args.append(row[k])
    return getattr(L, fn)(*args)
