"""zig_lz4_amd -- Python view of the MI355X-native LZ4 codec's C ABI (include/zlz4_amd.h).

The product is the HIP shared library `libzlz4_amd.so` built from csrc/; this module is
the thin ctypes layer the tests and bench.py use.  It mirrors the names of the reference's
public facade (src/root.zig:1-57): compressBound / compressDefault / compressFast /
compressHC / decompressSafe and the `lz4f` namespace, with the reference's error
behaviour (Zig error unions -> Python exceptions carrying the same error name).

There is no CPU implementation here: if the library is missing, importing any compute
entry point raises; if no gfx950 device is present the calls raise Lz4Error("DeviceError").
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZLZ4_AMD_LIB selects a diagnostic build of the same library (e.g. the -DZLZ4_STAMPS one); never a fallback
LIB_PATH = os.environ.get("ZLZ4_AMD_LIB") or os.path.join(_HERE, "libzlz4_amd.so")

# constants re-exported by src/root.zig:46-49 and src/lz4hc.zig:28-31
MINMATCH = 4
LZ4_MAX_INPUT_SIZE = 0x7E000000
LZ4_DISTANCE_MAX = 65535
LZ4HC_CLEVEL_MIN = 2
LZ4HC_CLEVEL_DEFAULT = 9
LZ4HC_CLEVEL_MAX = 12

ERR_DEVICE = -7
ERR_UNSUPPORTED = -8


class Lz4Error(Exception):
    """Mirror of lz4.Error / lz4f.Error (src/lz4.zig:48-55, src/lz4f.zig:31-55)."""

    def __init__(self, code, name):
        super().__init__("%s (%d)" % (name, code))
        self.code = code
        self.name = name


class Prefs(C.Structure):
    """zlz4f_prefs == lz4f.Preferences + FrameInfo flattened (src/lz4f.zig:106-122)."""
    _fields_ = [
        ("block_size_id", C.c_uint32),
        ("block_mode", C.c_uint32),
        ("content_checksum", C.c_uint32),
        ("block_checksum", C.c_uint32),
        ("content_size", C.c_uint64),
        ("dict_id", C.c_uint32),
        ("compression_level", C.c_int32),
    ]


class TrainParams(C.Structure):
    """zlz4_train_params: d-mer length d in {4, 6, 8}, segment length k in 16..1024, log2 f of the frequency table in
    10..24."""
    _fields_ = [("d", C.c_uint32), ("k", C.c_uint32), ("f", C.c_uint32), ("reserved", C.c_uint32)]


class LegacyPrefs(C.Structure):
    """zlz4f_legacy_prefs: block_size 0 = 8 MiB (what `lz4 -l` writes), 1 .. 8 MiB as given; compression_level <= 0 = fast,
    else compressHC's level."""
    _fields_ = [("block_size", C.c_uint32), ("compression_level", C.c_int32)]


# every symbol include/zlz4_amd.h declares: name -> (restype, argtypes)
_VP, _SZ, _I64, _I32, _U32 = C.c_void_p, C.c_size_t, C.c_int64, C.c_int32, C.c_uint32
_PP = C.POINTER(Prefs)
_LP = C.POINTER(LegacyPrefs)
SYMBOLS = {
    "zlz4_compress_bound": (_SZ, [_SZ]),
    "zlz4_compress_default": (_I64, [_VP, _SZ, _VP, _SZ]),
    "zlz4_compress_fast": (_I64, [_VP, _SZ, _VP, _SZ, _U32]),
    "zlz4_compress_hc": (_I64, [_VP, _SZ, _VP, _SZ, _I32]),
    "zlz4_sizeof_state_hc": (_SZ, []),
    "zlz4_compress_hc_ext_state": (_I64, [_VP, _SZ, _VP, _SZ, _VP, _SZ, _I32]),
    "zlz4_decompress_safe": (_I64, [_VP, _SZ, _VP, _SZ]),
    "zlz4_decompress_safe_partial": (_I64, [_VP, _SZ, _VP, _SZ, _SZ]),
    "zlz4_decompress_safe_using_dict": (_I64, [_VP, _SZ, _VP, _SZ, _VP, _SZ]),
    "zlz4_decompress_safe_partial_using_dict": (_I64, [_VP, _SZ, _VP, _SZ, _SZ, _VP, _SZ]),
    "zlz4_stream_load_dict": (_I64, [_VP, _VP, _SZ]),
    "zlz4_stream_compress_fast_continue": (_I64, [_VP, _VP, _SZ, _VP, _SZ, _U32]),
    "zlz4_compress_fast_using_dict": (_I64, [_VP, _SZ, _VP, _SZ, _VP, _SZ, _U32]),
    "zlz4_sizeof_state": (_SZ, []),
    "zlz4_compress_fast_ext_state": (_I64, [_VP, _SZ, _VP, _SZ, _VP, _SZ, _U32]),
    "zlz4_compress_dest_size": (_I64, [_VP, _VP, _SZ, C.POINTER(C.c_size_t)]),
    "zlz4_batch_compress_fast": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _U32]),
    "zlz4_batch_decompress_safe": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32]),
    "zlz4_batch_decompress_safe_using_dict": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32]),
    "zlz4_decompress_safe_prefix": (_I64, [_VP, _SZ, _VP, _SZ]),
    "zlz4_decompress_safe_prefix_using_dict": (_I64, [_VP, _SZ, _VP, _SZ, _VP, _SZ]),
    "zlz4_batch_decompress_safe_prefix": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32]),
    "zlz4_batch_decompress_safe_prefix_using_dict": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32]),
    "zlz4_decompressed_size": (_I64, [_VP, _SZ, _SZ]),
    "zlz4_batch_decompressed_size": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _U32]),
    "zlz4_batch_plan_outputs": (_I32, [_VP, _VP, _U32, _U32, _VP, _VP, _VP]),
    "zlz4f_frame_decompressed_size": (_I64, [_VP, _SZ]),
    "zlz4f_batch_frame_decompressed_size_workspace": (_SZ, [_U32, _U32]),
    "zlz4f_batch_frame_decompressed_size": (_I32, [_VP, _VP, _VP, _VP, _VP, _U32, _U32, _VP, _SZ]),
    "zlz4f_frame_decompressed_size_ex": (_I64, [_VP, _SZ, _U32]),
    "zlz4f_batch_frame_decompressed_size_workspace_ex": (_SZ, [_U32, _U32, _U32]),
    "zlz4f_batch_frame_decompressed_size_ex": (_I32, [_VP, _VP, _VP, _VP, _VP, _U32, _U32, _U32, _VP, _SZ]),
    "zlz4_batch_load_dict": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _U32]),
    "zlz4_batch_compress_fast_continue": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _U32]),
    "zlz4_batch_compress_fast_using_dict": (_I32, [_VP] * 13 + [_U32, _U32, _U32, _U32]),
    "zlz4_batch_compress_hc_workspace": (_SZ, [_U32, _U32]),
    "zlz4_compress_hc_using_dict": (_I64, [_VP, _SZ, _VP, _SZ, _VP, _SZ, _I32]),
    "zlz4_batch_compress_hc_using_dict_workspace": (_SZ, [_U32, _U32, _U32]),
    "zlz4_batch_compress_hc_using_dict": (_I32, [_VP] * 11 + [_U32, _U32, _U32, _I32, _VP, _SZ]),
    "zlz4_batch_train_dict_workspace": (_SZ, [_U32, C.c_uint64, _U32, _VP]),
    "zlz4_batch_train_dict": (_I32, [_VP] * 4 + [_U32, _VP, _U32] + [_VP] * 4 + [_U32, _VP, _VP, _SZ]),
    "zlz4_train_dict": (_I64, [_VP, _VP, _U32, _VP, _SZ, _VP]),
    "zlz4_batch_compress_hc": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _I32, _VP, _SZ]),
    "zlz4_batch_compress_dest_size_workspace": (_SZ, [_U32, _U32]),
    "zlz4_batch_compress_dest_size": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _VP, _SZ]),
    "zlz4_batch_verify": (_I64, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32]),
    "zlz4_stream_decode_init": (None, [_VP]),
    "zlz4_set_stream_decode": (None, [_VP, _VP, _SZ]),
    "zlz4_decompress_safe_continue": (_I64, [_VP, _VP, _SZ, _VP, _SZ]),
    "zlz4_decoder_ring_buffer_size": (_SZ, [_SZ]),
    "zlz4_batch_decompress_safe_continue_workspace": (_SZ, [_U32, _U32]),
    "zlz4_batch_decompress_safe_continue": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _VP, _SZ]),
    "zlz4f_compress_frame_bound": (_SZ, [_SZ, _PP]),
    "zlz4f_compress_frame": (_I64, [_VP, _SZ, _VP, _SZ, _PP]),
    "zlz4f_decompress_frame": (_I64, [_VP, _SZ, _VP, _SZ]),
    "zlz4f_header_size": (_I64, [_VP, _SZ]),
    "zlz4f_compress_frame_device": (_I64, [_VP, _VP, _SZ, _VP, _SZ, _PP]),
    "zlz4f_decompress_frame_device": (_I64, [_VP, _VP, _SZ, _VP, _SZ]),
    "zlz4f_compress_frame_segment_device": (_I64, [_VP, _VP, _SZ, _VP, _SZ, _PP, _U32]),
    "zlz4f_decompress_frame_segment_device": (_I64, [_VP, _VP, _SZ, _VP, _SZ, _PP, _U32]),
    "zlz4f_batch_compress_frame_workspace": (_SZ, [_U32, _U32, _PP]),
    "zlz4f_batch_compress_frame": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _PP, _U32, _VP, _SZ]),
    "zlz4f_batch_decompress_frame_workspace": (_SZ, [_U32, _U32]),
    "zlz4f_batch_decompress_frame": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _VP, _SZ]),
    "zlz4f_batch_compress_frame_workspace_ex": (_SZ, [_U32, _U32, _PP, _U32]),
    "zlz4f_batch_compress_frame_ex": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _PP, _U32, _VP, _SZ]),
    "zlz4f_compress_frame_device_ex": (_I64, [_VP, _VP, _SZ, _VP, _SZ, _PP, _U32]),
    "zlz4f_compress_frame_ex": (_I64, [_VP, _SZ, _VP, _SZ, _PP, _U32]),
    "zlz4f_batch_decompress_frame_workspace_ex": (_SZ, [_U32, _U32, _U32]),
    "zlz4f_batch_decompress_frame_ex": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _U32, _VP, _SZ]),
    "zlz4f_decompress_frame_device_ex": (_I64, [_VP, _VP, _SZ, _VP, _SZ, _U32]),
    "zlz4f_decompress_frame_ex": (_I64, [_VP, _SZ, _VP, _SZ, _U32]),
    "zlz4f_batch_compress_frame_using_dict_workspace": (_SZ, [_U32, _U32, _PP, _U32, _U32, C.c_uint64, _U32]),
    "zlz4f_batch_compress_frame_using_dict": (_I32, [_VP] * 8 + [_U32, _U32, _PP, _U32, _VP, _VP, _VP, _U32, _VP, C.c_uint64,
                                                     _U32, _VP, _SZ]),
    "zlz4f_batch_decompress_frame_using_dict_workspace": (_SZ, [_U32, _U32]),
    "zlz4f_batch_decompress_frame_using_dict": (_I32, [_VP] * 8 + [_U32, _U32, _VP, _VP, _VP, _U32, _VP, _VP, _SZ]),
    "zlz4f_batch_frame_decompressed_size_using_dict_workspace": (_SZ, [_U32, _U32]),
    "zlz4f_batch_frame_decompressed_size_using_dict": (_I32, [_VP] * 5 + [_U32, _U32, _VP, _U32, _VP, _VP, _SZ]),
    "zlz4f_batch_frame_dict_id": (_I32, [_VP, _VP, _VP, _VP, _VP, _U32]),
    "zlz4f_compress_frame_using_dict": (_I64, [_VP, _SZ, _VP, _SZ, _PP, _VP, _SZ]),
    "zlz4f_decompress_frame_using_dict": (_I64, [_VP, _SZ, _VP, _SZ, _VP, _SZ]),
    "zlz4f_frame_decompressed_size_using_dict": (_I64, [_VP, _SZ, _SZ]),
    "zlz4f_batch_compress_frame_using_dict_workspace_ex": (_SZ, [_U32, _U32, _PP, _U32, _U32, C.c_uint64, _U32]),
    "zlz4f_batch_compress_frame_using_dict_ex": (_I32, [_VP] * 8 + [_U32, _U32, _PP, _U32, _VP, _VP, _VP, _U32, _VP,
                                                        C.c_uint64, _U32, _VP, _SZ]),
    "zlz4f_compress_frame_using_dict_ex": (_I64, [_VP, _SZ, _VP, _SZ, _PP, _VP, _SZ]),
    "zlz4f_batch_decompress_frame_prefix": (_I32, [_VP] * 8 + [_U32]),
    "zlz4f_batch_decompress_frame_prefix_using_dict": (_I32, [_VP] * 8 + [_U32, _VP, _VP, _VP, _U32, _VP]),
    "zlz4f_decompress_frame_prefix": (_I64, [_VP, _SZ, _VP, _SZ]),
    "zlz4f_decompress_frame_prefix_using_dict": (_I64, [_VP, _SZ, _VP, _SZ, _VP, _SZ]),
    "zlz4f_batch_frame_index_workspace": (_SZ, [_U32, _U32]),
    "zlz4f_batch_frame_index": (_I32, [_VP] * 8 + [_U32, _U32, _VP, _SZ]),
    "zlz4f_batch_plan_frame_ranges": (_I32, [_VP] * 4 + [_U32, _VP, _U32, _U32, _VP, _VP, _VP]),
    "zlz4f_batch_decompress_frame_range_workspace": (_SZ, [_U32, _U32]),
    "zlz4f_batch_decompress_frame_range": (_I32, [_VP] * 7 + [_U32] + [_VP] * 6 + [_U32, _U32, _VP, _SZ]),
    "zlz4f_decompress_frame_range": (_I64, [_VP, _SZ, C.c_uint64, C.c_uint64, _VP, _SZ]),
    "zlz4f_batch_file_index_workspace": (_SZ, [_U32, _VP]),
    "zlz4f_batch_file_index": (_I32, [_VP] * 4 + [_U32] + [_VP] * 10 + [C.c_uint64, _VP, _VP, _SZ]),
    "zlz4f_batch_decompress_file_range_workspace": (_SZ, [_U32, _U32]),
    "zlz4f_batch_decompress_file_range": (_I32, [_VP] * 7 + [_U32] + [_VP] * 9 + [_U32, _U32, _VP, _SZ]),
    "zlz4f_decompress_file_range": (_I64, [_VP, _SZ, C.c_uint64, C.c_uint64, _VP, _SZ, _U32]),
    "zlz4f_seek_table_bound": (_SZ, [C.c_uint64, C.c_uint64]),
    "zlz4f_batch_append_seek_table": (_I32, [_VP] * 5 + [_U32] + [_VP] * 7),
    "zlz4f_batch_load_seek_table": (_I32, [_VP] * 4 + [_U32] + [_VP] * 8 + [C.c_uint64, _VP]),
    "zlz4f_batch_concat_workspace": (_SZ, [_U32]),
    "zlz4f_batch_concat": (_I32, [_VP] * 5 + [_U32, _U32] + [_VP] * 5 + [_SZ]),
    "zlz4f_seek_table": (_I64, [_VP, _SZ, _VP, _SZ, _U32]),
    "zlz4f_decompress_file_range_ex": (_I64, [_VP, _SZ, C.c_uint64, C.c_uint64, _VP, _SZ, _U32, _U32]),
    "zlz4f_batch_file_index_using_dict_workspace": (_SZ, [_U32, _VP]),
    "zlz4f_batch_file_index_using_dict": (_I32, [_VP] * 4 + [_U32] + [_VP] * 10 + [C.c_uint64, _VP, _VP, _U32, _VP, _VP, _SZ]),
    "zlz4f_batch_decompress_file_range_using_dict_workspace": (_SZ, [_U32, _U32]),
    "zlz4f_batch_decompress_file_range_using_dict": (_I32, [_VP] * 7 + [_U32] + [_VP] * 9 + [_U32, _U32] + [_VP] * 3 +
                                                     [_U32, _VP, _VP, _SZ]),
    "zlz4f_batch_multiframe_item_dicts": (_I32, [_VP, _VP, _U32, _U32, _VP, _VP]),
    "zlz4f_decompress_file_range_using_dict": (_I64, [_VP, _SZ, C.c_uint64, C.c_uint64, _VP, _SZ, _U32, _U32, _VP, _SZ]),
    "zlz4f_batch_multiframe_split": (_I32, [_VP] * 4 + [_U32] + [_VP] * 9),
    "zlz4f_batch_multiframe_plan": (_I32, [_VP] * 3 + [_U32, _U32] + [_VP] * 5),
    "zlz4f_batch_multiframe_finish": (_I32, [_VP] * 7 + [_U32, _VP]),
    "zlz4f_multiframe_decompressed_size": (_I64, [_VP, _SZ, _U32]),
    "zlz4f_decompress_multiframe": (_I64, [_VP, _SZ, _VP, _SZ, _U32]),
    "zlz4f_batch_multiframe_split_ex": (_I32, [_VP] * 4 + [_U32] + [_VP] * 9 + [_U32, _VP]),
    "zlz4f_batch_multiframe_select": (_I32, [_VP] * 7 + [_U32, _VP]),
    "zlz4f_multiframe_decompressed_size_ex": (_I64, [_VP, _SZ, _U32, _U32]),
    "zlz4f_decompress_multiframe_ex": (_I64, [_VP, _SZ, _VP, _SZ, _U32, _U32]),
    "zlz4f_legacy_compress_frame_bound": (_SZ, [_SZ, _LP]),
    "zlz4f_batch_compress_legacy_frame_workspace": (_SZ, [_U32, _U32, _LP]),
    "zlz4f_batch_compress_legacy_frame": (_I32, [_VP] * 8 + [_U32, _U32, _LP, _VP, _SZ]),
    "zlz4f_batch_legacy_frame_count": (_I32, [_VP] * 4 + [_U32] + [_VP] * 3),
    "zlz4f_batch_legacy_frame_decompressed_size_workspace": (_SZ, [_U32, _U32]),
    "zlz4f_batch_legacy_frame_decompressed_size": (_I32, [_VP] * 6 + [_U32, _U32, _VP, _SZ]),
    "zlz4f_batch_decompress_legacy_frame_workspace": (_SZ, [_U32, _U32]),
    "zlz4f_batch_decompress_legacy_frame": (_I32, [_VP] * 9 + [_U32, _U32, _VP, _SZ]),
    "zlz4f_compress_legacy_frame": (_I64, [_VP, _SZ, _VP, _SZ, _LP]),
    "zlz4f_legacy_frame_decompressed_size": (_I64, [_VP, _SZ, C.POINTER(C.c_size_t)]),
    "zlz4f_decompress_legacy_frame": (_I64, [_VP, _SZ, _VP, _SZ, C.POINTER(C.c_size_t)]),
    "zlz4_device_check": (_I32, []),
    "zlz4_version_string": (C.c_char_p, []),
    "zlz4_error_name": (C.c_char_p, [_I64]),
    "zlz4_release_device_cache": (None, []),
}

_lib = None


def lib():
    """Load libzlz4_amd.so (fails loudly: no fallback of any kind)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `make` (hipcc --offload-arch=gfx950) -- "
                "there is no CPU fallback" % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7).
        # If torch is going to be used in this process it must be loaded first, so that our library's
        # DT_NEEDED libamdhip64.so.7 binds to the same runtime (device pointers / streams are shared).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)      # AttributeError if the library does not export it
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def error_name(code):
    return lib().zlz4_error_name(code).decode()


def _check(r):
    if r < 0:
        raise Lz4Error(r, error_name(r))
    return r


def device_available():
    return lib().zlz4_device_check() == 0


# ----------------------------------------------------------------------------- root.zig names
def compressBound(input_size):
    """lz4.compressBound, src/lz4.zig:80-83."""
    return lib().zlz4_compress_bound(input_size)


def _in(b):
    b = bytes(b)
    buf = (C.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")
    return buf, len(b)


def _run(fn, src, cap, *extra):
    s, n = _in(src)
    d = (C.c_uint8 * max(1, cap))()
    r = _check(fn(C.addressof(s), n, C.addressof(d), cap, *extra))
    return bytes(d[:r])


def compressDefault(src, dst_cap=None):
    """lz4.compressDefault(src, dst), src/lz4.zig:283-285; dst_cap defaults to compressBound(len(src))."""
    cap = compressBound(len(src)) if dst_cap is None else dst_cap
    return _run(lib().zlz4_compress_default, src, cap)


def compressFast(src, acceleration, dst_cap=None):
    """lz4.compressFast(src, dst, acceleration), src/lz4.zig:292-447."""
    cap = compressBound(len(src)) if dst_cap is None else dst_cap
    return _run(lib().zlz4_compress_fast, src, cap, acceleration)


def compressHC(src, compression_level, dst_cap=None):
    """lz4hc.compressHC(src, dst, level), src/lz4hc.zig:1440-1453."""
    cap = compressBound(len(src)) if dst_cap is None else dst_cap
    return _run(lib().zlz4_compress_hc, src, cap, compression_level)


def sizeofStateHC():
    """lz4hc.sizeofStateHC, src/lz4hc.zig:1492-1494."""
    return lib().zlz4_sizeof_state_hc()


def compressHCExtState(state_len, src, compression_level, dst_cap=None):
    """lz4hc.compressHCExtState(ctx, src, dst, level), src/lz4hc.zig:1457-1489 (fresh context, given by its size)."""
    cap = compressBound(len(src)) if dst_cap is None else dst_cap
    s, n = _in(src)
    st = (C.c_uint8 * max(1, state_len))()
    d = (C.c_uint8 * max(1, cap))()
    r = _check(lib().zlz4_compress_hc_ext_state(C.addressof(st), state_len, C.addressof(s), n, C.addressof(d), cap, compression_level))
    return bytes(d[:r])


def decompressSafe(src, dst_cap):
    """lz4.decompressSafe(src, dst), src/lz4.zig:257-259; dst_cap == dst.len."""
    return _run(lib().zlz4_decompress_safe, src, dst_cap)


def decompressSafePartial(src, dst_cap, target_output_size):
    """lz4.decompressSafePartial(src, dst, targetOutputSize), src/lz4.zig:619-621."""
    return _run(lib().zlz4_decompress_safe_partial, src, dst_cap, target_output_size)


def decompressSafeUsingDict(src, dst_cap, dict):
    """lz4.decompressSafeUsingDict(src, dst, dict), src/lz4.zig:960-962; dst_cap == dst.len."""
    dk, dn = _in(dict)
    return _run(lib().zlz4_decompress_safe_using_dict, src, dst_cap, C.addressof(dk), dn)


def decompressSafePartialUsingDict(src, dst_cap, target_output_size, dict):
    """lz4.decompressSafePartialUsingDict(src, dst, targetOutputSize, dict), src/lz4.zig:967-969."""
    dk, dn = _in(dict)
    return _run(lib().zlz4_decompress_safe_partial_using_dict, src, dst_cap, target_output_size, C.addressof(dk), dn)


def decompressSafePrefix(src, n):
    """zlz4_decompress_safe_prefix (no counterpart in the reference): the first n bytes of the block, or all of it where it
    decodes to fewer; never OutputTooSmall (include/zlz4_amd.h)."""
    return _run(lib().zlz4_decompress_safe_prefix, src, n)


def decompressSafePrefixUsingDict(src, n, dict):
    """zlz4_decompress_safe_prefix_using_dict: decompressSafePrefix with the external dictionary `dict` in front of the
    output; dict None with nothing to stage is the empty dictionary."""
    if dict is None:
        return _run(lib().zlz4_decompress_safe_prefix_using_dict, src, n, None, 0)
    dk, dn = _in(dict)
    return _run(lib().zlz4_decompress_safe_prefix_using_dict, src, n, C.addressof(dk), dn)


def compressFastUsingDict(src, dict, acceleration=1, dst_cap=None):
    """zlz4_compress_fast_using_dict (no counterpart in the reference): compressFast's loop on dict-tail ++ src from the
    table Stream.loadDict(dict) leaves, so matches may reach into the dictionary; decodes with
    decompressSafeUsingDict(out, len(src), dict).  dst_cap defaults to compressBound(len(src))."""
    cap = compressBound(len(src)) if dst_cap is None else dst_cap
    dk, dn = _in(dict)
    return _run(lambda sp, n, dp, c: lib().zlz4_compress_fast_using_dict(sp, n, dp, c, C.addressof(dk), dn, acceleration),
                src, cap)


def compressHCUsingDict(src, dict, compression_level, dst_cap=None):
    """zlz4_compress_hc_using_dict (no counterpart in the reference): compressHashChain on dict-tail ++ src with the parse
    starting at the record, levels 3..9 (1 and below become 9; 2 and 10..12 raise Unsupported); decodes with
    decompressSafeUsingDict(out, len(src), dict).  dst_cap defaults to compressBound(len(src))."""
    cap = compressBound(len(src)) if dst_cap is None else dst_cap
    dk, dn = _in(dict)
    return _run(lambda sp, n, dp, c: lib().zlz4_compress_hc_using_dict(sp, n, dp, c, C.addressof(dk), dn, compression_level),
                src, cap)


def trainDict(samples, dict_size=65536, d=8, k=256, f=20):
    """zlz4_train_dict (no counterpart in the reference): one dictionary of at most dict_size (<= 65536) bytes from the
    byte strings of `samples`, by the fastCover-style selection of include/zlz4_amd.h; a host call that stages the samples.
    The result goes straight into compressFastUsingDict / compressHCUsingDict and the batch and frame calls with a
    dictionary.  Too few sample bytes give b""; bad parameters raise InvalidState."""
    items = [bytes(s) for s in samples]
    s, _ = _in(b"".join(items))
    sizes = (C.c_size_t * max(1, len(items)))(*[len(b) for b in items])
    out = (C.c_uint8 * max(1, dict_size))()
    p = TrainParams(d, k, f, 0)
    r = _check(lib().zlz4_train_dict(C.addressof(s), C.addressof(sizes), len(items), C.addressof(out), dict_size,
                                     C.addressof(p)))
    return bytes(out[:r])


def decompressedSize(src, dict_len=0):
    """zlz4_decompressed_size: what decompressSafe (dict_len == 0) or decompressSafeUsingDict with a dictionary of
    dict_len bytes returns for `src` into a destination of 0xFFFFFFFF bytes; errors raise Lz4Error.  Nothing is decoded."""
    s, n = _in(src)
    return _check(lib().zlz4_decompressed_size(C.addressof(s), n, dict_len))


STREAM_TABLE_ENTRIES = 4096                           # Stream.hashTable, src/lz4.zig:752 (LZ4_HASH_SIZE_U32, :33)


class Stream:
    """lz4.Stream, the streaming compressor (src/lz4.zig:751-866).  `hashTable` is a numpy uint32[4096]; loadDict and
    compressFastContinue compute it on the device (zlz4_stream_load_dict / zlz4_stream_compress_fast_continue), the rest
    is host bookkeeping with the reference's field names.  `dictionary` keeps a copy of the loaded tail (the reference
    borrows the caller's slice).  The reference reads every table entry as a position in the CURRENT block, so a loaded
    dictionary only changes which in-block matches are found: no block refers to it and every block decodes with plain
    decompressSafe (reproduced, not a defect of this binding)."""
    byU32, byU16, byPtr = 1, 2, 3                     # TableType, src/lz4.zig:744-748

    def __init__(self):                               # Stream.init, :776-786
        import numpy as np
        self.hashTable = np.zeros(STREAM_TABLE_ENTRIES, dtype=np.uint32)
        self.dictionary = None
        self.dictCtx = None
        self.currentOffset = 0
        self.tableType = Stream.byU32
        self.dictSize = 0

    @classmethod
    def create(cls):                                  # :761-766
        return cls()

    def destroy(self):                                # :769-773
        pass

    @classmethod
    def init(cls):
        return cls()

    def resetFast(self):                              # :789-795
        self.hashTable[:] = 0
        self.dictionary = None
        self.dictCtx = None
        self.currentOffset = 0
        self.dictSize = 0

    def _table(self):
        return C.c_void_p(self.hashTable.ctypes.data)

    def loadDict(self, dict):
        """Stream.loadDict (:798-820) -> dictSize = min(len(dict), 65536)."""
        self.resetFast()                              # :799
        dk, dn = _in(dict)
        size = _check(lib().zlz4_stream_load_dict(self._table(), C.addressof(dk), dn))
        if size:
            self.dictionary = bytes(dict)[dn - size:]  # :805-806
            self.dictSize = size                      # :807
        return size

    def compressFastContinue(self, src, acceleration=1, dst_cap=None):
        """Stream.compressFastContinue (:822-836) -> the compressed block; the table is updated only when a block of 13
        or more bytes compresses (errors raise Lz4Error and leave it unchanged)."""
        cap = compressBound(len(src)) if dst_cap is None else dst_cap
        out = _run(lambda sp, n, dp, c: lib().zlz4_stream_compress_fast_continue(self._table(), sp, n, dp, c, acceleration),
                   src, cap)
        if len(src) >= 13:                            # :833 (:824-827 return before it)
            self.currentOffset = min(self.currentOffset + len(src), 0xFFFFFFFF)
        return out

    def saveDict(self, safeBuffer, maxDictSize):
        """Stream.saveDict (:839-855): copies the tail of the LOADED dictionary (not the compressed history) to the front
        of the writable buffer `safeBuffer`; returns the number of bytes copied."""
        if maxDictSize == 0:                          # :840
            return 0
        if self.dictionary is None:                   # :841
            return 0
        d = self.dictionary
        size = min(min(len(d), maxDictSize), 64 * 1024)   # :844
        if size > len(safeBuffer):                    # :846-850
            size = min(size, len(safeBuffer))
        safeBuffer[0:size] = d[len(d) - size:]        # :848 / :852
        return size


def createStream():
    """lz4.createStream, src/lz4.zig:858-860."""
    return Stream.create()


def freeStream(stream):
    """lz4.freeStream, src/lz4.zig:863-865."""
    stream.destroy()


class _SdState(C.Structure):
    """zlz4_stream_decode_t: StreamDecode's fields as byte addresses (0 = null)."""
    _fields_ = [("dict", C.c_uint64), ("dict_len", C.c_uint64), ("prefix", C.c_uint64), ("prefix_len", C.c_uint64)]


def _addr(buf):
    """Address and length of a buffer the caller owns (numpy array, bytearray, memoryview, ctypes array): the stream
    state compares these addresses, so the data is never copied."""
    import numpy as np
    a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf.reshape(-1).view(np.uint8)
    return (a.ctypes.data if a.size else 0), a.size


class StreamDecode:
    """lz4.StreamDecode (src/lz4.zig:870-951).  `dst` of decompressSafeContinue is a WRITABLE buffer of the caller
    (numpy uint8 array, bytearray, writable memoryview): its address is what the state records, as in the reference.
    The dictionary of setStreamDecode is borrowed the same way (keep it alive until it is consumed).  The fields
    externalDict / extDictSize / prefixEnd / prefixSize mirror the reference's as addresses and lengths; see the WARNING
    of zlz4_decompress_safe_continue in include/zlz4_amd.h for output placed below the previous output."""

    def __init__(self):                               # init, :893-901
        self._st = _SdState()
        self._dict_ref = None

    @classmethod
    def create(cls):                                  # :877-882
        return cls()

    def destroy(self):                                # :885-889
        pass

    @classmethod
    def init(cls):
        return cls()

    externalDict = property(lambda self: self._st.dict)
    extDictSize = property(lambda self: self._st.dict_len)
    prefixEnd = property(lambda self: self._st.prefix)
    prefixSize = property(lambda self: self._st.prefix_len)

    def setStreamDecode(self, dict):
        """:904-909; dict None = the null slice.  A bytes object is pinned by this stream until the next call."""
        if dict is None:
            lib().zlz4_set_stream_decode(C.byref(self._st), None, 0)
            self._dict_ref = None
            return
        if isinstance(dict, (bytes, str)):
            dict = bytearray(dict)
        p, n = _addr(dict)
        if p == 0:                                    # an empty slice still has an address
            dict = bytearray(1)
            p, n = _addr(dict)[0], 0
        self._dict_ref = dict
        lib().zlz4_set_stream_decode(C.byref(self._st), C.c_void_p(p), n)

    def decompressSafeContinue(self, src, dst):
        """:912-939 -> bytes written to dst[0:r]; errors raise Lz4Error and leave the state unchanged."""
        s, n = _in(src)
        p, cap = _addr(dst)
        return _check(lib().zlz4_decompress_safe_continue(C.byref(self._st), C.addressof(s), n, C.c_void_p(p), cap))


def createStreamDecode():
    """lz4.createStreamDecode, src/lz4.zig:943-945."""
    return StreamDecode.create()


def freeStreamDecode(stream):
    """lz4.freeStreamDecode, src/lz4.zig:948-950."""
    stream.destroy()


def decoderRingBufferSize(maxBlockSize):
    """lz4.decoderRingBufferSize, src/lz4.zig:954-957."""
    return lib().zlz4_decoder_ring_buffer_size(maxBlockSize)


def sizeofState():
    """lz4.sizeofState, src/lz4.zig:524-526."""
    return lib().zlz4_sizeof_state()


def compressFastExtState(state_len, src, acceleration, dst_cap=None):
    """lz4.compressFastExtState(state, src, dst, acceleration), src/lz4.zig:531-546 (state given by its length)."""
    cap = compressBound(len(src)) if dst_cap is None else dst_cap
    s, n = _in(src)
    st = (C.c_uint8 * max(1, state_len))()
    d = (C.c_uint8 * max(1, cap))()
    r = _check(lib().zlz4_compress_fast_ext_state(C.addressof(st), state_len, C.addressof(s), n, C.addressof(d), cap, acceleration))
    return bytes(d[:r])


def compressDestSize(src, dst_cap):
    """lz4.compressDestSize(src, dst, &srcSize), src/lz4.zig:551-616 -> (compressed bytes, consumed source bytes)."""
    s, n = _in(src)
    d = (C.c_uint8 * max(1, dst_cap))()
    ss = C.c_size_t(n)
    r = _check(lib().zlz4_compress_dest_size(C.addressof(s), C.addressof(d), dst_cap, C.byref(ss)))
    return bytes(d[:r]), ss.value


class lz4f:
    """Mirror of the `lz4f` namespace (src/root.zig:54-55, src/lz4f.zig)."""
    MAGICNUMBER = 0x184D2204
    Preferences = Prefs

    @staticmethod
    def compressFrameBound(src_size, prefs=None):
        return lib().zlz4f_compress_frame_bound(src_size, C.byref(prefs) if prefs is not None else None)

    @staticmethod
    def compressFrame(src, prefs=None, dst_cap=None, flags=0):
        """flags 0: zlz4f_compress_frame.  Batch flags (lz4f.BATCH_LINK_BLOCKS, lz4f.BATCH_CONTENT_SIZE):
        zlz4f_compress_frame_ex, one frame through the batch pipeline -- linked blocks at the fast level and at the HC
        levels 3..9."""
        cap = lz4f.compressFrameBound(len(src), prefs) if dst_cap is None else dst_cap
        if flags == 0:
            return _run(lib().zlz4f_compress_frame, src, cap, C.byref(prefs) if prefs is not None else None)
        return _run(lib().zlz4f_compress_frame_ex, src, cap, C.byref(prefs) if prefs is not None else None, flags)

    @staticmethod
    def decompressFrame(src, dst_cap, flags=0):
        """flags 0: zlz4f_decompress_frame.  lz4f.DECODE_LINKED: zlz4f_decompress_frame_ex, which also reads frames whose
        blocks refer to earlier output (liblz4's default)."""
        if flags == 0:
            return _run(lib().zlz4f_decompress_frame, src, dst_cap)
        return _run(lib().zlz4f_decompress_frame_ex, src, dst_cap, flags)

    @staticmethod
    def headerSize(src):
        s, n = _in(src)
        return _check(lib().zlz4f_header_size(C.addressof(s), n))

    # device-resident variants (torch CUDA uint8 tensors in, frame / content size out)
    @staticmethod
    def compressFrameDevice(d_src, d_dst, prefs=None, flags=0):
        if flags:
            return _check(lib().zlz4f_compress_frame_device_ex(_stream(), _ptr(d_src), d_src.numel(), _ptr(d_dst),
                                                               d_dst.numel(), C.byref(prefs) if prefs is not None else None,
                                                               flags))
        return _check(lib().zlz4f_compress_frame_device(_stream(), _ptr(d_src), d_src.numel(), _ptr(d_dst), d_dst.numel(),
                                                        C.byref(prefs) if prefs is not None else None))

    @staticmethod
    def decompressFrameDevice(d_frame, frame_len, d_dst, flags=0):
        if flags:
            return _check(lib().zlz4f_decompress_frame_device_ex(_stream(), _ptr(d_frame), frame_len, _ptr(d_dst),
                                                                 d_dst.numel(), flags))
        return _check(lib().zlz4f_decompress_frame_device(_stream(), _ptr(d_frame), frame_len, _ptr(d_dst), d_dst.numel()))

    SEG_FIRST, SEG_LAST = 1, 2

    @staticmethod
    def compressFrameSegmentDevice(d_src, d_dst, prefs, seg_flags):
        """One rank's block segment of a frame split over several GPUs (include/zlz4_amd.h)."""
        return _check(lib().zlz4f_compress_frame_segment_device(_stream(), _ptr(d_src), d_src.numel(), _ptr(d_dst),
                                                                d_dst.numel(), C.byref(prefs) if prefs is not None else None,
                                                                seg_flags))

    @staticmethod
    def decompressFrameSegmentDevice(d_seg, seg_len, d_dst, prefs, seg_flags):
        return _check(lib().zlz4f_decompress_frame_segment_device(_stream(), _ptr(d_seg), seg_len, _ptr(d_dst), d_dst.numel(),
                                                                  C.byref(prefs) if prefs is not None else None, seg_flags))

    # batch frames (include/zlz4_amd.h section 3): N independent frames per call, device descriptors, asynchronous
    BATCH_CONTENT_SIZE = 1
    BATCH_LINK_BLOCKS = 4       # compress: block k against the 64 KiB of input in front of it (include/zlz4_amd.h)
    DECODE_LINKED = 1           # decode `flags`: frames that declare linked blocks are decoded with their history
    BLOCK_SIZES = {0: 64 << 10, 4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}     # BlockSizeID.toBlockSize

    @staticmethod
    def compressFrameBatchWorkspace(nframes, max_blocks, prefs=None, batch_flags=0):
        return lib().zlz4f_batch_compress_frame_workspace_ex(nframes, max_blocks,
                                                             C.byref(prefs) if prefs is not None else None, batch_flags)

    @staticmethod
    def decompressFrameBatchWorkspace(nframes, max_blocks, flags=0):
        return lib().zlz4f_batch_decompress_frame_workspace_ex(nframes, max_blocks, flags)

    @staticmethod
    def compressFrameBatch(d_src, src_off, src_len, d_dst, dst_off, dst_cap, result, prefs=None, batch_flags=0,
                           max_blocks=None, workspace=None):
        """zlz4f_batch_compress_frame_ex (the plain call, and linked blocks at the HC levels 3..9) on torch CUDA tensors: d_src / d_dst uint8, src_off / src_len / dst_off / dst_cap
        int64 (one entry per frame), result int64 (frame size or the frame's error code).  max_blocks defaults to the
        total block count of the lengths (read back once), workspace to a fresh buffer of the size the library asks for.
        Enqueued on the current stream; nothing is synchronised."""
        import torch
        if max_blocks is None:
            bs = lz4f.BLOCK_SIZES.get(prefs.block_size_id if prefs is not None else 0, 64 << 10)
            max_blocks = int(((src_len.cpu() + bs - 1) // bs).sum()) if src_len.numel() else 0
        pp = C.byref(prefs) if prefs is not None else None
        if workspace is None:
            workspace = torch.empty(max(1, lib().zlz4f_batch_compress_frame_workspace_ex(src_len.numel(), max_blocks, pp,
                                                                                         batch_flags)),
                                    dtype=torch.uint8, device=d_src.device)
        _check(lib().zlz4f_batch_compress_frame_ex(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(d_dst),
                                                   _ptr(dst_off), _ptr(dst_cap), _ptr(result), src_len.numel(), max_blocks,
                                                   pp, batch_flags, _ptr(workspace), workspace.numel()))

    @staticmethod
    def decompressFrameBatch(d_src, src_off, src_len, d_dst, dst_off, dst_cap, result, max_blocks=None, workspace=None,
                             flags=0):
        """zlz4f_batch_decompress_frame(_ex with `flags`, e.g. lz4f.DECODE_LINKED) on torch CUDA tensors (layout as
        compressFrameBatch; result = decompressed size or the frame's error code).  The block count of a frame is only known on the device, so the default max_blocks is
        one entry per started 256 frame bytes (reads the lengths back once): enough for frames whose blocks average 256
        bytes or more; pass the real count for anything denser, else such frames report InvalidState."""
        import torch
        if max_blocks is None:
            max_blocks = int((src_len.cpu() // 256 + 1).sum()) if src_len.numel() else 0
        if workspace is None:
            workspace = torch.empty(max(1, lib().zlz4f_batch_decompress_frame_workspace_ex(src_len.numel(), max_blocks,
                                                                                           flags)),
                                    dtype=torch.uint8, device=d_src.device)
        if flags == 0:
            _check(lib().zlz4f_batch_decompress_frame(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(d_dst),
                                                      _ptr(dst_off), _ptr(dst_cap), _ptr(result), src_len.numel(),
                                                      max_blocks, _ptr(workspace), workspace.numel()))
        else:
            _check(lib().zlz4f_batch_decompress_frame_ex(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(d_dst),
                                                         _ptr(dst_off), _ptr(dst_cap), _ptr(result), src_len.numel(),
                                                         max_blocks, flags, _ptr(workspace), workspace.numel()))

    @staticmethod
    def compressFrames(items, prefs=None, batch_flags=0, device="cuda"):
        """Every byte string of `items` as its own frame, in one batch call -> list of frames (bytes) or error codes."""
        import torch
        lens = [len(b) for b in items]
        caps = [lz4f.compressFrameBound(n, prefs) for n in lens]
        d_src, src_off, src_len = _stage(items, device)
        dst_off = torch.tensor(_offsets(caps), dtype=torch.int64, device=device)
        d_dst = torch.empty(max(1, sum(caps)), dtype=torch.uint8, device=device)
        result = torch.empty(len(items), dtype=torch.int64, device=device)
        lz4f.compressFrameBatch(d_src, src_off, src_len, d_dst, dst_off,
                                torch.tensor(caps, dtype=torch.int64, device=device), result, prefs, batch_flags)
        return _unstage(d_dst, _offsets(caps), result)

    @staticmethod
    def frameDecompressedSize(src, flags=0):
        """zlz4f_frame_decompressed_size(_ex with `flags`): what decompressFrame returns for `src` into a destination that
        is large enough (the content checksum is not verified); errors raise Lz4Error.  Nothing is decoded."""
        s, n = _in(src)
        if flags:
            return _check(lib().zlz4f_frame_decompressed_size_ex(C.addressof(s), n, flags))
        return _check(lib().zlz4f_frame_decompressed_size(C.addressof(s), n))

    @staticmethod
    def frameDecompressedSizeBatchWorkspace(nframes, max_blocks, flags=0):
        return lib().zlz4f_batch_frame_decompressed_size_workspace_ex(nframes, max_blocks, flags)

    @staticmethod
    def frameDecompressedSizeBatch(d_src, src_off, src_len, size, max_blocks=None, workspace=None, flags=0):
        """zlz4f_batch_frame_decompressed_size on torch CUDA tensors (layout as decompressFrameBatch; size int64 = decoded
        size or the frame's error code).  max_blocks defaults as in decompressFrameBatch."""
        import torch
        if max_blocks is None:
            max_blocks = int((src_len.cpu() // 256 + 1).sum()) if src_len.numel() else 0
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_frame_decompressed_size_workspace_ex(src_len.numel(),
                                                                                                   max_blocks, flags)),
                                    dtype=torch.uint8, device=d_src.device)
        if flags == 0:
            _check(lib().zlz4f_batch_frame_decompressed_size(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len),
                                                             _ptr(size), src_len.numel(), max_blocks, _ptr(workspace),
                                                             workspace.numel()))
        else:
            _check(lib().zlz4f_batch_frame_decompressed_size_ex(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len),
                                                                _ptr(size), src_len.numel(), max_blocks, flags,
                                                                _ptr(workspace), workspace.numel()))

    @staticmethod
    def decompressFrames(frames, caps=None, device="cuda", flags=0):
        """Every frame of `frames` decoded into a destination of caps[f] bytes, in one batch call -> list of contents
        (bytes) or error codes.  caps None: the sizes are queried first (frameDecompressedSizeBatch) and every frame gets
        exactly its size (a frame the query fails gets no room and reports the query's code)."""
        import torch
        d_src, src_off, src_len = _stage(frames, device)
        sizes = None
        if caps is None:
            size = torch.empty(len(frames), dtype=torch.int64, device=device)
            lz4f.frameDecompressedSizeBatch(d_src, src_off, src_len, size,
                                            max_blocks=sum(_chain_blocks(bytes(f)) for f in frames), flags=flags)
            sizes = size.cpu().tolist()
            caps = [max(s, 0) for s in sizes]
        caps = list(caps)
        dst_off = torch.tensor(_offsets(caps), dtype=torch.int64, device=device)
        d_dst = torch.empty(max(1, sum(caps)), dtype=torch.uint8, device=device)
        result = torch.empty(len(frames), dtype=torch.int64, device=device)
        lz4f.decompressFrameBatch(d_src, src_off, src_len, d_dst, dst_off,
                                  torch.tensor(caps, dtype=torch.int64, device=device), result,
                                  max_blocks=sum(_chain_blocks(bytes(f)) for f in frames), flags=flags)
        out = _unstage(d_dst, _offsets(caps), result)
        if sizes is not None:                         # (a frame the query failed got no room: the query's code stands)
            out = [o if s >= 0 else s for o, s in zip(out, sizes)]
        return out

    # dictionary frames (include/zlz4_amd.h: the _using_dict frame calls)
    @staticmethod
    def compressFrameUsingDict(src, dict, prefs=None, dst_cap=None):
        """zlz4f_compress_frame_using_dict: one frame whose blocks are compressed against `dict` (fast level;
        prefs.block_mode 1: every block, 0: block 0, the later blocks against the input in front of them)."""
        cap = lz4f.compressFrameBound(len(src), prefs) if dst_cap is None else dst_cap
        d, dn = _in(dict if dict is not None else b"")
        return _run(lib().zlz4f_compress_frame_using_dict, src, cap, C.byref(prefs) if prefs is not None else None,
                    C.addressof(d) if dn else None, dn)

    @staticmethod
    def compressFrameUsingDictEx(src, dict, prefs=None, dst_cap=None):
        """zlz4f_compress_frame_using_dict_ex: compressFrameUsingDict, and the HC levels 3..9 (prefs.compression_level;
        block 0 / every block is compressHCUsingDict against `dict`)."""
        cap = lz4f.compressFrameBound(len(src), prefs) if dst_cap is None else dst_cap
        d, dn = _in(dict if dict is not None else b"")
        return _run(lib().zlz4f_compress_frame_using_dict_ex, src, cap, C.byref(prefs) if prefs is not None else None,
                    C.addressof(d) if dn else None, dn)

    @staticmethod
    def decompressFrameUsingDict(src, dst_cap, dict):
        """zlz4f_decompress_frame_using_dict: what liblz4's LZ4F_decompress_usingDict gives for `src` and `dict`."""
        d, dn = _in(dict if dict is not None else b"")
        return _run(lib().zlz4f_decompress_frame_using_dict, src, dst_cap, C.addressof(d) if dn else None, dn)

    @staticmethod
    def frameDecompressedSizeUsingDict(src, dict_len):
        s, n = _in(src)
        return _check(lib().zlz4f_frame_decompressed_size_using_dict(C.addressof(s), n, dict_len))

    @staticmethod
    def compressFrameUsingDictBatchWorkspace(nframes, max_blocks, prefs=None, batch_flags=0, ndicts=1, max_src_len=0,
                                             max_dict_len=65536):
        return lib().zlz4f_batch_compress_frame_using_dict_workspace(nframes, max_blocks,
                                                                     C.byref(prefs) if prefs is not None else None,
                                                                     batch_flags, ndicts, max_src_len, max_dict_len)

    @staticmethod
    def compressFrameUsingDictBatchWorkspaceEx(nframes, max_blocks, prefs=None, batch_flags=0, ndicts=1, max_src_len=0,
                                               max_dict_len=65536):
        """zlz4f_batch_compress_frame_using_dict_workspace_ex (at levels 3..9 max_dict_len changes the size)."""
        return lib().zlz4f_batch_compress_frame_using_dict_workspace_ex(nframes, max_blocks,
                                                                        C.byref(prefs) if prefs is not None else None,
                                                                        batch_flags, ndicts, max_src_len, max_dict_len)

    @staticmethod
    def decompressFrameUsingDictBatchWorkspace(nframes, max_blocks):
        return lib().zlz4f_batch_decompress_frame_using_dict_workspace(nframes, max_blocks)

    @staticmethod
    def frameDecompressedSizeUsingDictBatchWorkspace(nframes, max_blocks):
        return lib().zlz4f_batch_frame_decompressed_size_using_dict_workspace(nframes, max_blocks)

    @staticmethod
    def compressFrameUsingDictBatch(d_src, src_off, src_len, d_dst, dst_off, dst_cap, result, d_dict, dict_off, dict_len,
                                    dict_idx=None, prefs=None, batch_flags=0, max_blocks=None, max_src_len=0,
                                    max_dict_len=65536, workspace=None):
        """zlz4f_batch_compress_frame_using_dict on torch CUDA tensors (layout as compressFrameBatch): dictionary d is
        d_dict[dict_off[d] .. + dict_len[d]) (int64 offsets, int32 lengths), frame f uses dictionary dict_idx[f] (int32;
        None: dictionary 0).  Enqueued on the current stream; nothing is synchronised."""
        import torch
        if max_blocks is None:
            bs = lz4f.BLOCK_SIZES.get(prefs.block_size_id if prefs is not None else 0, 64 << 10)
            max_blocks = int(((src_len.cpu() + bs - 1) // bs).sum()) if src_len.numel() else 0
        pp = C.byref(prefs) if prefs is not None else None
        nd = dict_len.numel()
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_compress_frame_using_dict_workspace(
                src_len.numel(), max_blocks, pp, batch_flags, nd, max_src_len, max_dict_len)), dtype=torch.uint8,
                device=d_src.device)
        _check(lib().zlz4f_batch_compress_frame_using_dict(
            _stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(d_dst), _ptr(dst_off), _ptr(dst_cap), _ptr(result),
            src_len.numel(), max_blocks, pp, batch_flags, _ptr(d_dict), _ptr(dict_off), _ptr(dict_len), nd, _ptr(dict_idx),
            max_src_len, max_dict_len, _ptr(workspace), workspace.numel()))

    @staticmethod
    def compressFrameUsingDictBatchEx(d_src, src_off, src_len, d_dst, dst_off, dst_cap, result, d_dict, dict_off, dict_len,
                                      dict_idx=None, prefs=None, batch_flags=0, max_blocks=None, max_src_len=0,
                                      max_dict_len=65536, workspace=None):
        """zlz4f_batch_compress_frame_using_dict_ex on torch CUDA tensors: compressFrameUsingDictBatch, and the HC levels
        3..9 (prefs.compression_level).  The same parameters; the workspace is that of
        compressFrameUsingDictBatchWorkspaceEx."""
        import torch
        if max_blocks is None:
            bs = lz4f.BLOCK_SIZES.get(prefs.block_size_id if prefs is not None else 0, 64 << 10)
            max_blocks = int(((src_len.cpu() + bs - 1) // bs).sum()) if src_len.numel() else 0
        pp = C.byref(prefs) if prefs is not None else None
        nd = dict_len.numel()
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_compress_frame_using_dict_workspace_ex(
                src_len.numel(), max_blocks, pp, batch_flags, nd, max_src_len, max_dict_len)), dtype=torch.uint8,
                device=d_src.device)
        _check(lib().zlz4f_batch_compress_frame_using_dict_ex(
            _stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(d_dst), _ptr(dst_off), _ptr(dst_cap), _ptr(result),
            src_len.numel(), max_blocks, pp, batch_flags, _ptr(d_dict), _ptr(dict_off), _ptr(dict_len), nd, _ptr(dict_idx),
            max_src_len, max_dict_len, _ptr(workspace), workspace.numel()))

    @staticmethod
    def decompressFrameUsingDictBatch(d_src, src_off, src_len, d_dst, dst_off, dst_cap, result, d_dict, dict_off, dict_len,
                                      dict_idx=None, max_blocks=None, workspace=None):
        """zlz4f_batch_decompress_frame_using_dict on torch CUDA tensors (layout as decompressFrameBatch, dictionaries as
        compressFrameUsingDictBatch); max_blocks defaults as in decompressFrameBatch."""
        import torch
        if max_blocks is None:
            max_blocks = int((src_len.cpu() // 256 + 1).sum()) if src_len.numel() else 0
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_decompress_frame_using_dict_workspace(src_len.numel(),
                                                                                                    max_blocks)),
                                    dtype=torch.uint8, device=d_src.device)
        _check(lib().zlz4f_batch_decompress_frame_using_dict(
            _stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(d_dst), _ptr(dst_off), _ptr(dst_cap), _ptr(result),
            src_len.numel(), max_blocks, _ptr(d_dict), _ptr(dict_off), _ptr(dict_len), dict_len.numel(), _ptr(dict_idx),
            _ptr(workspace), workspace.numel()))

    @staticmethod
    def frameDecompressedSizeUsingDictBatch(d_src, src_off, src_len, size, dict_len, dict_idx=None, max_blocks=None,
                                            workspace=None):
        """zlz4f_batch_frame_decompressed_size_using_dict on torch CUDA tensors: only the dictionary lengths (int32) are
        needed."""
        import torch
        if max_blocks is None:
            max_blocks = int((src_len.cpu() // 256 + 1).sum()) if src_len.numel() else 0
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_frame_decompressed_size_using_dict_workspace(
                src_len.numel(), max_blocks)), dtype=torch.uint8, device=d_src.device)
        _check(lib().zlz4f_batch_frame_decompressed_size_using_dict(
            _stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(size), src_len.numel(), max_blocks, _ptr(dict_len),
            dict_len.numel(), _ptr(dict_idx), _ptr(workspace), workspace.numel()))

    @staticmethod
    def frameDictIDBatch(d_src, src_off, src_len, dict_id):
        """zlz4f_batch_frame_dict_id: dict_id[f] (int64) = the header's dictID, 0 without one, or the header's error."""
        _check(lib().zlz4f_batch_frame_dict_id(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(dict_id),
                                               src_len.numel()))

    @staticmethod
    def frameDictIDs(frames, device="cuda"):
        """The dictID of every frame of `frames` (0: none; a negative code: the header's error) -> list of ints."""
        import torch
        if len(frames) == 0:
            return []
        d_src, src_off, src_len = _stage(frames, device)
        ids = torch.empty(len(frames), dtype=torch.int64, device=device)
        lz4f.frameDictIDBatch(d_src, src_off, src_len, ids)
        return ids.cpu().tolist()

    @staticmethod
    def _stage_dicts(dicts, dict_index, n, device):
        import torch
        dbytes = [bytes(d) if d is not None else b"" for d in dicts]
        d_dict, dict_off, dict_len = _stage(dbytes, device)
        idx = None if dict_index is None else torch.tensor([int(k) for k in dict_index], dtype=torch.int32, device=device)
        return d_dict, dict_off, dict_len.to(torch.int32), idx, dbytes

    @staticmethod
    def compressFramesUsingDict(items, dicts, dict_index=None, prefs=None, device="cuda"):
        """Every byte string of `items` as its own frame against dicts[dict_index[f]] (dict_index None: dicts[0] for every
        frame), in one batch call -> list of frames (bytes) or error codes.  Goes through the _ex call, so
        prefs.compression_level may be 3..9 (at the fast level the frames are compressFrameUsingDictBatch's)."""
        import torch
        if len(items) == 0:
            return []
        lens = [len(b) for b in items]
        caps = [lz4f.compressFrameBound(n, prefs) for n in lens]
        d_src, src_off, src_len = _stage(items, device)
        d_dict, dict_off, dict_len, idx, dbytes = lz4f._stage_dicts(dicts, dict_index, len(items), device)
        dst_off = torch.tensor(_offsets(caps), dtype=torch.int64, device=device)
        d_dst = torch.empty(max(1, sum(caps)), dtype=torch.uint8, device=device)
        result = torch.empty(len(items), dtype=torch.int64, device=device)
        lz4f.compressFrameUsingDictBatchEx(d_src, src_off, src_len, d_dst, dst_off,
                                           torch.tensor(caps, dtype=torch.int64, device=device), result, d_dict, dict_off,
                                           dict_len, idx, prefs, 0, max_src_len=max(lens),
                                           max_dict_len=min(65536, max((len(d) for d in dbytes), default=0)))
        return _unstage(d_dst, _offsets(caps), result)

    @staticmethod
    def decompressFramesUsingDict(frames, dicts, dict_index=None, caps=None, device="cuda"):
        """Every frame of `frames` decoded with dicts[dict_index[f]] (dict_index None: dicts[0]) into caps[f] bytes, in one
        batch call -> list of contents (bytes) or error codes.  caps None: the sizes are queried first, as in
        decompressFrames."""
        import torch
        if len(frames) == 0:
            return []
        d_src, src_off, src_len = _stage(frames, device)
        d_dict, dict_off, dict_len, idx, _ = lz4f._stage_dicts(dicts, dict_index, len(frames), device)
        mb = sum(_chain_blocks(bytes(f)) for f in frames)
        sizes = None
        if caps is None:
            size = torch.empty(len(frames), dtype=torch.int64, device=device)
            lz4f.frameDecompressedSizeUsingDictBatch(d_src, src_off, src_len, size, dict_len, idx, max_blocks=mb)
            sizes = size.cpu().tolist()
            caps = [max(s, 0) for s in sizes]
        caps = list(caps)
        dst_off = torch.tensor(_offsets(caps), dtype=torch.int64, device=device)
        d_dst = torch.empty(max(1, sum(caps)), dtype=torch.uint8, device=device)
        result = torch.empty(len(frames), dtype=torch.int64, device=device)
        lz4f.decompressFrameUsingDictBatch(d_src, src_off, src_len, d_dst, dst_off,
                                           torch.tensor(caps, dtype=torch.int64, device=device), result, d_dict, dict_off,
                                           dict_len, idx, max_blocks=mb)
        out = _unstage(d_dst, _offsets(caps), result)
        if sizes is not None:
            out = [o if s >= 0 else s for o, s in zip(out, sizes)]
        return out

    # frame prefix decoding (include/zlz4_amd.h)
    @staticmethod
    def decompressFramePrefix(src, n, dict=None):
        """zlz4f_decompress_frame_prefix(_using_dict with `dict`): the first n bytes of the frame's content, or all of it
        where the frame holds fewer; a defect met before n bytes were out raises Lz4Error, one behind the cut does not."""
        if dict is None:
            return _run(lib().zlz4f_decompress_frame_prefix, src, n)
        d, dn = _in(dict)
        return _run(lib().zlz4f_decompress_frame_prefix_using_dict, src, n, C.addressof(d) if dn else None, dn)

    @staticmethod
    def decompressFramePrefixes(frames, n, dicts=None, dict_index=None, device="cuda"):
        """The first n bytes of every frame of `frames` (n: one int for all, or one per frame) in one launch, without a size
        query, a block table or a workspace: frame f's slot is n[f] bytes.  dicts / dict_index as in
        decompressFramesUsingDict.  -> list of prefixes (bytes; a frame that holds fewer bytes gives all of them) or error
        codes."""
        import torch
        nf = len(frames)
        if nf == 0:
            return []
        want = [int(n)] * nf if isinstance(n, int) else [int(x) for x in n]
        if len(want) != nf or any(w < 0 for w in want):
            raise ValueError("n: one length per frame, each >= 0")
        d_src, src_off, src_len = _stage(frames, device)
        offs = _offsets(want)
        d_dst = torch.empty(max(1, sum(want)), dtype=torch.uint8, device=device)
        result = torch.empty(nf, dtype=torch.int64, device=device)
        dst_off = torch.tensor(offs, dtype=torch.int64, device=device)
        dst_cap = torch.tensor(want, dtype=torch.int64, device=device)
        if dicts is None:
            batch_decompress_frame_prefix(d_src, src_off, src_len, d_dst, dst_off, dst_cap, result)
        else:
            d_dict, dict_off, dict_len, idx, _ = lz4f._stage_dicts(dicts, dict_index, nf, device)
            batch_decompress_frame_prefix(d_src, src_off, src_len, d_dst, dst_off, dst_cap, result, d_dict, dict_off,
                                          dict_len, idx)
        return _unstage(d_dst, offs, result)


    # frame index and range decoding (include/zlz4_amd.h)
    @staticmethod
    def frameIndexBatchWorkspace(nframes, max_blocks):
        return lib().zlz4f_batch_frame_index_workspace(nframes, max_blocks)

    @staticmethod
    def frameIndexBatch(d_src, src_off, src_len, index, idx_off, idx_cap, result, max_blocks, workspace=None):
        """zlz4f_batch_frame_index on torch CUDA tensors: index int64 [entries, 2] = (pos, dec) per entry, idx_off / idx_cap
        int64 per frame in entries, result int64 = the frame's block count or its error code."""
        import torch
        nf = src_len.numel()
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_frame_index_workspace(nf, max_blocks)), dtype=torch.uint8,
                                    device=d_src.device)
        _check(lib().zlz4f_batch_frame_index(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(index),
                                             _ptr(idx_off), _ptr(idx_cap), _ptr(result), nf, max_blocks, _ptr(workspace),
                                             workspace.numel()))

    @staticmethod
    def packRanges(ranges):
        """[(frame, a, b)] -> numpy uint64 [n, 3], the memory layout of zlz4f_range (frame in the low word of column 0, the
        reserved word 0)."""
        import numpy as np
        arr = np.zeros((len(ranges), 3), dtype=np.uint64)
        for i, (f, a, b) in enumerate(ranges):
            if not (0 <= f < 1 << 32 and 0 <= a < 1 << 64 and 0 <= b < 1 << 64):
                raise ValueError("range %d: frame is a u32, a and b are u64" % i)
            arr[i] = (f, a, b)
        return arr

    @staticmethod
    def planFrameRanges(index, idx_off, idx_n, ranges, dst_off, dst_cap, totals, align=0):
        """zlz4f_batch_plan_frame_ranges: ranges int64 [n, 3] (packRanges), dst_off / dst_cap int64 [n], totals int64 [2] =
        (arena bytes, items)."""
        _check(lib().zlz4f_batch_plan_frame_ranges(_stream(), _ptr(index), _ptr(idx_off), _ptr(idx_n), idx_n.numel(),
                                                   _ptr(ranges), ranges.shape[0], align, _ptr(dst_off), _ptr(dst_cap),
                                                   _ptr(totals)))

    @staticmethod
    def decompressFrameRangeBatchWorkspace(nranges, max_items):
        return lib().zlz4f_batch_decompress_frame_range_workspace(nranges, max_items)

    @staticmethod
    def decompressFrameRangeBatch(d_src, src_off, src_len, index, idx_off, idx_n, ranges, d_dst, dst_off, dst_cap, skip,
                                  result, max_items, workspace=None):
        """zlz4f_batch_decompress_frame_range: range r's wanted bytes are d_dst[dst_off[r] + skip[r] ..][: result[r]]."""
        import torch
        nr = ranges.shape[0]
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_decompress_frame_range_workspace(nr, max_items)),
                                    dtype=torch.uint8, device=d_src.device)
        _check(lib().zlz4f_batch_decompress_frame_range(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(index),
                                                        _ptr(idx_off), _ptr(idx_n), idx_n.numel(), _ptr(ranges), _ptr(d_dst),
                                                        _ptr(dst_off), _ptr(dst_cap), _ptr(skip), _ptr(result), nr,
                                                        max_items, _ptr(workspace), workspace.numel()))

    class FrameIndex:
        """What frameIndex returns: the staged frames (d_src, src_off, src_len), the device index (index, idx_off) and the
        per-frame results: idx_n on the device, `results` on the host (a block count or an error code per frame)."""

        def __init__(self, d_src, src_off, src_len, index, idx_off, idx_n, results):
            self.d_src, self.src_off, self.src_len = d_src, src_off, src_len
            self.index, self.idx_off, self.idx_n, self.results = index, idx_off, idx_n, results

    @staticmethod
    def frameIndex(frames, device="cuda"):
        """Stage `frames` and index them (zlz4f_batch_frame_index) -> FrameIndex, to be read any number of times with
        decompressFrameRanges.  A frame the size query fails keeps its error code in .results."""
        import torch
        nf = len(frames)
        d_src, src_off, src_len = _stage(frames, device)
        blocks = [_chain_blocks(bytes(f)) for f in frames]
        caps = [b + 1 for b in blocks]
        index = torch.zeros((max(1, sum(caps)), 2), dtype=torch.int64, device=device)
        idx_off = torch.tensor(_offsets(caps), dtype=torch.int64, device=device)
        idx_n = torch.zeros(nf, dtype=torch.int64, device=device)
        if nf:
            lz4f.frameIndexBatch(d_src, src_off, src_len, index, idx_off,
                                 torch.tensor(caps, dtype=torch.int64, device=device), idx_n, sum(blocks))
        return lz4f.FrameIndex(d_src, src_off, src_len, index, idx_off, idx_n, idx_n.cpu().tolist())

    @staticmethod
    def decompressFrameRanges(indexed, ranges, align=0):
        """Bytes [a, b) of frame `frame` for every (frame, a, b) of `ranges` (both clamped to the frame's size) -> list of
        bytes or error codes.  Plan, one read-back of the totals, decode, one read-back of the data."""
        import torch
        nr = len(ranges)
        if nr == 0:
            return []
        dev = indexed.d_src.device
        d_range = torch.from_numpy(lz4f.packRanges(ranges).view("int64")).to(dev)
        dst_off = torch.empty(nr, dtype=torch.int64, device=dev)
        dst_cap = torch.empty(nr, dtype=torch.int64, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        lz4f.planFrameRanges(indexed.index, indexed.idx_off, indexed.idx_n, d_range, dst_off, dst_cap, totals, align)
        arena, items = totals.cpu().tolist()
        d_dst = torch.empty(max(1, arena), dtype=torch.uint8, device=dev)
        skip = torch.empty(nr, dtype=torch.int64, device=dev)
        result = torch.empty(nr, dtype=torch.int64, device=dev)
        lz4f.decompressFrameRangeBatch(indexed.d_src, indexed.src_off, indexed.src_len, indexed.index, indexed.idx_off,
                                       indexed.idx_n, d_range, d_dst, dst_off, dst_cap, skip, result, items)
        back = torch.stack((dst_off, skip, result)).cpu().tolist()
        host = d_dst.cpu().numpy().tobytes()
        return [host[o + s:o + s + r] if r >= 0 else r for o, s, r in zip(*back)]

    @staticmethod
    def decompressFrameRange(src, a, b):
        """zlz4f_decompress_frame_range: bytes [a, b) of one frame in host memory (both clamped to the frame's size).  The
        index is built on every call; several reads of one frame: frameIndex + decompressFrameRanges."""
        s, n = _in(src)
        cap = max(0, min(b, 1 << 62) - a)
        if cap > 1 << 20:                              # (b may lie far behind the frame's end)
            cap = min(cap, max(0, lz4f.frameDecompressedSize(src) - a))
        d = (C.c_uint8 * max(1, cap))()
        r = _check(lib().zlz4f_decompress_frame_range(C.addressof(s), n, a, b, C.addressof(d), cap))
        return bytes(d[:r])

    # multiframe buffers: concatenated and skippable frames (include/zlz4_amd.h)
    MEMBER_FRAME, MEMBER_SKIPPABLE, MEMBER_SKIPPABLE_TRUNCATED = 1, 2, 3

    @staticmethod
    def multiframeSplitBatch(d_src, src_off, src_len, count, totals, member=None, mem_off=None, mem_cap=None,
                             item_first=None, item_off=None, item_len=None, result=None):
        """zlz4f_batch_multiframe_split on torch CUDA tensors: count int64 [nbuf], totals int64 [2] = (members, chain blocks).
        member None: count mode.  Else member int64 [entries, 3] = (pos, len, kind | buf << 32) per entry, mem_off / mem_cap
        int64 [nbuf] in entries, item_first int64 [nbuf + 1], item_off / item_len int64 [members], result int64 [nbuf]."""
        _check(lib().zlz4f_batch_multiframe_split(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), src_len.numel(),
                                                  _ptr(count), _ptr(totals), _ptr(member), _ptr(mem_off), _ptr(mem_cap),
                                                  _ptr(item_first), _ptr(item_off), _ptr(item_len), _ptr(result)))

    @staticmethod
    def multiframePlanBatch(size, item_first, dst_off, dst_cap, out_off, out_size, totals, align=0):
        """zlz4f_batch_multiframe_plan: size / dst_off / dst_cap int64 per item, out_off / out_size int64 per buffer, totals
        int64 [2] = (arena bytes, decoded bytes)."""
        _check(lib().zlz4f_batch_multiframe_plan(_stream(), _ptr(size), _ptr(item_first), out_size.numel(), align,
                                                 _ptr(dst_off), _ptr(dst_cap), _ptr(out_off), _ptr(out_size), _ptr(totals)))

    @staticmethod
    def multiframeFinishBatch(member, mem_off, split_result, item_first, size, item_result, result):
        """zlz4f_batch_multiframe_finish: result int64 [nbuf] = the decoded size of buffer s or the code of its first member
        that is not OK."""
        _check(lib().zlz4f_batch_multiframe_finish(_stream(), _ptr(member), _ptr(mem_off), _ptr(split_result),
                                                   _ptr(item_first), _ptr(size), _ptr(item_result), result.numel(),
                                                   _ptr(result)))

    # whole .lz4 files: legacy members in multiframe buffers (include/zlz4_amd.h)
    SPLIT_LEGACY = 1
    MEMBER_LEGACY = 4

    @staticmethod
    def multiframeSplitBatchEx(d_src, src_off, src_len, count, totals, member=None, mem_off=None, mem_cap=None,
                               item_first=None, item_off=None, item_len=None, result=None, split_flags=0, leg_len=None):
        """zlz4f_batch_multiframe_split_ex: as multiframeSplitBatch with totals int64 [4] = (members, frame chain blocks,
        legacy members, legacy blocks) and, in record mode, leg_len int64 [members]: the length of every legacy member's
        item, 0 for the others (item_len: the other way round)."""
        _check(lib().zlz4f_batch_multiframe_split_ex(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), src_len.numel(),
                                                     _ptr(count), _ptr(totals), _ptr(member), _ptr(mem_off), _ptr(mem_cap),
                                                     _ptr(item_first), _ptr(item_off), _ptr(item_len), _ptr(result),
                                                     split_flags, _ptr(leg_len)))

    @staticmethod
    def multiframeSelectBatch(member, mem_off, split_result, item_first, from_frame, from_legacy, out):
        """zlz4f_batch_multiframe_select: out[i] = from_legacy[i] for the item of a legacy member, else from_frame[i] (all
        int64 per item; out may be from_frame)."""
        _check(lib().zlz4f_batch_multiframe_select(_stream(), _ptr(member), _ptr(mem_off), _ptr(split_result),
                                                   _ptr(item_first), _ptr(from_frame), _ptr(from_legacy),
                                                   split_result.numel(), _ptr(out)))

    class MultiframeSplit:
        """What splitMultiframes returns: the staged buffers (d_src, src_off, src_len), the member table (member, mem_off,
        count), the item arrays of the frame batch calls (item_first, item_off, item_len), the split results on the device
        (result) and on the host (results), and the totals (nitems, max_blocks).  For the legacy frame calls: leg_len (None
        without legacy=True) and the totals nlegacy and legacy_blocks (0 without)."""

    class MultiframeDecode:
        """What decodeMultiframes returns: per item size, dst_off, dst_cap and item_result, per buffer out_off, out_size and
        result, and the arena d_dst; all on the device."""

    @staticmethod
    def splitMultiframes(buffers, device="cuda", legacy=False):
        """Stage `buffers` and delimit their members: count mode, one read-back of the totals, record mode.  legacy: legacy
        frames are members too (the _ex split with SPLIT_LEGACY)."""
        return lz4f.splitStaged(*_stage(buffers, device), legacy=legacy)

    @staticmethod
    def splitStaged(d_src, src_off, src_len, legacy=False):
        """splitMultiframes over buffers that are on the device already: buffer s is src_len[s] bytes at d_src + src_off[s]."""
        import torch
        sp = lz4f.MultiframeSplit()
        nbuf, device = src_len.numel(), d_src.device
        sp.d_src, sp.src_off, sp.src_len = d_src, src_off, src_len

        def i64(n):
            return torch.zeros(max(1, n), dtype=torch.int64, device=device)[:n]

        sp.leg_len, sp.nlegacy, sp.legacy_blocks = None, 0, 0
        if legacy:
            sp.count, totals = i64(nbuf), i64(4)
            lz4f.multiframeSplitBatchEx(sp.d_src, sp.src_off, sp.src_len, sp.count, totals, split_flags=lz4f.SPLIT_LEGACY)
            sp.nitems, sp.max_blocks, sp.nlegacy, sp.legacy_blocks = totals.cpu().tolist()
        else:
            sp.count, totals = i64(nbuf), i64(2)
            lz4f.multiframeSplitBatch(sp.d_src, sp.src_off, sp.src_len, sp.count, totals)
            sp.nitems, sp.max_blocks = totals.cpu().tolist()
        sp.member = torch.zeros((max(1, sp.nitems), 3), dtype=torch.int64, device=device)
        sp.item_first, sp.item_off, sp.item_len, sp.result = i64(nbuf + 1), i64(sp.nitems), i64(sp.nitems), i64(nbuf)
        if legacy:
            sp.leg_len = i64(sp.nitems)
            lz4f.multiframeSplitBatchEx(sp.d_src, sp.src_off, sp.src_len, sp.count, totals, sp.member, sp.item_first[:nbuf],
                                        sp.count, sp.item_first, sp.item_off, sp.item_len, sp.result, lz4f.SPLIT_LEGACY,
                                        sp.leg_len)
        else:
            lz4f.multiframeSplitBatch(sp.d_src, sp.src_off, sp.src_len, sp.count, totals, sp.member, sp.item_first[:nbuf],
                                      sp.count, sp.item_first, sp.item_off, sp.item_len, sp.result)
        sp.mem_off = sp.item_first[:nbuf]             # the member table is laid out as the items are
        sp.results = sp.result.cpu().tolist()
        return sp

    @staticmethod
    def multiframeMembers(buffers, device="cuda", legacy=False):
        """Per buffer the list of its members (pos, len, kind, nibble) -- kind one of lz4f.MEMBER_*, nibble the low four
        bits of a skippable magic -- or the split's error code.  legacy: as splitMultiframes."""
        if not len(buffers):
            return []
        sp = lz4f.splitMultiframes(buffers, device, legacy)
        rows = sp.member.cpu().tolist()
        first = sp.item_first.cpu().tolist()
        out = []
        for s, r in enumerate(sp.results):
            if r < 0:
                out.append(r)
                continue
            out.append([(pos, ln, kb & 0xFF, (kb >> 8) & 15) for pos, ln, kb in rows[first[s]:first[s] + r]])
        return out

    @staticmethod
    def decodeMultiframes(sp, flags=0, align=0, d_dst=None, dicts=None):
        """Size query, plan, one read-back of the arena size, decode and finish over a MultiframeSplit -> MultiframeDecode.
        d_dst: an arena of the caller's (at least the planned bytes), else one is allocated.  Where the split recorded
        legacy members (sp.nlegacy) the legacy size query and decode run over the same items and multiframeSelectBatch
        merges their answers into size and item_result.  dicts (a FileDicts): one dictionary per buffer, spread over the
        items by multiframeItemDictsBatch; the size query and the decode are then the _using_dict
        frame calls (which decode linked frames with their history; `flags` is not used then).  Legacy items see none."""
        import torch
        dev = sp.d_src.device
        nbuf, ni = sp.src_len.numel(), sp.nitems
        dd = lz4f.MultiframeDecode()

        def i64(n):
            return torch.zeros(max(1, n), dtype=torch.int64, device=dev)[:n]

        dd.size, dd.dst_off, dd.dst_cap, dd.item_result = i64(ni), i64(ni), i64(ni), i64(ni)
        dd.out_off, dd.out_size, dd.result, totals = i64(nbuf), i64(nbuf), i64(nbuf), i64(2)
        if ni and dicts is not None:
            item_idx = torch.zeros(ni, dtype=torch.int32, device=dev)
            lz4f.multiframeItemDictsBatch(sp.item_first, ni, dicts.idx, item_idx)
            lz4f.frameDecompressedSizeUsingDictBatch(sp.d_src, sp.item_off, sp.item_len, dd.size, dicts.dict_len, item_idx,
                                                     max_blocks=sp.max_blocks)
        elif ni:
            lz4f.frameDecompressedSizeBatch(sp.d_src, sp.item_off, sp.item_len, dd.size, max_blocks=sp.max_blocks,
                                            flags=flags)
        if sp.nlegacy:
            from_legacy = i64(ni)
            lz4f.legacyFrameDecompressedSizeBatch(sp.d_src, sp.item_off, sp.leg_len, from_legacy, None, sp.legacy_blocks)
            lz4f.multiframeSelectBatch(sp.member, sp.mem_off, sp.result, sp.item_first, dd.size, from_legacy, dd.size)
        lz4f.multiframePlanBatch(dd.size, sp.item_first, dd.dst_off, dd.dst_cap, dd.out_off, dd.out_size, totals, align)
        dd.arena_bytes, dd.decoded_bytes = totals.cpu().tolist()
        if d_dst is None:
            d_dst = torch.empty(max(1, dd.arena_bytes), dtype=torch.uint8, device=dev)
        elif d_dst.numel() < dd.arena_bytes:
            raise ValueError("d_dst holds %d bytes, the plan needs %d" % (d_dst.numel(), dd.arena_bytes))
        dd.d_dst = d_dst
        if ni and dicts is not None:
            lz4f.decompressFrameUsingDictBatch(sp.d_src, sp.item_off, sp.item_len, d_dst, dd.dst_off, dd.dst_cap,
                                               dd.item_result, dicts.d_dict, dicts.dict_off, dicts.dict_len, item_idx,
                                               max_blocks=sp.max_blocks)
        elif ni:
            lz4f.decompressFrameBatch(sp.d_src, sp.item_off, sp.item_len, d_dst, dd.dst_off, dd.dst_cap, dd.item_result,
                                      max_blocks=sp.max_blocks, flags=flags)
        if sp.nlegacy:
            lz4f.decompressLegacyFrameBatch(sp.d_src, sp.item_off, sp.leg_len, d_dst, dd.dst_off, dd.dst_cap, from_legacy,
                                            None, sp.legacy_blocks)
            lz4f.multiframeSelectBatch(sp.member, sp.mem_off, sp.result, sp.item_first, dd.item_result, from_legacy,
                                       dd.item_result)
        if nbuf:
            lz4f.multiframeFinishBatch(sp.member, sp.mem_off, sp.result, sp.item_first, dd.size, dd.item_result, dd.result)
        return dd

    @staticmethod
    def decompressMultiframes(buffers, flags=0, align=0, device="cuda", legacy=False):
        """Every buffer of `buffers` -- frames and skippable frames back to back, what a .lz4 file holds -- decoded in one
        batch: -> list of contents (the members' contents concatenated) or the code of the first member that is not OK.
        legacy: legacy frames (`lz4 -l`) are members too."""
        if flags & ~lz4f.DECODE_LINKED:
            _check(lib().zlz4f_decompress_multiframe(None, 0, None, 0, flags))
        if not len(buffers):
            return []
        dd = lz4f.decodeMultiframes(lz4f.splitMultiframes(buffers, device, legacy), flags, align)
        return _unstage(dd.d_dst, dd.out_off.cpu().tolist(), dd.result)

    @staticmethod
    def multiframeDecompressedSize(src, flags=0, legacy=False):
        """zlz4f_multiframe_decompressed_size: what decompressMultiframe returns for `src` into a destination that is large
        enough (content checksums are not verified); errors raise Lz4Error.  Nothing is decoded.  legacy: the _ex call with
        SPLIT_LEGACY."""
        s, n = _in(src)
        if legacy:
            return _check(lib().zlz4f_multiframe_decompressed_size_ex(C.addressof(s), n, flags, lz4f.SPLIT_LEGACY))
        return _check(lib().zlz4f_multiframe_decompressed_size(C.addressof(s), n, flags))

    @staticmethod
    def decompressMultiframe(src, flags=0, dst_cap=None, legacy=False):
        """zlz4f_decompress_multiframe: one buffer in host memory.  dst_cap None: the size is queried first.  legacy: the _ex
        calls with SPLIT_LEGACY."""
        cap = lz4f.multiframeDecompressedSize(src, flags, legacy) if dst_cap is None else dst_cap
        if legacy:
            return _run(lib().zlz4f_decompress_multiframe_ex, src, cap, flags, lz4f.SPLIT_LEGACY)
        return _run(lib().zlz4f_decompress_multiframe, src, cap, flags)

    @staticmethod
    def decompressFiles(buffers, align=0, device="cuda"):
        """Every buffer a whole .lz4 file -- modern frames (linked blocks too), skippable frames and legacy frames in any
        order -- decoded in one batch: -> what `lz4 -dc` prints for each file, or the code of the first member that is not
        OK.  decompressMultiframes(buffers, flags=DECODE_LINKED, legacy=True); a device that is no GPU raises DeviceError.
        Files written against a dictionary: decompressFilesUsingDict."""
        import torch
        if torch.device(device).type != "cuda":
            _check(ERR_DEVICE)
        return lz4f.decompressMultiframes(buffers, lz4f.DECODE_LINKED, align, device, legacy=True)

    @staticmethod
    def decompressFilesUsingDict(buffers, dicts, dict_index=None, align=0, device="cuda"):
        """decompressFiles for files written against a dictionary: file s is decoded with dicts[dict_index[s]] (dict_index
        None: dicts[0]) -> what `lz4 -dc -D dict` prints for each file, or the code of the first member that is not OK.
        Linked members are decoded with their history behind the dictionary; legacy members see no dictionary.  A
        dict_index outside dicts raises ValueError.  (A function of its own: decompressFiles keeps its three parameters.)"""
        import torch
        if torch.device(device).type != "cuda":
            _check(ERR_DEVICE)
        if dict_index is not None and (len(dict_index) != len(buffers) or
                                       any(not 0 <= int(k) < len(dicts) for k in dict_index)):
            raise ValueError("dict_index: one index into dicts per buffer")
        if dict_index is None and len(buffers) and not len(dicts):
            raise ValueError("dicts: at least one dictionary")
        if not len(buffers):
            return []
        dd = lz4f.decodeMultiframes(lz4f.splitMultiframes(buffers, device, True), 0, align,
                                    dicts=lz4f.stageFileDicts(dicts, dict_index, device))
        return _unstage(dd.d_dst, dd.out_off.cpu().tolist(), dd.result)

    @staticmethod
    def decompressFile(src):
        """One whole .lz4 file in host memory: decompressMultiframe(src, flags=DECODE_LINKED, legacy=True)."""
        return lz4f.decompressMultiframe(src, lz4f.DECODE_LINKED, legacy=True)

    # file index and file range decoding (include/zlz4_amd.h)
    @staticmethod
    def _split_totals(totals):
        t = [int(x) for x in totals]
        if len(t) != 4:
            raise ValueError("totals: the four totals of the record-mode split")
        return (C.c_uint64 * 4)(*t)

    @staticmethod
    def fileIndexBatchWorkspace(nbuf, totals):
        return lib().zlz4f_batch_file_index_workspace(nbuf, lz4f._split_totals(totals))

    @staticmethod
    def fileIndexBatch(d_src, src_off, src_len, member, mem_off, split_result, item_first, item_off, item_len, leg_len, totals,
                       index, idx_off, result, idx_cap=None, workspace=None):
        """zlz4f_batch_file_index on torch CUDA tensors: the buffers, the outputs of a record-mode split over them and its
        four totals (host integers); index int64 [entries, 2] = (pos, dec), idx_off int64 [nbuf + 1] (written by the call),
        result int64 [nbuf] = the file's block count or its code.  idx_cap None: the entries `index` holds."""
        import torch
        nbuf = src_len.numel()
        t = lz4f._split_totals(totals)
        if idx_cap is None:
            idx_cap = index.shape[0]
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_file_index_workspace(nbuf, t)), dtype=torch.uint8,
                                    device=d_src.device)
        _check(lib().zlz4f_batch_file_index(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), nbuf, _ptr(member),
                                            _ptr(mem_off), _ptr(split_result), _ptr(item_first), _ptr(item_off),
                                            _ptr(item_len), _ptr(leg_len), t, _ptr(index), _ptr(idx_off), idx_cap,
                                            _ptr(result), _ptr(workspace), workspace.numel()))

    @staticmethod
    def decompressFileRangeBatchWorkspace(nranges, max_items):
        return lib().zlz4f_batch_decompress_file_range_workspace(nranges, max_items)

    @staticmethod
    def decompressFileRangeBatch(d_src, src_off, src_len, index, idx_off, idx_n, member, mem_off, split_result, ranges, d_dst,
                                 dst_off, dst_cap, skip, result, max_items, workspace=None):
        """zlz4f_batch_decompress_file_range: range r's wanted bytes are d_dst[dst_off[r] + skip[r] ..][: result[r]]; the
        range's first field names the buffer."""
        import torch
        nr = ranges.shape[0]
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_decompress_file_range_workspace(nr, max_items)),
                                    dtype=torch.uint8, device=d_src.device)
        _check(lib().zlz4f_batch_decompress_file_range(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(index),
                                                       _ptr(idx_off), _ptr(idx_n), idx_n.numel(), _ptr(member),
                                                       _ptr(mem_off), _ptr(split_result), _ptr(ranges), _ptr(d_dst),
                                                       _ptr(dst_off), _ptr(dst_cap), _ptr(skip), _ptr(result), nr, max_items,
                                                       _ptr(workspace), workspace.numel()))

    # dictionary .lz4 files: one dictionary per file (include/zlz4_amd.h)
    @staticmethod
    def fileIndexUsingDictBatchWorkspace(nbuf, totals):
        return lib().zlz4f_batch_file_index_using_dict_workspace(nbuf, lz4f._split_totals(totals))

    @staticmethod
    def fileIndexUsingDictBatch(d_src, src_off, src_len, member, mem_off, split_result, item_first, item_off, item_len,
                                leg_len, totals, index, idx_off, result, dict_len, dict_idx=None, idx_cap=None, workspace=None):
        """zlz4f_batch_file_index_using_dict: fileIndexBatch with the dictionary lengths (int32 [ndicts]) and the dictionary
        of every buffer (dict_idx int32 [nbuf]; None: dictionary 0)."""
        import torch
        nbuf = src_len.numel()
        t = lz4f._split_totals(totals)
        if idx_cap is None:
            idx_cap = index.shape[0]
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_file_index_using_dict_workspace(nbuf, t)), dtype=torch.uint8,
                                    device=d_src.device)
        _check(lib().zlz4f_batch_file_index_using_dict(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), nbuf,
                                                       _ptr(member), _ptr(mem_off), _ptr(split_result), _ptr(item_first),
                                                       _ptr(item_off), _ptr(item_len), _ptr(leg_len), t, _ptr(index),
                                                       _ptr(idx_off), idx_cap, _ptr(result), _ptr(dict_len),
                                                       dict_len.numel(), _ptr(dict_idx), _ptr(workspace), workspace.numel()))

    @staticmethod
    def decompressFileRangeUsingDictBatchWorkspace(nranges, max_items):
        return lib().zlz4f_batch_decompress_file_range_using_dict_workspace(nranges, max_items)

    @staticmethod
    def decompressFileRangeUsingDictBatch(d_src, src_off, src_len, index, idx_off, idx_n, member, mem_off, split_result,
                                          ranges, d_dst, dst_off, dst_cap, skip, result, max_items, d_dict, dict_off,
                                          dict_len, dict_idx=None, workspace=None):
        """zlz4f_batch_decompress_file_range_using_dict: decompressFileRangeBatch with the dictionaries (layout as
        compressFrameUsingDictBatch) and the dictionary of every buffer (dict_idx int32 [nbuf]; None: dictionary 0)."""
        import torch
        nr = ranges.shape[0]
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_decompress_file_range_using_dict_workspace(nr, max_items)),
                                    dtype=torch.uint8, device=d_src.device)
        _check(lib().zlz4f_batch_decompress_file_range_using_dict(
            _stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(index), _ptr(idx_off), _ptr(idx_n), idx_n.numel(),
            _ptr(member), _ptr(mem_off), _ptr(split_result), _ptr(ranges), _ptr(d_dst), _ptr(dst_off), _ptr(dst_cap),
            _ptr(skip), _ptr(result), nr, max_items, _ptr(d_dict), _ptr(dict_off), _ptr(dict_len), dict_len.numel(),
            _ptr(dict_idx), _ptr(workspace), workspace.numel()))

    @staticmethod
    def multiframeItemDictsBatch(item_first, nitems, dict_idx, item_dict_idx):
        """zlz4f_batch_multiframe_item_dicts: item_dict_idx (int32 [nitems]) = the dict_idx (int32 [nbuf]; None: 0) of every
        item's buffer; item_first int64 [nbuf + 1]."""
        _check(lib().zlz4f_batch_multiframe_item_dicts(_stream(), _ptr(item_first), item_first.numel() - 1, nitems,
                                                       _ptr(dict_idx), _ptr(item_dict_idx)))

    class FileDicts:
        """Dictionaries staged for the file calls: d_dict, dict_off (int64), dict_len (int32) and idx (int32, one per file,
        or None: dictionary 0 for every file)."""

        def __init__(self, d_dict, dict_off, dict_len, idx):
            self.d_dict, self.dict_off, self.dict_len, self.idx = d_dict, dict_off, dict_len, idx

    @staticmethod
    def stageFileDicts(dicts, dict_index=None, device="cuda"):
        """`dicts` (byte strings) and the dictionary of every file (dict_index; None: dicts[0]) on the device -> FileDicts;
        dicts None -> None.  A FileDicts passes through."""
        if dicts is None or isinstance(dicts, lz4f.FileDicts):
            return dicts
        d_dict, dict_off, dict_len, idx, _ = lz4f._stage_dicts(dicts, dict_index, 0, device)
        return lz4f.FileDicts(d_dict, dict_off, dict_len, idx)

    class FileIndex:
        """What fileIndex returns: the staged buffers and their split (.split, a MultiframeSplit), the device index (index,
        idx_off) and the per-file results: idx_n on the device, `results` on the host (a block count or a code per file).
        dicts: the staged dictionaries (a FileDicts) the index was built with, or None; decompressFileRanges uses them."""

        def __init__(self, split, index, idx_off, idx_n, results, dicts=None):
            self.split, self.index, self.idx_off, self.idx_n, self.results = split, index, idx_off, idx_n, results
            self.d_src, self.src_off, self.src_len = split.d_src, split.src_off, split.src_len
            self.dicts = dicts

    @staticmethod
    def fileIndex(buffers, device="cuda", legacy=True, dicts=None, dict_index=None):
        """Stage `buffers` -- whole .lz4 files -- split them and index them (zlz4f_batch_file_index) -> FileIndex, to be read
        any number of times with decompressFileRanges.  A file whose size query fails keeps its code in .results.  legacy:
        legacy frames are members (False: a legacy magic is FrameTypeUnknown).  dicts: file s was written against
        dicts[dict_index[s]] (dict_index None: dicts[0]); the FileIndex keeps the staged dictionaries."""
        import torch
        if torch.device(device).type != "cuda":
            _check(ERR_DEVICE)
        return lz4f.indexSplit(lz4f.splitMultiframes(buffers, device, legacy), dicts, dict_index)

    @staticmethod
    def indexSplit(sp, dicts=None, dict_index=None):
        """fileIndex over a MultiframeSplit (splitMultiframes, splitStaged) -> FileIndex.  dicts: as fileIndex, or a
        FileDicts."""
        import torch
        nbuf, device = sp.src_len.numel(), sp.d_src.device
        cap = sp.max_blocks + sp.legacy_blocks + nbuf
        index = torch.zeros((max(1, cap), 2), dtype=torch.int64, device=device)
        idx_off = torch.zeros(nbuf + 1, dtype=torch.int64, device=device)
        idx_n = torch.zeros(nbuf, dtype=torch.int64, device=device)
        fd = lz4f.stageFileDicts(dicts, dict_index, device)
        totals = (sp.nitems, sp.max_blocks, sp.nlegacy, sp.legacy_blocks)
        if nbuf and fd is not None:
            lz4f.fileIndexUsingDictBatch(sp.d_src, sp.src_off, sp.src_len, sp.member, sp.mem_off, sp.result, sp.item_first,
                                         sp.item_off, sp.item_len, sp.leg_len, totals, index, idx_off, idx_n, fd.dict_len,
                                         fd.idx, cap)
        elif nbuf:
            lz4f.fileIndexBatch(sp.d_src, sp.src_off, sp.src_len, sp.member, sp.mem_off, sp.result, sp.item_first, sp.item_off,
                                sp.item_len, sp.leg_len, totals, index, idx_off, idx_n, cap)
        return lz4f.FileIndex(sp, index, idx_off, idx_n, idx_n.cpu().tolist(), fd)

    @staticmethod
    def decompressFileRanges(indexed, ranges, align=0):
        """Bytes [a, b) of file `buf` for every (buf, a, b) of `ranges` (both clamped to the file's size) -> list of bytes
        or error codes.  An index that carries dictionaries (indexed.dicts) is read with them.  Plan (planFrameRanges: the plan reads the index alone), one read-back of the totals, decode, one
        read-back of the data."""
        import torch
        nr = len(ranges)
        if nr == 0:
            return []
        sp = indexed.split
        dev = sp.d_src.device
        d_range = torch.from_numpy(lz4f.packRanges(ranges).view("int64")).to(dev)
        dst_off = torch.empty(nr, dtype=torch.int64, device=dev)
        dst_cap = torch.empty(nr, dtype=torch.int64, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        lz4f.planFrameRanges(indexed.index, indexed.idx_off, indexed.idx_n, d_range, dst_off, dst_cap, totals, align)
        arena, items = totals.cpu().tolist()
        d_dst = torch.empty(max(1, arena), dtype=torch.uint8, device=dev)
        skip = torch.empty(nr, dtype=torch.int64, device=dev)
        result = torch.empty(nr, dtype=torch.int64, device=dev)
        fd = getattr(indexed, "dicts", None)
        if fd is not None:
            lz4f.decompressFileRangeUsingDictBatch(sp.d_src, sp.src_off, sp.src_len, indexed.index, indexed.idx_off,
                                                   indexed.idx_n, sp.member, sp.mem_off, sp.result, d_range, d_dst, dst_off,
                                                   dst_cap, skip, result, items, fd.d_dict, fd.dict_off, fd.dict_len, fd.idx)
        else:
            lz4f.decompressFileRangeBatch(sp.d_src, sp.src_off, sp.src_len, indexed.index, indexed.idx_off, indexed.idx_n,
                                          sp.member, sp.mem_off, sp.result, d_range, d_dst, dst_off, dst_cap, skip, result,
                                          items)
        back = torch.stack((dst_off, skip, result)).cpu().tolist()
        host = d_dst.cpu().numpy().tobytes()
        return [host[o + s:o + s + r] if r >= 0 else r for o, s, r in zip(*back)]

    @staticmethod
    def decompressFilePrefixes(buffers, n, device="cuda", legacy=True, dicts=None, dict_index=None):
        """The first n bytes of every file (n: one int, or one per file): fileIndex plus the ranges (s, 0, n).  dicts,
        dict_index: as fileIndex."""
        ns = [n] * len(buffers) if isinstance(n, int) else list(n)
        if len(ns) != len(buffers):
            raise ValueError("n: one int, or one per buffer")
        if not len(buffers):
            return []
        return lz4f.decompressFileRanges(lz4f.fileIndex(buffers, device, legacy, dicts, dict_index),
                                         [(s, 0, k) for s, k in enumerate(ns)])

    @staticmethod
    def decompressFileRange(src, a, b, legacy=True, seek_table=False, dict=None):
        """zlz4f_decompress_file_range: bytes [a, b) of one file in host memory (both clamped to the file's size).  The
        index is built on every call; several reads of one file: fileIndex + decompressFileRanges.  seek_table:
        zlz4f_decompress_file_range_ex with RANGE_SEEK_TABLE -- the tables come from the file's seek table where it ends in
        a well-formed one.  dict: zlz4f_decompress_file_range_using_dict -- the file was written against `dict`."""
        s, n = _in(src)
        flags = lz4f.SPLIT_LEGACY if legacy else 0
        cap = max(0, min(b, 1 << 62) - a)
        if cap > 1 << 20 and dict is None:             # (b may lie far behind the file's end)
            cap = min(cap, max(0, lz4f.multiframeDecompressedSize(src, 0, legacy) - a))
        if dict is not None:                           # (no host size query takes a dictionary: the room grows on
            dd, dn = _in(dict)                         # DstMaxSizeTooSmall, which the call answers in front of the decode)
            want, cap = cap, min(cap, 1 << 20)
            while True:
                d = (C.c_uint8 * max(1, cap))()
                r = lib().zlz4f_decompress_file_range_using_dict(C.addressof(s), n, a, b, C.addressof(d), cap, flags,
                                                                 lz4f.RANGE_SEEK_TABLE if seek_table else 0,
                                                                 C.addressof(dd) if dn else None, dn)
                if r != -111 or cap >= want:
                    return bytes(d[:_check(r)])
                cap = min(want, cap * 16)
        d = (C.c_uint8 * max(1, cap))()
        if seek_table:
            r = _check(lib().zlz4f_decompress_file_range_ex(C.addressof(s), n, a, b, C.addressof(d), cap, flags,
                                                            lz4f.RANGE_SEEK_TABLE))
        else:
            r = _check(lib().zlz4f_decompress_file_range(C.addressof(s), n, a, b, C.addressof(d), cap, flags))
        return bytes(d[:r])

    # seekable files: a stored seek table and a writer for such files (include/zlz4_amd.h)
    SEEK_TABLE_MAGICNUMBER = 0x184D2A5C
    RANGE_SEEK_TABLE = 1

    @staticmethod
    def seekTableBound(nmembers, nblocks):
        """zlz4f_seek_table_bound: the bytes of the table of a file of nmembers members and nblocks blocks (0: too large)."""
        return lib().zlz4f_seek_table_bound(nmembers, nblocks)

    @staticmethod
    def appendSeekTableBatch(d_buf, buf_off, buf_len, buf_cap, member, mem_off, split_result, index, idx_off, idx_n, result):
        """zlz4f_batch_append_seek_table on torch CUDA tensors: buffer s is buf_len[s] bytes at d_buf + buf_off[s] with
        buf_cap[s] bytes of room from there; the record-mode split and the file index over the buffers; result int64 [nbuf]
        = the file's length with its table, or the refusal's code."""
        _check(lib().zlz4f_batch_append_seek_table(_stream(), _ptr(d_buf), _ptr(buf_off), _ptr(buf_len), _ptr(buf_cap),
                                                   buf_len.numel(), _ptr(member), _ptr(mem_off), _ptr(split_result),
                                                   _ptr(index), _ptr(idx_off), _ptr(idx_n), _ptr(result)))

    @staticmethod
    def loadSeekTableBatch(d_src, src_off, src_len, count, totals, member=None, mem_off=None, mem_cap=None, split_result=None,
                           index=None, idx_off=None, idx_n=None, idx_cap=None):
        """zlz4f_batch_load_seek_table: count int64 [nbuf], totals int64 [2] = (member rows, index entries).  member None:
        count mode.  Else member int64 [rows, 3], mem_off / mem_cap / split_result / idx_n int64 [nbuf], index int64
        [entries, 2], idx_off int64 [nbuf + 1] (written by the call).  idx_cap None: the entries `index` holds."""
        if idx_cap is None:
            idx_cap = index.shape[0] if index is not None else 0
        _check(lib().zlz4f_batch_load_seek_table(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), src_len.numel(),
                                                 _ptr(count), _ptr(totals), _ptr(member), _ptr(mem_off), _ptr(mem_cap),
                                                 _ptr(split_result), _ptr(index), _ptr(idx_off), idx_cap, _ptr(idx_n)))

    @staticmethod
    def concatBatchWorkspace(nitems):
        return lib().zlz4f_batch_concat_workspace(nitems)

    @staticmethod
    def concatBatch(d_src, item_off, item_len, item_first, d_dst, dst_off, dst_cap, result, workspace=None):
        """zlz4f_batch_concat: file s is the items item_first[s] .. item_first[s + 1] (item_off / item_len int64 per item,
        item_len as the compress call's result), laid back to back at d_dst + dst_off[s]; result int64 [nbuf] = the total,
        the first negative item length, or DstMaxSizeTooSmall against dst_cap[s]."""
        import torch
        ni = item_len.numel()
        if workspace is None:
            workspace = torch.empty(max(8, lib().zlz4f_batch_concat_workspace(ni)), dtype=torch.uint8, device=d_dst.device)
        _check(lib().zlz4f_batch_concat(_stream(), _ptr(d_src), _ptr(item_off), _ptr(item_len), _ptr(item_first),
                                        result.numel(), ni, _ptr(d_dst), _ptr(dst_off), _ptr(dst_cap), _ptr(result),
                                        _ptr(workspace), workspace.numel()))

    @staticmethod
    def _appendTables(ix, d_buf, buf_off, buf_cap):
        """the append over a FileIndex whose buffers stand in d_buf with room -> result tensor"""
        import torch
        sp = ix.split
        result = torch.zeros(sp.src_len.numel(), dtype=torch.int64, device=d_buf.device)
        lz4f.appendSeekTableBatch(d_buf, buf_off, sp.src_len, buf_cap, sp.member, sp.mem_off, sp.result, ix.index, ix.idx_off,
                                  ix.idx_n, result)
        return result

    @staticmethod
    def appendSeekTables(buffers, legacy=True, device="cuda", dicts=None, dict_index=None):
        """Every file of `buffers` with its seek table appended -> list of files (bytes) or the refusal's code: fileIndex,
        a copy of the files into slots with room (concatBatch, one item per file), the append, one read-back.  dicts,
        dict_index: as fileIndex (the table does not name the dictionary; the reader passes it again)."""
        import torch
        if not len(buffers):
            return []
        ix = lz4f.fileIndex(buffers, device, legacy, dicts, dict_index)
        sp = ix.split
        nbuf = len(buffers)
        caps = [len(b) + lz4f.seekTableBound(max(0, nm), max(0, nb)) for b, nm, nb in zip(buffers, sp.results, ix.results)]
        slots = [(c + 15) & ~15 for c in caps]
        t = lambda v: torch.tensor(v, dtype=torch.int64, device=device)    # noqa: E731
        buf_off, buf_cap = t(_offsets(slots)), t(caps)
        d_buf = torch.zeros(max(1, sum(slots)), dtype=torch.uint8, device=device)
        copied = torch.zeros(nbuf, dtype=torch.int64, device=device)
        lz4f.concatBatch(sp.d_src, sp.src_off, sp.src_len, t(list(range(nbuf + 1))), d_buf, buf_off, buf_cap, copied)
        return _unstage(d_buf, _offsets(slots), lz4f._appendTables(ix, d_buf, buf_off, buf_cap))

    @staticmethod
    def loadFileIndex(buffers, device="cuda", dicts=None, dict_index=None):
        """Stage `buffers` -- files that end in a seek table -- and load their tables (zlz4f_batch_load_seek_table: count
        mode, one read-back of the totals, record mode) -> FileIndex, which decompressFileRanges takes as it takes
        fileIndex's.  No block header is walked.  A file without a table, or with one out of shape, keeps its code
        (InvalidState) in .results.  The FileIndex's .split carries d_src, src_off, src_len, member, mem_off and result.
        dicts, dict_index: the dictionaries the files were written against (the table does not name them); they are staged
        and kept in the FileIndex, as fileIndex keeps them."""
        import torch
        if torch.device(device).type != "cuda":
            _check(ERR_DEVICE)
        nbuf = len(buffers)
        sp = lz4f.MultiframeSplit()
        sp.d_src, sp.src_off, sp.src_len = _stage(buffers, device)

        def i64(n):
            return torch.zeros(max(1, n), dtype=torch.int64, device=device)[:n]

        sp.count, totals = i64(nbuf), i64(2)
        lz4f.loadSeekTableBatch(sp.d_src, sp.src_off, sp.src_len, sp.count, totals)
        sp.nitems, rooms = totals.cpu().tolist()
        sp.member = torch.zeros((max(1, sp.nitems), 3), dtype=torch.int64, device=device)
        sp.mem_off = torch.cumsum(sp.count, 0) - sp.count if nbuf else i64(0)
        sp.result = i64(nbuf)
        index = torch.zeros((max(1, rooms), 2), dtype=torch.int64, device=device)
        idx_off, idx_n = torch.zeros(nbuf + 1, dtype=torch.int64, device=device), i64(nbuf)
        lz4f.loadSeekTableBatch(sp.d_src, sp.src_off, sp.src_len, sp.count, totals, sp.member, sp.mem_off, sp.count, sp.result,
                                index, idx_off, idx_n, rooms)
        sp.results = sp.result.cpu().tolist()
        return lz4f.FileIndex(sp, index, idx_off, idx_n, idx_n.cpu().tolist(), lz4f.stageFileDicts(dicts, dict_index, device))

    @staticmethod
    def seekTable(src, legacy=True):
        """zlz4f_seek_table: the seek table member of one file in host memory -> bytes; the caller appends them."""
        s, n = _in(src)
        flags = lz4f.SPLIT_LEGACY if legacy else 0
        cap = 1 << 12
        while True:
            d = (C.c_uint8 * cap)()
            r = lib().zlz4f_seek_table(C.addressof(s), n, C.addressof(d), cap, flags)
            if r != -111 or cap >= 1 << 33:             # DstMaxSizeTooSmall: the table is larger
                return bytes(d[:_check(r)])
            cap *= 16

    @staticmethod
    def compressFiles(items, prefs=None, frame_size=4 << 20, seek_table=True, batch_flags=0, device="cuda", dicts=None,
                      dict_index=None):
        """Every byte string of `items` as one seekable .lz4 file -> list of files (bytes) or error codes.  An input becomes
        ceil(len / frame_size) independent frames (an empty one: one empty frame), compressed in place as chunks of the
        staged inputs by compressFrameBatch and laid back to back on the device (concatBatch); with seek_table the files
        are split and indexed there (splitStaged, indexSplit) and their table is appended.
        dicts: file s is written against dicts[dict_index[s]] (dict_index None: dicts[0]): the chunks are compressed by
        compressFrameUsingDictBatchEx (prefs.compression_level 3..9: the HC dictionary compressor; 2 and 10..12 keep its
        refusal) and the index is built with the dictionary.  The seek table does not name the dictionary: the reader
        passes it again (loadFileIndex(files, dicts=...)).  A small frame_size trades ratio -- every frame starts from the
        dictionary alone and pays its header -- for less decoded per read.  prefs.block_mode == 0 (linked
        blocks) with frame_size above the block size raises ValueError: a linked frame of several blocks cannot be indexed."""
        import torch
        if frame_size < 1:
            raise ValueError("frame_size: at least 1")
        bs = lz4f.BLOCK_SIZES.get(prefs.block_size_id if prefs is not None else 0, 64 << 10)
        if dicts is not None and (prefs is None or prefs.block_mode == 0) and frame_size > bs:
            raise ValueError("linked blocks (prefs.block_mode 0) with frame_size above the block size: not indexable")
        nbuf = len(items)
        if not nbuf:
            return []
        lens = [len(b) for b in items]
        d_src, _, _ = _stage(items, device)
        c_off, c_len, first, blocks = [], [], [0], []
        for o, n in zip(_offsets(lens), lens):
            for j in range(max(1, -(-n // frame_size))):
                c_off.append(o + j * frame_size)
                c_len.append(min(frame_size, n - j * frame_size))
            first.append(len(c_off))
            blocks.append(sum(-(-k // bs) for k in c_len[first[-2]:]))
        caps = [lz4f.compressFrameBound(n, prefs) for n in c_len]
        t = lambda v: torch.tensor(v, dtype=torch.int64, device=device)    # noqa: E731
        d_frames = torch.empty(max(1, sum(caps)), dtype=torch.uint8, device=device)
        f_off, f_len = t(_offsets(caps)), torch.zeros(len(caps), dtype=torch.int64, device=device)
        fd = lz4f.stageFileDicts(dicts, dict_index, device)
        if fd is not None:
            c_idx = None
            if fd.idx is not None:
                per_file = fd.idx.cpu().tolist()
                c_idx = torch.tensor([per_file[s] for s in range(nbuf) for _ in range(first[s + 1] - first[s])],
                                     dtype=torch.int32, device=device)
            # (the _ex call: at the fast level it is compressFrameUsingDictBatch)
            lz4f.compressFrameUsingDictBatchEx(
                d_src, t(c_off), t(c_len), d_frames, f_off, t(caps), f_len, fd.d_dict, fd.dict_off, fd.dict_len, c_idx, prefs,
                batch_flags, max_blocks=sum(blocks), max_src_len=max(c_len),
                max_dict_len=min(65536, int(fd.dict_len.max().item()) if fd.dict_len.numel() else 0))
        else:
            lz4f.compressFrameBatch(d_src, t(c_off), t(c_len), d_frames, f_off, t(caps), f_len, prefs, batch_flags,
                                    max_blocks=sum(blocks))
        room = [sum(caps[first[s]:first[s + 1]]) +
                (lz4f.seekTableBound(first[s + 1] - first[s], blocks[s]) if seek_table else 0) for s in range(nbuf)]
        slots = [(c + 15) & ~15 for c in room]
        file_off, file_cap = t(_offsets(slots)), t(room)
        d_files = torch.zeros(max(1, sum(slots)), dtype=torch.uint8, device=device)
        joined = torch.zeros(nbuf, dtype=torch.int64, device=device)
        lz4f.concatBatch(d_frames, f_off, f_len, t(first), d_files, file_off, file_cap, joined)
        if not seek_table:
            return _unstage(d_files, _offsets(slots), joined)
        ix = lz4f.indexSplit(lz4f.splitStaged(d_files, file_off, torch.clamp(joined, min=0), legacy=True), fd)
        result = lz4f._appendTables(ix, d_files, file_off, file_cap)
        return _unstage(d_files, _offsets(slots), torch.where(joined < 0, joined, result))

    # legacy frames: what `lz4 -l` writes (include/zlz4_amd.h)
    LegacyPrefs = LegacyPrefs
    LEGACY_MAGICNUMBER = 0x184C2102
    LEGACY_BLOCK_SIZE = 8 << 20
    LEGACY_BLOCK_BOUND = 8421520

    @staticmethod
    def _legacy_block_size(prefs):
        return (prefs.block_size if prefs is not None else 0) or lz4f.LEGACY_BLOCK_SIZE

    @staticmethod
    def legacyCompressFrameBound(src_size, prefs=None):
        return lib().zlz4f_legacy_compress_frame_bound(src_size, C.byref(prefs) if prefs is not None else None)

    @staticmethod
    def compressLegacyFrameBatchWorkspace(nframes, max_blocks, prefs=None):
        return lib().zlz4f_batch_compress_legacy_frame_workspace(nframes, max_blocks,
                                                                 C.byref(prefs) if prefs is not None else None)

    @staticmethod
    def legacyFrameDecompressedSizeBatchWorkspace(nframes, max_blocks):
        return lib().zlz4f_batch_legacy_frame_decompressed_size_workspace(nframes, max_blocks)

    @staticmethod
    def decompressLegacyFrameBatchWorkspace(nframes, max_blocks):
        return lib().zlz4f_batch_decompress_legacy_frame_workspace(nframes, max_blocks)

    @staticmethod
    def compressLegacyFrameBatch(d_src, src_off, src_len, d_dst, dst_off, dst_cap, result, prefs=None, max_blocks=None,
                                 workspace=None):
        """zlz4f_batch_compress_legacy_frame on torch CUDA tensors (layout as compressFrameBatch).  max_blocks defaults to
        the block count of the lengths (read back once), workspace to a fresh buffer of the size the library asks for."""
        import torch
        pp = C.byref(prefs) if prefs is not None else None
        if max_blocks is None:
            bs = lz4f._legacy_block_size(prefs)
            max_blocks = int(((src_len.cpu() + bs - 1) // bs).sum()) if src_len.numel() else 0
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_compress_legacy_frame_workspace(src_len.numel(), max_blocks, pp)),
                                    dtype=torch.uint8, device=d_src.device)
        _check(lib().zlz4f_batch_compress_legacy_frame(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(d_dst),
                                                       _ptr(dst_off), _ptr(dst_cap), _ptr(result), src_len.numel(),
                                                       max_blocks, pp, _ptr(workspace), workspace.numel()))

    @staticmethod
    def legacyFrameCountBatch(d_src, src_off, src_len, nblocks, consumed, totals):
        """zlz4f_batch_legacy_frame_count: nblocks / consumed int64 [nframes] (consumed may be None), totals int64 [1] = the
        blocks of all frames."""
        _check(lib().zlz4f_batch_legacy_frame_count(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), src_len.numel(),
                                                    _ptr(nblocks), _ptr(consumed), _ptr(totals)))

    @staticmethod
    def legacyFrameDecompressedSizeBatch(d_src, src_off, src_len, size, consumed, max_blocks, workspace=None):
        """zlz4f_batch_legacy_frame_decompressed_size: size int64 [nframes] = decoded size or the frame's error code;
        max_blocks = totals[0] of legacyFrameCountBatch."""
        import torch
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_legacy_frame_decompressed_size_workspace(src_len.numel(),
                                                                                                       max_blocks)),
                                    dtype=torch.uint8, device=d_src.device)
        _check(lib().zlz4f_batch_legacy_frame_decompressed_size(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len),
                                                                _ptr(size), _ptr(consumed), src_len.numel(), max_blocks,
                                                                _ptr(workspace), workspace.numel()))

    @staticmethod
    def decompressLegacyFrameBatch(d_src, src_off, src_len, d_dst, dst_off, dst_cap, result, consumed, max_blocks,
                                   workspace=None):
        """zlz4f_batch_decompress_legacy_frame (layout as decompressFrameBatch, consumed int64 [nframes] or None)."""
        import torch
        if workspace is None:
            workspace = torch.empty(max(16, lib().zlz4f_batch_decompress_legacy_frame_workspace(src_len.numel(), max_blocks)),
                                    dtype=torch.uint8, device=d_src.device)
        _check(lib().zlz4f_batch_decompress_legacy_frame(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(d_dst),
                                                         _ptr(dst_off), _ptr(dst_cap), _ptr(result), _ptr(consumed),
                                                         src_len.numel(), max_blocks, _ptr(workspace), workspace.numel()))

    @staticmethod
    def compressLegacyFrames(items, prefs=None, device="cuda"):
        """Every byte string of `items` as its own legacy frame, in one batch call -> list of frames (bytes) or error
        codes."""
        import torch
        if not len(items):
            return []
        caps = [lz4f.legacyCompressFrameBound(len(b), prefs) for b in items]
        d_src, src_off, src_len = _stage(items, device)
        dst_off = torch.tensor(_offsets(caps), dtype=torch.int64, device=device)
        d_dst = torch.empty(max(1, sum(caps)), dtype=torch.uint8, device=device)
        result = torch.empty(len(items), dtype=torch.int64, device=device)
        lz4f.compressLegacyFrameBatch(d_src, src_off, src_len, d_dst, dst_off,
                                      torch.tensor(caps, dtype=torch.int64, device=device), result, prefs)
        return _unstage(d_dst, _offsets(caps), result)

    @staticmethod
    def decompressLegacyFrames(frames, device="cuda"):
        """Every legacy frame of `frames` decoded in one batch -> list of (content or error code, consumed): count, one
        read-back of the block total, size query, zlz4_batch_plan_outputs, one read-back of the arena size, decode.
        frames[f][consumed:] is where the next member of a concatenated file starts."""
        import torch
        n = len(frames)
        if n == 0:
            return []
        d_src, src_off, src_len = _stage(frames, device)

        def i64(k):
            return torch.empty(k, dtype=torch.int64, device=device)

        nblocks, consumed, totals, size, dst_off, result = i64(n), i64(n), i64(1), i64(n), i64(n), i64(n)
        lz4f.legacyFrameCountBatch(d_src, src_off, src_len, nblocks, consumed, totals)
        max_blocks = int(totals.item())
        lz4f.legacyFrameDecompressedSizeBatch(d_src, src_off, src_len, size, None, max_blocks)
        cap32 = torch.empty(n, dtype=torch.int32, device=device)      # (a frame may hold more than 4 GiB: not used)
        batch_plan_outputs(size, dst_off, cap32, totals)
        dst_cap = size.clamp(min=0)
        d_dst = torch.empty(max(1, int(totals.item())), dtype=torch.uint8, device=device)
        lz4f.decompressLegacyFrameBatch(d_src, src_off, src_len, d_dst, dst_off, dst_cap, result, None, max_blocks)
        sizes = size.cpu().tolist()
        out = _unstage(d_dst, dst_off.cpu().tolist(), result)
        # (a frame the query failed got no room: the query's code stands)
        return [(o if s >= 0 else s, c) for o, s, c in zip(out, sizes, consumed.cpu().tolist())]

    @staticmethod
    def compressLegacyFrame(src, prefs=None, dst_cap=None):
        """zlz4f_compress_legacy_frame: one frame in host memory; dst_cap defaults to the bound."""
        cap = lz4f.legacyCompressFrameBound(len(src), prefs) if dst_cap is None else dst_cap
        return _run(lib().zlz4f_compress_legacy_frame, src, cap, C.byref(prefs) if prefs is not None else None)

    @staticmethod
    def legacyFrameDecompressedSize(src):
        """zlz4f_legacy_frame_decompressed_size -> (decoded size, consumed); errors raise Lz4Error."""
        s, n = _in(src)
        consumed = C.c_size_t(0)
        r = _check(lib().zlz4f_legacy_frame_decompressed_size(C.addressof(s), n, C.byref(consumed)))
        return r, consumed.value

    @staticmethod
    def decompressLegacyFrame(src, dst_cap=None):
        """zlz4f_decompress_legacy_frame -> (content, consumed).  dst_cap None: the size is queried first."""
        cap = lz4f.legacyFrameDecompressedSize(src)[0] if dst_cap is None else dst_cap
        consumed = C.c_size_t(0)
        return _run(lib().zlz4f_decompress_legacy_frame, src, cap, C.byref(consumed)), consumed.value


def _offsets(lens):
    out, pos = [], 0
    for n in lens:
        out.append(pos)
        pos += n
    return out


def _stage(items, device):
    """Byte strings back to back in one device tensor -> (tensor, int64 offsets, int64 lengths)."""
    import numpy as np
    import torch
    lens = [len(b) for b in items]
    buf = np.frombuffer(b"".join(bytes(b) for b in items) or b"\0", dtype=np.uint8)
    return (torch.from_numpy(buf.copy()).to(device), torch.tensor(_offsets(lens), dtype=torch.int64, device=device),
            torch.tensor(lens, dtype=torch.int64, device=device))


def _unstage(d_dst, offs, result):
    res = result.cpu().tolist()                       # (synchronises the stream)
    host = d_dst.cpu().numpy().tobytes()
    return [host[o:o + r] if r >= 0 else r for o, r in zip(offs, res)]


def _chain_blocks(f):
    """Upper bound of the blocks the device walk of frame `f` finds (src/lz4f.zig:563-600): every block header before the
    end mark or the end of the bytes, under the header size the FLG byte gives."""
    if len(f) < 7 or int.from_bytes(f[:4], "little") != lz4f.MAGICNUMBER:
        return 0
    flg = f[4]
    pos = 7 + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0)
    extra = 4 if flg & 0x10 else 0
    n = 0
    while pos + 4 <= len(f):
        h = int.from_bytes(f[pos:pos + 4], "little")
        if h == 0:
            break
        n += 1
        pos += 4 + (h & 0x7FFFFFFF) + extra
    return n


# ----------------------------------------------------------------------------- batch (device pointers)
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def batch_compress_fast(d_in, in_off, in_len, d_out, out_off, out_cap, result, max_in_len, acceleration=1):
    """zlz4_batch_compress_fast on torch CUDA tensors (uint8 / int64 offsets / int32 lengths / int64 result)."""
    _check(lib().zlz4_batch_compress_fast(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                          _ptr(out_off), _ptr(out_cap), _ptr(result), in_len.numel(),
                                          max_in_len, acceleration))


def batch_decompress_safe(d_in, in_off, in_len, d_out, out_off, out_cap, result):
    _check(lib().zlz4_batch_decompress_safe(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                            _ptr(out_off), _ptr(out_cap), _ptr(result), in_len.numel()))


def batch_decompress_safe_using_dict(d_in, in_off, in_len, d_out, out_off, out_cap, d_dict, dict_off, dict_len, result):
    """zlz4_batch_decompress_safe_using_dict: as batch_decompress_safe, block i with the dictionary
    d_dict[dict_off[i] .. + dict_len[i]) (int64 offsets / int32 lengths; a shared dictionary = equal offsets)."""
    _check(lib().zlz4_batch_decompress_safe_using_dict(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                                       _ptr(out_off), _ptr(out_cap), _ptr(d_dict), _ptr(dict_off),
                                                       _ptr(dict_len), _ptr(result), in_len.numel()))


def batch_decompressed_size(d_in, in_off, in_len, size, dict_len=None):
    """zlz4_batch_decompressed_size: size[i] (int64) = what batch_decompress_safe returns for block i into 0xFFFFFFFF
    bytes, or batch_decompress_safe_using_dict with a dictionary of dict_len[i] bytes (int32; None = no dictionary)."""
    _check(lib().zlz4_batch_decompressed_size(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(dict_len),
                                              _ptr(size), in_len.numel()))


def batch_plan_outputs(size, out_off, out_cap, total, align=0):
    """zlz4_batch_plan_outputs: packed slots from sizes (int64): out_off[i] (int64) = exclusive scan of max(size, 0)
    rounded up to `align`, out_cap[i] (int32) = size or 0 for a failed block, total[0] (int64) = bytes of all slots."""
    _check(lib().zlz4_batch_plan_outputs(_stream(), _ptr(size), size.numel(), align, _ptr(out_off), _ptr(out_cap),
                                         _ptr(total)))


def decompressBlocks(blocks, dicts=None, device="cuda"):
    """Every compressed block of `blocks` decoded without knowing its size: size query, output plan, one read-back of the
    total, allocation, decode.  dicts[i] (bytes or None) is block i's dictionary.  -> list of contents (bytes) or error
    codes."""
    import torch
    n = len(blocks)
    if n == 0:
        return []
    d_src, src_off, src_len = _stage(blocks, device)
    in_len = src_len.to(torch.int32)
    size = torch.empty(n, dtype=torch.int64, device=device)
    out_off = torch.empty(n, dtype=torch.int64, device=device)
    out_cap = torch.empty(n, dtype=torch.int32, device=device)
    total = torch.empty(1, dtype=torch.int64, device=device)
    result = torch.empty(n, dtype=torch.int64, device=device)
    if dicts is None:
        batch_decompressed_size(d_src, src_off, in_len, size)
    else:
        dbytes = [bytes(d) if d is not None else b"" for d in dicts]
        d_dict, dict_off, dl = _stage(dbytes, device)
        dict_len = dl.to(torch.int32)
        batch_decompressed_size(d_src, src_off, in_len, size, dict_len)
    batch_plan_outputs(size, out_off, out_cap, total)
    d_dst = torch.empty(max(1, int(total.item())), dtype=torch.uint8, device=device)
    if dicts is None:
        batch_decompress_safe(d_src, src_off, in_len, d_dst, out_off, out_cap, result)
    else:
        batch_decompress_safe_using_dict(d_src, src_off, in_len, d_dst, out_off, out_cap, d_dict, dict_off, dict_len, result)
    sizes = size.cpu().tolist()
    out = _unstage(d_dst, out_off.cpu().tolist(), result)
    return [o if s >= 0 else s for o, s in zip(out, sizes)]      # (a failed block has capacity 0: the query's code stands)


def batch_decompress_safe_prefix(d_in, in_off, in_len, d_out, out_off, out_cap, result):
    """zlz4_batch_decompress_safe_prefix: the tensors of batch_decompress_safe; out_cap[i] is the number of bytes wanted of
    block i and the size of its slot, result[i] = min(decoded size, out_cap[i]) or CorruptedData."""
    _check(lib().zlz4_batch_decompress_safe_prefix(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                                   _ptr(out_off), _ptr(out_cap), _ptr(result), in_len.numel()))


def batch_decompress_safe_prefix_using_dict(d_in, in_off, in_len, d_out, out_off, out_cap, d_dict, dict_off, dict_len,
                                            result):
    """zlz4_batch_decompress_safe_prefix_using_dict: the tensors of batch_decompress_safe_using_dict, out_cap as in
    batch_decompress_safe_prefix."""
    _check(lib().zlz4_batch_decompress_safe_prefix_using_dict(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len),
                                                              _ptr(d_out), _ptr(out_off), _ptr(out_cap), _ptr(d_dict),
                                                              _ptr(dict_off), _ptr(dict_len), _ptr(result),
                                                              in_len.numel()))


def batch_decompress_frame_prefix(d_src, src_off, src_len, d_dst, dst_off, dst_cap, result, d_dict=None, dict_off=None,
                                  dict_len=None, dict_idx=None):
    """zlz4f_batch_decompress_frame_prefix (dict_len None) / _using_dict on torch CUDA tensors: the layout of
    lz4f.decompressFrameBatch (int64 offsets, lengths and capacities) without max_blocks and workspace; dst_cap[f] is the
    number of bytes wanted of frame f and the size of its slot, result[f] = min(content size, dst_cap[f]) or the frame's
    error code.  Dictionaries as in lz4f.decompressFrameUsingDictBatch.  One launch on the current stream."""
    if dict_len is None:
        _check(lib().zlz4f_batch_decompress_frame_prefix(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(d_dst),
                                                         _ptr(dst_off), _ptr(dst_cap), _ptr(result), src_len.numel()))
    else:
        _check(lib().zlz4f_batch_decompress_frame_prefix_using_dict(
            _stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), _ptr(d_dst), _ptr(dst_off), _ptr(dst_cap), _ptr(result),
            src_len.numel(), _ptr(d_dict), _ptr(dict_off), _ptr(dict_len), dict_len.numel(), _ptr(dict_idx)))


def decompressBlockPrefixes(blocks, n, dicts=None, device="cuda"):
    """The first n bytes of every compressed block of `blocks` (n: one int for all, or one per block), staged like
    decompressBlocks but without a size query: block i's slot is n[i] bytes.  dicts[i] (bytes or None) is block i's
    dictionary.  -> list of prefixes (bytes; a block that decodes to fewer bytes gives all of them) or error codes."""
    import torch
    nb = len(blocks)
    if nb == 0:
        return []
    want = [int(n)] * nb if isinstance(n, int) else [int(x) for x in n]
    if len(want) != nb or any(w < 0 or w > 0xFFFFFFFF for w in want):
        raise ValueError("n: one length per block, each in [0, 0xFFFFFFFF]")
    d_src, src_off, src_len = _stage(blocks, device)
    in_len = src_len.to(torch.int32)
    offs = _offsets(want)
    out_off = torch.tensor(offs, dtype=torch.int64, device=device)
    # (int32 tensors carry the u32 capacities bit for bit)
    out_cap = torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in want], dtype=torch.int32, device=device)
    d_dst = torch.empty(max(1, sum(want)), dtype=torch.uint8, device=device)
    result = torch.empty(nb, dtype=torch.int64, device=device)
    if dicts is None:
        batch_decompress_safe_prefix(d_src, src_off, in_len, d_dst, out_off, out_cap, result)
    else:
        dbytes = [bytes(d) if d is not None else b"" for d in dicts]
        d_dict, dict_off, dl = _stage(dbytes, device)
        batch_decompress_safe_prefix_using_dict(d_src, src_off, in_len, d_dst, out_off, out_cap, d_dict, dict_off,
                                                dl.to(torch.int32), result)
    return _unstage(d_dst, offs, result)


def batch_load_dict(d_dict, dict_off, dict_len, tables, result):
    """zlz4_batch_load_dict: table i (tables.view(-1, 4096)[i], int32/uint32) = Stream.loadDict of dictionary
    d_dict[dict_off[i] .. + dict_len[i]); result[i] (int64) = dictSize."""
    _check(lib().zlz4_batch_load_dict(_stream(), _ptr(d_dict), _ptr(dict_off), _ptr(dict_len), _ptr(tables), _ptr(result),
                                      dict_len.numel()))


def batch_compress_fast_continue(d_in, in_off, in_len, d_out, out_off, out_cap, table_in, table_idx, table_out, result,
                                 max_in_len, acceleration=1):
    """zlz4_batch_compress_fast_continue: as batch_compress_fast, block i starting from table table_idx[i] of table_in
    (table_idx None = table i); its final table goes to table i of table_out (None = not written; table_out may be
    table_in itself when table_idx is None)."""
    _check(lib().zlz4_batch_compress_fast_continue(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                                   _ptr(out_off), _ptr(out_cap), _ptr(table_in), _ptr(table_idx),
                                                   _ptr(table_out), _ptr(result), in_len.numel(), max_in_len,
                                                   acceleration))


def batch_compress_fast_using_dict(d_in, in_off, in_len, d_out, out_off, out_cap, d_dict, dict_off, dict_len, table,
                                   table_idx, result, max_in_len, max_dict_len, acceleration=1):
    """zlz4_batch_compress_fast_using_dict: as batch_compress_fast, block i against the dictionary
    d_dict[dict_off[i] .. + dict_len[i]) (int64 offsets / int32 lengths) from table table_idx[i] of `table` (int32;
    table_idx None = table i), the tables being batch_load_dict's of the dictionaries."""
    _check(lib().zlz4_batch_compress_fast_using_dict(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                                     _ptr(out_off), _ptr(out_cap), _ptr(d_dict), _ptr(dict_off),
                                                     _ptr(dict_len), _ptr(table), _ptr(table_idx), _ptr(result),
                                                     in_len.numel(), max_in_len, max_dict_len, acceleration))


def compressBlocksUsingDict(blocks, dicts, dict_index=None, acceleration=1, device="cuda"):
    """Every byte string of `blocks` compressed against its dictionary in one batch: block i uses
    dicts[dict_index[i]] (dict_index None: dicts[i]; a shared dictionary is dicts = [d], dict_index = [0] * n).  Packs
    the data, loads one table per dictionary (batch_load_dict), compresses into compressBound slots and reads the
    streams back once.  -> list of streams (bytes) or error codes; decompressBlocks(streams, per-block dicts) gives
    the blocks back."""
    import numpy as np
    import torch
    n = len(blocks)
    if n == 0:
        return []
    idx = list(range(n)) if dict_index is None else [int(k) for k in dict_index]
    dbytes = [bytes(d) if d is not None else b"" for d in dicts]
    d_src, src_off, src_len = _stage(blocks, device)
    d_dict, dict_off, dict_len = _stage(dbytes, device)
    nd = len(dbytes)
    tables = torch.empty(max(1, nd) * STREAM_TABLE_ENTRIES, dtype=torch.int32, device=device)
    lres = torch.empty(max(1, nd), dtype=torch.int64, device=device)
    batch_load_dict(d_dict, dict_off, dict_len.to(torch.int32), tables, lres[:nd])
    t_idx = torch.tensor(idx, dtype=torch.int32, device=device)
    sel = t_idx.to(torch.int64)
    caps = [compressBound(len(b)) for b in blocks]
    dst_off = torch.tensor(_offsets(caps), dtype=torch.int64, device=device)
    d_dst = torch.empty(max(1, sum(caps)), dtype=torch.uint8, device=device)
    result = torch.empty(n, dtype=torch.int64, device=device)
    out_cap = torch.from_numpy(np.asarray(caps, dtype=np.uint32).view(np.int32)).to(device)
    max_in = max(len(b) for b in blocks)
    max_dict = min(65536, max((len(dbytes[k]) for k in idx), default=0))
    batch_compress_fast_using_dict(d_src, src_off, src_len.to(torch.int32), d_dst, dst_off, out_cap, d_dict,
                                   dict_off[sel].contiguous(), dict_len[sel].to(torch.int32).contiguous(), tables, t_idx,
                                   result, max_in, max_dict, acceleration)
    return _unstage(d_dst, _offsets(caps), result)


def batch_compress_hc_workspace(nblocks, max_in_len):
    return lib().zlz4_batch_compress_hc_workspace(nblocks, max_in_len)


def batch_compress_hc(d_in, in_off, in_len, d_out, out_off, out_cap, result, max_in_len, level, workspace):
    _check(lib().zlz4_batch_compress_hc(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                        _ptr(out_off), _ptr(out_cap), _ptr(result), in_len.numel(), max_in_len,
                                        level, _ptr(workspace), workspace.numel()))


def batch_compress_hc_using_dict_workspace(nblocks, max_in_len, max_dict_len):
    return lib().zlz4_batch_compress_hc_using_dict_workspace(nblocks, max_in_len, max_dict_len)


def batch_compress_hc_using_dict(d_in, in_off, in_len, d_out, out_off, out_cap, d_dict, dict_off, dict_len, result,
                                 max_in_len, max_dict_len, level, workspace):
    """zlz4_batch_compress_hc_using_dict: as batch_compress_hc, block i against the dictionary
    d_dict[dict_off[i] .. + dict_len[i]) (int64 offsets / int32 lengths).  `workspace` is a uint8 tensor of at least
    batch_compress_hc_using_dict_workspace(nblocks, max_in_len, max_dict_len) bytes."""
    _check(lib().zlz4_batch_compress_hc_using_dict(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                                   _ptr(out_off), _ptr(out_cap), _ptr(d_dict), _ptr(dict_off),
                                                   _ptr(dict_len), _ptr(result), in_len.numel(), max_in_len, max_dict_len,
                                                   level, _ptr(workspace), workspace.numel()))


def compressBlocksHCUsingDict(blocks, dicts, dict_index=None, level=9, device="cuda"):
    """compressBlocksUsingDict at an HC level (3..9): block i against dicts[dict_index[i]] (dict_index None: dicts[i]).
    -> list of streams (bytes) or error codes; decompressBlocks(streams, per-block dicts) gives the blocks back."""
    import numpy as np
    import torch
    n = len(blocks)
    if n == 0:
        return []
    idx = list(range(n)) if dict_index is None else [int(k) for k in dict_index]
    dbytes = [bytes(d) if d is not None else b"" for d in dicts]
    d_src, src_off, src_len = _stage(blocks, device)
    d_dict, dict_off, dict_len = _stage(dbytes, device)
    sel = torch.tensor(idx, dtype=torch.int64, device=device)
    caps = [compressBound(len(b)) for b in blocks]
    dst_off = torch.tensor(_offsets(caps), dtype=torch.int64, device=device)
    d_dst = torch.empty(max(1, sum(caps)), dtype=torch.uint8, device=device)
    result = torch.empty(n, dtype=torch.int64, device=device)
    out_cap = torch.from_numpy(np.asarray(caps, dtype=np.uint32).view(np.int32)).to(device)
    max_in = max(len(b) for b in blocks)
    max_dict = min(65536, max((len(dbytes[k]) for k in idx), default=0))
    ws = torch.empty(max(16, batch_compress_hc_using_dict_workspace(n, max_in, max_dict)), dtype=torch.uint8, device=device)
    batch_compress_hc_using_dict(d_src, src_off, src_len.to(torch.int32), d_dst, dst_off, out_cap, d_dict,
                                 dict_off[sel].contiguous(), dict_len[sel].to(torch.int32).contiguous(), result, max_in,
                                 max_dict, level, ws)
    return _unstage(d_dst, _offsets(caps), result)


def batch_train_dict_workspace(ngroups, total_sample_bytes, max_dict_cap, d=8, k=256, f=20):
    """zlz4_batch_train_dict_workspace: bytes of workspace for ngroups groups with total_sample_bytes of samples in all;
    0 for parameters the call refuses."""
    p = TrainParams(d, k, f, 0)
    return lib().zlz4_batch_train_dict_workspace(ngroups, total_sample_bytes, max_dict_cap, C.addressof(p))


def batch_train_dict(d_src, src_off, src_len, group_first, d_dict, dict_off, dict_cap, result, max_dict_cap, workspace,
                     d=8, k=256, f=20):
    """zlz4_batch_train_dict on torch CUDA tensors: sample i is d_src[src_off[i] .. + src_len[i]) (int64 offsets / int32
    lengths), group g is samples group_first[g] .. group_first[g + 1] - 1 (int32, result.numel() + 1 entries); its dictionary
    goes to d_dict[dict_off[g] .. + dict_cap[g]) (int64 / int32) and result[g] (int64) = its length or InvalidState.
    `workspace` is a uint8 tensor of at least batch_train_dict_workspace(...) bytes.  Asynchronous on the current stream."""
    p = TrainParams(d, k, f, 0)
    _check(lib().zlz4_batch_train_dict(_stream(), _ptr(d_src), _ptr(src_off), _ptr(src_len), src_len.numel(),
                                       _ptr(group_first), result.numel(), _ptr(d_dict), _ptr(dict_off), _ptr(dict_cap),
                                       _ptr(result), max_dict_cap, C.addressof(p), _ptr(workspace), workspace.numel()))


def trainDicts(groups, dict_size=65536, d=8, k=256, f=20, device="cuda"):
    """One dictionary per group of samples in one batch: groups[g] is a list of byte strings, dict_size one capacity for
    all or one per group.  Packs the samples, trains every group in the same launches (batch_train_dict) and reads the
    dictionaries back once.  -> list of dictionaries (bytes) or error codes, ready for compressBlocksUsingDict,
    compressBlocksHCUsingDict, lz4f.compressFramesUsingDict and lz4f.compressFiles(..., dicts=)."""
    import torch
    ng = len(groups)
    if ng == 0:
        return []
    caps = [int(dict_size)] * ng if isinstance(dict_size, int) else [int(c) for c in dict_size]
    if len(caps) != ng or any(c < 0 or c > 0xFFFFFFFF for c in caps):
        raise ValueError("dict_size: one capacity, or one per group, each in [0, 0xFFFFFFFF]")
    samples = [bytes(s) for grp in groups for s in grp]
    first = _offsets([len(grp) for grp in groups]) + [len(samples)]
    d_src, src_off, src_len = _stage(samples, device)
    slots = [min(c, 65536) for c in caps]             # (a capacity above 65536 is refused: its slot is never written)
    offs = _offsets(slots)
    d_dict = torch.empty(max(1, sum(slots)), dtype=torch.uint8, device=device)
    dict_off = torch.tensor(offs, dtype=torch.int64, device=device)
    dict_cap = torch.tensor([c - (1 << 32) if c >= (1 << 31) else c for c in caps], dtype=torch.int32, device=device)
    group_first = torch.tensor(first, dtype=torch.int32, device=device)
    result = torch.empty(ng, dtype=torch.int64, device=device)
    max_cap = max(slots)
    ws_bytes = batch_train_dict_workspace(ng, sum(len(s) for s in samples), max_cap, d, k, f)
    if ws_bytes == 0:
        raise Lz4Error(-5, error_name(-5))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    batch_train_dict(d_src, src_off, src_len.to(torch.int32), group_first, d_dict, dict_off, dict_cap, result, max_cap, ws,
                     d, k, f)
    return _unstage(d_dict, offs, result)


def batch_compress_dest_size_workspace(nblocks, max_in_len):
    return lib().zlz4_batch_compress_dest_size_workspace(nblocks, max_in_len)


def batch_compress_dest_size(d_in, in_off, in_len, d_out, out_off, out_cap, result, consumed, max_in_len, workspace):
    """zlz4_batch_compress_dest_size: lz4.compressDestSize per block (in_len[i] = bytes available, out_cap[i] = dst.len);
    result[i] (int64) = compressed size or error code, consumed[i] (int32) = source bytes consumed.  `workspace` is a
    uint8 tensor of at least batch_compress_dest_size_workspace(nblocks, max_in_len) bytes."""
    _check(lib().zlz4_batch_compress_dest_size(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                               _ptr(out_off), _ptr(out_cap), _ptr(result), _ptr(consumed),
                                               in_len.numel(), max_in_len, _ptr(workspace),
                                               workspace.numel() if workspace is not None else 0))


def compressDestSizeBatch(items, caps, device="cuda"):
    """lz4.compressDestSize of every byte string of `items` into a destination of caps[i] bytes, in one batch call
    -> list of (compressed bytes, consumed source bytes); a block that fails gives (error code, 0)."""
    import numpy as np
    import torch
    caps = list(caps)
    n = len(items)
    if n == 0:
        return []
    d_src, src_off, src_len = _stage(items, device)
    max_in = max(len(b) for b in items)
    dst_off = torch.tensor(_offsets(caps), dtype=torch.int64, device=device)
    d_dst = torch.empty(max(1, sum(caps)), dtype=torch.uint8, device=device)
    result = torch.empty(n, dtype=torch.int64, device=device)
    consumed = torch.empty(n, dtype=torch.int32, device=device)
    ws = torch.empty(max(1, batch_compress_dest_size_workspace(n, max_in)), dtype=torch.uint8, device=device)
    out_cap = torch.from_numpy(np.asarray(caps, dtype=np.uint32).view(np.int32)).to(device)
    batch_compress_dest_size(d_src, src_off, src_len.to(torch.int32), d_dst, dst_off, out_cap, result, consumed, max_in, ws)
    out = _unstage(d_dst, _offsets(caps), result)
    return [(o, c if isinstance(o, bytes) else 0) for o, c in zip(out, consumed.cpu().tolist())]


def batch_verify(d_in, in_off, in_len, d_comp, comp_off, comp_result, verify):
    """zlz4_batch_verify: decode every compressed block on the device and compare with its input; returns the number of
    blocks that do not round-trip (verify[i] = the compress result, or ZLZ4_ERR_VERIFY = -9)."""
    return _check(lib().zlz4_batch_verify(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_comp), _ptr(comp_off),
                                          _ptr(comp_result), _ptr(verify), in_len.numel()))


def batch_decompress_safe_continue_workspace(nblocks, nstreams):
    return lib().zlz4_batch_decompress_safe_continue_workspace(nblocks, nstreams)


def batch_decompress_safe_continue(d_in, in_off, in_len, d_out, out_off, out_cap, run_start, state, result, workspace):
    """zlz4_batch_decompress_safe_continue: stream s makes the calls [run_start[s], run_start[s + 1]) (int32, nstreams + 1
    entries) from state[s] (int64 tensor of shape (nstreams, 4): dict, dict_len, prefix, prefix_len as device addresses;
    updated in place); result[i] (int64) = what call i returns.  `workspace`: uint8 tensor of at least
    batch_decompress_safe_continue_workspace(nblocks, nstreams) bytes."""
    _check(lib().zlz4_batch_decompress_safe_continue(_stream(), _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                                     _ptr(out_off), _ptr(out_cap), _ptr(run_start), _ptr(state),
                                                     _ptr(result), in_len.numel(), run_start.numel() - 1,
                                                     _ptr(workspace), workspace.numel() if workspace is not None else 0))


def decompressStreams(runs, caps, dicts=None, device="cuda"):
    """Every run of `runs` (a list of lists of compressed blocks) decoded as one StreamDecode, in one batch call: call j
    of run s into its own slot of caps[s][j] bytes, the slots of a run back to back in call order.  dicts[s] (bytes or
    None) is set with setStreamDecode first.  -> (outputs, states): outputs[s][j] = bytes or an error code, states[s] =
    the final (dict, dict_len, prefix, prefix_len) with addresses made relative: prefix as ("slot", j) or 0, dict as
    ("dict", s) or 0."""
    import numpy as np
    import torch
    blocks = [b for r in runs for b in r]
    flat_caps = [int(c) for cs in caps for c in cs]
    n, ns = len(blocks), len(runs)
    d_src, src_off, src_len = _stage(blocks, device)
    offs = _offsets(flat_caps)
    d_dst = torch.empty(max(1, sum(flat_caps)), dtype=torch.uint8, device=device)
    dst_off = torch.tensor(offs, dtype=torch.int64, device=device)
    out_cap = torch.from_numpy(np.asarray(flat_caps, dtype=np.uint32).view(np.int32)).to(device)
    rs = [0]
    for r in runs:
        rs.append(rs[-1] + len(r))
    run_start = torch.tensor(rs, dtype=torch.int32, device=device)
    dicts = list(dicts) if dicts is not None else [None] * ns
    dbytes = [bytes(d) if d is not None else b"" for d in dicts]
    d_dict, dict_off, _ = _stage(dbytes, device)
    base = d_dict.data_ptr()
    doffs = dict_off.cpu().tolist()
    st = np.zeros((ns, 4), dtype=np.uint64)
    for s, d in enumerate(dicts):
        if d is not None:
            st[s, 0] = base + doffs[s]
            st[s, 1] = len(dbytes[s])
    state = torch.from_numpy(st.view(np.int64)).to(device)
    result = torch.empty(n, dtype=torch.int64, device=device)
    ws = torch.empty(max(16, batch_decompress_safe_continue_workspace(n, ns)), dtype=torch.uint8, device=device)
    batch_decompress_safe_continue(d_src, src_off, src_len.to(torch.int32), d_dst, dst_off, out_cap, run_start, state,
                                   result, ws)
    flat = _unstage(d_dst, offs, result)
    final = state.cpu().numpy().view(np.uint64)
    slot_of = {d_dst.data_ptr() + o: j for j, o in enumerate(offs)}
    outs, states = [], []
    for s in range(ns):
        outs.append(flat[rs[s]:rs[s + 1]])
        dct, dl, pre, pl = (int(x) for x in final[s])
        dct = ("dict", s) if dct and dct == int(st[s, 0]) else (0 if dct == 0 else dct)
        pre = ("slot", slot_of[pre] - rs[s]) if pre in slot_of else pre
        states.append((dct, dl, pre, pl))
    return outs, states
