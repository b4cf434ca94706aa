"""What the batch frame calls refuse, and in which order, on a machine WITH a device (where the refusals behind "no device"
become reachable): null and misaligned arrays, a null, short or misaligned workspace, unknown flags and unserved levels.
Every entry point has its own set and order (they differ, and callers see it); a refused call answers before any launch, so
sentinel-filled results and destinations stay untouched.  The plain compress and decompress calls are also held to what they
do NOT check.  Nothing here is provoked: every case is refused on the host or is a valid call.  Run: pytest -m gpu."""
import ctypes as C
import os
import re

import pytest

pytestmark = pytest.mark.gpu

NF, MB, LEN, DICT = 2, 2, 100, 64             # 2 frames of 100 bytes, one 64 KiB block each; one dictionary of 64 bytes
FILL, UNSET = 0xA5, -999
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zlz4_amd.h")


def _codes():
    text = open(HEADER).read()
    return {n: int(re.search(r"#define\s+%s\s+\((-\d+)\)" % n, text).group(1))
            for n in ("ZLZ4_ERR_INVALID_STATE", "ZLZ4F_ERR_PARAMETER_INVALID", "ZLZ4_ERR_UNSUPPORTED")}


ERR = _codes()
STATE, PARAM, UNSUP = ERR["ZLZ4_ERR_INVALID_STATE"], ERR["ZLZ4F_ERR_PARAMETER_INVALID"], ERR["ZLZ4_ERR_UNSUPPORTED"]

FRAME_ARRAYS = ("src", "src_off", "src_len", "dst", "dst_off", "dst_cap", "result")
QUERY_ARRAYS = ("src", "src_off", "src_len", "result")
# entry point -> (its arrays, the dictionary arguments it takes, the level it is called at, does it take flags)
ENTRIES = {
    "zlz4f_batch_compress_frame": (FRAME_ARRAYS, (), 0, True),
    "zlz4f_batch_compress_frame_ex": (FRAME_ARRAYS, (), 0, True),
    "zlz4f_batch_compress_frame_using_dict": (FRAME_ARRAYS, ("dict", "dict_off", "dict_len"), 0, True),
    "zlz4f_batch_compress_frame_using_dict_ex": (FRAME_ARRAYS, ("dict", "dict_off", "dict_len"), 9, True),
    "zlz4f_batch_decompress_frame": (FRAME_ARRAYS, (), None, False),
    "zlz4f_batch_decompress_frame_ex": (FRAME_ARRAYS, (), None, True),
    "zlz4f_batch_decompress_frame_using_dict": (FRAME_ARRAYS, ("dict", "dict_off", "dict_len"), None, False),
    "zlz4f_batch_frame_decompressed_size": (QUERY_ARRAYS, (), None, False),
    "zlz4f_batch_frame_decompressed_size_ex": (QUERY_ARRAYS, (), None, True),
    "zlz4f_batch_frame_decompressed_size_using_dict": (QUERY_ARRAYS, ("dict_len",), None, False),
    "zlz4f_batch_frame_dict_id": (QUERY_ARRAYS, (), None, False),
}


class Env:
    def __init__(self, zl, gpu):
        import torch
        self.zl, self.L, self.torch = zl, zl.lib(), torch
        self.cap = zl.lz4f.compressFrameBound(LEN, None)
        t = self.t = dict(
            src=(torch.arange(256, device=gpu) % 7).to(torch.uint8),
            src_off=torch.tensor([0, 128, 0], dtype=torch.int64, device=gpu),      # (one entry more: room behind ptr + 4)
            src_len=torch.tensor([LEN, LEN, 0], dtype=torch.int64, device=gpu),
            dst=torch.full((NF * self.cap,), FILL, dtype=torch.uint8, device=gpu),
            dst_off=torch.tensor([0, self.cap, 0], dtype=torch.int64, device=gpu),
            dst_cap=torch.tensor([self.cap, self.cap, 0], dtype=torch.int64, device=gpu),
            result=torch.full((NF + 1,), UNSET, dtype=torch.int64, device=gpu),
            dict=(torch.arange(DICT, device=gpu) % 5).to(torch.uint8),
            dict_off=torch.tensor([0, 0], dtype=torch.int64, device=gpu),
            dict_len=torch.tensor([DICT, 0], dtype=torch.int32, device=gpu))
        self.ws = torch.empty(max(self.need(fn) for fn in ENTRIES) + 64, dtype=torch.uint8, device=gpu)
        assert self.ws.data_ptr() % 16 == 0 and all(v.data_ptr() % 8 == 0 for v in t.values())
        self.ptr = {k: v.data_ptr() for k, v in t.items()}

    def prefs(self, level, **kw):
        p = self.zl.Prefs()
        p.compression_level = level or 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def need(self, fn):
        L, p = self.L, C.byref(self.prefs(ENTRIES[fn][2]))
        if fn == "zlz4f_batch_frame_dict_id":
            return 0
        if fn.startswith("zlz4f_batch_compress_frame_using_dict"):
            return getattr(L, fn.replace("_using_dict", "_using_dict_workspace"))(NF, MB, p, 0, 1, LEN, DICT)
        if fn.startswith("zlz4f_batch_compress_frame"):
            return L.zlz4f_batch_compress_frame_workspace_ex(NF, MB, p, 0)
        if fn.endswith("_ex"):
            return getattr(L, fn[:-3] + "_workspace_ex")(NF, MB, 0)
        return getattr(L, fn + "_workspace")(NF, MB)

    def call(self, fn, nframes=NF, flags=0, prefs=None, ws="aligned", ws_bytes=None, **over):
        """The entry point with this test's arguments; `over` replaces pointers by name (None: null)."""
        arrays, dict_args, level, takes_flags = ENTRIES[fn]
        g = dict(self.ptr)
        g.update(over)
        wsp = {"aligned": self.ws.data_ptr(), None: None}.get(ws, ws)
        a = [self.zl._stream()] + [g[k] for k in arrays] + [nframes]
        if fn != "zlz4f_batch_frame_dict_id":
            a.append(MB)
            if level is not None:
                a.append(C.byref(prefs if prefs is not None else self.prefs(level)))
            if takes_flags:
                a.append(flags)
            if dict_args:
                a += [g[k] for k in dict_args] + [1, None]
            if fn.startswith("zlz4f_batch_compress_frame_using_dict"):
                a += [LEN, DICT]
            a += [wsp, self.need(fn) if ws_bytes is None else ws_bytes]
        return getattr(self.L, fn)(*a)

    def untouched(self):
        t = self.t
        return bool((t["result"] == UNSET).all()) and bool((t["dst"] == FILL).all())


@pytest.fixture(scope="module")
def env(zl, gpu):
    return Env(zl, gpu)


def _refused(env, fn, want, what, **kw):
    got = env.call(fn, **kw)
    assert got == want, "%s, %s: %d, not %d" % (fn, what, got, want)
    assert env.untouched(), "%s, %s: a refused call wrote its results or its destination" % (fn, what)


def _nulls_pass_with_no_frames(env, fn):
    """nframes == 0 answers 0 in front of every array and workspace refusal: nothing is looked at."""
    arrays, dict_args, _, _ = ENTRIES[fn]
    nulls = {k: None for k in arrays + dict_args}
    assert env.call(fn, nframes=0, ws=None, ws_bytes=0, **nulls) == 0, fn
    assert env.untouched(), fn


def _workspace_cases(env, fn, aligned16):
    _refused(env, fn, STATE, "null workspace", ws=None)
    _refused(env, fn, STATE, "workspace one byte short", ws_bytes=env.need(fn) - 1)
    if aligned16:
        _refused(env, fn, STATE, "workspace + 8", ws=env.ws.data_ptr() + 8)


def _array_cases(env, fn, names, dict_names=()):
    for k in names + dict_names:
        _refused(env, fn, STATE, "null " + k, **{k: None})
    for k in names + dict_names:
        if k not in ("src", "dst", "dict", "dict_len"):          # the 64-bit arrays: 4 off is misaligned
            _refused(env, fn, STATE, k + " + 4", **{k: env.ptr[k] + 4})


@pytest.mark.parametrize("fn", ["zlz4f_batch_compress_frame", "zlz4f_batch_compress_frame_ex"])
def test_compress_refusals(env, fn):
    """bfc_refusal -> (no device) -> nframes == 0 -> workspace null or short -> (_ex) workspace not 16-aligned; no array is
    checked."""
    ex = fn.endswith("_ex")
    _refused(env, fn, PARAM, "unassigned flag 2", flags=2)
    _refused(env, fn, PARAM, "unassigned flag 2 before anything else", flags=2, ws=None, nframes=0)
    _refused(env, fn, PARAM, "content size given twice", flags=1, prefs=env.prefs(0, content_size=5))
    _refused(env, fn, PARAM, "linked blocks, FLG says independent", flags=4, prefs=env.prefs(0, block_mode=1))
    _refused(env, fn, UNSUP, "linked blocks at level 12", flags=4, prefs=env.prefs(12))
    if not ex:
        _refused(env, fn, UNSUP, "linked blocks at level 9", flags=4, prefs=env.prefs(9))
    _nulls_pass_with_no_frames(env, fn)
    misaligned = {k: env.ptr[k] + 4 for k in ("src_off", "src_len", "dst_off", "dst_cap", "result")}
    assert env.call(fn, nframes=0, **misaligned) == 0 and env.untouched()
    _workspace_cases(env, fn, aligned16=ex)


def test_plain_compress_takes_a_workspace_that_is_8_aligned(env):
    """zlz4f_batch_compress_frame asks for no 16-alignment: the same call at workspace + 8 (with the 8 bytes to spare) is a
    valid call and gives the aligned call's frames."""
    fn, t = "zlz4f_batch_compress_frame", env.t
    out = []
    try:
        for ws in (env.ws.data_ptr(), env.ws.data_ptr() + 8):
            t["result"].fill_(UNSET)
            t["dst"].fill_(FILL)
            assert env.call(fn, ws=ws) == 0
            res = t["result"][:NF].cpu().tolist()
            assert all(0 < r <= env.cap for r in res), res
            out.append((res, t["dst"].cpu().numpy().tobytes()))
        assert out[0] == out[1]
    finally:
        t["result"].fill_(UNSET)
        t["dst"].fill_(FILL)


@pytest.mark.parametrize("fn", ["zlz4f_batch_compress_frame_using_dict", "zlz4f_batch_compress_frame_using_dict_ex"])
def test_dictionary_compress_refusals(env, fn):
    """bfcd_refusal -> (no device) -> nframes == 0 -> null or misaligned arrays, the dictionary's included -> workspace null,
    short or not 16-aligned."""
    ex = fn.endswith("_ex")
    _refused(env, fn, PARAM, "ZLZ4F_BATCH_LINK_BLOCKS (block_mode says it)", flags=4)
    _refused(env, fn, PARAM, "content size given twice", flags=1, prefs=env.prefs(ENTRIES[fn][2], content_size=5))
    _refused(env, fn, UNSUP, "level 12", prefs=env.prefs(12))
    if not ex:
        _refused(env, fn, UNSUP, "level 9", prefs=env.prefs(9))
    _refused(env, fn, UNSUP, "the level before the arrays", prefs=env.prefs(12), src=None, ws=None)
    _nulls_pass_with_no_frames(env, fn)
    _array_cases(env, fn, FRAME_ARRAYS, ("dict", "dict_off", "dict_len"))
    _workspace_cases(env, fn, aligned16=True)


@pytest.mark.parametrize("fn", ["zlz4f_batch_decompress_frame", "zlz4f_batch_decompress_frame_ex",
                                "zlz4f_batch_decompress_frame_using_dict"])
def test_decompress_refusals(env, fn):
    """unknown flag -> (no device) -> nframes == 0 -> workspace null or short -> (dictionary call only) arrays and
    16-alignment."""
    with_dict = fn.endswith("_using_dict")
    if ENTRIES[fn][3]:
        _refused(env, fn, PARAM, "unknown decode flag", flags=2)
        _refused(env, fn, PARAM, "unknown decode flag before anything else", flags=2, nframes=0, ws=None)
    _nulls_pass_with_no_frames(env, fn)
    _workspace_cases(env, fn, aligned16=with_dict)
    if with_dict:
        _array_cases(env, fn, FRAME_ARRAYS, ("dict_off", "dict_len"))
    else:
        misaligned = {k: env.ptr[k] + 4 for k in ("src_off", "src_len", "dst_off", "dst_cap", "result")}
        assert env.call(fn, nframes=0, **misaligned) == 0 and env.untouched()


@pytest.mark.parametrize("fn", ["zlz4f_batch_frame_decompressed_size", "zlz4f_batch_frame_decompressed_size_ex",
                                "zlz4f_batch_frame_decompressed_size_using_dict"])
def test_size_query_refusals(env, fn):
    """unknown flag -> nframes == 0 -> arrays, workspace null, misaligned or short -> (dictionary only) alignment -> no
    device last."""
    with_dict = fn.endswith("_using_dict")
    if ENTRIES[fn][3]:
        _refused(env, fn, PARAM, "unknown decode flag", flags=2)
        _refused(env, fn, PARAM, "unknown decode flag before anything else", flags=2, nframes=0, ws=None)
    _nulls_pass_with_no_frames(env, fn)
    for k in QUERY_ARRAYS:
        _refused(env, fn, STATE, "null " + k, **{k: None})
    _workspace_cases(env, fn, aligned16=True)
    if with_dict:
        _refused(env, fn, STATE, "null dict_len", dict_len=None)
        for k in ("src_off", "src_len", "result"):
            _refused(env, fn, STATE, k + " + 4", **{k: env.ptr[k] + 4})


def test_dict_id_refusals(env):
    """nframes == 0 -> arrays -> (no device)."""
    fn = "zlz4f_batch_frame_dict_id"
    _nulls_pass_with_no_frames(env, fn)
    _array_cases(env, fn, QUERY_ARRAYS)
