"""Frame prefix decoding on the GPU (zlz4f_batch_decompress_frame_prefix(_using_dict), the two host calls,
lz4f.decompressFramePrefixes): results and bytes [0, result) against the model
tools/pyref/zig_lz4_frame_prefix.py over the corpus of tests/frameprefixgen.py -- every place a cut can fall, at every byte
of the small frames -- against results stated by hand for the defects, and the invariants against the full frame decoders
and the size queries.  Every slot is exactly n bytes between guard bands that must come back untouched, and the bytes of a
slot behind the result keep their fill (frameprefixgen.collect)."""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import frameprefixgen as g

pytestmark = pytest.mark.gpu
_RUNS = {}


def _family(zl, gpu, cases, key):
    """one batch over every cut of `cases`, run once per session and shared (the invariants read it again)"""
    if key not in _RUNS:
        its = g.items(cases)
        _RUNS[key] = (its, g.run_batch(zl, its, gpu))
    return _RUNS[key]


def _by_family(cases, fams):
    return [c for c in cases if c.family in fams]


@pytest.mark.parametrize("fams", [("literals",), ("disjoint", "stored", "cross", "empty"), ("far",), ("doubling",)])
def test_small_frames_every_cut(zl, gpu, fams):
    cases = _by_family(g.small_cases(), fams)
    assert cases
    its, got = _family(zl, gpu, cases, fams)
    assert len(its) >= sum(g.full(c.frame)[0] + 2 for c in cases)
    g.compare(its, got)
    for (name, f, n, d), (r, data) in zip(its, got):  # valid frames: min(S, n) and the first bytes of the content
        S, content = g.full(f)
        assert r == min(S, n) and data == content[:n], name


def test_small_frames_through_the_dictionary_call(zl, gpu):
    """the same frames through the _using_dict kernel with a dictionary of length 0"""
    its = g.items(_by_family(g.small_cases(), ("disjoint", "stored", "cross", "empty", "doubling")))
    g.compare(its, g.run_batch(zl, its, gpu, use_dict=True))


def test_dictionary_frames_every_cut(zl, gpu):
    cases = g.dict_cases()
    its, got = _family(zl, gpu, cases, "dict")
    g.compare(its, got)
    # what the corpus is there for: a cut inside and just behind the T part of a match, and every dictionary length class
    by = {c.name: c for c in cases}
    c = by["dict_linked2_match_crosses_T_end"]         # 30 literals, 5 bytes of T, then output[0:15]
    S, content = g.full(c.frame, c.dict)
    seen = {n: r for (name, f, n, d), (r, _) in zip(its, got) if f == c.frame and d == c.dict}
    assert [seen[n] for n in (31, 34, 35, 36, 50, S, S + 1)] == [31, 34, 35, 36, 50, S, S]
    for tag in ("linked", "indep"):
        res = {dn: [r for (name, f, n, d), (r, _) in zip(its, got) if name.startswith("dictlen_%s_%s@" % (tag, dn))]
               for dn in ("d0", "short", "exact", "d70000")}
        assert res["exact"] == res["d70000"] and res["exact"][:47] == list(range(47))
        # the match stands behind 30 literals: a dictionary that is too short is reported once n > 30
        assert res["d0"][:31] == list(range(31)) and set(res["d0"][31:]) == {g.FAILED}
        assert res["short"][:31] == list(range(31)) and set(res["short"][31:]) == {g.FAILED}


def test_long_frames_and_fixtures(zl, gpu):
    cases = g.long_cases() + g.fixture_cases()
    its, got = _family(zl, gpu, cases, "long")
    g.compare(its, got)
    inputs = g.fixture_inputs()                        # liblz4's frames: the first bytes of what liblz4 compressed
    seen = 0
    for (name, f, n, d), (r, data) in zip(its, got):
        if f in inputs:
            assert r == min(n, len(inputs[f])) and data == inputs[f][:n], name
            seen += 1
    assert seen >= 20
    # the history cap: the accepted offset decodes, the refused one is reported once it is reached and not before
    res = {name: r for (name, f, n, d), (r, _) in zip(its, got)}
    assert res["pos65530_off_accepted@65552"] == 65552 and res["pos65530_off_refused@65530"] == 65530
    assert res["pos65530_off_refused@65531"] == g.FAILED
    assert res["pos65236_T_first_byte@65438"] == 65438 and res["pos65236_in_front_of_T@65236"] == 65236
    assert res["pos65236_in_front_of_T@65237"] == g.FAILED and res["pos65236_cap_into_T@65647"] == 65645


def _prefs(P, **kw):
    p = P()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_frames_written_by_this_library(zl, gpu):
    data = [bytes(dg.text_bytes(150001, 3)), bytes(dg.text_bytes(70000, 4)), bytes(dg.text_bytes(999, 5)), b""]
    dct = bytes(dg.text_bytes(30000, 6))
    ns = [4097, 65537, 2000, 5]
    for kw, flags in ((dict(block_mode=1), 0), (dict(block_mode=0, block_checksum=1, content_checksum=1),
                                                zl.lz4f.BATCH_LINK_BLOCKS)):
        frames = zl.lz4f.compressFrames(data, _prefs(zl.Prefs, **kw), flags)
        assert all(isinstance(f, bytes) for f in frames)
        assert zl.lz4f.decompressFramePrefixes(frames, ns) == [b[:n] for b, n in zip(data, ns)]
        assert zl.lz4f.decompressFramePrefixes(frames, 150002) == data
    for mode in (0, 1):
        frames = zl.lz4f.compressFramesUsingDict(data, [dct], None, _prefs(zl.Prefs, block_mode=mode, dict_id=9))
        assert zl.lz4f.decompressFramePrefixes(frames, ns, dicts=[dct]) == [b[:n] for b, n in zip(data, ns)]
        assert zl.lz4f.decompressFramePrefixes(frames, 200000, dicts=[b"", dct], dict_index=[1, 1, 1, 1]) == data
        # without the dictionary the text frames fail once a match into it is reached; the header is still good
        got = zl.lz4f.decompressFramePrefixes(frames, [0, 0, 0, 0])
        assert got == [b"", b"", b"", b""]


def test_defects_on_both_sides_of_the_cut(zl, gpu):
    cases = [c for c, _ in g.defect_cases()]
    want = {c.frame: w for c, w in g.defect_cases()}
    its, got = _family(zl, gpu, cases, "defect")
    g.compare(its, got)
    for (name, f, n, d), (r, _) in zip(its, got):
        assert r == want[f](n), (name, r, want[f](n))
    # every header error, with n == 0 and n > 0, with and without dictionaries
    hits = [("%s@%d" % (name, n), f, n, None) for name, f, w in g.header_cases() for n in (0, 1, 300)]
    hw = [w for name, f, w in g.header_cases() for n in (0, 1, 300)]
    for use_dict in (False, True):
        got = g.run_batch(zl, hits, gpu, use_dict=use_dict)
        assert [r for r, _ in got] == hw


def test_invariants_full_decode_and_size_query(zl, gpu):
    """on the whole corpus: with R the full decoder's result into a capacity that is large enough, a prefix result is
    min(R, n) with the decode's first bytes where R >= 0, and n or R itself where the frame fails; where the size query
    gives S >= 0, min(S, n) for n <= S"""
    groups = [("small", g.small_cases()), ("dict", g.dict_cases()), ("long", g.long_cases() + g.fixture_cases()),
              ("defect", [c for c, _ in g.defect_cases()])]
    cases = [c for _, cs in groups for c in cs]
    cases += [g.Case("hdr_" + name, "header", f, None, [0, 7], False) for name, f, w in g.header_cases()]
    frames = [c.frame for c in cases]
    dicts, didx = [b""], []
    for c in cases:
        d = c.dict or b""
        if d not in dicts:
            dicts.append(d)
        didx.append(dicts.index(d))
    # (room to spare also for the frames that fail: no stored block of theirs is as long as 70000 bytes)
    caps = [g.full(c.frame, c.dict)[0] + 600 if g.full(c.frame, c.dict)[0] >= 0 else 70000 for c in cases]
    full = zl.lz4f.decompressFramesUsingDict(frames, dicts, didx, caps)
    plain = [k for k, c in enumerate(cases) if not c.dict]
    linked = zl.lz4f.decompressFrames([frames[k] for k in plain], [caps[k] for k in plain], flags=zl.lz4f.DECODE_LINKED)
    assert linked == [full[k] for k in plain]          # D == 0: the linked decode
    import torch
    d_src, src_off, src_len = zl._stage(frames, gpu)
    size = torch.empty(len(frames), dtype=torch.int64, device=gpu)
    dl = torch.tensor([len(d) for d in dicts], dtype=torch.int32, device=gpu)
    zl.lz4f.frameDecompressedSizeUsingDictBatch(d_src, src_off, src_len, size, dl,
                                                torch.tensor(didx, dtype=torch.int32, device=gpu),
                                                max_blocks=sum(zl._chain_blocks(f) for f in frames))
    sizes = size.cpu().tolist()
    R = {(c.frame, c.dict or b""): (full[k], sizes[k]) for k, c in enumerate(cases)}
    assert sum(1 for v in full if isinstance(v, bytes)) > 50 and sum(1 for v in full if not isinstance(v, bytes)) > 25
    keys = [("literals",), ("disjoint", "stored", "cross", "empty"), ("far",), ("doubling",)]
    runs = [_family(zl, gpu, _by_family(g.small_cases(), k), k) for k in keys]
    runs += [_family(zl, gpu, cs, key) for key, cs in groups[1:]]
    hdr = g.items(cases[-len(g.header_cases()):])
    runs.append((hdr, g.run_batch(zl, hdr, gpu)))
    checked = 0
    for its, got in runs:
        for (name, f, n, d), (r, data) in zip(its, got):
            whole, S = R[(f, d or b"")]
            if isinstance(whole, bytes):
                assert r == min(len(whole), n) and data == whole[:n], name
            else:
                assert r == n or r == whole, name
            if S >= 0 and n <= S:
                assert r == n, name
            checked += 1
    assert checked > 18000
    for c, _ in g.defect_cases():                      # a failing frame, with room to spare: R itself
        got = zl.lz4f.decompressFramePrefixes([c.frame], 100000)
        assert got == [R[(c.frame, b"")][0]], c.name


def _mixed(seed=25):
    rng = np.random.default_rng(seed)
    pool = g.items(g.small_cases()) + g.items(g.dict_cases()) + g.items(g.long_cases())
    its = [pool[i] for i in sorted(rng.choice(len(pool), size=260, replace=False))]
    its += g.items(g.fixture_cases())[::3]
    for c, _ in g.defect_cases():
        its += [g.items([c])[i] for i in (0, 70, 140, -2, -1)]
    its += [("%s@%d" % (name, n), f, n, None) for name, f, w in g.header_cases() for n in (0, 9)]
    order = rng.permutation(len(its))
    return [its[i] for i in order]


def test_mixed_batch_dictionary_index_and_refusals(zl, gpu):
    import torch
    its = _mixed()
    assert len(its) > 300 and len({it[2] for it in its}) > 150
    got = g.run_batch(zl, its, gpu)
    g.compare(its, got)
    # d_dict_idx[f] >= ndicts for single frames: InvalidState in front of every other status (a header error included),
    # nothing written, the other frames unaffected
    s = g.stage(its, gpu)
    nd = s["dict_len"].numel()
    idx = s["dict_idx"].cpu().numpy().copy()
    bad = list(range(3, len(its), 17))
    for k, i in enumerate(bad):
        idx[i] = nd + (k % 3) * 1000
    s["dict_idx"] = torch.from_numpy(idx).to(gpu)
    zl.batch_decompress_frame_prefix(s["d_src"], s["src_off"], s["src_len"], s["d_dst"], s["dst_off"], s["dst_cap"],
                                     s["result"], s["d_dict"], s["dict_off"], s["dict_len"], s["dict_idx"])
    again = g.collect(its, s)
    for i, (r, data) in enumerate(again):
        assert (r, data) == ((g.INVALID_STATE, b"") if i in bad else got[i]), its[i][0]
    # ndicts == 0 is the plain call: the frames without a dictionary, with and without an index array
    plain = [it for it in its if not it[3]]
    want = [w for it, w in zip(its, got) if not it[3]]
    L, p = zl.lib(), lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_idx in (False, True):
        s = g.stage(plain, gpu)
        a = [p(s[k]) for k in ("d_src", "src_off", "src_len", "d_dst", "dst_off", "dst_cap", "result")]
        assert L.zlz4f_batch_decompress_frame_prefix_using_dict(st, *a, len(plain), None, None, None, 0,
                                                                p(s["dict_idx"]) if with_idx else None) == 0
        assert g.collect(plain, s) == want
    # refusals: a null or misaligned array returns InvalidState and nothing runs; nframes == 0 returns 0
    few = plain[:4]
    s = g.stage(few, gpu)
    raw = torch.zeros(512, dtype=torch.uint8, device=gpu)
    odd = lambda k: C.c_void_p(raw.data_ptr() + k)    # (raw is 256-byte aligned: + 4 breaks 8, + 2 breaks 4)
    a = [p(s[k]) for k in ("d_src", "src_off", "src_len", "d_dst", "dst_off", "dst_cap", "result")]
    dd = [p(s["d_dict"]), p(s["dict_off"]), p(s["dict_len"])]
    n = len(few)
    for k in range(7):
        b = list(a); b[k] = None
        assert L.zlz4f_batch_decompress_frame_prefix(st, *b, n) == g.INVALID_STATE, k
        assert L.zlz4f_batch_decompress_frame_prefix_using_dict(st, *b, n, *dd, 1, None) == g.INVALID_STATE, k
    for k in (1, 2, 4, 5, 6):
        b = list(a); b[k] = odd(4)
        assert L.zlz4f_batch_decompress_frame_prefix(st, *b, n) == g.INVALID_STATE, k
        assert L.zlz4f_batch_decompress_frame_prefix_using_dict(st, *b, n, *dd, 1, None) == g.INVALID_STATE, k
    assert L.zlz4f_batch_decompress_frame_prefix_using_dict(st, *a, n, dd[0], None, dd[2], 1, None) == g.INVALID_STATE
    assert L.zlz4f_batch_decompress_frame_prefix_using_dict(st, *a, n, dd[0], dd[1], None, 1, None) == g.INVALID_STATE
    assert L.zlz4f_batch_decompress_frame_prefix_using_dict(st, *a, n, dd[0], odd(4), dd[2], 1, None) == g.INVALID_STATE
    assert L.zlz4f_batch_decompress_frame_prefix_using_dict(st, *a, n, dd[0], dd[1], odd(2), 1, None) == g.INVALID_STATE
    assert L.zlz4f_batch_decompress_frame_prefix_using_dict(st, *a, n, dd[0], dd[1], dd[2], 1, odd(2)) == g.INVALID_STATE
    assert L.zlz4f_batch_decompress_frame_prefix(st, *a, 0) == 0
    assert L.zlz4f_batch_decompress_frame_prefix_using_dict(st, *a, 0, *dd, 1, None) == 0
    torch.cuda.synchronize()
    assert (s["result"].cpu() == -999).all() and (s["d_dst"].cpu() == 0xA5).all()
    # d_dict may be null when every dictionary is empty
    zero = torch.zeros(1, dtype=torch.int32, device=gpu)
    assert L.zlz4f_batch_decompress_frame_prefix_using_dict(st, *a, n, None, dd[1], p(zero), 1, None) == 0
    assert g.collect(few, s) == want[:4]


def test_graph_capture(zl, gpu):
    import torch
    its = _mixed(seed=7)[:64]
    s = g.stage(its, gpu)

    def run():
        zl.batch_decompress_frame_prefix(s["d_src"], s["src_off"], s["src_len"], s["d_dst"], s["dst_off"], s["dst_cap"],
                                         s["result"], s["d_dict"], s["dict_off"], s["dict_len"], s["dict_idx"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    s["result"].fill_(-999)
    s["d_dst"].fill_(0xA5)
    graph.replay()
    g.compare(its, g.collect(its, s))


def test_host_calls(zl, gpu):
    by = {c.name: c for c in g.small_cases() + g.dict_cases() + g.long_cases()}
    for name in ("literals_indep_cks", "cross_block_overlap", "dict_linked2_match_crosses_T_end", "dictlen_linked_d70000",
                 "pos65236_cap_into_T", "empty_frame"):
        c = by[name]
        S = g.full(c.frame, c.dict)[0]
        for n in (0, 1, 37, S - 1, S, S + 1, S + 1000):
            if n < 0:
                continue
            wn, wd = g.expected(c.frame, n, c.dict)
            assert wn == min(S, n)
            assert zl.lz4f.decompressFramePrefix(c.frame, n, c.dict) == wd, (name, n)
            if not c.dict:
                assert zl.lz4f.decompressFramePrefix(c.frame, n) == wd, (name, n)
    # a defect before the cut raises, behind it does not; a header error raises also for n == 0
    bad = {c.name: c for c, _ in g.defect_cases()}
    c = bad["defect_bad_content_cks"]
    assert len(zl.lz4f.decompressFramePrefix(c.frame, 170)) == 170
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.decompressFramePrefix(c.frame, 171)
    assert e.value.code == g.CONTENT_CHECKSUM
    c = bad["defect_corrupt_block2"]
    assert len(zl.lz4f.decompressFramePrefix(c.frame, 138)) == 138
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.decompressFramePrefix(c.frame, 139)
    assert e.value.code == g.FAILED
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.decompressFramePrefix(g.header_cases()[2][1], 0)
    assert e.value.code == g.TYPE_UNKNOWN
    # dict == NULL with dict_len > 0
    buf = (C.c_uint8 * 16)()
    f = by["literals_indep_cks"].frame
    assert zl.lib().zlz4f_decompress_frame_prefix_using_dict(f, len(f), C.addressof(buf), 16, None, 5) == g.INVALID_STATE
