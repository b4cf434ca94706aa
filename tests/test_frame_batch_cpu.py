"""Batch frame calls (zlz4f_batch_compress_frame / zlz4f_batch_decompress_frame): the parts that need no GPU -- exported
symbols, workspace arithmetic, and the loud failure without a device."""

NEW = ("zlz4f_batch_compress_frame_workspace", "zlz4f_batch_compress_frame",
       "zlz4f_batch_decompress_frame_workspace", "zlz4f_batch_decompress_frame")


def _prefs(zl, **kw):
    p = zl.Prefs()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_batch_frame_symbols_exported(zl):
    L = zl.lib()
    for name in NEW:
        assert name in zl.SYMBOLS, name
        assert hasattr(L, name), "libzlz4_amd.so does not export %s" % name
    assert zl.lz4f.BATCH_CONTENT_SIZE == 1


def test_workspace_sizes_are_monotone(zl):
    for kw in (dict(), dict(block_checksum=1, content_checksum=1), dict(block_size_id=7), dict(compression_level=9)):
        p = _prefs(zl, **kw)
        prev = None
        for nf in (1, 2, 100, 4096, 100000):
            row = [zl.lz4f.compressFrameBatchWorkspace(nf, mb, p) for mb in (0, 1, 7, 1000, 65536)]
            assert row == sorted(row), (kw, nf, row)
            if prev is not None:
                assert all(a >= b for a, b in zip(row, prev)), (kw, nf)
            prev = row
    prev = None
    for nf in (1, 2, 100, 4096, 100000):
        row = [zl.lz4f.decompressFrameBatchWorkspace(nf, mb) for mb in (0, 1, 7, 1000, 65536)]
        assert row == sorted(row) and row[-1] > row[0]
        if prev is not None:
            assert all(a >= b for a, b in zip(row, prev))
        prev = row


def test_compress_workspace_holds_slots_and_the_hc_workspace(zl):
    for bsid, bs in ((4, 65536), (5, 262144), (7, 4 << 20)):
        for mb in (1, 100, 9000):
            fast = zl.lz4f.compressFrameBatchWorkspace(10, mb, _prefs(zl, block_size_id=bsid))
            assert fast >= mb * zl.compressBound(bs)                       # one compressBound slot per table entry
            for level in (1, 2, 9, 12):
                hc = zl.lz4f.compressFrameBatchWorkspace(10, mb, _prefs(zl, block_size_id=bsid, compression_level=level))
                assert hc >= fast + zl.batch_compress_hc_workspace(mb, bs), (bsid, mb, level)
            neg = zl.lz4f.compressFrameBatchWorkspace(10, mb, _prefs(zl, block_size_id=bsid, compression_level=-3))
            assert neg == fast                                             # level <= 0 is the fast path: no HC workspace


def test_batch_calls_without_device_fail_loudly(zl):
    """No gfx950 device: both calls return DeviceError and launch nothing (skipped where a device is present, as
    test_no_device_means_loud_failure does)."""
    if zl.device_available():
        return
    L = zl.lib()
    ws = 1 << 20
    assert L.zlz4f_batch_compress_frame(None, None, None, None, None, None, None, None, 4, 16, None, 0, None, ws) == -7
    assert L.zlz4f_batch_compress_frame(None, None, None, None, None, None, None, None, 4, 16, None,
                                        zl.lz4f.BATCH_CONTENT_SIZE, None, ws) == -7
    assert L.zlz4f_batch_decompress_frame(None, None, None, None, None, None, None, None, 4, 16, None, ws) == -7


def test_compress_batch_rejects_bad_flags_before_anything_else(zl):
    """Parameter errors are host arithmetic (ParameterInvalid, -104), checked before the device is looked at."""
    L = zl.lib()
    p = _prefs(zl, content_size=100)
    assert L.zlz4f_batch_compress_frame(None, None, None, None, None, None, None, None, 1, 1, p,
                                        zl.lz4f.BATCH_CONTENT_SIZE, None, 0) == -104
    assert L.zlz4f_batch_compress_frame(None, None, None, None, None, None, None, None, 1, 1, None, 2, None, 0) == -104
