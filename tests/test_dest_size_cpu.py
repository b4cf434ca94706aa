"""Batch compressDestSize (zlz4_batch_compress_dest_size): the parts that need no GPU -- the Python restatement of the
derivation and the search (tools/pyref/zig_lz4_dest_size.py) against the oracle, exported symbols, workspace arithmetic,
the loud failure without a device and the Zig binding's text."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import datagen as dg  # noqa: E402
import dsz_blocks  # noqa: E402
import numpy as np  # noqa: E402
import zig_lz4_dest_size as zd  # noqa: E402

NEW = ("zlz4_batch_compress_dest_size_workspace", "zlz4_batch_compress_dest_size")
DISTS = ("text", "reptext", "mixed", "random", "zero", "ramp")


def _small_blocks():
    """36 blocks, 13..1500 bytes, six per distribution"""
    out = []
    for k, dist in enumerate(DISTS):
        for j, n in enumerate((13, 14, 40, 200, 777, 1500)):
            out.append(bytes(dg.make_blocks(dist, 1, n, seed=31 * k + j + 1)[0]))
    return out


def test_derivation_equals_the_oracle_on_every_prefix(oracle):
    blocks = _small_blocks()
    assert len(blocks) >= 30
    for b in blocks:
        plan = zd.Plan(b, oracle.compress_default(b))
        for m in range(len(b) + 1):
            want = oracle.compress_default(b[:m])
            got = plan.derive(m)
            assert got == want, (len(b), m)
            assert plan.size(m) == len(want), (len(b), m)


def test_search_equals_the_oracle_on_every_cap(oracle):
    for b in _small_blocks()[::3] + [bytes(dg.make_blocks("text", 1, 3000, seed=5)[0])]:
        full = oracle.compress_default(b)
        for cap in range(zd.compress_bound(len(b)) + 2):
            r, consumed, out = zd.compress_dest_size(b, cap, full)
            assert (r, consumed) == oracle.compress_dest_size(b, cap), (len(b), cap)
            assert out == oracle.compress_default(b[:consumed]) and len(out) == r, (len(b), cap)


def _reference_steps(limit):
    """the search loop of src/lz4.zig:327-333 (acceleration 1) from s = 0: {ip - s: forwardIp - ip} at the first attempt
    that visits ip, for every ip it visits up to `limit`"""
    first, fwd, step, nb = {}, 0, 1, 1
    while True:
        ip = fwd
        fwd += step
        step = nb >> 6
        nb += 1
        if ip > limit:
            return first
        first.setdefault(ip, fwd - ip)


def _kernel_step(lit):
    """dsz_step of zig-lz4_amd/csrc/zlz4_dest_size.hip, statement for statement (float32 square root included)"""
    if lit == 1:
        return 1
    if lit == 2:
        return 0
    D = lit - 2
    q = int(np.sqrt(np.float32(D) * np.float32(1.0 / 32.0), dtype=np.float32))
    q = max(q, 1)
    while q > 1 and 32 * q * (q - 1) > D:
        q -= 1
    while 32 * (q + 1) * q <= D:
        q += 1
    return q


def test_step_rule_matches_the_reference_loop():
    """the step after the attempt that finds a match `lit` bytes after its literal start (search from s = a + 1, so
    p - s = lit - 1), for every position the search visits up to 16 MiB in"""
    steps = _reference_steps(1 << 24)
    assert len(steps) > 40000
    for d, want in steps.items():
        lit = d + 1
        assert zd.step_after(lit) == want, lit
        assert _kernel_step(lit) == want, lit


def test_edge_literal_runs_on_every_cap(oracle):
    """first literal runs of 32 q (q + 1) + 2 bytes, where the step after the finding attempt grows"""
    for lit in dsz_blocks.EDGE_RUNS:
        b = dsz_blocks.block_with_first_run(oracle.compress_default, lit)
        full = oracle.compress_default(b)
        plan = zd.Plan(b, full)
        assert plan.seqs[0][2] == lit
        for cap in range(zd.compress_bound(len(b)) + 2):
            r, consumed, out = zd.compress_dest_size(b, cap, full)
            assert (r, consumed) == oracle.compress_dest_size(b, cap), (lit, cap)
            assert out == oracle.compress_default(b[:consumed]), (lit, cap)


def test_fits_is_not_monotone():
    """the reason the search is replayed probe for probe: a prefix can compress smaller than the one a byte shorter"""
    from oracle import binding as ob
    b = bytes(dg.make_blocks("text", 1, 6000, seed=3)[0])
    plan = zd.Plan(b, ob.compress_default(b))
    sizes = [plan.size(m) for m in range(len(b) + 1)]
    assert any(sizes[m] < sizes[m - 1] for m in range(1, len(sizes)))


def test_symbols_exported(zl):
    L = zl.lib()
    for name in NEW:
        assert name in zl.SYMBOLS, name
        assert hasattr(L, name), "libzlz4_amd.so does not export %s" % name


def test_workspace_holds_a_bound_slot_per_block_and_is_monotone(zl):
    prev = None
    for nb in (1, 2, 7, 100, 8192, 262144):
        row = [zl.batch_compress_dest_size_workspace(nb, mx) for mx in (0, 1, 12, 13, 4096, 65536, 65547, 200000, 1 << 20)]
        for mx, ws in zip((0, 1, 12, 13, 4096, 65536, 65547, 200000, 1 << 20), row):
            assert ws >= nb * zl.compressBound(mx), (nb, mx)
        assert row == sorted(row), (nb, row)
        if prev is not None:
            assert all(a >= b for a, b in zip(row, prev)), nb
        prev = row
    assert zl.batch_compress_dest_size_workspace(0, 65536) == 0


def test_batch_call_without_device_fails_loudly(zl):
    """No gfx950 device: DeviceError, nothing launched (a no-op where a device is present, as the other batch tests)."""
    if zl.device_available():
        return
    L = zl.lib()
    assert L.zlz4_batch_compress_dest_size(None, None, None, None, None, None, None, None, None, 4, 16, None, 1 << 20) == -7
    assert L.zlz4_batch_compress_dest_size(None, None, None, None, None, None, None, None, None, 4, 16, None, 0) == -7


def test_root_zig_binds_the_batch_call():
    txt = open(os.path.join(ROOT, "zig-lz4_amd", "zig", "root.zig")).read()
    for name in NEW:
        assert re.search(r'extern "c" fn %s\(' % name, txt), name
    assert "pub fn compressDestSizeBatch(" in txt
    assert "zlz4_batch_compress_dest_size(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.result, " \
           "consumed, b.nblocks, max_in_len, workspace, workspace_bytes)" in txt
