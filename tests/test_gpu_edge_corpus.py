"""The edge corpus (tests/edgegen.py) through the plain batch compressors on the HIP path, status for status and byte for
byte against the oracle.  tests/test_edge_corpus_cpu.py proves on the oracle that each case's parse turns on the one
comparison it is about (reach 65535 / 65536, the walk's early exit, the attempt count, the pattern step's clamp,
position 0), so a kernel that is off by one there gives other bytes here.

One batch per (call, level or acceleration, declared bound): the accept and the refuse twin of every pair, and the decoy
variants of one level, lie next to each other in it, i.e. in neighbouring wavefronts.  Run on the GPU box: pytest -m gpu.
"""
import pytest

import edgegen as eg
import gpu_harness as gh
from test_gpu_declared_bound import BOUNDS
from test_gpu_dest_size_batch import Batch
from test_gpu_dest_size_batch import _check as _check_dest_size
from test_gpu_parity import _cmp

pytestmark = pytest.mark.gpu

_want = {}


def _oracle(oracle, sel, kind, v):
    """the oracle's stream of every selected case, computed once per setting"""
    out = []
    for _, name, b, _ in sel:
        key = (name, kind, v)
        if key not in _want:
            _want[key] = oracle.compress_fast(b, v) if kind == "fast" else oracle.compress_hc(b, v)
        out.append(_want[key])
    return out


@pytest.mark.parametrize("layout", [None, gh.Packed(seed=23, fill="cont")], ids=["aligned", "packed"])
@pytest.mark.parametrize("max_in", BOUNDS)
@pytest.mark.parametrize("accel", eg.ACCELS)
def test_compress_fast(zl, oracle, gpu, accel, max_in, layout):
    """every family (the HC-specific ones simply add blocks) under every declared bound that admits the block: the
    16-bit table for the small families, the tagged and the untagged 32-bit table for all"""
    sel = [c for c in eg.cases() if c[3]["fast"] and len(c[2]) <= max_in]
    assert {c[0] for c in sel} >= {"early_exit", "budget", "pos0"}
    assert max_in < (1 << 24) or {c[0] for c in sel} >= {"far", "pattern_far"}   # (65547 and 65548 admit the small only)
    got = gh.compress_fast(zl, [c[2] for c in sel], gpu, accel=accel, layout=layout, max_in=max_in)
    _cmp([c[1] for c in sel], got, _oracle(oracle, sel, "fast", accel))


@pytest.mark.parametrize("links", ["lds", "hbm", "far"])
@pytest.mark.parametrize("level", eg.HC_LEVELS)
def test_compress_hc(zl, oracle, gpu, level, links):
    """every family at every level: the small families with their natural bound (links in LDS) and under
    max_in_len = 65537 (32-bit links in HBM), the far families in HBM by their size"""
    sel = eg.large() if links == "far" else eg.small()
    max_in = 65537 if links == "hbm" else None
    assert (min(len(c[2]) for c in sel) > 65547) if links == "far" else (max(len(c[2]) for c in sel) <= 65536)
    got = gh.compress_hc(zl, [c[2] for c in sel], gpu, level, max_in=max_in)
    _cmp([c[1] for c in sel], got, _oracle(oracle, sel, "hc", level))


def test_compress_dest_size(zl, oracle, gpu):
    """the far and pos0 blocks at capacity = bound and at half the oracle's size: the replay of the last window runs
    the same reach test"""
    items, caps = [], []
    for fam, name, b, m in eg.cases():
        if fam in ("pos0", "far"):
            for cap in (zl.compressBound(len(b)), len(oracle.compress_default(b)) // 2):
                items.append(b)
                caps.append(cap)
    assert len(items) == 2 * (64 + 4)
    bt = Batch(zl, items, caps, gpu)
    bt.call()
    _check_dest_size(oracle, items, caps, bt.collect())
