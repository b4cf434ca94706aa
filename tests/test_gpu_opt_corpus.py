"""The price-parser corpus (tests/optgen.py) through zlz4_batch_compress_hc at levels 10-12, status for status and byte
for byte against the oracle.  tests/test_opt_corpus_cpu.py proves on the oracle's counters what each block reaches:
windows that grow across record 1000 (where k_hc_opt_parse_wave's opt[] passes from packed LDS records to HBM structs),
both early-encode exits with the streams that do not decode and the block that ends in OutputTooSmall, price ties, and
windows cut by the end of the block.

Every level runs on both parse kernels: the natural bound selects k_hc_opt_parse_wave, max_in_len = 65537 sends the
same blocks through k_hc_opt_parse<uint64_t>; the wave kernel also runs on the packed layout and with the batch
reversed (a record a block reads without having written it would hold its neighbour's).  The 65 536-byte block is the
last of the batch in one order: the reload of its search results then runs past the result area.
Run on the GPU box: pytest -m gpu.
"""
import pytest

import gpu_harness as gh
import optgen as og
from test_gpu_parity import _cmp

pytestmark = pytest.mark.gpu

_want = {}


def _oracle(oracle, sel, level, caps=None):
    out = []
    for i, (_, name, b, _) in enumerate(sel):
        key = (name, level, None if caps is None else caps[i])
        if key not in _want:
            _want[key] = oracle.compress_hc(b, level) if caps is None else oracle.compress_hc_expected(b, level, caps[i])
        out.append(_want[key])
    return out


def _wave_batch(level):
    """the cases of the level that fit the wave kernel, the full-size block last"""
    sel = og.for_level(og.wave(), level)
    sel.sort(key=lambda c: len(c[2]) == og.FULL)
    assert sel[-1][1] == "ends/full" and {c[0] for c in sel} == {"window", "optnum", "sufficient", "price", "ends"}
    return sel


def _lane_batch(level):
    """the same without the two large blocks (the one-lane kernel takes a block per lane)"""
    return [c for c in _wave_batch(level) if not c[3].get("big")]


_got = {}


def _run(zl, gpu, level, path):
    """-> {case name: (status, bytes)}; each (level, path) runs once per session"""
    if (level, path) not in _got:
        sel = _lane_batch(level) if path == "lane" else _wave_batch(level)
        if path == "reversed":
            sel = sel[::-1]
        got = gh.compress_hc(zl, [c[2] for c in sel], gpu, level, max_in=65537 if path == "lane" else None,
                             layout=gh.Packed(seed=23, fill="cont") if path == "packed" else None)
        _got[(level, path)] = dict(zip([c[1] for c in sel], got))
    return _got[(level, path)]


@pytest.mark.parametrize("path", ["wave", "lane", "packed", "reversed"])
@pytest.mark.parametrize("level", og.LEVELS)
def test_against_the_oracle(zl, oracle, gpu, level, path):
    sel = _lane_batch(level) if path == "lane" else _wave_batch(level)
    assert max(len(c[2]) for c in sel) <= 65536 and len(sel) >= 50
    got = _run(zl, gpu, level, path)
    want = _oracle(oracle, sel, level)
    _cmp([c[1] for c in sel], [got[c[1]] for c in sel], want)
    # the batch holds what the module is about: an exit whose stream exists, and (level 12) the defect's status
    assert any(c[1].startswith("optnum/chain100") for c in sel)
    assert (oracle.OUTPUT_TOO_SMALL in [w for w in want if isinstance(w, int)]) == (level == 12)


@pytest.mark.parametrize("level", og.LEVELS)
def test_both_kernels_and_both_orders_agree(zl, gpu, level):
    wave, lane, rev = (_run(zl, gpu, level, p) for p in ("wave", "lane", "reversed"))
    assert set(lane) < set(wave) == set(rev)
    assert [n for n in lane if lane[n] != wave[n]] == []
    assert [n for n in wave if rev[n] != wave[n]] == []


@pytest.mark.parametrize("level", og.LEVELS)
def test_wide_blocks(zl, oracle, gpu, level):
    """70 001 bytes: k_hc_opt_parse<uint64_t> by size, the window and the OPT_NUM exit past offset 65 536"""
    sel = [c for c in og.cases() if c[0] == "wide"]
    assert len(sel) == 2 and all(len(c[2]) == og.WIDE for c in sel)
    got = gh.compress_hc(zl, [c[2] for c in sel], gpu, level)
    _cmp([c[1] for c in sel], got, _oracle(oracle, sel, level))


def _sweep_cases(level):
    """one window beyond the split, one OPT_NUM exit, one sufficient_len exit at cur > 0, and (level 12) the block whose
    exit ends in OutputTooSmall, scaled by its twin's size"""
    s = og.SUFFICIENT[level]
    names = ["window/t1063", "optnum/chain100/s1/f15",
             "sufficient/l%d/chained/len%d" % (level, s + 1) if level < 12 else "sufficient/l12/cur/pre50/len4096"]
    if level == 12:
        names.append("optnum/long_pair/sum4096")
    by_name = {c[1]: c for c in og.cases()}
    return [by_name[n] for n in names]


@pytest.mark.parametrize("wide", [False, True], ids=["wave", "lane"])
@pytest.mark.parametrize("level", og.LEVELS)
def test_capacity_sweep(zl, oracle, gpu, level, wide):
    """destinations of w - 40 .. w + 1 and w // 2 bytes (w = the size at the bound): statuses and bytes as
    oracle.compress_hc_expected, nothing written past the capacity (gpu_harness' guard bands)"""
    sel, caps = [], []
    for c in _sweep_cases(level):
        r = oracle.compress_hc(c[2], level)
        if isinstance(r, int):
            assert c[1] == "optnum/long_pair/sum4096"
            r = oracle.compress_hc([x for x in og.cases() if x[1] == c[3]["twin"]][0][2], level)
        w = len(r)
        for cap in sorted(set(range(w - 40, w + 2)) | {w // 2}):
            sel.append(c)
            caps.append(cap)
    want = _oracle(oracle, sel, level, caps)
    got = gh.compress_hc(zl, [c[2] for c in sel], gpu, level, caps=caps, max_in=65537 if wide else None)
    _cmp(["%s/cap%d" % (c[1], cap) for c, cap in zip(sel, caps)], got, want)
    fit = sum(not isinstance(w, int) for w in want)
    assert len(sel) == 43 * (4 if level == 12 else 3)
    assert fit == 3 * 2, fit                         # cap = w and w + 1 of the three blocks that have a stream
