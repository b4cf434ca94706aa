"""compressHC with destinations shorter than the bound, on every HC emit kernel: statuses and bytes against
oracle.binding.compress_hc_expected, no byte written past the capacity (gpu_harness' guard bands).

The batch's max_in_len picks the kernels (zlz4_launch_compress_hc):

  level 2           k_hc_mid_serial
  levels 3-9        k_hc_parse_emit<uint32_t> (max_in_len <= 65536) / k_hc_parse_emit<uint64_t> (> 65536)
  levels 10-12      k_hc_opt_parse_wave (<= 65536) / k_hc_opt_parse<uint64_t> (> 65536)

so each level runs twice: once on the inputs of tests/hccapgen.py alone, once with a 70 001-byte block added.  Every
batch must meet the case where the reference writes the final run's length-extension bytes past `cap` (DESIGN.md
section 2), and the kernel must refuse it."""
import pytest

import datagen as dg
import gpu_harness as gh
import hccapgen as hg

pytestmark = pytest.mark.gpu

LEVELS = (2, 3, 6, 9, 10, 11, 12)
WIDE_BLOCK = ("text/70001", bytes(dg.text_bytes(70001, 1403)))


def _kernel(level, wide):
    if level == 2:
        return "k_hc_mid_serial"
    if level <= 9:
        return "k_hc_parse_emit<uint64_t>" if wide else "k_hc_parse_emit<uint32_t>"
    return "k_hc_opt_parse<uint64_t>" if wide else "k_hc_opt_parse_wave"


_CACHE = {}


def _case(oracle, name, b, level, cap, w):
    """-> (expected status or bytes, whether the reference wrote past cap); the same for both widths.  w = the size at
    the bound; the reference can overrun only a cap within the final run's extension bytes below w."""
    key = (name, level, cap)
    if key not in _CACHE:
        overran = w - 8 <= cap < w and not isinstance(oracle.compress_hc(b, level, cap), int)
        _CACHE[key] = (oracle.compress_hc_expected(b, level, cap), overran)
    return _CACHE[key]


def _batch(oracle, level, wide):
    items, caps, names, want, overran = [], [], [], [], []

    def add(name, b, c, w):
        e, o = _case(oracle, name, b, level, c, w)
        items.append(b); caps.append(c); names.append("%s/cap%d(w%d)" % (name, c, w)); want.append(e); overran.append(o)
    for name, b in hg.swept_inputs() + ([WIDE_BLOCK] if wide else []):
        w = len(oracle.compress_hc(b, level))
        for c in hg.sweep_caps(w):
            add(name, b, c, w)
    for name, b, c in hg.tiny_inputs():
        add(name, b, c, len(b) + 1)
    return items, caps, names, want, overran


def _cmp(got, want, names):
    bad = []
    for name, (n, data), w in zip(names, got, want):
        if isinstance(w, int):
            if n != w:
                bad.append("%s: status %d, expected %d" % (name, n, w))
        elif n != len(w) or data != w:
            bad.append("%s: size %d vs expected %d%s" % (name, n, len(w), " (bytes differ)" if n == len(w) else ""))
    assert not bad, "%d/%d mismatches: %s" % (len(bad), len(names), "; ".join(bad[:8]))


@pytest.mark.parametrize("wide", [False, True], ids=["le64k", "gt64k"])
@pytest.mark.parametrize("level", LEVELS)
def test_capacity_sweep(zl, oracle, gpu, level, wide):
    items, caps, names, want, overran = _batch(oracle, level, wide)
    assert (max(len(b) for b in items) > 65536) == wide
    got = gh.compress_hc(zl, items, gpu, level, caps=caps)
    _cmp(got, want, names)
    ndiv = sum(overran)
    nok = sum(not isinstance(w, int) for w in want)
    print("level %d %s: %d blocks, %d fit, %d where the reference overruns cap -> OutputTooSmall"
          % (level, _kernel(level, wide), len(items), nok, ndiv))
    assert ndiv >= 20, "the divergent case was not reached in the %s batch" % _kernel(level, wide)
    assert all(got[i][0] == oracle.OUTPUT_TOO_SMALL for i in range(len(items)) if overran[i])


@pytest.mark.parametrize("level", [2, 9, 12])
def test_single_buffer_short_destination(zl, oracle, gpu, level):
    """zl.compressHC(src, level, dst_cap): the single-buffer call reports the same statuses"""
    picks = [x for x in hg.swept_inputs() if x[0] in ("zeros+final525", "text+rep+final270", "mid270", "mlcode270")]
    bad = []
    picks += [(name, b) for name, b, cap in hg.tiny_inputs() if cap == 0 and len(b) in (1, 7, 12)]
    for name, b in picks:
        w = len(oracle.compress_hc(b, level))
        for cap in sorted({w + 1, w, w - 1, w - 2, w - 3, w // 2, 1, 0}):
            if cap < 0:
                continue
            e = oracle.compress_hc_expected(b, level, cap)
            try:
                g = zl.compressHC(b, level, cap)
            except zl.Lz4Error as err:
                g = err.code
            if g != e:
                bad.append("%s/cap%d: %r vs %r" % (name, cap, g if isinstance(g, int) else len(g),
                                                    e if isinstance(e, int) else len(e)))
    assert not bad, "; ".join(bad[:8])
