"""CPU tests of oracle.binding.compress_hc_expected: the restatement of compressHC keeps the reference's final-literals
guard (src/lz4hc.zig:1037, :944, :1364), which lets the length-extension bytes of the final run land past `cap`
(DESIGN.md section 2).  The binding gives the restatement room for them, and the helper maps such a result to
OutputTooSmall, as the kernels return."""
import pytest

import hccapgen as hg

FAMILIES = [(2, "compressMID"), (3, "compressHashChain"), (9, "compressHashChain"), (10, "compressOptimal"),
            (12, "compressOptimal")]


def _ext_bytes(fl):
    return 0 if fl < 15 else 1 + (fl - 15) // 255


@pytest.mark.parametrize("level,family", FAMILIES)
def test_divergent_final_run_maps_to_output_too_small(oracle, level, family):
    for L in hg.FINAL_RUNS:
        name, b = [x for x in hg.final_run_inputs() if x[0] == "zeros+final%d" % L][0]
        full = oracle.compress_hc(b, level)
        w = len(full)
        assert oracle.decompress_safe(full, len(b)) == b
        assert full[-L:] == b[-L:]                           # the block ends in a literal run of exactly L bytes
        diverged = []
        for cap in range(w - 8, w + 2):
            raw = oracle.compress_hc(b, level, cap)
            want = oracle.compress_hc_expected(b, level, cap)
            if cap >= w:
                assert raw == full and want == full, (name, cap)
            elif isinstance(raw, int):
                assert raw == want == oracle.OUTPUT_TOO_SMALL, (name, cap)
            else:
                # the reference's case: it passed op + fl + 1 <= oend and wrote the extension bytes past cap
                assert raw == full and len(raw) > cap, (name, cap)
                assert want == oracle.OUTPUT_TOO_SMALL, (name, cap)
                diverged.append(cap)
        # exactly the caps that hold everything but some of the extension bytes
        assert diverged == list(range(w - _ext_bytes(L), w)), (family, name, w, diverged)


@pytest.mark.parametrize("level", [2, 3, 9, 10, 12])
def test_expected_passes_other_results_through(oracle, level):
    for name, b in hg.mid_run_inputs() + hg.match_code_inputs()[:2]:
        full = oracle.compress_hc(b, level)
        w = len(full)
        for cap in (None, w, w + 1, w - 1, w // 2, 1, 0):
            raw = oracle.compress_hc(b, level, cap)
            want = oracle.compress_hc_expected(b, level, cap)
            if isinstance(raw, int) or len(raw) <= (w if cap is None else cap):
                assert want == raw, (name, cap)
            else:
                assert want == oracle.OUTPUT_TOO_SMALL
    for name, b, cap in hg.tiny_inputs():
        # encodeLiterals (:1394-1425) checks its whole output: the restatement never exceeds cap there
        want = oracle.compress_hc_expected(b, level, cap)
        if cap > len(b):
            assert want == bytes([len(b) << 4]) + b, name
        else:
            assert want == oracle.OUTPUT_TOO_SMALL, name


def test_sweep_reaches_every_guard_family(oracle):
    """the GPU capacity sweep's inputs reach the divergent case in every family (tests/test_gpu_hc_capacity.py
    asserts the same per kernel batch)"""
    for level, family in FAMILIES:
        n = 0
        for name, b in hg.final_run_inputs()[:4] + hg.mid_run_inputs():
            w = len(oracle.compress_hc(b, level))
            n += sum(1 for c in range(w - 4, w) if not isinstance(oracle.compress_hc(b, level, c), int))
        assert n > 0, family
