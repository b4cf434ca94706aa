"""Inputs and destination capacities that reach every OutputTooSmall guard of compressHC (src/lz4hc.zig): the literal
guard (:320-325), the match-length guard (:355-359), the final-literals guard (:1037, :944, :1364) and the tiny-block
guard (:1395).  Shared by tests/test_oracle_hc_capacity.py (CPU) and tests/test_gpu_hc_capacity.py."""
import datagen as dg

FINAL_RUNS = (14, 15, 16, 269, 270, 271, 525)      # final literal runs: no / one / two length-extension bytes
MID_RUNS = (15, 270)                               # literal runs in the middle of a block
ML_CODES = (14, 15, 16, 269, 270, 271)             # match length - MINMATCH


def _tail(n, seed, avoid):
    """n random bytes whose first byte is not `avoid` (so the match before them ends where they start)"""
    t = bytearray(dg.random_bytes(n, seed))
    if t and t[0] == avoid:
        t[0] ^= 0x80
    return bytes(t)


def final_run_inputs():
    """a long match (a text repeat, or a run of zeros) followed by a final literal run of exactly L bytes"""
    out = []
    for L in FINAL_RUNS:
        head = bytes(dg.text_bytes(700, 100 + L))
        out.append(("text+rep+final%d" % L, head + head[100:500] + _tail(L, 200 + L, head[500])))
        out.append(("zeros+final%d" % L, bytes(dg.text_bytes(40, 300 + L)) + b"\0" * 400 + _tail(L, 400 + L, 0)))
    return out


def mid_run_inputs():
    """literal runs of 15 and 270 bytes between matches, then a short final run"""
    out = []
    for L in MID_RUNS:
        head = bytes(dg.text_bytes(600, 500 + L))
        mid = _tail(L, 600 + L, head[0])
        b = head + mid + head[:200] + _tail(L, 700 + L, head[200]) + head[200:400] + _tail(20, 800 + L, head[400])
        out.append(("mid%d" % L, b))
    return out


def match_code_inputs():
    """one match of length code + 4 for each code around 15 and 270 (two blocks: a single match, and the match
    followed by a 15-byte final run)"""
    out = []
    for code in ML_CODES:
        ml = code + 4
        x = bytes(dg.random_bytes(600, 900 + code))
        gap = _tail(40, 1000 + code, x[99])
        m = x[100:100 + ml]
        out.append(("mlcode%d" % code, x + gap + m + _tail(40, 1100 + code, x[100 + ml])))
        out.append(("mlcode%d+final15" % code, x + gap + m + _tail(15, 1200 + code, x[100 + ml])))
    return out


def tiny_inputs():
    """blocks of 1..13 bytes (13 is the first that is not encodeLiterals-only) with cap n, n + 1 and 0"""
    out = []
    for n in range(1, 14):
        b = bytes(dg.text_bytes(n, 1300 + n))
        for cap in (n, n + 1, 0):
            out.append(("tiny%d/cap%d" % (n, cap), b, cap))
    return out


def ordinary_inputs():
    return [("text/65536", bytes(dg.text_bytes(65536, 1401))), ("reptext/65536", bytes(dg.reptext_bytes(65536, 1402)))]


def swept_inputs():
    return final_run_inputs() + mid_run_inputs() + match_code_inputs() + ordinary_inputs()


def sweep_caps(w):
    """every cap from w - 300 to w + 1, a coarse sweep from 0 to w, and w // 2 (w = the size at the bound)"""
    caps = set(range(max(0, w - 300), w + 2)) | set(range(0, w + 1, max(1, w // 16))) | {w // 2}
    return sorted(caps)
