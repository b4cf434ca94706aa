"""Models of the identities k_compress_fast's window relies on since the ring is read in one hop (no GPU needed).

The window's dwords: the ring's registers r0 / r1 hold the 128 dwords from rbase on, a window at A starts s0 = (A - rbase) >> 2
dwords in.  Two hops: W = bpermute(sel, (s0 + lane) & 63) with sel = lane >= s0 ? r0 : r1, then lane l reads W[jw + k],
jw = ((A & 3) + l) >> 2.  One hop: lane l reads sel at the byte address (ja + 4 k) & 0xFF, ja = (4 s0 + 4 jw) & 0xFF.  Both
must deliver dword s0 + jw + k of r0 ++ r1, for every s0, every A & 3, every lane and k = 0..12 -- also where
s0 + jw + k passes lane 63.

The lane idioms: lane_rank(m) (v_mbcnt_lo + v_mbcnt_hi) against popcount(m & lanes_below), in_mask(m) (the mask used as the
lane's condition) against (m >> lane) & 1."""
import numpy as np

LANES = np.arange(64, dtype=np.int64)
R0 = (0x10000 + np.arange(64)).astype(np.int64)          # distinct dwords
R1 = (0x20000 + np.arange(64)).astype(np.int64)
RING = np.concatenate([R0, R1])


def bpermute(addr, v):
    """ds_bpermute_b32 as the kernels use it: every address is below 256 and a multiple of 4 (asserted, nothing is left
    to what the hardware does with more), lane l reads v[addr[l] / 4]"""
    addr = np.asarray(addr)
    assert ((addr >= 0) & (addr < 256) & (addr % 4 == 0)).all()
    return v[addr >> 2]


def add_wrap_byte(a, off):
    return (a + off) & 0xFF


def snapshot(s0):
    return np.where(LANES >= s0, R0, R1)


def two_hops(s0, a3, k):
    W = bpermute(((s0 + LANES) & 63) << 2, snapshot(s0))
    jw = (a3 + LANES) >> 2
    assert (jw + k < 64).all()
    return bpermute((jw + k) << 2, W)


def one_hop(s0, a3, k):
    rel = 4 * s0 + a3                                     # A - rbase: rbase is a multiple of 4
    ja = ((rel & ~3) + ((a3 + LANES) & ~3)) & 0xFF
    return bpermute(add_wrap_byte(ja, 4 * k), snapshot(s0))


def test_one_hop_delivers_the_window_dword():
    wrapped = 0
    for s0 in range(64):
        for a3 in range(4):
            jw = (a3 + LANES) >> 2
            for k in range(13):
                want = RING[s0 + jw + k]                  # < 128: s0 <= 63, jw <= 16, k <= 12
                got2, got1 = two_hops(s0, a3, k), one_hop(s0, a3, k)
                assert np.array_equal(got2, want), (s0, a3, k)
                assert np.array_equal(got1, want), (s0, a3, k)
                wrapped += int((s0 + jw + k > 63).sum())
    assert wrapped > 0


def test_snapshot_never_needs_a_third_register():
    # the last dword a window reads (lane 63, A & 3 = 3, k = 12) lies inside r0 ++ r1 for every s0
    assert 63 + ((3 + 63) >> 2) + 12 < 128


# ---- lane idioms ----
def mbcnt_lo(mask_lo, acc, lane):
    below = (1 << lane) - 1 if lane < 32 else 0xFFFFFFFF
    return acc + bin(mask_lo & below).count("1")


def mbcnt_hi(mask_hi, acc, lane):
    below = 0 if lane < 32 else (1 << (lane - 32)) - 1
    return acc + bin(mask_hi & below).count("1")


def lane_rank(m, lane):
    return mbcnt_hi(m >> 32, mbcnt_lo(m & 0xFFFFFFFF, 0, lane), lane)


def in_mask(m, lane):
    half = (m >> 32) if lane >= 32 else (m & 0xFFFFFFFF)   # the condition register's half this lane belongs to
    return (half >> (lane & 31)) & 1


def _masks():
    rng = np.random.default_rng(15)
    full = (1 << 64) - 1
    ms = [0, full] + [1 << b for b in range(64)] + [full ^ (1 << b) for b in range(64)]
    for b in (31, 32):
        ms += [(1 << b) - 1, (1 << (b + 1)) - 1, full ^ ((1 << b) - 1), (1 << b) | 1, (1 << b) | (1 << 63),
               (1 << 31) | (1 << 32), 0xFFFFFFFF, 0xFFFFFFFF00000000, 0x7FFFFFFF, 0x1FFFFFFFF, 0xFFFFFFFE00000000]
    ms += [int(x) for x in rng.integers(0, 1 << 63, 400, dtype=np.uint64) * 2 + rng.integers(0, 2, 400, dtype=np.uint64)]
    ms += [int(a) & int(b) for a, b in zip(rng.integers(0, 1 << 63, 100, dtype=np.uint64) * 2,
                                             rng.integers(0, 1 << 63, 100, dtype=np.uint64) * 2 + 1)]   # sparse ones
    return ms


def test_lane_rank_is_the_prefix_popcount():
    for m in _masks():
        for lane in range(64):
            assert lane_rank(m, lane) == bin(m & ((1 << lane) - 1)).count("1"), (hex(m), lane)


def test_in_mask_is_the_lanes_own_bit():
    for m in _masks():
        for lane in range(64):
            assert in_mask(m, lane) == (m >> lane) & 1, (hex(m), lane)
