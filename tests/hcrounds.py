"""Batches that take batch_compress_hc through every round of launch_hc_chunked (tests/test_gpu_hc_rounds.py; the
conditions are checked without a GPU in tests/test_big_block_inputs_cpu.py).

The launcher works in rounds of half a chunk and alternates between the two halves of its result area (levels 10-12: of
its link area too).  A half is first reused in round 2 (the first half) and round 3 (the second), after an event wait
and, on the greedy path, a memset.  With more than two chunks of blocks there are at least five rounds: both halves are
reused and the first one twice.
"""
import numpy as np

import datagen as dg

SMALL_N = 16900                                  # blocks of the small-block batch (chunk 8192, rounds of 4096)
SMALL_BIG = 20000                                # its one larger block, which is the batch's max_in_len
HBM_MAX_IN = (1 << 24) + 1                       # declared bound of the HBM-link batch: the 6 GiB cap leaves ~31 blocks per chunk
MID_TABLES = 2 * 16384 * 4                       # bytes of level 2's two tables per block (zlz4_hc_mid_workspace_bytes(1))


def chunk_of(zl, n, max_in):
    """blocks per chunk for a call with n blocks: the workspace is a whole number of per-block shares"""
    return zl.batch_compress_hc_workspace(n, max_in) // zl.batch_compress_hc_workspace(1, max_in)


def small_blocks():
    """SMALL_N blocks of 100..900 bytes, the same length every 8192 blocks, so that block i of rounds 2 and 3 lies where
    block i - 8192 lay in the result area.
      * even i: D-text, one vocabulary, another seed per block: a stale table or link candidate passes the 4-byte compare;
      * odd i: D-reptext in rounds 0, 1 and 4, random bytes of the same length in rounds 2 and 3: a match left behind by
        the earlier round would be emitted where the oracle has literals;
      * the blocks on both sides of every round boundary, and the last: empty, 12 bytes, 13 bytes, 300 x "A", in turn;
      * one 20 000-byte text block in the last round."""
    rng = np.random.default_rng(1609)
    lens = rng.integers(100, 901, 8192)
    items = []
    for i in range(SMALL_N):
        n = int(lens[i % 8192])
        if i % 2 == 0:
            items.append(bytes(dg.text_bytes(n, 70000 + i)))
        elif (i // 4096) in (2, 3):
            items.append(bytes(dg.random_bytes(n, 70000 + i)))
        else:
            items.append(bytes(dg.reptext_bytes(n, 70000 + i)))
    edge = (b"", b"abcabcabcabc", b"abcabcabcabcd", b"A" * 300)
    for k, i in enumerate((4095, 4096, 8191, 8192, 12287, 12288, 16383, 16384, SMALL_N - 1)):
        items[i] = edge[k % 4]
    items[16700] = bytes(dg.text_bytes(SMALL_BIG, 99))
    return items


def round_blocks(n, chunk):
    """blocks per round of a call with n blocks whose chunk holds `chunk`: half a chunk once there is more than one round"""
    return chunk // 2 if chunk >= 2 and n > chunk // 2 else chunk


def boundary_blocks(n, sub, seed, empty=True):
    """n blocks of 200..599 bytes for rounds of `sub` blocks (tests/test_gpu_hc_round_boundaries.py).  Block i lies in
    result slot (round & 1) * sub + i % sub; the blocks that share a slot have the same length; rounds 0 and 1 hold
    D-reptext, the rounds that reuse a half hold random bytes: a match left behind by the earlier round would be emitted
    where the reference has literals.  Block 1 has 13 bytes; block sub + 1 (round 1) is empty if `empty` and n >= 5."""
    lens = np.random.default_rng(seed).integers(200, 600, 2 * sub)
    items = []
    for i in range(n):
        k = int(lens[((i // sub) & 1) * sub + i % sub])
        items.append(bytes((dg.random_bytes if i // sub >= 2 else dg.reptext_bytes)(k, seed + 1 + i)))
    if n >= 2:
        items[1] = b"abcabcabcabcd"
    if empty and n >= 5:
        items[sub + 1] = b""
    return items


def periodic_items(level):
    """Blocks with a period (random content repeated every 1 .. 40000 bytes, some with noise in the middle or two periods
    in a row): the inputs of test_gpu_parity.test_compress_hc_periodic_inputs."""
    rng = np.random.default_rng(4242 + level)
    items = []
    for period in (1, 2, 3, 5, 16, 40, 63, 64, 100, 255, 256, 257, 1000, 1024, 4096, 5000, 40000):
        for total in (65536, 30011, period * 2 + 70):
            pat = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
            b = bytearray((pat * (total // period + 2))[:max(total, 13)])
            items.append(bytes(b))
            if total > 20000:
                for _ in range(3):                                # a few damaged bytes: runs that end early
                    b[int(rng.integers(0, len(b)))] ^= 0x55
                items.append(bytes(b))
                pat2 = rng.integers(0, 256, max(1, period // 2 + 1), dtype=np.uint8).tobytes()
                half = len(b) // 2
                items.append(bytes(b[:half]) + (pat2 * (half // len(pat2) + 2))[:len(b) - half])   # two periods in a row
    return items
