"""The crafted frame corpus of tests/linkedseqgen.py, no GPU: the generator's plaintext, the CPU models
(tools/pyref/zig_lz4_linked_frame.py, zig_lz4_dict_frame.py) and liblz4 agree on it; its census reaches every class of
decode_block_wave's copy (zig-lz4_amd/csrc/zlz4_device.hpp); and a restatement of how that function copies, with a
`mutant=` switch, shows that the corpus tells a subtly wrong copy from the right one.  The GPU side is
tests/test_gpu_linked_sequences.py."""
import hashlib
import os
import sys

import pytest

import dictframegen
import linkedgen
import linkedseqgen as lsg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_dict_frame as df  # noqa: E402
import zig_lz4_linked_frame as lf  # noqa: E402

CORPUS_SHA256 = "71a66ce59132bc51150c4fbe8ae11adb2f23ce780edd455f6f0d3fb7476176b9"
CORRUPTED, OUTPUT_TOO_SMALL = -3, -1


@pytest.fixture(scope="module")
def items():
    return lsg.corpus()


def pyref(it):
    """-> ((result, bytes), size) of the CPU model for one item"""
    if it.dict_bytes is None:
        return lf.decompress_frame_linked(it.frame, it.cap), lf.frame_size_linked(it.frame)
    return df.decompress_frame_using_dict(it.frame, it.cap, it.dict_bytes), df.frame_size_using_dict(it.frame, len(it.dict_bytes))


@pytest.fixture(scope="module")
def model(items):
    return [pyref(it) for it in items]


# ------------------------------------------------------------------------------------------------ the copy model
class _Unreadable(Exception):
    """a mutant read in front of its buffer"""


def copy_bytes(W, d, s, n, mutant=None):
    """copy_bytes (zlz4_device.hpp): 1 KiB chunks of sixty-four 16-byte pieces in address order (all loads of a chunk,
    then all its stores), then the byte tail on lanes 0..15"""
    if s < 0:
        raise _Unreadable
    if len(W) < d + n:
        W.extend(bytes(d + n - len(W)))
    full = n & ~15
    for k in range(0, full, 1024):
        m = min(1024, full - k)
        W[d + k:d + k + m] = W[s + k:s + k + m]
    tail = n - full
    if mutant == "tail_skipped_at_mod16_1" and tail == 1:
        return
    m = min(tail, {"tail_15_lanes": 15, "tail_14_lanes": 14}.get(mutant, 16))
    W[d + full:d + full + m] = W[s + full:s + full + m]


def decode_block_wave(src, oend, T, history, write=True, mutant=None):
    """decode_block_wave<write, kDict> on one block: T the dictionary tail (b"" without one), `history` the frame's
    output in front of the block (at most 65536 bytes of it) -> (result, the block's bytes)"""
    iend = len(src)
    if iend == 0 or oend == 0:
        return 0, b""
    D, inframe = len(T), len(history)
    hist = inframe + D if mutant == "hist_not_capped" else min(inframe + D, 65536)
    tend = D                                          # W = T ++ history ++ the block's output
    out = D + inframe
    W = bytearray(T) + bytearray(history)
    ip = op = 0
    while ip < iend:
        token = src[ip]; ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if ip >= iend:
                    return CORRUPTED, b""
                b = src[ip]; ip += 1
                lit += b
                if b != 255:
                    break
        if lit > 0:
            if lit > iend - ip:
                return CORRUPTED, b""
            if lit > oend - op:
                return OUTPUT_TOO_SMALL, b""
            if write:
                W.extend(bytes(out + op + lit - len(W)))
                n16 = lit & ~15                       # (the source is the block itself: nothing to overlap)
                tail = lit - n16
                if mutant == "tail_skipped_at_mod16_1" and tail == 1:
                    tail = 0
                else:
                    tail = min(tail, {"tail_15_lanes": 15, "tail_14_lanes": 14}.get(mutant, 16))
                W[out + op:out + op + n16 + tail] = src[ip:ip + n16 + tail]
            ip += lit; op += lit
        if ip >= iend:
            break
        if iend - ip < 2:
            return CORRUPTED, b""
        offset = src[ip] | (src[ip + 1] << 8); ip += 2
        if offset == 0:
            return CORRUPTED, b""
        ml = token & 15
        if ml == 15:
            while True:
                if ip >= iend:
                    return CORRUPTED, b""
                b = src[ip]; ip += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if ml > oend - op:
            return OUTPUT_TOO_SMALL, b""
        bound = hist + {"hist_bound_plus_1": 1, "hist_bound_minus_1": -1}.get(mutant, 0)
        if offset > op and offset - op > bound:
            return CORRUPTED, b""
        if write:
            o, n = out + op, ml
            if D and offset > op + (0 if mutant == "split_without_inframe" else inframe):
                a = offset - op - (0 if mutant == "split_without_inframe" else inframe)
                n1 = min(a, n)
                copy_bytes(W, o, tend - (offset if mutant == "T_part_from_tend_minus_offset" else a), n1, mutant)
                o += n1
                n -= n1
            m = o - offset
            if n == 0:
                pass
            elif offset >= n or offset >= (1023 if mutant == "far_copy_from_1023" else 1024):
                copy_bytes(W, o, m, n, mutant)
            else:
                made = 0
                while made < n:
                    if mutant == "doubling_step_made":
                        have = made or offset
                    elif mutant == "doubling_step_twice_made":
                        have = 2 * made or offset
                    else:
                        have = made + offset
                    n1 = min(have, n - made)
                    copy_bytes(W, o + made, m, n1, mutant)
                    made += n1
        op += ml
    return op, (bytes(W[out:out + op]) if write else bytes(op))      # (the size walk keeps only the lengths)


def wave_model(it, mutant=None):
    """-> ((result, bytes), size): the frame walk of the CPU model over decode_block_wave above"""
    T = (it.dict_bytes or b"")[-65536:]

    def decoder(write):
        def decode(block, room, history):
            try:
                return decode_block_wave(block, 0xFFFFFFFF if room is None else room, T, history or b"", write, mutant)
            except _Unreadable:
                return CORRUPTED, b""
        return decode
    return lf._walk(it.frame, it.cap, decoder(True)), lf._walk(it.frame, None, decoder(False))[0]


# Three restatements that no frame can tell from the right one.  Offsets are 16 bits, so offset - op never exceeds 65535
# and the cap of hist at 65536 never decides.  The doubling loop's source [m, m + made) repeats the same period as
# [m, m + made + offset) as long as `made` is a multiple of offset (the first copy taken as `offset` bytes).  The tail is
# n % 16 <= 15 bytes, so its sixteenth lane never stores.  Each has a neighbour among MUTANTS that frames do tell apart:
# the bound off by one, the step 2 * made, fourteen lanes.
EQUIVALENT = ("hist_not_capped", "doubling_step_made", "tail_15_lanes")
MUTANTS = ("far_copy_from_1023", "doubling_step_twice_made", "tail_skipped_at_mod16_1", "tail_14_lanes",
           "hist_bound_plus_1", "hist_bound_minus_1", "split_without_inframe", "T_part_from_tend_minus_offset")


# ------------------------------------------------------------------------------------------------ the tests
def test_generator_has_not_drifted(items):
    h = hashlib.sha256()
    for it in items:
        h.update(it.frame)
    assert h.hexdigest() == CORPUS_SHA256
    assert len({it.name for it in items}) == len(items)
    assert sum(len(it.plain) for it in items if it.plain is not None) < 32 << 20


def test_generator_model_and_liblz4_agree(items, model):
    z, zd = linkedgen.liblz4f(), dictframegen.liblz4fd()
    checked = 0
    for it, ((r, got), size) in zip(items, model):
        want = it.expected()
        if want is not None:
            assert (r, got, size) == (len(want), want, len(want)), it.name
        if it.status is not None:
            assert r == it.status, (it.name, r, it.status)
        if it.twin_of is not None and want is not None:
            whole = next(x for x in items if x.name == it.twin_of)
            assert whole.plain is None or whole.plain.startswith(want), it.name
        if it.liblz4_ok:
            assert want is not None
            if it.dict_bytes is None and z is not None:
                assert z.decompress(it.frame, it.cap) == want, it.name
                checked += 1
            elif it.dict_bytes is not None and zd is not None:
                assert zd.decompress(it.frame, it.cap, it.dict_bytes) == want, it.name
                checked += 1
    if z is not None and zd is not None:
        assert checked > 300, checked


def test_census_reaches_every_class(items):
    c = lsg.census(items)
    for key in ("doubling_lt64", "doubling_64_1023", "far_overlap", "inside_T", "crosses_T", "crosses_T_overlaps",
                "crosses_T_overlaps_inframe", "earlier_block", "crosses_block_overlapping"):
        assert c[key] > 0, (key, c)
    assert all(v > 0 for v in c["run_mod16"].values()), c["run_mod16"]
    every = set(lsg.OVERLAP_OFFSETS)
    for p in "abc":
        assert c["place"][p] >= every, (p, sorted(every - c["place"][p]))
    assert c["place"]["d"] >= every - {1}                              # (d) needs 0 < inframe < offset
    for h in [D + pos for D, pos in lsg.HIST_PAIRS] + [65534]:
        assert c["hist"][h][0] > 0 and c["hist"][h][1] > 0, (h, c["hist"])
    assert c["hist"][65535][0] > 0                                     # (offset 65536 does not exist: nothing to refuse)
    lens = {(s["off"], s["ml"]) for it in items if it.family == "overlap" for s in it.seqs or ()}
    for o in lsg.OVERLAP_OFFSETS:
        assert all((o, ml) in lens for ml in lsg.overlap_lengths(o)), o


def test_damaged_frames_fall_on_both_sides(items, model):
    res = [m[0][0] for it, m in zip(items, model) if it.family == "damaged"]
    decoded, failed = sum(r >= 0 for r in res), sum(r < 0 for r in res)
    assert len(res) > 600 and 3 * decoded >= len(res) and 3 * failed >= len(res), (len(res), decoded, failed)


def test_wave_copy_model_reproduces_the_corpus(items, model):
    for it, m in zip(items, model):
        assert wave_model(it) == m, it.name


@pytest.mark.parametrize("mutant", EQUIVALENT)
def test_restatements_no_frame_can_tell_apart(items, model, mutant):
    for it, m in zip(items, model):
        assert wave_model(it, mutant) == m, it.name


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_is_caught(items, model, mutant):
    caught = [it.name for it, m in zip(items, model) if it.family != "damaged" and wave_model(it, mutant) != m]
    assert caught, mutant
