"""Test-side model of legacy lz4 frames (tests/test_legacy_cpu.py, tests/test_gpu_legacy_frame.py; include/zlz4_amd.h,
DESIGN.md section 4.4i): what `lz4 -l` writes -- the magic 0x184C2102, then { u32 LE size, block } repeated.

* `write(data, bs, level)`: the writer, oracle.compress_fast / compress_hc per chunk of bs bytes.
* `build(blocks)`: a frame around compressed blocks of any size, for the decode side; `literal_block`, `zeros_block`,
  `CORRUPT` and `EMPTY` are hand-made blocks.
* `walk(buf)`: the walk written from the format -> Walk(verdict, blocks, consumed).
* `read(buf, cap)`: the reader -- the walk, oracle.decompress_safe per block at a capacity of 8 MiB, the first defect in
  stream order decides -> Read(result, content, consumed, nb).
* `endings()` / `defects()`: crafted frames with the result and `consumed` stated by hand, so that the tests also pin the
  model.
"""
import collections
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import datagen as dg  # noqa: E402
from oracle import binding as oracle  # noqa: E402

MAGIC, MODERN_MAGIC, SKIP_MAGIC = 0x184C2102, 0x184D2204, 0x184D2A50
BLOCK_SIZE = 8 << 20
BLOCK_BOUND = 8421520
INVALID_STATE, MAX_BLOCK_SIZE_INVALID, SRC_TOO_LARGE, DST_TOO_SMALL = -5, -102, -110, -111
HEADER_INCOMPLETE, TYPE_UNKNOWN, SIZE_WRONG, FAILED = -112, -113, -114, -116

Walk = collections.namedtuple("Walk", "verdict blocks consumed")       # blocks: [(offset, size)]
Read = collections.namedtuple("Read", "result content consumed nb")    # content: bytes, or None with result < 0


def u32(b, pos):
    return int.from_bytes(b[pos:pos + 4], "little")


def le32(v):
    return v.to_bytes(4, "little")


# ----------------------------------------------------------------------------- writing
def chunks(data, bs=0):
    bs = bs or BLOCK_SIZE
    return [data[p:p + bs] for p in range(0, len(data), bs)]


def bound(n, bs=0):
    """zlz4f_legacy_compress_frame_bound: the magic, then a size word and a compressBound per chunk"""
    bs = bs or BLOCK_SIZE
    full, rest = divmod(n, bs)
    cb = lambda x: x + x // 255 + 16                                    # noqa: E731
    return 4 + full * (4 + cb(bs)) + ((4 + cb(rest)) if rest else 0)


def build(blocks):
    return le32(MAGIC) + b"".join(le32(len(b)) + bytes(b) for b in blocks)


def write(data, bs=0, level=0):
    """the frame the compress calls write: compressFast(chunk, 1) for level <= 0, else compressHC(chunk, level)"""
    data = bytes(data)
    return build([oracle.compress_fast(c, 1) if level <= 0 else oracle.compress_hc(c, level) for c in chunks(data, bs)])


# ----------------------------------------------------------------------------- hand-made blocks
def _length(n):
    """the extension bytes of a length field whose nibble is 15"""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


def literal_block(data):
    """one sequence of literals alone: decodes to `data` (the single token 0x00 for no data)"""
    data = bytes(data)
    n = len(data)
    return (bytes([n << 4]) if n < 15 else b"\xf0" + _length(n)) + data


def zeros_block(n):
    """n >= 32 zeros: a literal, a match at distance 1, and 12 last literals (liblz4 wants a match to end 5 bytes in front
    of the destination's end)"""
    ml = n - 1 - 12
    return b"\x1f\x00\x01\x00" + _length(ml - 4) + b"\xc0" + b"\x00" * 12


EMPTY = b"\x00"                  # decodes to 0 bytes: valid
CORRUPT = b"\x10A\x00\x00"       # a match at distance 0


# ----------------------------------------------------------------------------- reading
def walk(buf):
    buf = bytes(buf)
    n = len(buf)
    if n < 4:
        return Walk(HEADER_INCOMPLETE, [], n)
    if u32(buf, 0) != MAGIC:
        return Walk(TYPE_UNKNOWN, [], n)
    pos, blocks = 4, []
    while True:
        if pos == n:
            return Walk(0, blocks, n)
        if n - pos < 4:
            return Walk(SIZE_WRONG, blocks, n)
        w = u32(buf, pos)
        if w > BLOCK_BOUND:
            return Walk(0, blocks, pos)
        if w == 0:
            return Walk(FAILED, blocks, n)
        if pos + 4 + w > n:
            return Walk(SIZE_WRONG, blocks, n)
        blocks.append((pos + 4, w))
        pos += 4 + w


def decode_block(block):
    """decompressSafe into 8 MiB -> bytes or None (a block of k bytes decodes to less than 255 k + 64, so the smaller
    destination answers the same)"""
    r = oracle.decompress_safe(block, min(BLOCK_SIZE, 255 * len(block) + 64))
    return None if isinstance(r, int) else r


def read(buf, cap=None):
    buf = bytes(buf)
    w = walk(buf)
    parts = []
    for off, size in w.blocks:
        d = decode_block(buf[off:off + size])
        if d is None:
            return Read(FAILED, None, w.consumed, len(w.blocks))
        parts.append(d)
    if w.verdict:
        return Read(w.verdict, None, w.consumed, len(w.blocks))
    out = b"".join(parts)
    if cap is not None and len(out) > cap:
        return Read(DST_TOO_SMALL, None, w.consumed, len(w.blocks))
    return Read(len(out), out, w.consumed, len(w.blocks))


# ----------------------------------------------------------------------------- crafted frames
@functools.lru_cache(maxsize=None)
def text(n, seed=41):
    return bytes(dg.text_bytes(n, seed))


def small_blocks(count, seed):
    """`count` compressed blocks of 1..300 decoded bytes each -> (blocks, content)"""
    src = text(300 * 64, 7)
    r = dg.u64_stream(seed, 2 * count)
    blocks, parts = [], []
    for k in range(count):
        n = 1 + int(r[2 * k]) % 300
        o = int(r[2 * k + 1]) % (len(src) - n)
        parts.append(src[o:o + n])
        blocks.append(oracle.compress_fast(parts[-1], 1))
    return blocks, b"".join(parts)


def skippable(payload=b"meta"):
    return le32(SKIP_MAGIC | 3) + le32(len(payload)) + payload


Case = collections.namedtuple("Case", "name buf result consumed")      # result: the content's length or a code


def _good():
    blocks, content = small_blocks(3, 5)
    return build(blocks), content


def endings():
    """every way the walk ends without a defect, and the one with: a word of exactly the bound"""
    f, content = _good()
    n = len(content)
    modern = oracle.compress_frame(b"the next member")
    return [
        Case("end_of_buffer", f, n, len(f)),
        Case("magic_alone", le32(MAGIC), 0, 4),
        Case("modern_frame_follows", f + modern, n, len(f)),
        Case("skippable_frame_follows", f + skippable(), n, len(f)),
        Case("legacy_frame_follows", f + f, n, len(f)),
        Case("magic_alone_then_legacy", le32(MAGIC) + f, 0, 4),
        Case("word_bound_plus_1", f + le32(BLOCK_BOUND + 1) + b"xyz", n, len(f)),
        Case("word_bound_too_few_bytes", f + le32(BLOCK_BOUND) + b"x" * 40, SIZE_WRONG, len(f) + 44),
    ]


def defects():
    blocks, _ = small_blocks(3, 5)
    a, b, c = blocks
    out = []
    for k in (1, 2, 3):
        out.append(Case("stray_%d" % k, build(blocks) + b"\x07" * k, SIZE_WRONG, None))
        out.append(Case("stray_%d_behind_the_magic" % k, le32(MAGIC) + b"\x07" * k, SIZE_WRONG, None))
    out.append(Case("block_runs_off", build([a, b]) + le32(len(c) + 1) + c, SIZE_WRONG, None))
    for name, bad in (("zero_size", b""), ("corrupt_block", CORRUPT)):
        out.append(Case(name + "_first", build([bad, a, b]), FAILED, None))
        out.append(Case(name + "_middle", build([a, bad, b]), FAILED, None))
        out.append(Case(name + "_last", build([a, b, bad]), FAILED, None))
    out.append(Case("corrupt_block_then_torn_tail", build([a, CORRUPT, b]) + b"\x01\x00", FAILED, None))
    out.append(Case("corrupt_block_then_zero_size", build([CORRUPT, a, b""]), FAILED, None))
    out.append(Case("torn_tail_alone", build([a]) + b"\x01\x00\x00", SIZE_WRONG, None))
    for k in range(4):
        out.append(Case("only_%d_bytes" % k, le32(MAGIC)[:k], HEADER_INCOMPLETE, None))
    out.append(Case("modern_magic", oracle.compress_frame(b"abc"), TYPE_UNKNOWN, None))
    out.append(Case("skippable_magic", skippable(), TYPE_UNKNOWN, None))
    out.append(Case("magic_one_bit_off", le32(MAGIC ^ 0x100) + build(blocks)[4:], TYPE_UNKNOWN, None))
    return [x._replace(consumed=len(x.buf)) for x in out]               # every defect of the walk: consumed = n


@functools.lru_cache(maxsize=None)
def table():
    """endings and defects, and frames whose blocks are special"""
    big = zeros_block(BLOCK_SIZE)
    special = [
        Case("token_00_block", build([EMPTY]), 0, 9),
        Case("token_00_between_blocks", build([literal_block(b"ab"), EMPTY, literal_block(b"c")]), 3, None),
        Case("block_of_8mib", build([big]), BLOCK_SIZE, None),
        Case("block_of_8mib_plus_1", build([zeros_block(BLOCK_SIZE + 1)]), FAILED, None),
        Case("block_of_8mib_plus_1_then_torn", build([zeros_block(BLOCK_SIZE + 1)]) + b"\x00", FAILED, None),
        Case("short_blocks_anywhere", build([literal_block(b"x" * 20), big, literal_block(b"y")]), BLOCK_SIZE + 21, None),
    ]
    return endings() + defects() + [x._replace(consumed=len(x.buf)) for x in special]
