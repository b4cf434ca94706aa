"""Inputs of the decompressed-size tests (tests/test_decompressed_size_cpu.py, tests/test_gpu_decompressed_size.py):
compressed blocks, dictionary records and frames, whole and damaged (test infrastructure).

Every block stream here allows an oracle destination of oracle_cap(stream) = 255 x len + 64 bytes: an LZ4 block cannot
decode to more (one extension byte adds at most 255 output bytes), so that capacity behaves like the query's 0xFFFFFFFF.
The 1 MiB inputs are the compressible ones (text, zeros): their streams keep that buffer at ~150 MB.
"""
import numpy as np

import cases
import datagen as dg
import dictgen
import seqgen

SIZES = (0, 1, 12, 13, 4096, 65536, 70000)
LEVELS = (2, 9, 12)


def oracle_cap(src):
    return 255 * len(src) + 64


def _damaged(c, rng):
    """truncated and corrupted variants of a stream"""
    out = []
    if len(c) > 1:
        out += [c[:len(c) // 2], c[:-1], c[:int(rng.integers(1, len(c)))]]
    if c:
        for _ in range(2):
            m = bytearray(c)
            m[int(rng.integers(0, len(m)))] ^= 1 << int(rng.integers(0, 8))
            out.append(bytes(m))
        m = bytearray(c)
        m[int(rng.integers(0, len(m)))] = 0xFF
        out.append(bytes(m))
    return out


def plain_inputs():
    """(name, bytes): the named cases, the seeded boundary cases up to 4 KiB, every distribution at SIZES, 1 MiB text/zero"""
    out = list(cases.reference_test_inputs())
    out += cases.seeded_cases(max_size=4097)
    for dist in dg.GENERATORS:
        for n in SIZES:
            out.append(("%s/%d" % (dist, n), bytes(dg.GENERATORS[dist](n, 31 + n))))
    out.append(("text/1MiB", bytes(dg.text_bytes(1 << 20, 5))))
    out.append(("zero/1MiB", b"\0" * (1 << 20)))
    return out


def block_streams(oracle, damaged=True):
    """-> [(name, stream, plain or None)]: every input compressed with acceleration 1 and levels 2, 9, 12 (plain None for
    level 12: lz4opt streams do not always decode back, include/zlz4_amd.h), the crafted sequence streams of seqgen, and
    damaged variants of every third stream"""
    rng = np.random.default_rng(77)
    out = []
    for name, b in plain_inputs():
        out.append((name + "/a1", oracle.compress_fast(b, 1), b))
        for lvl in LEVELS:
            out.append(("%s/hc%d" % (name, lvl), oracle.compress_hc(b, lvl), b if lvl < 10 else None))
    seen = set()
    for it in seqgen.corpus(scale=0.5):
        if it.src not in seen:
            seen.add(it.src)
            out.append(("seq/" + it.name, it.src, it.plain))
    if damaged:
        base = list(out)
        for k in range(0, len(base), 3):
            name, c, _ = base[k]
            if len(c) <= 70000:
                out += [(name + "/dmg%d" % j, v, None) for j, v in enumerate(_damaged(c, rng))]
    return out


def dict_records(tmpdir):
    """-> [(name, stream, dict bytes)]: blocks whose matches reach into their dictionary -- the encoder of
    tests/dict_encoder.c on text, the crafted cases of dictgen and the dictionary families of seqgen"""
    enc = dictgen.encoder(tmpdir)
    text = bytes(dg.text_bytes(500000, 77))
    out = []
    for k in range(8):
        dct, blk = text[:65536], text[70000 + 4096 * k: 70000 + 4096 * (k + 1)]
        out.append(("enc4k/%d" % k, enc(dct, blk)[0], dct))
    out.append(("enc64k", enc(text[:200000], text[200000:265536])[0], text[:200000]))
    out.append(("enc70000", enc(text[300000:310000], text[310000:380000])[0], text[300000:310000]))
    out.append(("enc_small", enc(b"abc", b"abcabcabcabcabcabcabcabc0123456789")[0], b"abc"))
    out.append(("enc_nodict", enc(b"", text[:5000])[0], b""))
    for name, s, dct, cap, target in dictgen.crafted_cases():
        if target is None:
            out.append(("crafted/" + name, s, dct))
    seen = set()
    for it in seqgen.dict_corpus(count=150):
        if it.src not in seen:
            seen.add(it.src)
            out.append(("seqdict/" + it.name, it.src, it.dict_bytes))
    return out


def edge_block(total, end_inside=False):
    """A block built arithmetically that decodes to `total` bytes (15 + 4 + 1 < total): token 0x1F, one literal, offset 1,
    k bytes 0xFF and one final byte (src/lz4.zig:160-171: match length 15 + 255 k + f + 4).  end_inside: the stream ends
    inside the run of 0xFF (CorruptedData, :162)."""
    ml = total - 1 - 4 - 15
    k, f = divmod(ml, 255)
    head = bytes([0x1F, 0x41, 0x01, 0x00])
    if end_inside:
        return head + b"\xff" * k
    return head + b"\xff" * k + bytes([f])


def frame_corpus(oracle):
    """-> [(name, frame, content or None)]: compressFrame over the preference matrix of the frame tests (all four block
    sizes, both checksums, stored blocks, an empty frame), their hand-built foreign frames with short, empty and stored
    blocks, and the header / chain damage their _variants() makes (content None: judged by the oracle)"""
    import test_gpu_frame_batch as fb                 # generators only; nothing there runs on import
    rng = np.random.default_rng(99)
    ins = [b"", b"A", bytes(dg.text_bytes(13, 1)), bytes(dg.text_bytes(4096, 2)), bytes(dg.text_bytes(65537, 7)),
           bytes(dg.random_bytes(70000, 4)), bytes(dg.mixed_bytes(300001, 5)), bytes(dg.zero_bytes(70000))]
    base = []
    for kw in fb._pref_matrix():
        for b in ins:
            if len(b) > 100000 and kw.get("compression_level", 0) >= 10:
                continue
            readable = kw.get("compression_level", 0) < 10
            base.append((b if readable else None, oracle.compress_frame(b, fb._prefs(oracle.Prefs, **kw))))
    base += fb._hand_frames(oracle)
    out = []
    for k, (b, f) in enumerate(base):
        out.append(("frame%d" % k, f, b))
        if k % 4 == 0 or k >= len(base) - 9:
            out += [("frame%d/v%d" % (k, j), v, None) for j, v in enumerate(fb._variants(f, rng))]
    out.append(("skippable", bytes([0x50, 0x2A, 0x4D, 0x18, 4, 0, 0, 0]) + b"skip", None))
    return out
