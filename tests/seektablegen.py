"""Corpus and batch runners for seek tables (tests/test_seek_table_cpu.py, tests/test_gpu_seek_table.py; DESIGN.md section
4.4l).  Test infrastructure on top of filerangegen (the files and views of the file range tests), lz4filegen (the model of
whole files), legacygen and multiframegen; expectations come from tools/pyref/zig_lz4_seek_table.py and -- for the stated
cases -- from figures written in the tests by hand.

A File is (name, buf): a .lz4 file WITHOUT a table.  A Mutation is (name, bytes, code): a file that ends in a table with one
field changed, and the loader's split result for it, stated here field by field.
"""
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools", "pyref"))
import filerangegen as g  # noqa: E402
import legacygen as lg  # noqa: E402
import multiframegen as mg  # noqa: E402
import zig_lz4_seek_table as st  # noqa: E402

ff, frg = g.ff, g.frg
INVALID_STATE, UNSUPPORTED, DST_TOO_SMALL = -5, -8, -111
SLICE = 256                                            # rows (load) or 8-byte words (append) of one slice of a table


# ----------------------------------------------------------------------------- files
@functools.lru_cache(maxsize=None)
def cpu_files():
    """the files of the file range tests -> [(name, buf)]"""
    out = [(v.name, v.buf) for v in g.tiny_views() + g.range_views() + g.lane_edge_views() if v.name != "tiny_not_legacy"]
    out += [("ordering_%d" % (997 * k), buf) for k, buf in enumerate(g.orderings()[::997])]
    return out


@functools.lru_cache(maxsize=None)
def refused_files():
    """files the append refuses -> [(name, buf, code)], the code stated by hand: each kind of last member that cannot be
    delimited, and members that are not OK"""
    tiny = {v.name: v for v in g.tiny_views()}
    tf = tiny["tiny_one_frame"].buf                    # 46 bytes, the end mark at 42
    tl = lg.build([lg.literal_block(b"abcdef"), lg.EMPTY, lg.literal_block(b"ghi")])
    sk = g.members()["SK"]
    return [("chain_without_end_mark", tf[:42], INVALID_STATE),          # ends on a block boundary: the index is fine
            ("chain_without_end_mark_after_members", sk + tl + tf[:42], INVALID_STATE),
            ("skippable_cut_in_header", tf + sk[:6], lg.HEADER_INCOMPLETE),
            ("skippable_cut_in_payload", tf + sk[:-1], lg.SIZE_WRONG),
            ("legacy_torn_size_word", tl + b"\x07", lg.SIZE_WRONG),
            ("legacy_corrupt_block", lg.build([lg.CORRUPT]) + tf, lg.FAILED),
            ("frame_cut_in_block", tf[:30], lg.SIZE_WRONG),
            ("linked_member_with_history", frg.linked_views()[0].frame, g.FAILED)]


def _tiny_blocks(count, seed=0):
    return [lg.literal_block(g.pat(1 + (k + seed) % 5, 100 + k + seed)) for k in range(count)]


@functools.lru_cache(maxsize=None)
def shape_files():
    """the smallest shapes at which the kernels can go wrong -> [(name, buf)]: entry counts nb + 1 and member counts nm at
    the 64-lane edges, tables of SLICE - 1, SLICE and SLICE + 1 rows and of more rows than all slices of one pass hold,
    and every alignment of the table"""
    m = g.members()
    out = []
    for rows in (1, 2, 63, 64, 65, 128, 129):                          # nb + 1
        nb = rows - 1
        out.append(("legacy_%d_entries" % rows, lg.build(_tiny_blocks(nb)) if nb else g.MAGIC))
        out.append(("frame_%d_entries" % rows, g.build([(g.seq(g.pat(1 + k % 5, 300 + k)), False) for k in range(nb)], block_mode=1)))
    for nm in (1, 2, 64, 65, 66):                                      # the table's own row is one of them
        k = nm - 1
        out.append(("%d_empty_frames" % k, m["FE"] * k))
        out.append(("%d_skippables" % k, b"".join(mg.skippable(j % 16, b"x" * (j % 7)) for j in range(k))))
        out.append(("%d_legacy_frames" % k, b"".join(lg.build(lg.small_blocks(2, 11 + j)[0]) for j in range(k))))
    for total in (SLICE - 1, SLICE, SLICE + 1):                        # rows = nm + nb + 1 = 2 + nb + 1
        out.append(("legacy_%d_rows" % total, lg.build(_tiny_blocks(total - 3, 3))))
    # the append slices 8-byte words: T / 8 = 5 + 3 nm + 2 (nb + 1) = SLICE - 1, SLICE, SLICE + 1
    words = [("legacy_%d_words" % (SLICE - 1), lg.build(_tiny_blocks(121, 4))), ("legacy_%d_words" % (SLICE + 1), lg.build(_tiny_blocks(122, 5))),
             ("skippable_legacy_%d_words" % SLICE, m["SK"] + lg.build(_tiny_blocks(120, 6)))]
    assert [st.bound(len(ff.split(b)), ff.file_index(b)[0]) // 8 for _, b in words] == [SLICE - 1, SLICE + 1, SLICE]
    out += words
    out.append(("legacy_3000_blocks", lg.build(_tiny_blocks(3000, 1))))
    out.append(("1500_empty_frames_then_legacy", m["FE"] * 1500 + lg.build(_tiny_blocks(700, 2))))
    tf = g.tiny_views()[5].buf
    for pad in range(16):                                              # 26 + pad + 46 bytes: every residue mod 16
        out.append(("aligned_%d" % pad, mg.skippable(pad, b"p" * pad) + m["SK"] + tf))
    assert sorted(len(b) % 16 for n, b in out if n.startswith("aligned_")) == list(range(16))
    return out


# ----------------------------------------------------------------------------- mutations
@functools.lru_cache(maxsize=None)
def mutation_base():
    """F SK L3 FC: four members and the table's row, seven blocks -> (file, rows, entries, T, n)"""
    F = g.join("F", "SK", "L3", "FC")
    tab = st.table(F)
    idx_n, entries = ff.file_index(F)
    rows = st.members(F) + [(len(F), len(tab), st.SELF_KIND)]
    assert (len(rows), idx_n, len(tab)) == (5, 7, 40 + 24 * 5 + 16 * 8)
    return F, rows, entries, len(tab), len(F) + len(tab)


def _row(rows, k, pos=None, ln=None, kind=None):
    out = list(rows)
    p, l, kd = out[k]
    out[k] = (p if pos is None else pos, l if ln is None else ln, kd if kind is None else kind)
    return out


def _ent(entries, k, pos=None, dec=None):
    out = list(entries)
    p, d = out[k]
    out[k] = (p if pos is None else pos, d if dec is None else dec)
    return out


@functools.lru_cache(maxsize=None)
def mutations():
    """every single-field mutation of the valid table of mutation_base() -> [(name, file, split result)].  The code is
    stated here: InvalidState for a table out of shape, 0 where the tail magic is gone."""
    F, R, E, T, n = mutation_base()
    BAD = INVALID_STATE
    P = lambda rows=R, entries=E, **kw: F + st.pack(rows, entries, n, **kw)       # noqa: E731
    good = P()
    assert good == F + st.table(F)
    out = [("valid", good, 5)]
    # the footer, field by field
    out += [("version_0", P(version=0), BAD), ("version_2", P(version=2), BAD),
            ("nm_plus_1", P(nm=6), BAD), ("nm_minus_1", P(nm=4), BAD), ("nm_0", P(nm=0), BAD),
            ("nm_overflows", P(nm=1 << 61), BAD), ("nm_huge", P(nm=(1 << 64) - 1), BAD),
            ("nb_plus_1", P(nb=8), BAD), ("nb_minus_1", P(nb=6), BAD), ("nb_overflows", P(nb=1 << 60), BAD),
            ("file_len_plus_1", F + st.pack(R, E, n + 1), BAD), ("file_len_minus_1", F + st.pack(R, E, n - 1), BAD),
            ("file_len_0", F + st.pack(R, E, 0), BAD),
            ("footer_magic", P(footer_magic=st.FOOTER_MAGIC ^ 1), 0), ("footer_magic_swapped", P(footer_magic=st.MAGIC), 0),
            ("magic_other_nibble", P(magic=st.MAGIC ^ 1), BAD), ("magic_frame", P(magic=0x184D2204), BAD),
            ("payload_plus_1", P(payload=T - 7), BAD), ("payload_minus_1", P(payload=T - 9), BAD), ("payload_T", P(payload=T), BAD)]
    # T larger than the file; the table alone, with the rows of the file that is gone
    out += [("T_exceeds_n", P(nb=1 << 20), BAD), ("table_without_its_file", st.pack(R, E, T), BAD)]
    # member rows, each field and each neighbour relation
    out += [("pos0_not_0", P(_row(R, 0, pos=1)), BAD),
            ("len1_0", P(_row(R, 1, ln=0)), BAD), ("len0_0", P(_row(R, 0, ln=0)), BAD),
            ("len1_plus_1", P(_row(R, 1, ln=R[1][1] + 1)), BAD), ("len1_minus_1", P(_row(R, 1, ln=R[1][1] - 1)), BAD),
            ("pos2_plus_1", P(_row(R, 2, pos=R[2][0] + 1)), BAD), ("pos2_minus_1", P(_row(R, 2, pos=R[2][0] - 1)), BAD),
            # pos[1] + len[1] wraps around 2^64 onto pos[2] (rows 0 and 1 agree with each other)
            ("pos_len_wraps", P(_row(_row(R, 0, ln=(1 << 64) - 10), 1, pos=(1 << 64) - 10, ln=10 + R[2][0])), BAD),
            ("last_pos_plus_1", P(_row(R, 4, pos=R[4][0] + 1)), BAD), ("last_pos_minus_1", P(_row(R, 4, pos=R[4][0] - 1)), BAD),
            ("last_len_plus_1", P(_row(R, 4, ln=T + 1)), BAD), ("last_len_minus_1", P(_row(R, 4, ln=T - 1)), BAD),
            ("last_len_0", P(_row(R, 4, ln=0)), BAD),
            ("last_kind_nibble", P(_row(R, 4, kind=ff.SKIPPABLE | 0xB << 8)), BAD),
            ("last_kind_no_nibble", P(_row(R, 4, kind=ff.SKIPPABLE)), BAD),
            ("last_kind_frame", P(_row(R, 4, kind=ff.FRAME)), BAD),
            ("last_kind_high_bit", P(_row(R, 4, kind=st.SELF_KIND | 0x1000)), BAD),
            ("kind1_truncated", P(_row(R, 1, kind=ff.SKIPPABLE_TRUNCATED | 5 << 8)), BAD),
            ("kind0_0", P(_row(R, 0, kind=0)), BAD), ("kind2_5", P(_row(R, 2, kind=5)), BAD),
            ("kind2_bit_12", P(_row(R, 2, kind=ff.LEGACY | 0x1000)), BAD), ("kind3_bit_31", P(_row(R, 3, kind=ff.FRAME | 1 << 31)), BAD),
            ("kind0_nibble_on_frame", P(_row(R, 0, kind=ff.FRAME | 7 << 8)), 5),           # (shape only: bits inside 0xFFF)
            ("reserved0", P(reserved={0: 1}), BAD), ("reserved3", P(reserved={3: 1 << 31}), BAD), ("reserved_last", P(reserved={4: 7}), BAD)]
    # entries, each field and each neighbour relation
    out += [("entry_pos3_is_pos2", P(entries=_ent(E, 3, pos=E[2][0])), BAD),
            ("entry_pos3_below_pos2", P(entries=_ent(E, 3, pos=E[2][0] - 1)), BAD),
            ("entry_pos0_is_pos1", P(entries=_ent(E, 0, pos=E[1][0])), BAD),
            ("entry_last_pos_is_previous", P(entries=_ent(E, 7, pos=E[6][0])), BAD),
            ("entry_dec4_below_dec3", P(entries=_ent(E, 4, dec=E[3][1] - 1)), BAD),
            ("entry_last_dec_below", P(entries=_ent(E, 7, dec=E[6][1] - 1)), BAD),
            ("entry_dec4_is_dec3", P(entries=_ent(E, 4, dec=E[3][1])), 5),                 # (an empty block is well shaped)
            ("entry_last_pos_behind_table", P(entries=_ent(E, 7, pos=len(F) + 1)), BAD),
            ("entry_last_pos_at_table", P(entries=_ent(E, 7, pos=len(F))), 5),
            ("entry_last_pos_huge", P(entries=_ent(E, 7, pos=(1 << 64) - 1)), BAD),
            ("entry_pos_moved_in_bound", P(entries=_ent(E, 3, pos=E[3][0] + 1)), 5)]       # (not this file's: the range call judges)
    # one byte less, one byte more: in front of the footer, so the tail magic stands and the table is malformed; at the
    # very end the tail magic itself is gone and the file has no table
    out += [("cut_one_byte", good[:n - 33] + good[n - 32:], BAD), ("cut_first_byte", F + good[len(F) + 1:], BAD),
            ("one_byte_added", good[:n - 32] + b"\0" + good[n - 32:], BAD), ("one_byte_added_in_front", F + b"\0" + good[len(F):], BAD),
            ("cut_at_the_end", good[:-1], 0), ("one_byte_added_at_the_end", good + b"\0", 0),
            ("short_79", good[-79:], 0), ("footer_alone_80", b"\0" * 48 + good[-32:], BAD)]
    return out


# ----------------------------------------------------------------------------- the GPU side
def _t(torch, v, dev):
    return torch.tensor(v, dtype=torch.int64, device=dev)


CANARY = 0xA5


def run_append(zl, files, dev, legacy=True, cap_delta=None, pad=0):
    """one zlz4f_batch_append_seek_table call over fileIndex of `files`, every buffer in a slot of its own between canary
    bytes, `pad` bytes in front of the first so the tables start at other addresses -> [(result, the slot's bytes up to
    max(result, n))]; asserts that no byte outside [n, n + T) changed.  cap_delta: {file: delta} on the capacity n + T."""
    import numpy as np
    import torch
    ix = zl.lz4f.fileIndex(files, device=dev, legacy=legacy)
    want = [st.table(f, legacy) for f in files]
    room = [len(f) + (len(w) if not isinstance(w, int) else 80) for f, w in zip(files, want)]
    caps = [r + (cap_delta or {}).get(s, 0) for s, r in enumerate(room)]
    offs, pos = [], 32 + pad
    for r in room:
        offs.append(pos)
        pos += r + 40
    host = bytearray([CANARY]) * pos
    for f, o in zip(files, offs):
        host[o:o + len(f)] = f
    d_buf = torch.from_numpy(np.frombuffer(bytes(host), dtype=np.uint8).copy()).to(dev)
    result = torch.full((len(files),), -999, dtype=torch.int64, device=dev)
    sp = ix.split
    zl.lz4f.appendSeekTableBatch(d_buf, _t(torch, offs, dev), sp.src_len, _t(torch, caps, dev), sp.member, sp.mem_off, sp.result,
                                 ix.index, ix.idx_off, ix.idx_n, result)
    torch.cuda.synchronize()
    got = bytes(d_buf.cpu().numpy().tobytes())
    res = result.cpu().tolist()
    out, at = [], 0
    for s, (f, o, r) in enumerate(zip(files, offs, res)):
        end = o + (r if r >= 0 else len(f))
        assert got[at:o] == bytes(host[at:o]), "file %d: bytes in front of the buffer changed" % s
        assert got[o:o + len(f)] == f, "file %d: bytes [0, n) changed" % s
        out.append((r, got[o:end]))
        at = end
    assert got[at:] == bytes(host[at:]), "bytes behind the last table changed"
    return out


def run_load(zl, files, dev, mem_short=(), idx_short=None):
    """count mode and record mode of zlz4f_batch_load_seek_table over `files`, the member and index arrays filled with a
    canary and every file's member rows followed by one spare row -> (counts, totals, [(split_result, rows, idx_n,
    entries)], idx_off).  mem_short: files whose d_mem_cap is one short; idx_short: idx_cap is short by that much.  Asserts
    that no row outside the rows of the files that loaded changed."""
    import torch
    lz = zl.lz4f
    nbuf = len(files)
    d_src, src_off, src_len = zl._stage(files, dev)
    count = torch.full((nbuf,), -999, dtype=torch.int64, device=dev)
    totals = torch.full((2,), -999, dtype=torch.int64, device=dev)
    lz.loadSeekTableBatch(d_src, src_off, src_len, count, totals)
    counts, tot = count.cpu().tolist(), totals.cpu().tolist()
    mem_off, pos = [], 1
    for c in counts:
        mem_off.append(pos)
        pos += c + 1
    member = torch.full((pos + 1, 3), -2, dtype=torch.int64, device=dev)
    idx_cap = tot[1] - (idx_short or 0)
    index = torch.full((tot[1] + 2, 2), -3, dtype=torch.int64, device=dev)
    idx_off = torch.full((nbuf + 1,), -999, dtype=torch.int64, device=dev)
    split_result = torch.full((nbuf,), -999, dtype=torch.int64, device=dev)
    idx_n = torch.full((nbuf,), -999, dtype=torch.int64, device=dev)
    mem_cap = [c - (1 if s in mem_short else 0) for s, c in enumerate(counts)]
    before = d_src.clone()
    lz.loadSeekTableBatch(d_src, src_off, src_len, count, totals, member, _t(torch, mem_off, dev), _t(torch, mem_cap, dev),
                          split_result, index, idx_off, idx_n, idx_cap)
    torch.cuda.synchronize()
    assert torch.equal(d_src, before), "the source arena changed"
    assert count.cpu().tolist() == counts and totals.cpu().tolist() == tot
    rows, ents = member.cpu().tolist(), index.cpu().tolist()
    sr, ns, io = split_result.cpu().tolist(), idx_n.cpu().tolist(), idx_off.cpu().tolist()
    out = []
    mem_used, idx_used = set(), set()
    for s in range(nbuf):
        if sr[s] > 0:
            r = [(p, l, kb & 0xFFFFFFFF) for p, l, kb in rows[mem_off[s]:mem_off[s] + sr[s]]]
            assert all(kb >> 32 == s for _, _, kb in rows[mem_off[s]:mem_off[s] + sr[s]]), "file %d: buf is not the file" % s
            out.append((sr[s], r, ns[s], [tuple(e) for e in ents[io[s]:io[s] + ns[s] + 1]]))
        else:
            out.append((sr[s], [], ns[s], []))
        if sr[s] > 0 or sr[s] == INVALID_STATE:                        # (the rows of a malformed table are not promised)
            mem_used |= set(range(mem_off[s], mem_off[s] + counts[s]))
            idx_used |= set(range(io[s], io[s + 1]))
    assert all(rows[k] == [-2, -2, -2] for k in range(len(rows)) if k not in mem_used), "a member row outside the tables changed"
    assert all(ents[k] == [-3, -3] for k in range(len(ents)) if k not in idx_used), "an index row outside the tables changed"
    return counts, tot, out, io


def check_loaded(files, loaded):
    """the loaded tables against the model's load, file by file"""
    bad = []
    for s, (f, got) in enumerate(zip(files, loaded)):
        want = st.load(f)
        if tuple(got) != (want[0], [tuple(r) for r in want[1]], want[2], [tuple(e) for e in want[3]]):
            bad.append("file %d: GPU (%d, %d) vs model (%d, %d)" % (s, got[0], got[2], want[0], want[2]))
    assert not bad, "%d of %d loads differ:\n%s" % (len(bad), len(files), "\n".join(bad[:10]))
