"""The workspace sizes of the three HC pipelines as rows of arguments: the grid of tests/golden/hc_workspaces.json, dense
where the chunk rule bends (a chunk is at most 8192 blocks, at most nblocks, about 6 GiB, at least one block), and how one
row is asked of a loaded library.  Pure host arithmetic: no device is touched.

  plain   zlz4_batch_compress_hc_workspace(nblocks, max_in_len)
  dict    zlz4_batch_compress_hc_using_dict_workspace(nblocks, max_in_len, max_dict_len)
  linked  zlz4f_batch_compress_frame_workspace_ex(1 frame, max_blocks = nblocks, block size, level 3 or 9, LINK_BLOCKS):
          the linked launcher's size has no call of its own; this one embeds it"""
import ctypes as C
import itertools

NBLOCKS = (0, 1, 2, 3, 31, 4096, 8191, 8192, 8193, 16900, 100000)
MAX_IN_LEN = (0, 1, 12, 13, 200, 65535, 65536, 65537, 1 << 20, (1 << 24) + 1, 0x7E000000, 0xFFFFFFFF)
MAX_DICT_LEN = (0, 100, 65535, 65536, 65537, 1 << 20)
BLOCK_SIZE_IDS = (4, 5, 6, 7)
LINKED_LEVELS = (3, 9)
LINK_BLOCKS = 4                          # ZLZ4F_BATCH_LINK_BLOCKS

KINDS = ("plain", "dict", "linked")


def rows(kind):
    """every argument tuple of one kind, in a fixed order"""
    if kind == "plain":
        return list(itertools.product(NBLOCKS, MAX_IN_LEN))
    if kind == "dict":
        return list(itertools.product(NBLOCKS, MAX_IN_LEN, MAX_DICT_LEN))
    return list(itertools.product(NBLOCKS, BLOCK_SIZE_IDS, LINKED_LEVELS))


def call(zl, L, kind, row):
    """The size one row gets; `L` is a ctypes library bound like zig_lz4_amd.lib()."""
    if kind == "plain":
        return L.zlz4_batch_compress_hc_workspace(*row)
    if kind == "dict":
        return L.zlz4_batch_compress_hc_using_dict_workspace(*row)
    nblocks, bsid, level = row
    p = zl.Prefs()
    p.block_size_id, p.compression_level = bsid, level
    return L.zlz4f_batch_compress_frame_workspace_ex(1, nblocks, C.byref(p), LINK_BLOCKS)
