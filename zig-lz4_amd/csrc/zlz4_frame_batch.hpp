// zlz4_frame_batch.hpp -- what the lz4f kernels and host calls share: the per-frame record and the block flags of the batch
// frame calls, XXH32, the frame header parse, and the block chain: the
// decode of a block word and the one step of the chain walk that every walker is written on, the regions a call carves
// out of its workspace, the walk of a legacy frame (section 4.4i) and the delimiter of a multiframe's members (sections
// 4.4h, 4.4j).  Included by zlz4_frame.hip (the pipelines), zlz4_frame_linked.hip (the linked-block kernels of
// section 4.4c, the frame prefix decoder of section 4.4f), zlz4_frame_multi.hip (the multiframe split of section 4.4h) and
// zlz4_frame_legacy.hip (the legacy frame calls of section 4.4i).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/zlz4_amd.h"

namespace {

constexpr uint32_t kNoFrame = 0xFFFFFFFFu;
constexpr uint32_t kBlkStored = 1u, kBlkNoCks = 2u, kBlkCks = 4u;   // block flags (decompress table)

struct BFrame {
    uint64_t nb;        // block count: ceil(len / bs) (compress), what the block chain holds (decompress)
    uint64_t base;      // first table entry (exclusive scan of nb)
    int64_t status;     // compress: 0, DstMaxSizeTooSmall or SrcSizeTooLarge; decompress: header size or header error
    uint64_t end;       // compress: frame bytes in front of the end mark; decompress: srcPos after the walk
    int64_t err;        // compress: first failing block's code; decompress: the walk's error, then the plan's
    uint64_t total;     // decompress: decoded bytes
    uint64_t bs;        // decompress: block size from BD
    uint32_t flg;       // decompress: FLG
    uint32_t proven;    // decompress: 1 = the speculative layout is proven
};

// ------------------------------------------------------------------ XXH32 (host + device)
#define ZX_P1 2654435761u
#define ZX_P2 2246822519u
#define ZX_P3 3266489917u
#define ZX_P4 668265263u
#define ZX_P5 374761393u

__host__ __device__ inline uint32_t zx_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__host__ __device__ inline uint32_t zx_rd32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__host__ __device__ inline uint32_t zx_round(uint32_t acc, uint32_t in) { return zx_rotl(acc + in * ZX_P2, 13) * ZX_P1; }

__host__ __device__ inline uint32_t xxh32(const uint8_t *p, uint64_t len, uint32_t seed) {
    const uint8_t *const end = p + len;
    uint32_t h;
    if (len >= 16) {
        uint32_t v1 = seed + ZX_P1 + ZX_P2, v2 = seed + ZX_P2, v3 = seed, v4 = seed - ZX_P1;
        const uint8_t *const limit = end - 16;
        do {
            v1 = zx_round(v1, zx_rd32(p)); v2 = zx_round(v2, zx_rd32(p + 4));
            v3 = zx_round(v3, zx_rd32(p + 8)); v4 = zx_round(v4, zx_rd32(p + 12));
            p += 16;
        } while (p <= limit);
        h = zx_rotl(v1, 1) + zx_rotl(v2, 7) + zx_rotl(v3, 12) + zx_rotl(v4, 18);
    } else {
        h = seed + ZX_P5;
    }
    h += (uint32_t)len;
    while (p + 4 <= end) { h = zx_rotl(h + zx_rd32(p) * ZX_P3, 17) * ZX_P4; p += 4; }
    while (p < end) { h = zx_rotl(h + (*p) * ZX_P5, 11) * ZX_P1; p += 1; }
    h ^= h >> 15; h *= ZX_P2; h ^= h >> 13; h *= ZX_P3; h ^= h >> 16;
    return h;
}

// ------------------------------------------------------------------ frame header
struct ParsedHeader { int64_t size; uint8_t flg; size_t block_size; };

// parseFrameHeader, src/lz4f.zig:483-538 (decodeFLG :187-221, decodeBD :235-249); `have` = bytes available
__host__ __device__ inline ParsedHeader parse_header(const uint8_t *src, size_t have) {
    ParsedHeader r = {0, 0, 0};
    if (have < 7) { r.size = ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE; return r; }
    const uint32_t magic = zx_rd32(src);
    if (magic != ZLZ4F_MAGICNUMBER) { r.size = ZLZ4F_ERR_FRAME_TYPE_UNKNOWN; return r; }
    size_t pos = 4;
    const uint8_t flg = src[pos];
    if (((flg >> 6) & 3) != 1) { r.size = ZLZ4F_ERR_HEADER_VERSION_WRONG; return r; }
    if (flg & 0x02) { r.size = ZLZ4F_ERR_RESERVED_FLAG_SET; return r; }
    pos += 1;
    const uint8_t bd = src[pos];
    if (bd & 0x8F) { r.size = ZLZ4F_ERR_RESERVED_FLAG_SET; return r; }
    switch ((bd >> 4) & 7) {
        case 0: case 4: r.block_size = 64u * 1024; break;
        case 5: r.block_size = 256u * 1024; break;
        case 6: r.block_size = 1024u * 1024; break;
        case 7: r.block_size = 4u * 1024 * 1024; break;
        default: r.size = ZLZ4F_ERR_MAX_BLOCK_SIZE_INVALID; return r;
    }
    pos += 1;
    if (flg & 0x08) { if (have < pos + 8) { r.size = ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE; return r; } pos += 8; }
    if (flg & 0x01) { if (have < pos + 4) { r.size = ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE; return r; } pos += 4; }
    if (have < pos + 1) { r.size = ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE; return r; }
    if (src[pos] != (uint8_t)((xxh32(src + 4, pos - 4, 0) >> 8) & 0xFF)) { r.size = ZLZ4F_ERR_HEADER_CHECKSUM_INVALID; return r; }
    pos += 1;
    r.size = (int64_t)pos;
    r.flg = flg;
    return r;
}

// the header of the frame at s, n bytes available: staged so that parse_header reads no global byte twice
__host__ __device__ __forceinline__ ParsedHeader frame_header(const uint8_t *__restrict__ s, uint64_t n) {
    uint8_t head[19];
    const uint32_t have = n < sizeof head ? (uint32_t)n : (uint32_t)sizeof head;
    for (uint32_t k = 0; k < have; k++) head[k] = s[k];
    return parse_header(head, have);
}

// ------------------------------------------------------------------ block chain (src/lz4f.zig:563-600)
// A block word: 0 is the end mark, bit 31 means stored, the low 31 bits are the payload size (:573, :578-579).
struct BlockWord { uint32_t size; bool stored, end_mark; };
__host__ __device__ __forceinline__ BlockWord block_word(uint32_t h) { return {h & 0x7FFFFFFFu, (h >> 31) != 0, h == 0}; }

// What a step finds: a block (the first two) or how the walk ends without one.
enum ChainEnd : uint32_t {
    kChainBlock,        // a block; the cursor stands behind it and behind its checksum word when the frame has them
    kChainCksCut,       // :591 a block whose checksum word is cut (kBlkNoCks): the cursor stands behind the payload, the walk
                        // ends after this block, and decoding it is FrameSizeWrong
    kChainBoundary,     // :563 the input ends at a block boundary; the cursor has not moved
    kChainWordCut,      // :565 the input ends inside a block word; the cursor has not moved
    kChainEndMark,      // :573 the cursor stands behind the mark
    kChainDataCut,      // :582 the input ends inside the payload; the cursor stands behind the block word
};
struct ChainBlock {
    uint64_t off;       // payload offset
    uint64_t cks_off;   // 0 without a checksum word
    uint32_t size;      // payload bytes
    uint32_t flags;     // kBlkStored; with block checksums kBlkCks (the word is at cks_off) or kBlkNoCks
};
struct Rd32 { __host__ __device__ __forceinline__ uint32_t operator()(const uint8_t *p) const { return zx_rd32(p); } };

// One step of the chain of the n bytes at s from the cursor `pos` on; bc = the frame has block checksums; rd reads a
// 32-bit word (the prefix decoder's is wave-uniform).  b is written only when a block is found.
template <class Rd = Rd32>
__host__ __device__ __forceinline__ ChainEnd chain_step(const uint8_t *s, uint64_t n, bool bc, uint64_t &pos, ChainBlock &b,
                                                        Rd rd = Rd()) {
    if (pos >= n) return kChainBoundary;                              // :563
    if (pos + 4 > n) return kChainWordCut;                            // :565
    const BlockWord w = block_word(rd(s + pos));
    pos += 4;
    if (w.end_mark) return kChainEndMark;                             // :573
    if (pos + w.size > n) return kChainDataCut;                       // :582
    b.off = pos; b.cks_off = 0; b.size = w.size; b.flags = w.stored ? kBlkStored : 0u;
    pos += w.size;
    if (bc) {                                                         // :590
        if (pos + 4 > n) { b.flags |= kBlkNoCks; return kChainCksCut; }             // :591
        b.cks_off = pos; pos += 4; b.flags |= kBlkCks;
    }
    return kChainBlock;
}

// the walk's own error: the two places where the input ends inside a block (:565, :582)
__host__ __device__ __forceinline__ int64_t chain_error(ChainEnd e) {
    return e == kChainWordCut || e == kChainDataCut ? (int64_t)ZLZ4F_ERR_FRAME_SIZE_WRONG : 0;
}

// The walk: each(k, block) for block k = 0, 1, .. of at most nb_max (~0: no bound) -> how it ended (kChainBlock: at
// nb_max); nb = the blocks found, pos = the cursor after the walk.
template <class Each>
__host__ __device__ __forceinline__ ChainEnd chain_walk(const uint8_t *s, uint64_t n, bool bc, uint64_t &pos, uint64_t nb_max,
                                                        uint64_t &nb, Each each) {
    for (nb = 0; nb_max == ~0ull || nb < nb_max;) {
        ChainBlock b;
        const ChainEnd e = chain_step(s, n, bc, pos, b);
        if (e > kChainCksCut) return e;
        each(nb++, b);
        if (e == kChainCksCut) return e;
    }
    return kChainBlock;
}

// blocks the chain of a frame holds from its parsed header on: the count of the device walks, for the host calls that size
// a block table before the device fills it
inline uint64_t chain_blocks(const uint8_t *s, uint64_t n, const ParsedHeader &ph) {
    uint64_t pos = (uint64_t)ph.size, nb;
    chain_walk(s, n, (ph.flg & 0x10u) != 0, pos, ~0ull, nb, [](uint64_t, const ChainBlock &) {});
    return nb;
}

// ------------------------------------------------------------------ workspace layout
// A region of the caller's workspace: a typed pointer and `bytes`, the room it holds up to the next region.  A layout
// function carves its regions in the order the workspace holds them, each rounded up to 256 bytes, and is the only place
// that knows that order; the _workspace functions and the call itself both go through it.  A region the call's branch does
// not have is never carved and stays null.
template <typename T> struct Region {
    T *p = nullptr;
    size_t bytes = 0;
    operator T *() const { return p; }
};

struct Carver {
    uint8_t *ws;           // null: the _workspace functions, which want the total alone
    size_t bytes = 0;
    template <typename T> void one(size_t count, Region<T> &r) {
        const size_t off = bytes;
        bytes = (off + count * sizeof(T) + 255) & ~(size_t)255;
        r.p = ws ? reinterpret_cast<T *>(ws + off) : nullptr;
        r.bytes = bytes - off;
    }
    template <typename... R> void take(size_t count, R &...r) { (one(count, r), ...); }   // `count` elements each
};

// ------------------------------------------------------------------ legacy frames
// The walk of a legacy frame (what `lz4 -l` writes; include/zlz4_amd.h): the magic, then { u32 LE size, block } up to the
// end of the n bytes at s or up to a size word above ZLZ4F_LEGACY_BLOCK_BOUND, which is the next member of a concatenated
// file (every lz4 magic is such a word).  each(k, off, size) for block k = 0, 1, .. of at most nb_max (~0: no bound) -> the
// walk's own verdict: 0, the header error of bytes that are no legacy frame, FrameSizeWrong for a torn size word or a block
// that runs off the input, DecompressionFailed for a size word of 0 (the block decoders answer 0 for an empty block; liblz4
// fails it).  A defect ends the walk, so it stands behind all nb blocks in stream order.  consumed = where the frame ends:
// n, or the position of the foreign word.
template <class Each>
__host__ __device__ __forceinline__ int64_t legacy_walk(const uint8_t *s, uint64_t n, uint64_t nb_max, uint64_t &nb,
                                                        uint64_t &consumed, Each each) {
    nb = 0;
    consumed = n;
    if (n < 4) return ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE;
    if (zx_rd32(s) != ZLZ4F_LEGACY_MAGICNUMBER) return ZLZ4F_ERR_FRAME_TYPE_UNKNOWN;
    uint64_t pos = 4;
    while (nb_max == ~0ull || nb < nb_max) {
        if (pos == n) return 0;
        if (n - pos < 4) return ZLZ4F_ERR_FRAME_SIZE_WRONG;
        const uint32_t w = zx_rd32(s + pos);
        if (w > ZLZ4F_LEGACY_BLOCK_BOUND) { consumed = pos; return 0; }
        if (w == 0) return ZLZ4F_ERR_DECOMPRESSION_FAILED;
        if (w > n - pos - 4) return ZLZ4F_ERR_FRAME_SIZE_WRONG;
        each(nb++, pos + 4, w);
        pos += 4ull + w;
    }
    return 0;
}

// ------------------------------------------------------------------ multiframe members (DESIGN.md sections 4.4h, 4.4j)
struct MfMember { uint64_t len; uint64_t nb; uint32_t kind; bool last; };

// The member that starts at s[0] of the n bytes that remain (n >= 1).  A frame member is delimited by frame_header and
// chain_walk up to the end mark; with ZLZ4F_SPLIT_LEGACY in split_flags the legacy magic starts a legacy member, delimited
// by legacy_walk: it ends at the end of the bytes or in front of a foreign word, and is not the last one unless the walk
// meets a defect.  Whatever cannot be delimited reaches to n and is the last member.  nb = the blocks of the member's
// chain -- chain_walk's count, as k_bfd_walk<false> takes it for the same bytes, or legacy_walk's, as k_lf_walk<false>
// does: the caller keeps the two apart by `kind`.
__host__ __device__ inline MfMember mf_member(const uint8_t *__restrict__ s, uint64_t n, uint32_t split_flags) {
    MfMember m = {n, 0, ZLZ4F_MEMBER_FRAME, true};
    if (n >= 4) {
        const uint32_t magic = zx_rd32(s);
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
            const uint32_t nib = (magic & 15u) << 8;
            m.kind = ZLZ4F_MEMBER_SKIPPABLE_TRUNCATED | nib;
            if (n < 8) return m;
            const uint64_t len = 8ull + zx_rd32(s + 4);
            if (len > n) return m;
            m.len = len; m.kind = ZLZ4F_MEMBER_SKIPPABLE | nib; m.last = false;
            return m;
        }
        if ((split_flags & ZLZ4F_SPLIT_LEGACY) && magic == ZLZ4F_LEGACY_MAGICNUMBER) {
            m.kind = ZLZ4F_MEMBER_LEGACY;
            m.last = legacy_walk(s, n, ~0ull, m.nb, m.len, [](uint64_t, uint64_t, uint32_t) {}) < 0;    // (then len = n)
            return m;
        }
    }
    const ParsedHeader ph = frame_header(s, n);
    if (ph.size < 0) return m;
    uint64_t pos = (uint64_t)ph.size;
    const bool bc = (ph.flg & 0x10u) != 0;
    if (chain_walk(s, n, bc, pos, ~0ull, m.nb, [](uint64_t, const ChainBlock &) {}) != kChainEndMark) return m;
    if (ph.flg & 0x04u) {
        if (pos + 4 > n) return m;
        pos += 4;
    }
    m.len = pos; m.last = false;
    return m;
}

__device__ __forceinline__ bool bf_fits(const BFrame &F, uint32_t max_blocks) { return F.nb == 0 || F.base + F.nb <= max_blocks; }

// Dictionary frames: which frames the one-wavefront decoder takes.  A linked-declared frame of one
// block has T alone as its history -- what the block of an independent frame sees -- so it stays on the parallel decodes
// (the default preferences write such frames for small records).
__device__ __forceinline__ bool bfd_dict_serial(const BFrame &F) { return !(F.flg & 0x20u) && F.nb > 1; }

}  // namespace

// ------------------------------------------------------------------ seek tables
// The last member of a seekable file (include/zlz4_amd.h states the format): a skippable frame of T bytes that holds the
// file's member rows, its index entries and a 32-byte footer at the file's very end.  One statement of the footer parse
// and of the per-row checks, for the loader's kernels (zlz4_frame_seek.hip) and the host check (tests/seek_table_check.cpp).
// The checks are SHAPE ONLY: no position of a table becomes an address here.
namespace {

constexpr uint32_t kSeekFooterMagic = 0x4B53345Au;                    // "Z4SK"
constexpr uint32_t kSeekSelfKind = ZLZ4F_MEMBER_SKIPPABLE | (ZLZ4F_SEEK_TABLE_MAGICNUMBER & 15u) << 8;

__host__ __device__ inline uint64_t zx_rd64(const uint8_t *p) { return (uint64_t)zx_rd32(p) | ((uint64_t)zx_rd32(p + 4) << 32); }
struct Rd64 { __host__ __device__ __forceinline__ uint64_t operator()(const uint8_t *p) const { return zx_rd64(p); } };

// T for nm member rows (the table's own row included) and nb + 1 entries; false: T does not fit 64 bits
__host__ __device__ inline bool seek_table_bytes(uint64_t nm, uint64_t nb, uint64_t &T) {
    if (nm > (~0ull - 56u) / 24u) return false;
    const uint64_t t = 56u + 24u * nm;
    if (nb > (~0ull - t) / 16u) return false;
    T = t + 16u * nb;
    return true;
}

enum SeekVerdict : int32_t { kSeekNone = 0, kSeekOk = 1, kSeekMalformed = -1 };
struct SeekFooter { uint64_t nm, nb, T; };

// The footer of the n bytes at s: kSeekNone when n < 80 or the tail magic is absent, kSeekMalformed when it is there and
// the version is not 1, T overflows or exceeds n, file_len is not n, there is no member row, or the 8 bytes at n - T are
// not the skippable magic and P = T - 8.  Reads the last 32 bytes and those 8, byte by byte.
__host__ __device__ inline SeekVerdict seek_footer(const uint8_t *s, uint64_t n, SeekFooter &F) {
    F.nm = F.nb = F.T = 0;
    if (n < 80u || zx_rd32(s + n - 4u) != kSeekFooterMagic) return kSeekNone;
    if (zx_rd32(s + n - 8u) != 1u) return kSeekMalformed;
    const uint64_t nm = zx_rd64(s + n - 32u), nb = zx_rd64(s + n - 24u), file_len = zx_rd64(s + n - 16u);
    uint64_t T;
    if (nm == 0 || !seek_table_bytes(nm, nb, T) || T > n || file_len != n) return kSeekMalformed;
    if (zx_rd32(s + n - T) != ZLZ4F_SEEK_TABLE_MAGICNUMBER || (uint64_t)zx_rd32(s + n - T + 4u) != T - 8u) return kSeekMalformed;
    F.nm = nm; F.nb = nb; F.T = T;
    return kSeekOk;
}

// Member row k of the table of footer F that ends the n bytes at s, compared with its neighbour k + 1 -> the row is well
// shaped; m = the row as it stands in the file (buf = the reserved word).  rd reads 8 bytes at any alignment.
template <class Rd = Rd64>
__host__ __device__ __forceinline__ bool seek_member_row(const uint8_t *s, uint64_t n, const SeekFooter &F, uint64_t k,
                                                         zlz4f_member &m, Rd rd = Rd()) {
    const uint8_t *row = s + (n - F.T) + 8u + 24u * k;
    m.pos = rd(row); m.len = rd(row + 8);
    const uint64_t w = rd(row + 16);
    m.kind = (uint32_t)w; m.buf = (uint32_t)(w >> 32);
    if (m.buf != 0 || m.len == 0 || (k == 0 && m.pos != 0)) return false;
    if (k + 1u == F.nm) return m.pos == n - F.T && m.len == F.T && m.kind == kSeekSelfKind;
    const uint32_t kind = m.kind & 0xFFu;
    if ((m.kind & ~0xFFFu) || (kind != ZLZ4F_MEMBER_FRAME && kind != ZLZ4F_MEMBER_SKIPPABLE && kind != ZLZ4F_MEMBER_LEGACY))
        return false;
    return m.len <= ~0ull - m.pos && m.pos + m.len == rd(row + 24);
}

// Entry row k (0 .. nb) compared with its neighbour k + 1
template <class Rd = Rd64>
__host__ __device__ __forceinline__ bool seek_entry_row(const uint8_t *s, uint64_t n, const SeekFooter &F, uint64_t k,
                                                        zlz4f_index_entry &e, Rd rd = Rd()) {
    const uint8_t *row = s + (n - F.T) + 8u + 24u * F.nm + 16u * k;
    e.pos = rd(row); e.dec = rd(row + 8);
    if (e.pos > n - F.T) return false;
    return k == F.nb || (rd(row + 16) > e.pos && rd(row + 24) >= e.dec);
}

// Why zlz4f_batch_append_seek_table refuses a file of n bytes with room for cap: 0 = it does not.  nm = the split's result,
// last = the split's last member row (read only when nm > 0), nb = the index result, end_pos = entry[nb].pos.
__host__ __device__ inline int64_t seek_append_refusal(int64_t nm, const zlz4f_member &last, int64_t nb, uint64_t end_pos,
                                                       uint64_t n, uint64_t cap, uint64_t &T) {
    T = 0;
    if (nm < 0) return nm;
    if (nb < 0) return nb;
    if (nm > 0 && (last.kind & 0xFFu) == ZLZ4F_MEMBER_FRAME && end_pos + 4u > last.pos + last.len) return ZLZ4_ERR_INVALID_STATE;
    if (!seek_table_bytes((uint64_t)nm + 1u, (uint64_t)nb, T) || T - 8u > 0xFFFFFFFFull) { T = 0; return ZLZ4_ERR_UNSUPPORTED; }
    if (T > cap || n > cap - T) return ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
    return 0;
}

}  // namespace
