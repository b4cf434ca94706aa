// zlz4_frame_linked.hip -- linked-block lz4f frames in the batch frame pipeline.
//
// Decode (ZLZ4F_DECODE_LINKED): in a frame whose FLG has the block-independence bit (0x20) clear, block k may refer to
// the 64 KiB of output in front of it, so block k is decompressSafeUsingDict(block_k, dst[pos..], dict = dst[max(0, pos -
// 65536) .. pos]) (src/lz4.zig:89-251 with its dictionary branch :181-225).  The history is contiguous with the output:
// the dictionary branch collapses to a lower bound on op - offset, a match may reach min(pos, 65536) bytes in front of
// the block and never in front of the frame's first output byte.  Every byte can depend on the 64 KiB before it, so a
// frame is one serial chain: one wavefront walks the frame's blocks in order (k_bfl_decode), and the parallelism is
// across frames.  The kernel consumes the block table k_bfd_walk / k_bf_scan / k_bfd_verify of zlz4_frame.hip produce and
// leaves F.total / F.err for k_bfd_finish; k_bfl_mask takes the frame's entries out of the speculative and the exact
// parallel decodes (length and capacity 0), so that the frame is decoded once.
//
// Compress (ZLZ4F_BATCH_LINK_BLOCKS): block k of a frame is compressFastUsingDict(block_k, dict = the 64 KiB of INPUT in
// front of it); k_bfl_dict_desc writes the dictionary descriptors, the dictionary compressor does the rest.  At HC levels
// 3..9 (zlz4f_batch_compress_frame_ex) block k is compressHCUsingDict of the same pair: V_k = tail ++ block is a contiguous
// stretch of the input, so k_bfl_hc_desc describes it where it lies and the HC kernels run on the caller's bytes.
//
// Dictionary frames (the zlz4f_*_using_dict calls): the history of a linked-declared frame starts
// inside an external buffer, the tail T of the frame's dictionary (k_bfl_decode<.., kDict = true>); the k_bfdd_* kernels
// describe each frame's and each table entry's dictionary for the decode, the k_bfcd_* kernels the two compressor launches
// (against the dictionary, against the input in front of the block) and the merge of their results.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zlz4_amd.h"
#include "zlz4_device.hpp"
#include "zlz4_frame_batch.hpp"
#include "zlz4_launch.hpp"

namespace {

using namespace zlz4;

// One wavefront per linked-declared frame, four per workgroup: src/lz4f.zig:563-621 in block order with the history-aware
// decode; the error order is k_bfd_plan's (:591, :596, a stored block's DstMaxSizeTooSmall, :611), then the walk's error.
// kWrite: decodes into the frame's slot and leaves F.total / F.err for k_bfd_finish.  !kWrite: a destination that is
// never too small, nothing written but size[f] (k_bfq_total's result for the frame, the content checksum excepted).
// kDict: frame f's dictionary tail is dict[fd_end[f] - fd_len[f] .. fd_end[f]) (k_bfdd_frame); the size query reads fd_len
// only.  The dictionary arguments come last and the kDict == false instantiations never read them.
template <bool kWrite, bool kDict = false>
__global__ __launch_bounds__(256) void k_bfl_decode(BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                                                    const uint8_t *__restrict__ src, const uint64_t *__restrict__ data_off,
                                                    const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags,
                                                    const uint32_t *__restrict__ cks_ok, const int64_t *__restrict__ walk_err,
                                                    uint8_t *dst, const uint64_t *__restrict__ dst_off,
                                                    const uint64_t *__restrict__ dst_cap, const uint64_t *__restrict__ src_len,
                                                    int64_t *__restrict__ size, const uint8_t *__restrict__ dict,
                                                    const uint64_t *__restrict__ fd_end, const uint32_t *__restrict__ fd_len) {
    const uint32_t f = rfl(blockIdx.x * 4u + threadIdx.x / 64u), lane = threadIdx.x & 63u;
    if (f >= nframes) return;
    const BFrame F = fr[f];
    if (F.status < 0 || (F.flg & 0x20u)) return;                       // header error, or declared independent: not ours
    if (kDict && !bfd_dict_serial(F)) return;                          // one block: T is its whole history (parallel path)
    if (!bf_fits(F, max_blocks)) {
        if (!kWrite && lane == 0) size[f] = ZLZ4_ERR_INVALID_STATE;
        return;
    }
    const bool bc = (F.flg & 0x10u) != 0;
    const uint64_t nb = rfl64(F.nb), base = rfl64(F.base);
    const uint64_t cap = kWrite ? rfl64(dst_cap[f]) : ~0ull;
    uint8_t *out = kWrite ? dst + rfl64(dst_off[f]) : nullptr;
    const uint32_t D = kDict ? rfl(fd_len[f]) : 0u;                    // <= 65536
    const uint8_t *tend = kDict && kWrite ? dict + rfl64(fd_end[f]) : nullptr;
    uint64_t pos = 0;
    int64_t err = 0;
    for (uint64_t j = 0; j < nb; j++) {
        const uint64_t i = base + j;
        if (bc) {
            const uint32_t ok = rfl(cks_ok[i]);
            if (ok == 2u) { err = ZLZ4F_ERR_FRAME_SIZE_WRONG; break; }              // :591
            if (ok == 0u) { err = ZLZ4F_ERR_BLOCK_CHECKSUM_INVALID; break; }        // :596
        }
        const uint32_t len = rfl(data_len[i]);
        const uint8_t *p = src + rfl64(data_off[i]);
        const uint64_t rem = cap - pos;
        if (rfl(flags[i]) & kBlkStored) {                              // :603-608; history for the blocks after it
            if (len > rem) { err = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL; break; }
            if (kWrite) copy_bytes(out + pos, p, len, lane);
            pos += len;
        } else {                                                       // :610
            const uint32_t oend = rem < 0xFFFFFFFFull ? (uint32_t)rem : 0xFFFFFFFFu;
            const uint32_t inframe = pos < 65536u ? (uint32_t)pos : 65536u;
            const uint32_t hist = inframe + D < 65536u ? inframe + D : 65536u;
            const int64_t r = decode_block_wave<kWrite, kDict>(p, len, kWrite ? out + pos : nullptr, oend, hist, lane, tend,
                                                                 inframe);
            if (r < 0) { err = ZLZ4F_ERR_DECOMPRESSION_FAILED; break; }             // :611
            pos += (uint64_t)r;
        }
    }
    if (!err) err = walk_err[f];                                       // :565, :582
    if (lane != 0) return;
    if (kWrite) {
        fr[f].total = pos;
        fr[f].err = err;
    } else {
        size[f] = err ? err : (((F.flg & 0x04u) && F.end + 4 > src_len[f]) ? (int64_t)ZLZ4F_ERR_FRAME_SIZE_WRONG   // :626
                                                                          : (int64_t)pos);
    }
}

// Frame prefix decoding, FP(frame, n, T) of DESIGN.md section 4.4f: the first n = dst_cap[f] bytes of frame f.  One
// wavefront per frame, four per workgroup, and the wavefront does all of it in one serial walk that ends at the cut: the
// header (:547), the chain (:563-600, chain_step with a wave-uniform word reader), a reached block's checksum (one lane
// hashes, the verdict is broadcast), the stored copy, the history-aware decode cut at the bytes still wanted, and --
// only when the chain ended first -- the content checksum (:625-635).  No block table, no workspace; every scalar is
// wave-uniform (rfl / byte_at).
// The stop rule stands in front of the loop's own condition: once n bytes are out nothing more of the source is read.
// kDict: frame f's dictionary is number dict_idx[f] (nullptr: 0) of ndicts; an index that names none gives InvalidState
// in front of every other status.  The kDict == false instantiation never reads the dictionary arguments.
template <bool kDict>
__global__ __launch_bounds__(256) void k_bfp_decode(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                    const uint64_t *__restrict__ src_len, uint8_t *dst,
                                                    const uint64_t *__restrict__ dst_off,
                                                    const uint64_t *__restrict__ dst_cap, int64_t *__restrict__ result,
                                                    uint32_t nframes, const uint8_t *__restrict__ dict,
                                                    const uint64_t *__restrict__ dict_off,
                                                    const uint32_t *__restrict__ dict_len, uint32_t ndicts,
                                                    const uint32_t *__restrict__ dict_idx) {
    const uint32_t f = rfl(blockIdx.x * 4u + threadIdx.x / 64u), lane = threadIdx.x & 63u;
    if (f >= nframes) return;
    uint32_t D = 0;
    const uint8_t *tend = nullptr;
    if constexpr (kDict) {
        const uint32_t d = dict_idx ? rfl(dict_idx[f]) : 0u;
        if (d >= ndicts) {
            if (lane == 0) result[f] = ZLZ4_ERR_INVALID_STATE;
            return;
        }
        const uint32_t len = rfl(dict_len[d]);
        D = len < 65536u ? len : 65536u;
        tend = dict + rfl64(dict_off[d]) + len;
    }
    const uint64_t n = rfl64(src_len[f]), want = rfl64(dst_cap[f]);
    const uint8_t *s = src + rfl64(src_off[f]);
    uint8_t *out = dst + rfl64(dst_off[f]);
    const ParsedHeader ph = parse_header(s, n < 19u ? (size_t)n : (size_t)19u);   // :547, every lane the same bytes
    const int64_t hs = (int64_t)rfl64((uint64_t)ph.size);
    if (hs < 0) {
        if (lane == 0) result[f] = hs;
        return;
    }
    const uint32_t flg = rfl((uint32_t)ph.flg);
    const bool bc = (flg & 0x10u) != 0, indep = (flg & 0x20u) != 0;
    uint64_t sp = (uint64_t)hs, pos = 0;
    int64_t err = 0;
    bool cut = false;
    const auto rd = [](const uint8_t *p) {                             // a block word, wave-uniform
        return byte_at(p) | (byte_at(p + 1) << 8) | (byte_at(p + 2) << 16) | (byte_at(p + 3) << 24);
    };
    for (;;) {
        if (pos == want) { cut = true; break; }                        // the stop rule: nothing behind is read
        ChainBlock c;
        const ChainEnd end = chain_step(s, n, bc, sp, c, rd);          // :563-591
        if (end > kChainCksCut) { err = chain_error(end); break; }
        if (end == kChainCksCut) { err = ZLZ4F_ERR_FRAME_SIZE_WRONG; break; }       // :591
        const uint8_t *p = s + c.off;
        const uint32_t sz = c.size;
        if (c.flags & kBlkCks) {                                       // :590: over the whole block, in front of the decode
            uint32_t ok = 0;
            if (lane == 0) ok = xxh32(p, sz, 0) == zx_rd32(s + c.cks_off) ? 1u : 0u;
            if (rfl(ok) == 0u) { err = ZLZ4F_ERR_BLOCK_CHECKSUM_INVALID; break; }   // :596
        }
        const uint64_t rem = want - pos;                               // >= 1
        if (c.flags & kBlkStored) {                                    // :603-608: the bytes that fit; history
            const uint32_t c = sz < rem ? sz : (uint32_t)rem;
            copy_bytes(out + pos, p, c, lane);
            pos += c;
        } else {                                                       // :610
            const uint32_t oend = rem < 0xFFFFFFFFull ? (uint32_t)rem : 0xFFFFFFFFu;
            const uint32_t inframe = indep ? 0u : (pos < 65536u ? (uint32_t)pos : 65536u);
            const uint32_t hist = inframe + D < 65536u ? inframe + D : 65536u;
            const int64_t r = decode_block_wave<true, kDict, false, true>(p, sz, out + pos, oend, hist, lane, tend, inframe);
            if (r < 0) { err = ZLZ4F_ERR_DECOMPRESSION_FAILED; break; }             // :611
            pos += (uint64_t)r;
        }
    }
    if (!cut && !err && (flg & 0x04u)) {                               // the whole frame is out: :625-635
        if (sp + 4 > n) err = ZLZ4F_ERR_FRAME_SIZE_WRONG;              // :626
        else {
            uint32_t ok = 0;
            if (lane == 0) ok = xxh32(out, pos, 0) == zx_rd32(s + sp) ? 1u : 0u;
            if (rfl(ok) == 0u) err = ZLZ4F_ERR_CONTENT_CHECKSUM_INVALID;            // :631
        }
    }
    if (lane == 0) result[f] = err ? err : (int64_t)pos;
}

// one lane per frame: the chain walk's error, before k_bfd_plan replaces F.err
__global__ void k_bfl_save(const BFrame *__restrict__ fr, uint32_t nframes, int64_t *__restrict__ walk_err) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < nframes) walk_err[f] = fr[f].err;
}

// one lane per table entry: an entry of a linked-declared frame takes no part in a parallel decode (length and capacity 0)
__global__ void k_bfl_mask(const BFrame *__restrict__ fr, const uint32_t *__restrict__ fidx, uint32_t max_blocks,
                           uint32_t *__restrict__ cap, uint32_t *__restrict__ len) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        const uint32_t f = fidx[i];
        if (f == kNoFrame || (fr[f].flg & 0x20u)) continue;
        if (cap) cap[i] = 0;
        len[i] = 0;
    }
}

// compress, one lane per table entry: block k of frame f (in_off = src_off[f] + k * bs) has the min(k * bs, 65536) input
// bytes in front of it as its dictionary; entries without a block (length 0) have none
__global__ void k_bfl_dict_desc(const BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                                const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ in_off,
                                const uint32_t *__restrict__ in_len, uint64_t *__restrict__ dict_off,
                                uint32_t *__restrict__ dict_len) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        uint64_t o = 0;
        uint32_t len = 0;
        if (in_len[i] != 0) {
            uint32_t lo = 0, hi = nframes;                             // the last frame whose base is <= i (k_bfc_desc)
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (fr[mid].base <= i) lo = mid + 1u; else hi = mid;
            }
            const uint64_t before = in_off[i] - src_off[lo - 1u];      // k * bs
            len = before < 65536u ? (uint32_t)before : 65536u;
            o = in_off[i] - len;
        }
        dict_off[i] = o;
        dict_len[i] = len;
    }
}

// compress at HC levels, one lane per table entry: V_k = input[k * bs - D_k .. k * bs + n_k) with D_k = min(k * bs, 65536),
// as the three HC kernels consume it (zlz4_launch_compress_hc_linked): v_off absolute in the source arena, v_len = D_k + n_k
// for K1, the pair { v_len, start = D_k } for K2s and K3.  Entries without a block (length 0) get an empty V: K1 and K2s
// skip it, K3 writes the result 0.
__global__ void k_bfl_hc_desc(const BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                              const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ in_off,
                              const uint32_t *__restrict__ in_len, uint64_t *__restrict__ v_off, uint32_t *__restrict__ v_len,
                              uint32_t *__restrict__ v_pair) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        uint64_t o = 0;
        uint32_t len = 0, start = 0;
        const uint32_t n = in_len[i];
        if (n != 0) {
            uint32_t lo = 0, hi = nframes;                             // the last frame whose base is <= i (k_bfc_desc)
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (fr[mid].base <= i) lo = mid + 1u; else hi = mid;
            }
            const uint64_t before = in_off[i] - src_off[lo - 1u];      // k * bs
            start = before < 65536u ? (uint32_t)before : 65536u;
            o = in_off[i] - start;
            len = start + n;
        }
        v_off[i] = o;
        v_len[i] = len;
        v_pair[2u * i] = len;
        v_pair[2u * i + 1u] = start;
    }
}

// ------------------------------------------------------------------ dictionary frames
// decode, one lane per frame, between the counting walk and the scan: frame f's dictionary is number idx[f] (idx == nullptr:
// 0) of `ndicts`; T = its last D = min(len, 65536) bytes, described by where it ends (absolute in the dictionary arena)
// and D.  A frame whose index names no dictionary gets InvalidState and owns no table entries.  dict_off == nullptr (the
// size query knows lengths only): fd_end is not written.
__global__ void k_bfdd_frame(BFrame *__restrict__ fr, uint32_t nframes, const uint64_t *__restrict__ dict_off,
                             const uint32_t *__restrict__ dict_len, uint32_t ndicts, const uint32_t *__restrict__ dict_idx,
                             uint64_t *__restrict__ fd_end, uint32_t *__restrict__ fd_len) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const uint32_t d = dict_idx ? dict_idx[f] : 0u;
    if (d >= ndicts) {
        fr[f].status = ZLZ4_ERR_INVALID_STATE;
        fr[f].nb = 0;
        if (fd_end) fd_end[f] = 0;
        fd_len[f] = 0;
        return;
    }
    const uint32_t len = dict_len[d];
    if (fd_end) fd_end[f] = dict_off[d] + len;
    fd_len[f] = len < 65536u ? len : 65536u;
}

// decode, one lane per table entry: the dictionary descriptor of an entry whose frame declares independent blocks or has
// one block (every block sees T, decompressSafeUsingDict); the other entries are decoded by k_bfl_decode and get none
__global__ void k_bfdd_entry(const BFrame *__restrict__ fr, const uint32_t *__restrict__ fidx, uint32_t max_blocks,
                             const uint64_t *__restrict__ fd_end, const uint32_t *__restrict__ fd_len,
                             uint64_t *__restrict__ e_off, uint32_t *__restrict__ e_len) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        const uint32_t f = fidx[i];
        const bool mine = f != kNoFrame && !bfd_dict_serial(fr[f]);
        const uint32_t D = mine ? fd_len[f] : 0u;
        if (e_off) e_off[i] = mine && fd_end ? fd_end[f] - D : 0u;
        e_len[i] = D;
    }
}

// k_bfl_mask for a call with dictionaries: the entries of the frames k_bfl_decode<.., true> takes
__global__ void k_bfdd_mask(const BFrame *__restrict__ fr, const uint32_t *__restrict__ fidx, uint32_t max_blocks,
                            uint32_t *__restrict__ cap, uint32_t *__restrict__ len) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        const uint32_t f = fidx[i];
        if (f == kNoFrame || !bfd_dict_serial(fr[f])) continue;
        if (cap) cap[i] = 0;
        len[i] = 0;
    }
}

// compress, one lane per frame, after k_bfc_count: the preconditions of the call.  A frame that names no dictionary, is
// longer than max_src_len (0: no bound) or whose T is longer than max_dict_len gets InvalidState in front of every other
// status; k_bfc_desc then gives its entries length 0.
__global__ void k_bfcd_pre(BFrame *__restrict__ fr, uint32_t nframes, const uint64_t *__restrict__ src_len,
                           const uint32_t *__restrict__ dict_len, uint32_t ndicts, const uint32_t *__restrict__ dict_idx,
                           uint64_t max_src_len, uint32_t max_dict_len) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const uint32_t d = dict_idx ? dict_idx[f] : 0u;
    bool bad = d >= ndicts || (max_src_len != 0 && src_len[f] > max_src_len);
    if (!bad) {
        const uint32_t len = dict_len[d];
        bad = (len < 65536u ? len : 65536u) > max_dict_len;
    }
    if (bad) fr[f].status = ZLZ4_ERR_INVALID_STATE;
}

// compress, one lane per table entry (next to k_bfl_dict_desc).  Launch A compresses against the frame's dictionary, read
// from the dictionary arena with the dictionary's own loadDict table: every block of an independent frame, block 0 of a
// linked one.  Launch B is the linked path of section 4.4c for the blocks k >= 1 of a linked frame (dictionary = the input
// in front of the block, read from the source arena).  len_a / len_b are the complementary length arrays of the two
// launches (an entry that takes no part has length 0 there: result 0, nothing written); a_off / a_len / a_tix describe
// launch A's dictionary and table.  !with_b (independent frames, or linked ones that cannot have a second block): every
// entry is launch A's and len_b, which the caller then does not have, is not written.
__global__ void k_bfcd_desc(const BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks, bool with_b,
                            const uint64_t *__restrict__ dict_off, const uint32_t *__restrict__ dict_len,
                            const uint32_t *__restrict__ dict_idx, const uint32_t *__restrict__ in_len,
                            uint32_t *__restrict__ len_a, uint32_t *__restrict__ len_b, uint64_t *__restrict__ a_off,
                            uint32_t *__restrict__ a_len, uint32_t *__restrict__ a_tix) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        const uint32_t n = in_len[i];
        uint32_t la = 0, lb = 0, tix = 0, dl = 0;
        uint64_t off = 0;
        if (n != 0) {                                                  // (a frame with a block passed k_bfcd_pre)
            uint32_t lo = 0, hi = nframes;                             // the last frame whose base is <= i (k_bfc_desc)
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (fr[mid].base <= i) lo = mid + 1u; else hi = mid;
            }
            const uint32_t f = lo - 1u;
            if (with_b && i != fr[f].base) lb = n;
            else {
                la = n;
                tix = dict_idx ? dict_idx[f] : 0u;
                off = dict_off[tix];
                dl = dict_len[tix];
            }
        }
        len_a[i] = la;
        if (with_b) len_b[i] = lb;
        a_off[i] = off;
        a_len[i] = dl;
        a_tix[i] = tix;
    }
}

// compress, one lane per table entry: launch B's result for the entries that took part in it; launch A's stands elsewhere
__global__ void k_bfcd_merge(const uint32_t *__restrict__ len_b, const int64_t *__restrict__ csize_b,
                             int64_t *__restrict__ csize, uint32_t max_blocks) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x)
        if (len_b[i] != 0) csize[i] = csize_b[i];
}

}  // namespace

// `frames` is the pipeline's BFrame array.  All launchers: 0, or ZLZ4_ERR_DEVICE when a launch fails.
extern "C" int zlz4_launch_bfl_save(hipStream_t st, const void *frames, uint32_t nframes, int64_t *walk_err) {
    hipLaunchKernelGGL(k_bfl_save, dim3(grid_of(nframes, 256)), dim3(256), 0, st, static_cast<const BFrame *>(frames), nframes,
                       walk_err);
    return zlz4_launch_status();
}

extern "C" int zlz4_launch_bfl_mask(hipStream_t st, const void *frames, const uint32_t *fidx, uint32_t max_blocks,
                                    uint32_t *cap, uint32_t *len) {
    if (max_blocks == 0) return 0;
    hipLaunchKernelGGL(k_bfl_mask, dim3(grid_of(max_blocks, 256, 4096)), dim3(256), 0, st,
                       static_cast<const BFrame *>(frames), fidx, max_blocks, cap, len);
    return zlz4_launch_status();
}

// write != 0: the decode (F.total / F.err); write == 0: the size query (d_size receives the frame's result)
extern "C" int zlz4_launch_bfl_decode(hipStream_t st, int write, void *frames, uint32_t nframes, uint32_t max_blocks,
                                      const uint8_t *src, const uint64_t *data_off, const uint32_t *data_len,
                                      const uint32_t *flags, const uint32_t *cks_ok, const int64_t *walk_err, uint8_t *dst,
                                      const uint64_t *dst_off, const uint64_t *dst_cap, const uint64_t *src_len,
                                      int64_t *d_size) {
    BFrame *fr = static_cast<BFrame *>(frames);
    const dim3 grid(grid_of(nframes, 4)), block(256);
    if (write)
        hipLaunchKernelGGL(k_bfl_decode<true>, grid, block, 0, st, fr, nframes, max_blocks, src, data_off, data_len, flags,
                           cks_ok, walk_err, dst, dst_off, dst_cap, src_len, d_size, nullptr, nullptr, nullptr);
    else
        hipLaunchKernelGGL(k_bfl_decode<false>, grid, block, 0, st, fr, nframes, max_blocks, src, data_off, data_len, flags,
                           cks_ok, walk_err, dst, dst_off, dst_cap, src_len, d_size, nullptr, nullptr, nullptr);
    return zlz4_launch_status();
}

// the same with a dictionary per frame: fd_end / fd_len are k_bfdd_frame's
extern "C" int zlz4_launch_bfl_decode_dict(hipStream_t st, int write, void *frames, uint32_t nframes, uint32_t max_blocks,
                                           const uint8_t *src, const uint64_t *data_off, const uint32_t *data_len,
                                           const uint32_t *flags, const uint32_t *cks_ok, const int64_t *walk_err,
                                           uint8_t *dst, const uint64_t *dst_off, const uint64_t *dst_cap,
                                           const uint64_t *src_len, int64_t *d_size, const uint8_t *dict,
                                           const uint64_t *fd_end, const uint32_t *fd_len) {
    BFrame *fr = static_cast<BFrame *>(frames);
    const dim3 grid(grid_of(nframes, 4)), block(256);
    if (write)
        hipLaunchKernelGGL((k_bfl_decode<true, true>), grid, block, 0, st, fr, nframes, max_blocks, src, data_off, data_len,
                           flags, cks_ok, walk_err, dst, dst_off, dst_cap, src_len, d_size, dict, fd_end, fd_len);
    else
        hipLaunchKernelGGL((k_bfl_decode<false, true>), grid, block, 0, st, fr, nframes, max_blocks, src, data_off, data_len,
                           flags, cks_ok, walk_err, dst, dst_off, dst_cap, src_len, d_size, dict, fd_end, fd_len);
    return zlz4_launch_status();
}

// Frame prefix decoding: one launch, no workspace.  d_dst_cap[f] is the number of bytes wanted of
// frame f and the size of its slot.  ndicts == 0: no dictionaries (the plain call; the dictionary arguments are not read).
extern "C" int zlz4_launch_bfp_decode(hipStream_t st, const uint8_t *src, const uint64_t *src_off, const uint64_t *src_len,
                                      uint8_t *dst, const uint64_t *dst_off, const uint64_t *dst_cap, int64_t *result,
                                      uint32_t nframes) {
    return zlz4_launch_bfp_decode_dict(st, src, src_off, src_len, dst, dst_off, dst_cap, result, nframes, nullptr, nullptr,
                                       nullptr, 0, nullptr);
}

extern "C" int zlz4_launch_bfp_decode_dict(hipStream_t st, const uint8_t *src, const uint64_t *src_off,
                                           const uint64_t *src_len, uint8_t *dst, const uint64_t *dst_off,
                                           const uint64_t *dst_cap, int64_t *result, uint32_t nframes, const uint8_t *dict,
                                           const uint64_t *dict_off, const uint32_t *dict_len, uint32_t ndicts,
                                           const uint32_t *dict_idx) {
    if (nframes == 0) return 0;
    const dim3 grid(grid_of(nframes, 4)), block(256);
    if (ndicts == 0)
        hipLaunchKernelGGL(k_bfp_decode<false>, grid, block, 0, st, src, src_off, src_len, dst, dst_off, dst_cap, result,
                           nframes, nullptr, nullptr, nullptr, 0u, nullptr);
    else
        hipLaunchKernelGGL(k_bfp_decode<true>, grid, block, 0, st, src, src_off, src_len, dst, dst_off, dst_cap, result,
                           nframes, dict, dict_off, dict_len, ndicts, dict_idx);
    return zlz4_launch_status();
}

extern "C" int zlz4_launch_bfdd_frame(hipStream_t st, void *frames, uint32_t nframes, const uint64_t *dict_off,
                                      const uint32_t *dict_len, uint32_t ndicts, const uint32_t *dict_idx, uint64_t *fd_end,
                                      uint32_t *fd_len) {
    hipLaunchKernelGGL(k_bfdd_frame, dim3(grid_of(nframes, 256)), dim3(256), 0, st, static_cast<BFrame *>(frames), nframes,
                       dict_off, dict_len, ndicts, dict_idx, fd_end, fd_len);
    return zlz4_launch_status();
}

extern "C" int zlz4_launch_bfdd_entry(hipStream_t st, const void *frames, const uint32_t *fidx, uint32_t max_blocks,
                                      const uint64_t *fd_end, const uint32_t *fd_len, uint64_t *e_off, uint32_t *e_len) {
    if (max_blocks == 0) return 0;
    hipLaunchKernelGGL(k_bfdd_entry, dim3(grid_of(max_blocks, 256, 4096)), dim3(256), 0, st,
                       static_cast<const BFrame *>(frames), fidx, max_blocks, fd_end, fd_len, e_off, e_len);
    return zlz4_launch_status();
}

extern "C" int zlz4_launch_bfdd_mask(hipStream_t st, const void *frames, const uint32_t *fidx, uint32_t max_blocks,
                                     uint32_t *cap, uint32_t *len) {
    if (max_blocks == 0) return 0;
    hipLaunchKernelGGL(k_bfdd_mask, dim3(grid_of(max_blocks, 256, 4096)), dim3(256), 0, st,
                       static_cast<const BFrame *>(frames), fidx, max_blocks, cap, len);
    return zlz4_launch_status();
}

extern "C" int zlz4_launch_bfcd_pre(hipStream_t st, void *frames, uint32_t nframes, const uint64_t *src_len,
                                    const uint32_t *dict_len, uint32_t ndicts, const uint32_t *dict_idx, uint64_t max_src_len,
                                    uint32_t max_dict_len) {
    hipLaunchKernelGGL(k_bfcd_pre, dim3(grid_of(nframes, 256)), dim3(256), 0, st, static_cast<BFrame *>(frames), nframes,
                       src_len, dict_len, ndicts, dict_idx, max_src_len, max_dict_len);
    return zlz4_launch_status();
}

extern "C" int zlz4_launch_bfcd_desc(hipStream_t st, const void *frames, uint32_t nframes, uint32_t max_blocks, int with_b,
                                     const uint64_t *dict_off, const uint32_t *dict_len, const uint32_t *dict_idx,
                                     const uint32_t *in_len, uint32_t *len_a, uint32_t *len_b, uint64_t *a_off,
                                     uint32_t *a_len, uint32_t *a_tix) {
    if (max_blocks == 0) return 0;
    if (with_b && !len_b) return ZLZ4_ERR_INVALID_STATE;
    hipLaunchKernelGGL(k_bfcd_desc, dim3(grid_of(max_blocks, 256, 4096)), dim3(256), 0, st,
                       static_cast<const BFrame *>(frames), nframes, max_blocks, with_b != 0, dict_off, dict_len, dict_idx,
                       in_len, len_a, len_b, a_off, a_len, a_tix);
    return zlz4_launch_status();
}

extern "C" int zlz4_launch_bfcd_merge(hipStream_t st, const uint32_t *len_b, const int64_t *csize_b, int64_t *csize,
                                      uint32_t max_blocks) {
    if (max_blocks == 0) return 0;
    hipLaunchKernelGGL(k_bfcd_merge, dim3(grid_of(max_blocks, 256, 4096)), dim3(256), 0, st, len_b, csize_b, csize,
                       max_blocks);
    return zlz4_launch_status();
}

extern "C" int zlz4_launch_bfl_dict_desc(hipStream_t st, const void *frames, uint32_t nframes, uint32_t max_blocks,
                                         const uint64_t *src_off, const uint64_t *in_off, const uint32_t *in_len,
                                         uint64_t *dict_off, uint32_t *dict_len) {
    if (max_blocks == 0) return 0;
    hipLaunchKernelGGL(k_bfl_dict_desc, dim3(grid_of(max_blocks, 256, 4096)), dim3(256), 0, st,
                       static_cast<const BFrame *>(frames), nframes, max_blocks, src_off, in_off, in_len, dict_off, dict_len);
    return zlz4_launch_status();
}

extern "C" int zlz4_launch_bfl_hc_desc(hipStream_t st, const void *frames, uint32_t nframes, uint32_t max_blocks,
                                       const uint64_t *src_off, const uint64_t *in_off, const uint32_t *in_len,
                                       uint64_t *v_off, uint32_t *v_len, uint32_t *v_pair) {
    if (max_blocks == 0) return 0;
    hipLaunchKernelGGL(k_bfl_hc_desc, dim3(grid_of(max_blocks, 256, 4096)), dim3(256), 0, st,
                       static_cast<const BFrame *>(frames), nframes, max_blocks, src_off, in_off, in_len, v_off, v_len, v_pair);
    return zlz4_launch_status();
}
