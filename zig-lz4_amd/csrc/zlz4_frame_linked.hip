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
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zlz4_amd.h"
#include "zlz4_device.hpp"
#include "zlz4_frame_batch.hpp"
#include "zlz4_launch.hpp"

namespace {

using namespace zlz4;

__device__ __forceinline__ uint64_t rfl64(uint64_t v) { return ((uint64_t)rfl((uint32_t)(v >> 32)) << 32) | rfl((uint32_t)v); }
__device__ __forceinline__ uint32_t byte_at(const uint8_t *p) { return rfl((uint32_t)*p); }   // wave-uniform address

// decompressGeneric (src/lz4.zig:89-251) of one block by one wavefront, after decode_wave of zlz4_stream_decode.hip.
// `out` is where the block's output starts, `hist` the bytes of the same frame that lie directly in front of it and may
// be referenced (<= 65536).  :181-192 with dict.len = hist: CorruptedData iff offset > op + hist; every other match is a
// plain copy from out + op - offset, whether it starts in the history, spans its end or lies in the block.
// kWrite false: the same walk without a byte written or read from the output (the size query).
template <bool kWrite>
__device__ int64_t decode_linked_block(const uint8_t *src, uint32_t iend, uint8_t *out, uint32_t oend, uint32_t hist,
                                       uint32_t lane) {
    if (iend == 0 || oend == 0) return 0;                              // :97-98
    uint32_t ip = 0, op = 0;
    for (;;) {
        if (ip >= iend) break;                                         // :113
        const uint32_t token = byte_at(src + ip++);                    // :116
        uint32_t lit = token >> 4;
        if (lit == 15u) {                                              // :123-131
            for (;;) {
                if (ip >= iend) return kErrCorrupted;
                const uint32_t b = byte_at(src + ip++);
                lit += b;
                if (lit > 0xFFFF0000u) lit = 0xFFFF0000u;
                if (b != 255u) break;
            }
        }
        if (lit > 0) {                                                 // :134-144
            if (lit > iend - ip) return kErrCorrupted;
            if (lit > oend - op) return kErrOutputTooSmall;
            if (kWrite) copy_bytes(out + op, src + ip, lit, lane);
            ip += lit; op += lit;
        }
        if (ip >= iend) break;                                         // :146
        if (iend - ip < 2u) return kErrCorrupted;                      // :149
        const uint32_t offset = byte_at(src + ip) | (byte_at(src + ip + 1) << 8);
        ip += 2;
        if (offset == 0) return kErrCorrupted;                         // :154
        uint32_t ml = token & 15u;
        if (ml == 15u) {                                               // :160-168
            for (;;) {
                if (ip >= iend) return kErrCorrupted;
                const uint32_t b = byte_at(src + ip++);
                ml += b;
                if (ml > 0xFFFF0000u) ml = 0xFFFF0000u;
                if (b != 255u) break;
            }
        }
        ml += kMinMatch;                                               // :171
        if (ml > oend - op) return kErrOutputTooSmall;                 // :174
        if (offset > op && offset - op > hist) return kErrCorrupted;   // :181-192: in front of the history
        if (kWrite) {                                                  // :195-248: out[op + k] = out[op - offset + k]
            uint8_t *o = out + op;
            const uint8_t *m = o - offset;
            if (offset >= ml || offset >= 1024u) {
                copy_bytes(o, m, ml, lane);
            } else {
                // overlap (:235-241): what is made so far is copied again as a whole -- offset bytes, then 2 x, 4 x ... --
                // each copy disjoint from its source
                uint32_t made = 0;
                while (made < ml) {
                    const uint32_t have = made + offset, left = ml - made;
                    const uint32_t n1 = have < left ? have : left;
                    copy_bytes(o + made, m, n1, lane);
                    made += n1;
                }
            }
        }
        op += ml;
    }
    return (int64_t)op;                                                // :250
}

// One wavefront per linked-declared frame, four per workgroup: src/lz4f.zig:563-621 in block order with the history-aware
// decode; the error order is k_bfd_plan's (:591, :596, a stored block's DstMaxSizeTooSmall, :611), then the walk's error.
// kWrite: decodes into the frame's slot and leaves F.total / F.err for k_bfd_finish.  !kWrite: a destination that is
// never too small, nothing written but size[f] (k_bfq_total's result for the frame, the content checksum excepted).
template <bool kWrite>
__global__ __launch_bounds__(256) void k_bfl_decode(BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                                                    const uint8_t *__restrict__ src, const uint64_t *__restrict__ data_off,
                                                    const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags,
                                                    const uint32_t *__restrict__ cks_ok, const int64_t *__restrict__ walk_err,
                                                    uint8_t *dst, const uint64_t *__restrict__ dst_off,
                                                    const uint64_t *__restrict__ dst_cap, const uint64_t *__restrict__ src_len,
                                                    int64_t *__restrict__ size) {
    const uint32_t f = rfl(blockIdx.x * 4u + threadIdx.x / 64u), lane = threadIdx.x & 63u;
    if (f >= nframes) return;
    const BFrame F = fr[f];
    if (F.status < 0 || (F.flg & 0x20u)) return;                       // header error, or declared independent: not ours
    if (!bf_fits(F, max_blocks)) {
        if (!kWrite && lane == 0) size[f] = ZLZ4_ERR_INVALID_STATE;
        return;
    }
    const bool bc = (F.flg & 0x10u) != 0;
    const uint64_t nb = rfl64(F.nb), base = rfl64(F.base);
    const uint64_t cap = kWrite ? rfl64(dst_cap[f]) : ~0ull;
    uint8_t *out = kWrite ? dst + rfl64(dst_off[f]) : nullptr;
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
            const uint32_t hist = pos < 65536u ? (uint32_t)pos : 65536u;
            const int64_t r = decode_linked_block<kWrite>(p, len, kWrite ? out + pos : nullptr, oend, hist, lane);
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

inline uint32_t grid_of(uint64_t items, uint32_t threads, uint32_t cap = 0xFFFFFFFFu) {
    const uint64_t g = (items + threads - 1) / threads;
    return g == 0 ? 1u : (g > cap ? cap : (uint32_t)g);
}

}  // namespace

// `frames` is the pipeline's BFrame array.  All launchers: 0, or -7 when a launch fails.
extern "C" int zlz4_launch_bfl_save(hipStream_t st, const void *frames, uint32_t nframes, int64_t *walk_err) {
    hipLaunchKernelGGL(k_bfl_save, dim3(grid_of(nframes, 256)), dim3(256), 0, st, static_cast<const BFrame *>(frames), nframes,
                       walk_err);
    return hipGetLastError() == hipSuccess ? 0 : -7;
}

extern "C" int zlz4_launch_bfl_mask(hipStream_t st, const void *frames, const uint32_t *fidx, uint32_t max_blocks,
                                    uint32_t *cap, uint32_t *len) {
    if (max_blocks == 0) return 0;
    hipLaunchKernelGGL(k_bfl_mask, dim3(grid_of(max_blocks, 256, 4096)), dim3(256), 0, st,
                       static_cast<const BFrame *>(frames), fidx, max_blocks, cap, len);
    return hipGetLastError() == hipSuccess ? 0 : -7;
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
                           cks_ok, walk_err, dst, dst_off, dst_cap, src_len, d_size);
    else
        hipLaunchKernelGGL(k_bfl_decode<false>, grid, block, 0, st, fr, nframes, max_blocks, src, data_off, data_len, flags,
                           cks_ok, walk_err, dst, dst_off, dst_cap, src_len, d_size);
    return hipGetLastError() == hipSuccess ? 0 : -7;
}

extern "C" int zlz4_launch_bfl_dict_desc(hipStream_t st, const void *frames, uint32_t nframes, uint32_t max_blocks,
                                         const uint64_t *src_off, const uint64_t *in_off, const uint32_t *in_len,
                                         uint64_t *dict_off, uint32_t *dict_len) {
    if (max_blocks == 0) return 0;
    hipLaunchKernelGGL(k_bfl_dict_desc, dim3(grid_of(max_blocks, 256, 4096)), dim3(256), 0, st,
                       static_cast<const BFrame *>(frames), nframes, max_blocks, src_off, in_off, in_len, dict_off, dict_len);
    return hipGetLastError() == hipSuccess ? 0 : -7;
}

extern "C" int zlz4_launch_bfl_hc_desc(hipStream_t st, const void *frames, uint32_t nframes, uint32_t max_blocks,
                                       const uint64_t *src_off, const uint64_t *in_off, const uint32_t *in_len,
                                       uint64_t *v_off, uint32_t *v_len, uint32_t *v_pair) {
    if (max_blocks == 0) return 0;
    hipLaunchKernelGGL(k_bfl_hc_desc, dim3(grid_of(max_blocks, 256, 4096)), dim3(256), 0, st,
                       static_cast<const BFrame *>(frames), nframes, max_blocks, src_off, in_off, in_len, v_off, v_len, v_pair);
    return hipGetLastError() == hipSuccess ? 0 : -7;
}
