// zlz4_frame_legacy.hip -- legacy frames (include/zlz4_amd.h): what `lz4 -l` writes and the Linux
// kernel's unlz4 reads.  A frame is the magic 0x184C2102 and { u32 LE size, block } repeated: no checksums, no stored
// blocks, no end mark, every block an independent LZ4 block of at most 8 MiB of content.  So the per-block work is that of
// the block batch calls, and this file is the frame layer around their launchers (zlz4_launch.hpp): the walk that finds
// the blocks (legacy_walk of zlz4_frame_batch.hpp, one lane per frame), a block table of max_blocks entries that all
// frames share, one wavefront per frame that folds and places its blocks, and the scatter of the compressed blocks to
// their unaligned places.  Every call is a fixed sequence of kernels on the caller's stream: nothing allocated, nothing
// read back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zlz4_device.hpp"
#include "zlz4_frame_batch.hpp"
#include "zlz4_host.hpp"
#include "zlz4_launch.hpp"

using namespace zlz4host;

namespace {

// what the calls keep per frame between their kernels
struct LFrame {
    uint64_t nb;        // blocks: what the chain holds (decode), ceil(len / bs) (compress)
    uint64_t base;      // first table entry (exclusive scan of nb)
    int64_t status;     // decode: the walk's verdict; compress: 0, SrcSizeTooLarge or DstMaxSizeTooSmall
    int64_t err;        // decode: the frame's error after the fold (first defect in stream order, then the capacity)
    uint64_t total;     // decode: decoded bytes
};

__device__ __forceinline__ bool lf_fits(const LFrame &F, uint32_t max_blocks) { return F.nb == 0 || F.base + F.nb <= max_blocks; }

inline bool lf_misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// exclusive scan of fr[].nb into fr[].base (k_bf_scan of zlz4_frame.hip on this file's record): one workgroup, thread t sums
// a contiguous run of frames, the 1024 run sums are scanned in LDS, then every thread writes its run's bases
__global__ __launch_bounds__(1024) void k_lf_scan(LFrame *__restrict__ fr, uint32_t nframes) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (nframes + 1023u) / 1024u;
    const uint64_t b0 = (uint64_t)t * chunk;
    const uint32_t lo = b0 < nframes ? (uint32_t)b0 : nframes;
    const uint32_t hi = b0 + chunk < nframes ? (uint32_t)(b0 + chunk) : nframes;
    uint64_t s = 0;
    for (uint32_t f = lo; f < hi; f++) s += fr[f].nb;
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - s;
    for (uint32_t f = lo; f < hi; f++) { fr[f].base = run; run += fr[f].nb; }
}

// One step of a wavefront's walk over a frame's entries, 64 at a time: `run` bytes stand in front of the 64, this lane's
// entry takes `bytes` (0 for a lane without one; 64 entries stay below 2^32) -> what stands in front of this lane's entry.
__device__ __forceinline__ uint64_t lf_place(uint32_t bytes, uint64_t &run) {
    const uint32_t incl = zlz4::wave_incl_scan(bytes);
    const uint64_t front = run + (incl - bytes);
    run += zlz4::rdlane(incl, 63);
    return front;
}

// ====================================================================== decode side
// One lane per frame, a dependent 4-byte load per block (DESIGN.md section 4.4h says why not a wavefront per frame).  The
// counting pass leaves the block count, the verdict and `consumed`; the record pass writes the blocks of every frame that
// fits the table at its base.
template <bool kRecord>
__global__ __launch_bounds__(64) void k_lf_walk(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                const uint64_t *__restrict__ src_len, uint32_t nframes, uint32_t max_blocks,
                                                LFrame *__restrict__ fr, uint64_t *__restrict__ nblocks,
                                                uint64_t *__restrict__ consumed, unsigned long long *__restrict__ totals,
                                                uint64_t *__restrict__ data_off, uint32_t *__restrict__ data_len) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long blocks = 0;
    if (f < nframes) {
        const uint64_t so = src_off[f], n = src_len[f];
        uint64_t nb, end;
        if (kRecord) {
            const LFrame F = fr[f];
            if (F.nb != 0 && lf_fits(F, max_blocks))
                (void)legacy_walk(src + so, n, F.nb, nb, end, [&](uint64_t k, uint64_t off, uint32_t size) {
                    data_off[F.base + k] = so + off;                  // (the record pass never leaves the frame's range)
                    data_len[F.base + k] = size;
                });
        } else {
            const int64_t verdict = legacy_walk(src + so, n, ~0ull, nb, end, [](uint64_t, uint64_t, uint32_t) {});
            if (fr) { LFrame F = {}; F.nb = nb; F.status = verdict; fr[f] = F; }
            if (nblocks) nblocks[f] = nb;
            if (consumed) consumed[f] = end;
            blocks = nb;
        }
    }
    if (!kRecord && totals) {
        for (uint32_t d = 32u; d >= 1u; d >>= 1) blocks += __shfl_xor(blocks, (int)d);
        if ((threadIdx.x & 63u) == 0 && blocks) atomicAdd(&totals[0], blocks);
    }
}

// every entry empty: an entry no frame records stays so, and the block kernels answer 0 for it without a byte moved
__global__ void k_lf_init(uint32_t max_blocks, uint64_t *__restrict__ data_off, uint32_t *__restrict__ data_len,
                          uint64_t *__restrict__ out_off, uint32_t *__restrict__ out_cap) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        data_off[i] = 0; data_len[i] = 0;
        if (out_off) { out_off[i] = 0; out_cap[i] = 0; }
    }
}

// One wavefront per frame over the block sizes of its entries: the first-defect fold (a block that fails or decodes to
// more than 8 MiB stands in front of whatever ended the walk), the content size, and -- the decode -- each block's place
// inside the frame's slot, the capacity check, and the entries of a failed frame emptied so that nothing of it is written.
// The query writes its answer here; the decode's comes from k_lf_finish.
template <bool kQuery>
__global__ __launch_bounds__(256) void k_lf_plan(LFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                                                 const int64_t *__restrict__ sizes, const uint64_t *__restrict__ dst_off,
                                                 const uint64_t *__restrict__ dst_cap, uint32_t *__restrict__ data_len,
                                                 uint64_t *__restrict__ out_off, uint32_t *__restrict__ out_cap,
                                                 int64_t *__restrict__ result) {
    const uint32_t f = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (f >= nframes) return;
    const LFrame F = fr[f];
    int64_t err = F.status;
    uint64_t total = 0;
    if (!lf_fits(F, max_blocks)) err = ZLZ4_ERR_INVALID_STATE;
    else if (F.nb != 0) {
        const uint64_t o = kQuery ? 0 : dst_off[f];
        for (uint64_t b0 = 0; b0 < F.nb; b0 += 64u) {                  // (wave-uniform trip count)
            const uint64_t j = b0 + lane, i = F.base + j;
            const int64_t s = j < F.nb ? sizes[i] : 0;
            if (zlz4::ballot(s < 0 || s > (int64_t)ZLZ4F_LEGACY_BLOCK_SIZE) != 0) {      // (a size is at most 0xFFFFFFFF)
                err = ZLZ4F_ERR_DECOMPRESSION_FAILED;
                break;
            }
            const uint64_t front = lf_place((uint32_t)s, total);
            if (!kQuery && j < F.nb) { out_off[i] = o + front; out_cap[i] = (uint32_t)s; }
        }
        if (!kQuery) {
            if (!err && total > dst_cap[f]) err = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
            if (err)
                for (uint64_t j = lane; j < F.nb; j += 64u) { data_len[F.base + j] = 0; out_cap[F.base + j] = 0; }
        }
    }
    if (lane == 0) {
        if (kQuery) result[f] = err ? err : (int64_t)total;
        else { fr[f].err = err; fr[f].total = total; }
    }
}

// one wavefront per frame: the frame's error, or its size once every block decoded to the size the query gave it
__global__ __launch_bounds__(256) void k_lf_finish(const LFrame *__restrict__ fr, uint32_t nframes,
                                                   const int64_t *__restrict__ sizes, const int64_t *__restrict__ decoded,
                                                   int64_t *__restrict__ result) {
    const uint32_t f = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (f >= nframes) return;
    const LFrame F = fr[f];
    int64_t out = F.err ? F.err : (int64_t)F.total;
    if (!F.err) {
        bool same = true;
        for (uint64_t j = lane; j < F.nb; j += 64u) same = same && decoded[F.base + j] == sizes[F.base + j];
        if (zlz4::ballot(!same) != 0) out = ZLZ4F_ERR_DECOMPRESSION_FAILED;
    }
    if (lane == 0) result[f] = out;
}

// ====================================================================== compress side
__host__ __device__ inline uint64_t lf_block_bound(uint64_t n) { return n + n / 255u + 16u; }      // zlz4_compress_bound
// zlz4f_legacy_compress_frame_bound: the magic, then a size word and a compressBound per chunk of bs bytes
__host__ __device__ inline uint64_t lf_frame_bound(uint64_t n, uint64_t bs) {
    const uint64_t rest = n % bs;
    return 4u + (n / bs) * (4u + lf_block_bound(bs)) + (rest ? 4u + lf_block_bound(rest) : 0u);
}

// one lane per frame: block count, then the refusals a frame can earn on its own
__global__ void k_lfc_count(const uint64_t *__restrict__ src_len, const uint64_t *__restrict__ dst_cap, uint32_t nframes,
                            uint64_t bs, LFrame *__restrict__ fr) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const uint64_t n = src_len[f];
    LFrame F = {};
    if (n > ZLZ4_MAX_INPUT_SIZE) F.status = ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    else {
        F.nb = n / bs + (n % bs != 0);
        if (dst_cap[f] < lf_frame_bound(n, bs)) F.status = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
    }
    fr[f] = F;
}

// one lane per table entry: its frame (the last frame whose base is <= i: frames without blocks share the next frame's
// base), the chunk's source range and its workspace slot.  Entries of refused frames and unused entries get length 0.
__global__ void k_lfc_desc(const LFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                           const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ src_len, uint64_t bs,
                           uint64_t slot, uint64_t *__restrict__ in_off, uint32_t *__restrict__ in_len,
                           uint64_t *__restrict__ out_off, uint32_t *__restrict__ out_cap, uint32_t *__restrict__ csz) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = nframes;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (fr[mid].base <= i) lo = mid + 1u; else hi = mid;
        }
        uint64_t o = 0;
        uint32_t len = 0;
        if (lo > 0) {
            const uint32_t f = lo - 1u;
            const LFrame F = fr[f];
            const uint64_t k = i - F.base;
            if (k < F.nb && F.status == 0 && lf_fits(F, max_blocks)) {
                const uint64_t n = src_len[f], b = k * bs;
                len = (uint32_t)((n - b) < bs ? (n - b) : bs);
                o = src_off[f] + b;
            }
        }
        in_off[i] = o;
        in_len[i] = len;
        out_off[i] = (uint64_t)i * slot;
        out_cap[i] = (uint32_t)slot;
        csz[i] = 0;
    }
}

// One wavefront per frame: the frame's refusal, or the prefix sums of 4 + csize over its entries -- where each size word
// goes in dst, csz[i] = the word -- the magic and the frame's size; a block whose compressor failed gives the frame its code
// (the first such block's) and leaves csz of all the frame's entries 0, so that the scatter writes nothing of it.
__global__ __launch_bounds__(256) void k_lfc_plan(const LFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                                                  const int64_t *__restrict__ csize, const uint64_t *__restrict__ dst_off_f,
                                                  uint8_t *__restrict__ dst, uint64_t *__restrict__ dst_off,
                                                  uint32_t *__restrict__ csz, int64_t *__restrict__ result) {
    const uint32_t f = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (f >= nframes) return;
    const LFrame F = fr[f];
    int64_t err = F.status;
    if (!err && !lf_fits(F, max_blocks)) err = ZLZ4_ERR_INVALID_STATE;
    uint64_t total = 4;
    if (!err) {
        const uint64_t o = dst_off_f[f];
        for (uint64_t b0 = 0; b0 < F.nb; b0 += 64u) {                  // (wave-uniform trip count)
            const uint64_t j = b0 + lane, i = F.base + j;
            const int64_t c = j < F.nb ? csize[i] : 0;
            const uint64_t bad = zlz4::ballot(c < 0);
            if (bad != 0) {
                err = (int64_t)(int32_t)zlz4::rdlane((uint32_t)c, zlz4::first_lane(bad));
                break;
            }
            const uint64_t front = lf_place(j < F.nb ? 4u + (uint32_t)c : 0u, total);
            if (j < F.nb) { dst_off[i] = o + front; csz[i] = (uint32_t)c; }
        }
        if (err)
            for (uint64_t j = lane; j < F.nb; j += 64u) csz[F.base + j] = 0;
        else if (lane < 4u)
            dst[o + lane] = (uint8_t)(ZLZ4F_LEGACY_MAGICNUMBER >> (8u * lane));
    }
    if (lane == 0) result[f] = err ? err : (int64_t)total;
}

// The scatter: entry i's size word and block from its 16-aligned workspace slot to dst_off[i], which has any alignment.
// blockIdx.x = the entry, blockIdx.y = a 64 KiB segment of the block (256 lanes x 16 bytes x 16 steps), so that an 8 MiB
// block is the work of 129 workgroups and a 4 KiB one of a single one.  The destination decides the split: the bytes in
// front of its first 16-aligned address and behind its last one go out one per lane with segment 0, everything between
// as aligned 16-byte stores of unaligned 16-byte loads.  Entries without a block (csz 0: every block has at least its
// token) write nothing.
constexpr uint32_t kScatterSeg = 65536u;

__global__ __launch_bounds__(256) void k_lfc_scatter(const uint8_t *__restrict__ slots, const uint64_t *__restrict__ slot_off,
                                                     const uint32_t *__restrict__ csz, const uint64_t *__restrict__ dst_off,
                                                     uint8_t *__restrict__ dst) {
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    const uint32_t n = csz[i];
    if (n == 0) return;
    const uint8_t *p = slots + slot_off[i];
    uint8_t *o = dst + dst_off[i], *q = o + 4;
    const uint32_t to16 = (uint32_t)(-reinterpret_cast<uintptr_t>(q) & 15u);
    const uint32_t head = to16 < n ? to16 : n, body = (n - head) & ~15u, tail = n - head - body;
    if (blockIdx.y == 0) {
        if (t < 4u) o[t] = (uint8_t)(n >> (8u * t));
        else if (t >= 16u && t < 16u + head) q[t - 16u] = p[t - 16u];
        else if (t >= 32u && t < 32u + tail) q[head + body + (t - 32u)] = p[head + body + (t - 32u)];
    }
    const uint32_t s0 = blockIdx.y * kScatterSeg;
    if (s0 >= body) return;
    const uint32_t s1 = body - s0 < kScatterSeg ? body : s0 + kScatterSeg;
    for (uint32_t k = s0 + t * 16u; k < s1; k += 256u * 16u)
        *reinterpret_cast<zlz4::u32x4 *>(q + head + k) = zlz4::ld128(p + head + k);
}

// ====================================================================== layouts and arguments
int32_t lf_hc_level(const zlz4f_legacy_prefs &p) {    // as zlz4_batch_compress_hc reads a level; 0 = the fast level
    if (p.compression_level <= 0) return 0;
    return p.compression_level < ZLZ4HC_CLEVEL_MIN ? ZLZ4HC_CLEVEL_DEFAULT
                                                   : (p.compression_level > ZLZ4HC_CLEVEL_MAX ? ZLZ4HC_CLEVEL_MAX : p.compression_level);
}

// 0 for a block_size the format has no room for
uint32_t lf_block_size(const zlz4f_legacy_prefs &p) {
    return p.block_size == 0 ? ZLZ4F_LEGACY_BLOCK_SIZE : (p.block_size <= ZLZ4F_LEGACY_BLOCK_SIZE ? p.block_size : 0u);
}

uint64_t lf_slot(uint32_t bs) { return (lf_block_bound(bs) + 15u) & ~15ull; }

constexpr zlz4f_legacy_prefs kDefaultLegacyPrefs = {0, 0};

struct LfcLayout {
    Region<LFrame> frames;
    Region<uint64_t> in_off, out_off, dst_off;
    Region<uint32_t> in_len, out_cap, csz;
    Region<int64_t> csize;
    Region<uint8_t> slots, hc;
    size_t bytes = 0;
};

LfcLayout lfc_layout(uint32_t nframes, uint32_t max_blocks, const zlz4f_legacy_prefs &p, void *ws = nullptr) {
    const uint32_t bs = lf_block_size(p);
    const size_t m = max_blocks;
    LfcLayout L;
    Carver c{static_cast<uint8_t *>(ws)};
    c.take(nframes, L.frames);
    c.take(m, L.in_off, L.out_off, L.dst_off, L.in_len, L.out_cap, L.csz, L.csize);
    c.take(m * lf_slot(bs), L.slots);
    c.take(lf_hc_level(p) ? zlz4_hc_workspace_bytes(max_blocks, bs) : 0, L.hc);
    L.bytes = c.bytes;
    return L;
}

// the size query and the decode share the walk's table; the decode adds where the blocks go and what they decoded to
struct LfdLayout {
    Region<LFrame> frames;
    Region<uint64_t> data_off, out_off;
    Region<uint32_t> data_len, out_cap;
    Region<int64_t> sizes, decoded;
    size_t bytes = 0;
};

LfdLayout lfd_layout(uint32_t nframes, uint32_t max_blocks, bool query, void *ws = nullptr) {
    const size_t m = max_blocks;
    LfdLayout L;
    Carver c{static_cast<uint8_t *>(ws)};
    c.take(nframes, L.frames);
    c.take(m, L.data_off);
    if (!query) c.take(m, L.out_off);
    c.take(m, L.data_len);
    if (!query) c.take(m, L.out_cap);
    c.take(m, L.sizes);
    if (!query) c.take(m, L.decoded);
    L.bytes = c.bytes;
    return L;
}

struct LfArrays {
    const uint8_t *src; const uint64_t *src_off, *src_len;
    uint8_t *dst; const uint64_t *dst_off, *dst_cap;
    int64_t *result; uint64_t *consumed; uint32_t nframes, max_blocks;
};

// the entry refusals of the three batch calls with a workspace: null or misaligned arrays (the query has no destination),
// then the workspace
bool lf_args_refused(const LfArrays &a, bool with_dst, const void *ws, size_t ws_bytes, size_t need) {
    if (!a.src || !a.src_off || !a.src_len || !a.result) return true;
    if (with_dst && (!a.dst || !a.dst_off || !a.dst_cap)) return true;
    if (lf_misaligned(a.src_off, 8) || lf_misaligned(a.src_len, 8) || lf_misaligned(a.result, 8) ||
        lf_misaligned(a.consumed, 8) || lf_misaligned(a.dst_off, 8) || lf_misaligned(a.dst_cap, 8))
        return true;
    return !ws || ws_bytes < need || lf_misaligned(ws, 16);
}

// walk (count, scan, record) and the block sizes: what the size query and the decode start with
int32_t lfd_open(hipStream_t st, const LfArrays &a, const LfdLayout &L) {
    const uint32_t g = grid_of(a.nframes, 64);
    hipLaunchKernelGGL(k_lf_walk<false>, dim3(g), dim3(64), 0, st, a.src, a.src_off, a.src_len, a.nframes, a.max_blocks,
                       L.frames.p, (uint64_t *)nullptr, a.consumed, (unsigned long long *)nullptr, (uint64_t *)nullptr,
                       (uint32_t *)nullptr);
    hipLaunchKernelGGL(k_lf_scan, dim3(1), dim3(1024), 0, st, L.frames.p, a.nframes);
    if (a.max_blocks == 0) return 0;
    hipLaunchKernelGGL(k_lf_init, dim3(grid_of(a.max_blocks, 256, 4096)), dim3(256), 0, st, a.max_blocks, L.data_off.p,
                       L.data_len.p, L.out_off.p, L.out_cap.p);
    hipLaunchKernelGGL(k_lf_walk<true>, dim3(g), dim3(64), 0, st, a.src, a.src_off, a.src_len, a.nframes, a.max_blocks,
                       L.frames.p, (uint64_t *)nullptr, (uint64_t *)nullptr, (unsigned long long *)nullptr, L.data_off.p,
                       L.data_len.p);
    return zlz4_launch_decompressed_size(st, a.src, L.data_off, L.data_len, nullptr, L.sizes, a.max_blocks);
}

}  // namespace

extern "C" {

size_t zlz4f_legacy_compress_frame_bound(size_t src_size, const zlz4f_legacy_prefs *prefs) {
    const uint32_t bs = lf_block_size(prefs ? *prefs : kDefaultLegacyPrefs);
    return bs ? (size_t)lf_frame_bound(src_size, bs) : 0;
}

size_t zlz4f_batch_compress_legacy_frame_workspace(uint32_t nframes, uint32_t max_blocks, const zlz4f_legacy_prefs *prefs) {
    const zlz4f_legacy_prefs p = prefs ? *prefs : kDefaultLegacyPrefs;
    return lf_block_size(p) ? lfc_layout(nframes, max_blocks, p).bytes : 0;
}

int32_t zlz4f_batch_compress_legacy_frame(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                          const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                          const uint64_t *d_dst_cap, int64_t *d_result, uint32_t nframes, uint32_t max_blocks,
                                          const zlz4f_legacy_prefs *prefs, void *d_workspace, size_t workspace_bytes) {
    const zlz4f_legacy_prefs p = prefs ? *prefs : kDefaultLegacyPrefs;
    const uint32_t bs = lf_block_size(p);
    if (bs == 0) return ZLZ4F_ERR_MAX_BLOCK_SIZE_INVALID;
    if (nframes == 0) return 0;
    const LfArrays a = {d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_result, nullptr, nframes, max_blocks};
    const LfcLayout L = lfc_layout(nframes, max_blocks, p, d_workspace);
    if (lf_args_refused(a, true, d_workspace, workspace_bytes, L.bytes)) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lfc_count, dim3(grid_of(nframes, 256)), dim3(256), 0, st, d_src_len, d_dst_cap, nframes, (uint64_t)bs,
                       L.frames.p);
    hipLaunchKernelGGL(k_lf_scan, dim3(1), dim3(1024), 0, st, L.frames.p, nframes);
    if (max_blocks) {
        const uint64_t slot = lf_slot(bs);
        hipLaunchKernelGGL(k_lfc_desc, dim3(grid_of(max_blocks, 256, 4096)), dim3(256), 0, st, L.frames.p, nframes, max_blocks,
                           d_src_off, d_src_len, (uint64_t)bs, slot, L.in_off.p, L.in_len.p, L.out_off.p, L.out_cap.p, L.csz.p);
        const int32_t level = lf_hc_level(p);
        const int rc = level == 0 ? zlz4_launch_compress_fast(st, d_src, L.in_off, L.in_len, L.slots, L.out_off, L.out_cap,
                                                              L.csize, max_blocks, bs, 1)
                                  : zlz4_launch_compress_hc(st, d_src, L.in_off, L.in_len, L.slots, L.out_off, L.out_cap,
                                                            L.csize, max_blocks, bs, level, L.hc, L.hc.bytes);
        if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(k_lfc_plan, dim3(grid_of(nframes, 4)), dim3(256), 0, st, L.frames.p, nframes, max_blocks, L.csize.p,
                       d_dst_off, d_dst, L.dst_off.p, L.csz.p, d_result);
    if (max_blocks)
        hipLaunchKernelGGL(k_lfc_scatter, dim3(max_blocks, grid_of(lf_slot(bs), kScatterSeg)), dim3(256), 0, st, L.slots.p,
                           L.out_off.p, L.csz.p, L.dst_off.p, d_dst);
    return zlz4_launch_status();
}

int32_t zlz4f_batch_legacy_frame_count(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                       const uint64_t *d_src_len, uint32_t nframes, uint64_t *d_nblocks, uint64_t *d_consumed,
                                       uint64_t *d_totals) {
    if (!d_totals || lf_misaligned(d_totals, 8)) return ZLZ4_ERR_INVALID_STATE;
    if (nframes && (!d_src || !d_src_off || !d_src_len || !d_nblocks)) return ZLZ4_ERR_INVALID_STATE;
    if (lf_misaligned(d_src_off, 8) || lf_misaligned(d_src_len, 8) || lf_misaligned(d_nblocks, 8) ||
        lf_misaligned(d_consumed, 8))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_totals, 0, 8, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
    if (nframes == 0) return 0;
    hipLaunchKernelGGL(k_lf_walk<false>, dim3(grid_of(nframes, 64)), dim3(64), 0, st, d_src, d_src_off, d_src_len, nframes, 0u,
                       (LFrame *)nullptr, d_nblocks, d_consumed, reinterpret_cast<unsigned long long *>(d_totals),
                       (uint64_t *)nullptr, (uint32_t *)nullptr);
    return zlz4_launch_status();
}

size_t zlz4f_batch_legacy_frame_decompressed_size_workspace(uint32_t nframes, uint32_t max_blocks) {
    return lfd_layout(nframes, max_blocks, true).bytes;
}

int32_t zlz4f_batch_legacy_frame_decompressed_size(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                                   const uint64_t *d_src_len, int64_t *d_size, uint64_t *d_consumed,
                                                   uint32_t nframes, uint32_t max_blocks, void *d_workspace,
                                                   size_t workspace_bytes) {
    if (nframes == 0) return 0;
    const LfArrays a = {d_src, d_src_off, d_src_len, nullptr, nullptr, nullptr, d_size, d_consumed, nframes, max_blocks};
    const LfdLayout L = lfd_layout(nframes, max_blocks, true, d_workspace);
    if (lf_args_refused(a, false, d_workspace, workspace_bytes, L.bytes)) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const int32_t rc = lfd_open(st, a, L);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(k_lf_plan<true>, dim3(grid_of(nframes, 4)), dim3(256), 0, st, L.frames.p, nframes, max_blocks,
                       L.sizes.p, (const uint64_t *)nullptr, (const uint64_t *)nullptr, (uint32_t *)nullptr,
                       (uint64_t *)nullptr, (uint32_t *)nullptr, d_size);
    return zlz4_launch_status();
}

size_t zlz4f_batch_decompress_legacy_frame_workspace(uint32_t nframes, uint32_t max_blocks) {
    return lfd_layout(nframes, max_blocks, false).bytes;
}

int32_t zlz4f_batch_decompress_legacy_frame(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                            const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                            const uint64_t *d_dst_cap, int64_t *d_result, uint64_t *d_consumed,
                                            uint32_t nframes, uint32_t max_blocks, void *d_workspace, size_t workspace_bytes) {
    if (nframes == 0) return 0;
    const LfArrays a = {d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_result, d_consumed, nframes, max_blocks};
    const LfdLayout L = lfd_layout(nframes, max_blocks, false, d_workspace);
    if (lf_args_refused(a, true, d_workspace, workspace_bytes, L.bytes)) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    int32_t rc = lfd_open(st, a, L);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(k_lf_plan<false>, dim3(grid_of(nframes, 4)), dim3(256), 0, st, L.frames.p, nframes, max_blocks,
                       L.sizes.p, d_dst_off, d_dst_cap, L.data_len.p, L.out_off.p, L.out_cap.p, (int64_t *)nullptr);
    if (max_blocks) {
        rc = zlz4_launch_decompress_safe(st, d_src, L.data_off, L.data_len, d_dst, L.out_off, L.out_cap, L.decoded, max_blocks);
        if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(k_lf_finish, dim3(grid_of(nframes, 4)), dim3(256), 0, st, L.frames.p, nframes, L.sizes.p, L.decoded.p,
                       d_result);
    return zlz4_launch_status();
}

}  // extern "C"

// ====================================================================== one frame in host memory
namespace {

struct LegacyRec { uint64_t src_off, src_len, dst_off, dst_cap, consumed; int64_t result; };

// The size query (dst null) or the decode of one frame as a batch of one.  The walk runs here first, on the host bytes:
// step 1 of the read rules is answered before the device check, and the block count sizes the table.
int64_t host_legacy_decode(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, bool want_size, size_t *consumed) {
    if ((!src && n) || (!want_size && !dst && cap)) return ZLZ4_ERR_INVALID_STATE;
    uint64_t nb = 0, end = 0;
    const int64_t verdict = legacy_walk(src, n, ~0ull, nb, end, [](uint64_t, uint64_t, uint32_t) {});
    if (consumed) *consumed = (size_t)end;
    if (nb == 0 && verdict != 0) return verdict;                       // step 1, and a defect in front of the first block
    if (nb > 0xFFFFFFFFull) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    const uint32_t max_blocks = (uint32_t)nb;
    const uint64_t most = nb * (uint64_t)ZLZ4F_LEGACY_BLOCK_SIZE;      // no frame of nb blocks holds more
    const size_t d_cap = want_size ? 0 : (cap < most ? cap : (size_t)most);
    const size_t wsn = want_size ? zlz4f_batch_legacy_frame_decompressed_size_workspace(1, max_blocks)
                                 : zlz4f_batch_decompress_legacy_frame_workspace(1, max_blocks);
    DevBuf d_src(n, &dc), d_dst(d_cap, &dc), d_ws(wsn, &dc);
    Staged<LegacyRec> rec(&dc);
    if (!d_src.p || !d_dst.p || !d_ws.p || !rec.d) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.src_len = n;
    rec.h.dst_cap = cap;
    dc.launched();
    if (!upload(d_src, src, n, st) || !rec.upload(st)) return ZLZ4_ERR_DEVICE;
    LegacyRec *r = rec.d;
    const int32_t rc =
        want_size ? zlz4f_batch_legacy_frame_decompressed_size(st, d_src.as<uint8_t>(), &r->src_off, &r->src_len, &r->result,
                                                               &r->consumed, 1, max_blocks, d_ws.p, d_ws.n)
                  : zlz4f_batch_decompress_legacy_frame(st, d_src.as<uint8_t>(), &r->src_off, &r->src_len, d_dst.as<uint8_t>(),
                                                        &r->dst_off, &r->dst_cap, &r->result, &r->consumed, 1, max_blocks,
                                                        d_ws.p, d_ws.n);
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result)) return ZLZ4_ERR_DEVICE;
    if (!want_size && !copy_back(dst, cap, d_dst, result)) return ZLZ4_ERR_DEVICE;
    return result;
}

}  // namespace

extern "C" {

int64_t zlz4f_compress_legacy_frame(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const zlz4f_legacy_prefs *prefs) {
    if ((!src && n) || (!dst && cap)) return ZLZ4_ERR_INVALID_STATE;
    const zlz4f_legacy_prefs p = prefs ? *prefs : kDefaultLegacyPrefs;
    const uint32_t bs = lf_block_size(p);
    if (bs == 0) return ZLZ4F_ERR_MAX_BLOCK_SIZE_INVALID;
    const size_t bound = (size_t)lf_frame_bound(n, bs);
    if (n > ZLZ4_MAX_INPUT_SIZE) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;     // (k_lfc_count's two refusals: nothing to stage)
    if (cap < bound) return ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    const uint32_t max_blocks = (uint32_t)(n / bs + (n % bs != 0));
    DevBuf d_src(n, &dc), d_dst(bound, &dc), d_ws(zlz4f_batch_compress_legacy_frame_workspace(1, max_blocks, &p), &dc);
    Staged<LegacyRec> rec(&dc);
    if (!d_src.p || !d_dst.p || !d_ws.p || !rec.d) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.src_len = n;
    rec.h.dst_cap = cap;
    dc.launched();
    if (!upload(d_src, src, n, st) || !rec.upload(st)) return ZLZ4_ERR_DEVICE;
    LegacyRec *r = rec.d;
    const int32_t rc = zlz4f_batch_compress_legacy_frame(st, d_src.as<uint8_t>(), &r->src_off, &r->src_len, d_dst.as<uint8_t>(),
                                                         &r->dst_off, &r->dst_cap, &r->result, 1, max_blocks, &p, d_ws.p,
                                                         d_ws.n);
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result)) return ZLZ4_ERR_DEVICE;
    if (!copy_back(dst, cap, d_dst, result)) return ZLZ4_ERR_DEVICE;
    return result;
}

int64_t zlz4f_legacy_frame_decompressed_size(const uint8_t *src, size_t n, size_t *consumed) {
    return host_legacy_decode(src, n, nullptr, 0, true, consumed);
}

int64_t zlz4f_decompress_legacy_frame(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *consumed) {
    return host_legacy_decode(src, n, dst, cap, false, consumed);
}

}  // extern "C"
