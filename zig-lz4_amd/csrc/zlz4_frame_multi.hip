// zlz4_frame_multi.hip -- multiframe buffers (include/zlz4_amd.h): a buffer holds zero or more lz4
// frames and skippable frames back to back, its MEMBERS.  The split delimits the members of every buffer and writes them as
// the item arrays of the batch frame calls; the size query and the decode are those calls, unchanged, over the items; the
// plan packs the items of one buffer into one run of bytes and the finish folds the item results into one per buffer.
// Every call is a fixed sequence of kernels on the caller's stream: nothing allocated, nothing read back.
// With ZLZ4F_SPLIT_LEGACY (the _ex calls, section 4.4j) a legacy frame is a member too: the split writes its length to a
// second length array, the legacy frame calls run over the same items, and the select merges the two families' answers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zlz4_frame_batch.hpp"
#include "zlz4_host.hpp"
#include "zlz4_launch.hpp"

using namespace zlz4host;

namespace {

inline bool mf_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

// ------------------------------------------------------------------ split
// One lane per buffer, a dependent 4-byte load per block (DESIGN.md section 4.4h says why not a wavefront per buffer).
// The counting pass leaves count[s] and adds the members and chain blocks of the wave to totals; the record pass writes
// the member entries, the item arrays and the buffer's result.  kLegacy: ZLZ4F_SPLIT_LEGACY (section 4.4j) -- legacy
// members are delimited, counted into totals[2] and totals[3], and their lengths go to leg_len.  Without it the legacy
// branch of mf_member is compiled out, totals has two entries and leg_len, where the _ex call passes one, gets zeros.
template <bool kRecord, bool kLegacy>
__global__ __launch_bounds__(64) void k_mf_split(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                 const uint64_t *__restrict__ src_len, uint32_t nbuf,
                                                 uint64_t *__restrict__ count, unsigned long long *__restrict__ totals,
                                                 zlz4f_member *__restrict__ member, const uint64_t *__restrict__ mem_off,
                                                 const uint64_t *__restrict__ mem_cap, const uint64_t *__restrict__ item_first,
                                                 uint64_t *__restrict__ item_off, uint64_t *__restrict__ item_len,
                                                 uint64_t *__restrict__ leg_len, int64_t *__restrict__ result) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long members = 0, blocks = 0, leg_members = 0, leg_blocks = 0;
    if (b < nbuf) {
        const uint64_t so = src_off[b], n = src_len[b];
        const uint8_t *s = src + so;
        uint64_t first = 0;
        zlz4f_member *out = nullptr;
        if (kRecord) {
            first = item_first[b];
            const uint64_t cnt = count[b];
            if (cnt <= mem_cap[b]) { out = member + mem_off[b]; result[b] = (int64_t)cnt; }
            else result[b] = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
        }
        const uint64_t room = kRecord ? count[b] : ~0ull;             // (the record pass never leaves the buffer's items)
        uint64_t pos = 0;
        while (pos < n && members < room) {
            const MfMember m = mf_member(s + pos, n - pos, kLegacy ? ZLZ4F_SPLIT_LEGACY : 0u);
            const bool legacy = kLegacy && m.kind == ZLZ4F_MEMBER_LEGACY;
            if (kRecord) {
                const bool frame = (m.kind & 0xFFu) == ZLZ4F_MEMBER_FRAME;
                item_off[first + members] = so + pos;
                item_len[first + members] = out && frame ? m.len : 0u;
                if (leg_len) leg_len[first + members] = out && legacy ? m.len : 0u;
                if (out) {
                    zlz4f_member e;
                    e.pos = pos; e.len = m.len; e.kind = m.kind; e.buf = b;
                    out[members] = e;
                }
            }
            members++;
            if (legacy) { leg_members++; leg_blocks += m.nb; }
            else blocks += m.nb;
            pos += m.len;
            if (m.last) break;
        }
        if (!kRecord) count[b] = members;
    }
    if (!kRecord) {
        for (uint32_t d = 32u; d >= 1u; d >>= 1) {
            members += __shfl_xor(members, (int)d);
            blocks += __shfl_xor(blocks, (int)d);
            if (kLegacy) {
                leg_members += __shfl_xor(leg_members, (int)d);
                leg_blocks += __shfl_xor(leg_blocks, (int)d);
            }
        }
        if ((threadIdx.x & 63u) == 0 && (members | blocks)) {
            atomicAdd(&totals[0], members);
            atomicAdd(&totals[1], blocks);
            if (kLegacy && leg_members) {
                atomicAdd(&totals[2], leg_members);
                atomicAdd(&totals[3], leg_blocks);
            }
        }
    }
}

// exclusive scan of 1024 per-thread sums in LDS: returns what stands in front of thread t, total = the sum of all
__device__ uint64_t mf_wg_scan(uint64_t s, uint64_t *part, uint64_t &total) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    total = part[1023];
    return part[t] - s;
}

// one workgroup: out[0..n] = the exclusive scan of in[0..n) rounded up to `align` (a power of two), out[n] = the total;
// thread t owns a contiguous run of entries.  `out` has n or n + 1 entries (with_end); totals = { that total, the sum of
// in[] as it stands }.
__global__ __launch_bounds__(1024) void k_mf_scan(const uint64_t *__restrict__ in, uint32_t n, uint64_t align, int with_end,
                                                  uint64_t *__restrict__ out, uint64_t *__restrict__ totals) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + 1023u) / 1024u;
    const uint64_t b0 = (uint64_t)t * chunk;
    const uint32_t lo = b0 < n ? (uint32_t)b0 : n;
    const uint32_t hi = b0 + chunk < n ? (uint32_t)(b0 + chunk) : n;
    auto slot = [&](uint64_t c) -> uint64_t { return (c + (align - 1u)) & ~(align - 1u); };
    uint64_t s = 0, raw = 0;
    for (uint32_t i = lo; i < hi; i++) { s += slot(in[i]); raw += in[i]; }
    uint64_t total, raw_total;
    (void)mf_wg_scan(raw, part, raw_total);
    uint64_t run = mf_wg_scan(s, part, total);
    for (uint32_t i = lo; i < hi; i++) { const uint64_t c = slot(in[i]); out[i] = run; run += c; }
    if (t == 0) {
        if (with_end) out[n] = total;
        if (totals) { totals[0] = total; totals[1] = raw_total; }
    }
}

// ------------------------------------------------------------------ plan
// one wavefront per buffer: out_size[s] = the sum of its items' sizes (an item whose size query failed, or a skippable
// one -- its item has length 0, which the query answers with FrameHeaderIncomplete -- takes no room)
__global__ __launch_bounds__(256) void k_mf_plan_sum(const int64_t *__restrict__ size, const uint64_t *__restrict__ item_first,
                                                     uint32_t nbuf, uint64_t *__restrict__ out_size) {
    const uint32_t b = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (b >= nbuf) return;
    const uint64_t i0 = item_first[b], i1 = item_first[b + 1];
    unsigned long long sum = 0;
    for (uint64_t i = i0 + lane; i < i1; i += 64u) { const int64_t v = size[i]; sum += v > 0 ? (uint64_t)v : 0u; }
    for (uint32_t d = 32u; d >= 1u; d >>= 1) sum += __shfl_xor(sum, (int)d);
    if (lane == 0) out_size[b] = sum;
}

// one wavefront per buffer: its items back to back from out_off[s], in member order
__global__ __launch_bounds__(256) void k_mf_plan_items(const int64_t *__restrict__ size, const uint64_t *__restrict__ item_first,
                                                       const uint64_t *__restrict__ out_off, uint32_t nbuf,
                                                       uint64_t *__restrict__ dst_off, uint64_t *__restrict__ dst_cap) {
    const uint32_t b = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (b >= nbuf) return;
    const uint64_t i0 = item_first[b], i1 = item_first[b + 1];
    uint64_t run = out_off[b];
    for (uint64_t base = i0; base < i1; base += 64u) {                // (wave-uniform trip count)
        const uint64_t i = base + lane;
        const int64_t v = i < i1 ? size[i] : 0;
        const unsigned long long c = v > 0 ? (uint64_t)v : 0u;
        unsigned long long incl = c;
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (i < i1) { dst_off[i] = run + (incl - c); dst_cap[i] = c; }
        run += __shfl(incl, 63);
    }
}

// ------------------------------------------------------------------ finish
// one wavefront per buffer: the first member in member order that is not OK decides, else the sum of the decoded sizes
__global__ __launch_bounds__(256) void k_mf_finish(const zlz4f_member *__restrict__ member, const uint64_t *__restrict__ mem_off,
                                                   const int64_t *__restrict__ split_result,
                                                   const uint64_t *__restrict__ item_first, const int64_t *__restrict__ size,
                                                   const int64_t *__restrict__ item_result, uint32_t nbuf,
                                                   int64_t *__restrict__ result) {
    const uint32_t b = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (b >= nbuf) return;
    const int64_t sr = split_result[b];
    if (sr < 0) { if (lane == 0) result[b] = sr; return; }
    const uint64_t i0 = item_first[b], cnt = item_first[b + 1] - i0;
    const zlz4f_member *m = member + mem_off[b];
    unsigned long long sum = 0, bad = ~0ull;
    int64_t code = 0;
    for (uint64_t k = lane; k < cnt && bad == ~0ull; k += 64u) {
        const uint32_t kind = m[k].kind & 0xFFu;
        int64_t r = 0;
        if (kind == ZLZ4F_MEMBER_FRAME || kind == ZLZ4F_MEMBER_LEGACY) {
            const int64_t q = size[i0 + k];
            r = q < 0 ? q : item_result[i0 + k];
        } else if (kind == ZLZ4F_MEMBER_SKIPPABLE_TRUNCATED) {
            r = m[k].len < 8 ? ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE : ZLZ4F_ERR_FRAME_SIZE_WRONG;
        }
        if (r < 0) { bad = k; code = r; } else sum += (uint64_t)r;
    }
    unsigned long long first = bad;
    for (uint32_t d = 32u; d >= 1u; d >>= 1) {
        const unsigned long long o = __shfl_xor(first, (int)d);
        first = o < first ? o : first;
    }
    if (first != ~0ull) {
        if (bad == first) result[b] = code;                            // (one lane: member indexes differ from lane to lane)
        return;
    }
    for (uint32_t d = 32u; d >= 1u; d >>= 1) sum += __shfl_xor(sum, (int)d);
    if (lane == 0) result[b] = (int64_t)sum;
}

// ------------------------------------------------------------------ select
// one wavefront per buffer: every item takes the legacy call's answer where the split recorded a legacy member, else the
// frame call's -- also for a buffer without a member table (a split result < 0).  out may be from_frame itself.
__global__ __launch_bounds__(256) void k_mf_select(const zlz4f_member *__restrict__ member, const uint64_t *__restrict__ mem_off,
                                                   const int64_t *__restrict__ split_result,
                                                   const uint64_t *__restrict__ item_first, const int64_t *from_frame,
                                                   const int64_t *__restrict__ from_legacy, uint32_t nbuf, int64_t *out) {
    const uint32_t b = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (b >= nbuf) return;
    const bool table = split_result[b] >= 0;
    const uint64_t i0 = item_first[b], cnt = item_first[b + 1] - i0;
    const zlz4f_member *m = member + mem_off[b];
    for (uint64_t k = lane; k < cnt; k += 64u) {
        const bool legacy = table && (m[k].kind & 0xFFu) == ZLZ4F_MEMBER_LEGACY;
        out[i0 + k] = legacy ? from_legacy[i0 + k] : from_frame[i0 + k];
    }
}

// The split of both entry points.  ex: zlz4f_batch_multiframe_split_ex -- four totals, and in record mode d_leg_len beside
// d_item_len; the caller has refused unknown split_flags bits.
int32_t mf_split(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len, uint32_t nbuf,
                 uint64_t *d_count, uint64_t *d_totals, zlz4f_member *d_member, const uint64_t *d_mem_off,
                 const uint64_t *d_mem_cap, uint64_t *d_item_first, uint64_t *d_item_off, uint64_t *d_item_len,
                 int64_t *d_result, bool ex, uint32_t split_flags, uint64_t *d_leg_len) {
    const bool record = d_member != nullptr;
    if (!d_totals || mf_misaligned(d_totals)) return ZLZ4_ERR_INVALID_STATE;
    if (nbuf && (!d_src || !d_src_off || !d_src_len || !d_count)) return ZLZ4_ERR_INVALID_STATE;
    if (nbuf && record && (!d_mem_off || !d_mem_cap || !d_item_first || !d_item_off || !d_item_len || !d_result ||
                           (ex && !d_leg_len)))
        return ZLZ4_ERR_INVALID_STATE;
    if (mf_misaligned(d_src_off) || mf_misaligned(d_src_len) || mf_misaligned(d_count) || mf_misaligned(d_member) ||
        (record && (mf_misaligned(d_mem_off) || mf_misaligned(d_mem_cap) || mf_misaligned(d_item_first) ||
                    mf_misaligned(d_item_off) || mf_misaligned(d_item_len) || mf_misaligned(d_result) ||
                    mf_misaligned(d_leg_len))))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_totals, 0, ex ? 32 : 16, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
    if (nbuf == 0) {
        if (record && d_item_first && hipMemsetAsync(d_item_first, 0, 8, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
        return 0;
    }
    unsigned long long *totals = reinterpret_cast<unsigned long long *>(d_totals);
    const uint32_t g = grid_of(nbuf, 64);
    const bool legacy = (split_flags & ZLZ4F_SPLIT_LEGACY) != 0;
    const auto k_count = legacy ? k_mf_split<false, true> : k_mf_split<false, false>;
    const auto k_record = legacy ? k_mf_split<true, true> : k_mf_split<true, false>;
    hipLaunchKernelGGL(k_count, dim3(g), dim3(64), 0, st, d_src, d_src_off, d_src_len, nbuf, d_count, totals, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (record) {
        hipLaunchKernelGGL(k_mf_scan, dim3(1), dim3(1024), 0, st, d_count, nbuf, (uint64_t)1, 1, d_item_first, nullptr);
        hipLaunchKernelGGL(k_record, dim3(g), dim3(64), 0, st, d_src, d_src_off, d_src_len, nbuf, d_count, totals, d_member,
                           d_mem_off, d_mem_cap, d_item_first, d_item_off, d_item_len, d_leg_len, d_result);
    }
    return zlz4_launch_status();
}

}  // namespace

extern "C" {

int32_t zlz4f_batch_multiframe_split(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                     uint32_t nbuf, uint64_t *d_count, uint64_t *d_totals, zlz4f_member *d_member,
                                     const uint64_t *d_mem_off, const uint64_t *d_mem_cap, uint64_t *d_item_first,
                                     uint64_t *d_item_off, uint64_t *d_item_len, int64_t *d_result) {
    return mf_split(stream, d_src, d_src_off, d_src_len, nbuf, d_count, d_totals, d_member, d_mem_off, d_mem_cap, d_item_first,
                    d_item_off, d_item_len, d_result, false, 0, nullptr);
}

int32_t zlz4f_batch_multiframe_split_ex(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                        const uint64_t *d_src_len, uint32_t nbuf, uint64_t *d_count, uint64_t *d_totals,
                                        zlz4f_member *d_member, const uint64_t *d_mem_off, const uint64_t *d_mem_cap,
                                        uint64_t *d_item_first, uint64_t *d_item_off, uint64_t *d_item_len, int64_t *d_result,
                                        uint32_t split_flags, uint64_t *d_leg_len) {
    if (split_flags & ~ZLZ4F_SPLIT_LEGACY) return ZLZ4F_ERR_PARAMETER_INVALID;
    return mf_split(stream, d_src, d_src_off, d_src_len, nbuf, d_count, d_totals, d_member, d_mem_off, d_mem_cap, d_item_first,
                    d_item_off, d_item_len, d_result, true, split_flags, d_leg_len);
}

int32_t zlz4f_batch_multiframe_select(void *stream, const zlz4f_member *d_member, const uint64_t *d_mem_off,
                                      const int64_t *d_split_result, const uint64_t *d_item_first, const int64_t *d_from_frame,
                                      const int64_t *d_from_legacy, uint32_t nbuf, int64_t *d_out) {
    if (nbuf == 0) return 0;
    if (!d_member || !d_mem_off || !d_split_result || !d_item_first || !d_from_frame || !d_from_legacy || !d_out)
        return ZLZ4_ERR_INVALID_STATE;
    if (mf_misaligned(d_member) || mf_misaligned(d_mem_off) || mf_misaligned(d_split_result) || mf_misaligned(d_item_first) ||
        mf_misaligned(d_from_frame) || mf_misaligned(d_from_legacy) || mf_misaligned(d_out))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipLaunchKernelGGL(k_mf_select, dim3(grid_of(nbuf, 4)), dim3(256), 0, (hipStream_t)stream, d_member, d_mem_off,
                       d_split_result, d_item_first, d_from_frame, d_from_legacy, nbuf, d_out);
    return zlz4_launch_status();
}

int32_t zlz4f_batch_multiframe_plan(void *stream, const int64_t *d_size, const uint64_t *d_item_first, uint32_t nbuf,
                                    uint32_t align, uint64_t *d_dst_off, uint64_t *d_dst_cap, uint64_t *d_out_off,
                                    uint64_t *d_out_size, uint64_t *d_totals) {
    if (align > 4096u || (align & (align - 1u))) return ZLZ4_ERR_INVALID_STATE;      // 0, 1 or a power of two up to 4096
    if (!d_totals || mf_misaligned(d_totals)) return ZLZ4_ERR_INVALID_STATE;
    if (nbuf && (!d_size || !d_item_first || !d_dst_off || !d_dst_cap || !d_out_off || !d_out_size))
        return ZLZ4_ERR_INVALID_STATE;
    if (mf_misaligned(d_size) || mf_misaligned(d_item_first) || mf_misaligned(d_dst_off) || mf_misaligned(d_dst_cap) ||
        mf_misaligned(d_out_off) || mf_misaligned(d_out_size))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (nbuf == 0) return hipMemsetAsync(d_totals, 0, 16, st) == hipSuccess ? 0 : ZLZ4_ERR_DEVICE;
    const uint32_t g = grid_of(nbuf, 4);
    hipLaunchKernelGGL(k_mf_plan_sum, dim3(g), dim3(256), 0, st, d_size, d_item_first, nbuf, d_out_size);
    hipLaunchKernelGGL(k_mf_scan, dim3(1), dim3(1024), 0, st, d_out_size, nbuf, (uint64_t)(align ? align : 1u), 0, d_out_off,
                       d_totals);
    hipLaunchKernelGGL(k_mf_plan_items, dim3(g), dim3(256), 0, st, d_size, d_item_first, d_out_off, nbuf, d_dst_off, d_dst_cap);
    return zlz4_launch_status();
}

int32_t zlz4f_batch_multiframe_finish(void *stream, const zlz4f_member *d_member, const uint64_t *d_mem_off,
                                      const int64_t *d_split_result, const uint64_t *d_item_first, const int64_t *d_size,
                                      const int64_t *d_item_result, uint32_t nbuf, int64_t *d_result) {
    if (nbuf == 0) return 0;
    if (!d_member || !d_mem_off || !d_split_result || !d_item_first || !d_size || !d_item_result || !d_result)
        return ZLZ4_ERR_INVALID_STATE;
    if (mf_misaligned(d_member) || mf_misaligned(d_mem_off) || mf_misaligned(d_split_result) || mf_misaligned(d_item_first) ||
        mf_misaligned(d_size) || mf_misaligned(d_item_result) || mf_misaligned(d_result))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipLaunchKernelGGL(k_mf_finish, dim3(grid_of(nbuf, 4)), dim3(256), 0, (hipStream_t)stream, d_member, d_mem_off,
                       d_split_result, d_item_first, d_size, d_item_result, nbuf, d_result);
    return zlz4_launch_status();
}

}  // extern "C"

// ====================================================================== one buffer in host memory
namespace {

// Count, record, size query, plan and -- with a destination -- decode and finish, as a batch of one.  want_size: the
// finish folds the size query's answers (what the decode returns into a destination that is large enough, the content
// checksums aside).  split_flags 0: the calls of section 4.4h and nothing else.  Otherwise the split is the _ex one, and
// where it finds legacy members the legacy size query and decode run over the same items and a select merges their
// answers with the frame calls' (section 4.4j).
int64_t host_multiframe(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, uint32_t decode_flags, uint32_t split_flags,
                        bool want_size) {
    if (decode_flags & ~ZLZ4F_DECODE_LINKED) return ZLZ4F_ERR_PARAMETER_INVALID;
    if (split_flags & ~ZLZ4F_SPLIT_LEGACY) return ZLZ4F_ERR_PARAMETER_INVALID;
    if ((!src && n) || (!want_size && !dst && cap)) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    struct Rec {
        uint64_t src_off, src_len, count, totals[4], mem_off, mem_cap, item_first[2], out_off, out_size, plan_totals[2];
        int64_t split_result, result;
    };
    // leg_len: null for the split of section 4.4h
    auto split = [&](Rec *r, const uint8_t *s, zlz4f_member *mem, uint64_t *item_off, uint64_t *item_len, uint64_t *leg_len) {
        const bool rec = mem != nullptr;
        return split_flags
                   ? zlz4f_batch_multiframe_split_ex(st, s, &r->src_off, &r->src_len, 1, &r->count, r->totals, mem,
                                                     rec ? &r->mem_off : nullptr, rec ? &r->mem_cap : nullptr,
                                                     rec ? r->item_first : nullptr, item_off, item_len,
                                                     rec ? &r->split_result : nullptr, split_flags, leg_len)
                   : zlz4f_batch_multiframe_split(st, s, &r->src_off, &r->src_len, 1, &r->count, r->totals, mem,
                                                  rec ? &r->mem_off : nullptr, rec ? &r->mem_cap : nullptr,
                                                  rec ? r->item_first : nullptr, item_off, item_len,
                                                  rec ? &r->split_result : nullptr);
    };
    DevBuf d_src(n, &dc);
    Staged<Rec> rec(&dc, 256);
    if (!d_src.p || !rec.d) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.src_len = n;
    dc.launched();
    if (!upload(d_src, src, n, st) || !rec.upload(st)) return ZLZ4_ERR_DEVICE;
    Rec *r = rec.d;
    const uint8_t *s = d_src.as<uint8_t>();
    int32_t rc = split(r, s, nullptr, nullptr, nullptr, nullptr);
    if (rc != 0) return rc;
    uint64_t totals[4] = {0, 0, 0, 0};
    if (hipMemcpyAsync(totals, r->totals, split_flags ? 32 : 16, hipMemcpyDeviceToHost, st) != hipSuccess || !dc.sync())
        return ZLZ4_ERR_DEVICE;
    if (totals[0] == 0) return 0;                                      // the empty buffer
    if (totals[0] > 0xFFFFFFFFull || totals[1] > 0xFFFFFFFFull || totals[3] > 0xFFFFFFFFull) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    const uint32_t nitems = (uint32_t)totals[0], max_blocks = (uint32_t)totals[1], leg_blocks = (uint32_t)totals[3];
    const bool legacy = totals[2] != 0;                                // (no legacy member: the legacy calls and selects are skipped)
    size_t wsn = zlz4f_batch_frame_decompressed_size_workspace_ex(nitems, max_blocks, decode_flags);
    auto at_least = [&](size_t v) { wsn = v > wsn ? v : wsn; };        // (the calls run one after the other on st)
    if (!want_size) at_least(zlz4f_batch_decompress_frame_workspace_ex(nitems, max_blocks, decode_flags));
    if (legacy) {
        at_least(zlz4f_batch_legacy_frame_decompressed_size_workspace(nitems, leg_blocks));
        if (!want_size) at_least(zlz4f_batch_decompress_legacy_frame_workspace(nitems, leg_blocks));
    }
    // per item: off, len, dst_off, dst_cap, size, result; with legacy members also leg_len and the legacy calls' answers
    DevBuf d_mem((size_t)nitems * sizeof(zlz4f_member), &dc), d_items((size_t)nitems * (split_flags ? 72u : 48u), &dc),
        d_ws(wsn, &dc);
    if (!d_mem.p || !d_items.p || !d_ws.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.mem_cap = nitems;
    dc.launched();
    if (hipMemcpyAsync(&r->mem_cap, &rec.h.mem_cap, 8, hipMemcpyHostToDevice, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
    zlz4f_member *mem = d_mem.as<zlz4f_member>();
    uint64_t *item_off = d_items.as<uint64_t>(), *item_len = item_off + nitems, *dst_off = item_len + nitems,
             *dst_cap = dst_off + nitems;
    int64_t *size = reinterpret_cast<int64_t *>(dst_cap + nitems), *item_result = size + nitems;
    uint64_t *leg_len = split_flags ? reinterpret_cast<uint64_t *>(item_result + nitems) : nullptr;
    int64_t *leg_size = split_flags ? reinterpret_cast<int64_t *>(leg_len + nitems) : nullptr,
            *leg_result = split_flags ? leg_size + nitems : nullptr;
    rc = split(r, s, mem, item_off, item_len, leg_len);
    if (rc != 0) return rc;
    rc = zlz4f_batch_frame_decompressed_size_ex(st, s, item_off, item_len, size, nitems, max_blocks, decode_flags, d_ws.p,
                                                d_ws.n);
    if (rc != 0) return rc;
    if (legacy) {
        rc = zlz4f_batch_legacy_frame_decompressed_size(st, s, item_off, leg_len, leg_size, nullptr, nitems, leg_blocks,
                                                        d_ws.p, d_ws.n);
        if (rc != 0) return rc;
        rc = zlz4f_batch_multiframe_select(st, mem, &r->mem_off, &r->split_result, r->item_first, size, leg_size, 1, size);
        if (rc != 0) return rc;
    }
    if (want_size) {
        rc = zlz4f_batch_multiframe_finish(st, mem, &r->mem_off, &r->split_result, r->item_first, size, size, 1, &r->result);
        if (rc != 0) return rc;
        int64_t result = 0;
        if (!read_result(dc, &r->result, result)) return ZLZ4_ERR_DEVICE;
        return result;
    }
    rc = zlz4f_batch_multiframe_plan(st, size, r->item_first, 1, 0, dst_off, dst_cap, &r->out_off, &r->out_size,
                                     r->plan_totals);
    if (rc != 0) return rc;
    uint64_t arena = 0;
    if (hipMemcpyAsync(&arena, r->plan_totals, 8, hipMemcpyDeviceToHost, st) != hipSuccess || !dc.sync()) return ZLZ4_ERR_DEVICE;
    if (arena > cap) return ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
    DevBuf d_dst(arena, &dc);
    if (!d_dst.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    dc.launched();
    rc = zlz4f_batch_decompress_frame_ex(st, s, item_off, item_len, d_dst.as<uint8_t>(), dst_off, dst_cap, item_result, nitems,
                                         max_blocks, decode_flags, d_ws.p, d_ws.n);
    if (rc != 0) return rc;
    if (legacy) {
        rc = zlz4f_batch_decompress_legacy_frame(st, s, item_off, leg_len, d_dst.as<uint8_t>(), dst_off, dst_cap, leg_result,
                                                 nullptr, nitems, leg_blocks, d_ws.p, d_ws.n);
        if (rc != 0) return rc;
        rc = zlz4f_batch_multiframe_select(st, mem, &r->mem_off, &r->split_result, r->item_first, item_result, leg_result, 1,
                                           item_result);
        if (rc != 0) return rc;
    }
    rc = zlz4f_batch_multiframe_finish(st, mem, &r->mem_off, &r->split_result, r->item_first, size, item_result, 1, &r->result);
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result)) return ZLZ4_ERR_DEVICE;
    if (!copy_back(dst, cap, d_dst, result)) return ZLZ4_ERR_DEVICE;
    return result;
}

}  // namespace

extern "C" {

int64_t zlz4f_multiframe_decompressed_size(const uint8_t *src, size_t src_len, uint32_t decode_flags) {
    return host_multiframe(src, src_len, nullptr, 0, decode_flags, 0, true);
}

int64_t zlz4f_decompress_multiframe(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, uint32_t decode_flags) {
    return host_multiframe(src, src_len, dst, dst_cap, decode_flags, 0, false);
}

int64_t zlz4f_multiframe_decompressed_size_ex(const uint8_t *src, size_t src_len, uint32_t decode_flags, uint32_t split_flags) {
    return host_multiframe(src, src_len, nullptr, 0, decode_flags, split_flags, true);
}

int64_t zlz4f_decompress_multiframe_ex(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, uint32_t decode_flags,
                                       uint32_t split_flags) {
    return host_multiframe(src, src_len, dst, dst_cap, decode_flags, split_flags, false);
}

}  // extern "C"
