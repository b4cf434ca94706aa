// zlz4_frame_seek.hip -- seekable .lz4 files (include/zlz4_amd.h): a file carries its member
// table and its block index as a last, skippable member, the SEEK TABLE.  The append writes that member behind every
// buffer from the record-mode split and the file index; the load reads both tables back from the file's tail without
// walking one block header; the concat lays compressed frames back to back, which is what a device-side writer of
// many-frame files lacked.  Every batch call is a fixed sequence of kernels on the caller's stream: nothing allocated,
// nothing read back.  The footer parse and the row checks are those of zlz4_frame_batch.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <optional>

#include "zlz4_frame_batch.hpp"
#include "zlz4_host.hpp"
#include "zlz4_launch.hpp"

using namespace zlz4host;

namespace {

inline bool sk_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

// A table is SLICED: workgroup j of the gx that a file has takes the 256 rows (load) or 8-byte words (append) j, j + gx,
// .. of that file.  gx depends on nbuf alone, so the launch is fixed: few files get many workgroups each, many files one.
constexpr uint32_t kSkSlice = 256;
inline uint32_t sk_slices(uint32_t nbuf) {
    const uint32_t gx = 1024u / nbuf;
    return gx < 1u ? 1u : (gx > 64u ? 64u : gx);
}
inline uint32_t sk_grid(uint32_t nbuf, uint32_t gx) {
    const uint64_t g = (uint64_t)nbuf * gx;
    return g > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)g;
}

// 8 bytes at any alignment from the two aligned words that hold them.  Both words hold at least one of the wanted bytes,
// so neither leaves the 8-byte granule of a byte that may be read.
struct RdAligned {
    __device__ __forceinline__ uint64_t operator()(const uint8_t *p) const {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        const uint32_t sh = (uint32_t)(a & 7u) * 8u;
        const uint64_t *w = reinterpret_cast<const uint64_t *>(a - (a & 7u));
        const uint64_t lo = w[0];
        return sh == 0 ? lo : (lo >> sh) | (w[1] << (64u - sh));
    }
};

// ------------------------------------------------------------------ append
// The table of buffer s as T / 8 little-endian 64-bit fields: the skippable header, three per member row, two per entry,
// four of the footer.  Field i depends on i alone, so the fields are spread over lanes and slices, and a table that starts
// at an odd address is written as the aligned words between its first and last bytes, each funnelled from two
// neighbouring fields, with the head and tail bytes stored one by one.  Nothing in front of n or behind n + T is written.
__global__ __launch_bounds__(256) void k_sk_append(uint8_t *buf, const uint64_t *__restrict__ buf_off,
                                                   const uint64_t *__restrict__ buf_len, const uint64_t *__restrict__ buf_cap,
                                                   uint32_t nbuf, uint32_t gx, const zlz4f_member *__restrict__ member,
                                                   const uint64_t *__restrict__ mem_off, const int64_t *__restrict__ split_result,
                                                   const zlz4f_index_entry *__restrict__ index,
                                                   const uint64_t *__restrict__ idx_off, const int64_t *__restrict__ idx_n,
                                                   int64_t *__restrict__ result) {
    const uint32_t tid = threadIdx.x;
    for (uint64_t u = blockIdx.x; u < (uint64_t)nbuf * gx; u += gridDim.x) {
        const uint32_t s = (uint32_t)(u / gx), j = (uint32_t)(u % gx);
        const int64_t nm = split_result[s], nb = idx_n[s];
        const uint64_t n = buf_len[s];
        zlz4f_member last = {};
        uint64_t end_pos = 0;
        if (nm >= 0 && nb >= 0) {
            if (nm > 0) last = member[mem_off[s] + (uint64_t)nm - 1u];
            end_pos = index[idx_off[s] + (uint64_t)nb].pos;
        }
        uint64_t T;
        const int64_t why = seek_append_refusal(nm, last, nb, end_pos, n, buf_cap[s], T);
        if (why != 0) {
            if (j == 0 && tid == 0) result[s] = why;
            continue;
        }
        const uint64_t rows = (uint64_t)nm + 1u, ents = 2u * ((uint64_t)nb + 1u), nf = T / 8u;
        const uint64_t *m64 = reinterpret_cast<const uint64_t *>(member) + 3u * mem_off[s];
        const uint64_t *e64 = reinterpret_cast<const uint64_t *>(index) + 2u * idx_off[s];
        auto field = [&](uint64_t i) -> uint64_t {
            if (i == 0) return (uint64_t)ZLZ4F_SEEK_TABLE_MAGICNUMBER | ((T - 8u) << 32);
            i -= 1u;
            if (i < 3u * rows) {
                const uint64_t r = i / 3u, c = i - 3u * r;
                if (r < (uint64_t)nm) return c == 2u ? (m64[i] & 0xFFFFFFFFull) : m64[i];        // (buf is 0 in the file)
                return c == 0 ? n : (c == 1u ? T : (uint64_t)kSeekSelfKind);
            }
            i -= 3u * rows;
            if (i < ents) return e64[i];
            i -= ents;
            return i == 0 ? rows : (i == 1u ? (uint64_t)nb : (i == 2u ? n + T : 1ull | ((uint64_t)kSeekFooterMagic << 32)));
        };
        uint8_t *p0 = buf + (uint64_t)(buf_off[s] + n);
        const uint32_t h = (uint32_t)((8u - (reinterpret_cast<uintptr_t>(p0) & 7u)) & 7u);
        uint64_t *body = reinterpret_cast<uint64_t *>(p0 + h);
        if (h == 0) {
            for (uint64_t i = (uint64_t)j * kSkSlice + tid; i < nf; i += (uint64_t)gx * kSkSlice) body[i] = field(i);
        } else {
            for (uint64_t i = (uint64_t)j * kSkSlice + tid; i + 1u < nf; i += (uint64_t)gx * kSkSlice)
                body[i] = (field(i) >> (8u * h)) | (field(i + 1u) << (64u - 8u * h));
            if (j == 0 && tid < 8u) {
                if (tid < h) p0[tid] = (uint8_t)(field(0) >> (8u * tid));
                else p0[T - 8u + tid] = (uint8_t)(field(nf - 1u) >> (8u * tid));
            }
        }
        if (j == 0 && tid == 0) result[s] = (int64_t)(n + T);
    }
}

// ------------------------------------------------------------------ load
// one lane per file, the footer alone: count[s] = nm, room[s] = nb + 1 (both 0 without a well-formed footer), and in
// count mode the two sums
__global__ __launch_bounds__(64) void k_sk_count(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                 const uint64_t *__restrict__ src_len, uint32_t nbuf,
                                                 uint64_t *__restrict__ count, uint64_t *__restrict__ room,
                                                 unsigned long long *__restrict__ totals) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long members = 0, rooms = 0;
    if (s < nbuf) {
        SeekFooter F;
        if (seek_footer(src + src_off[s], src_len[s], F) == kSeekOk) { members = F.nm; rooms = F.nb + 1u; }
        count[s] = members;
        if (room) room[s] = rooms;
    }
    for (uint32_t d = 32u; d >= 1u; d >>= 1) {
        members += __shfl_xor(members, (int)d);
        rooms += __shfl_xor(rooms, (int)d);
    }
    if ((threadIdx.x & 63u) == 0 && (members | rooms)) {
        atomicAdd(&totals[0], members);
        atomicAdd(&totals[1], rooms);
    }
}

// one workgroup, in place: a[0..n] = the exclusive scan of a[0..n), a[n] = the total; thread t owns a contiguous run
__global__ __launch_bounds__(1024) void k_sk_scan(uint64_t *a, uint32_t n) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + 1023u) / 1024u;
    const uint64_t b0 = (uint64_t)t * chunk;
    const uint32_t lo = b0 < n ? (uint32_t)b0 : n;
    const uint32_t hi = b0 + chunk < n ? (uint32_t)(b0 + chunk) : n;
    uint64_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += a[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - sum;
    const uint64_t total = part[1023];
    for (uint32_t i = lo; i < hi; i++) { const uint64_t c = a[i]; a[i] = run; run += c; }
    if (t == 0) a[n] = total;
}

// one lane per file: the verdict of the footer and of the two capacities; the rows may lower it (k_sk_rows)
__global__ __launch_bounds__(64) void k_sk_head(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                const uint64_t *__restrict__ src_len, uint32_t nbuf,
                                                const uint64_t *__restrict__ mem_cap, const uint64_t *__restrict__ idx_off,
                                                uint64_t idx_cap, int64_t *__restrict__ split_result,
                                                int64_t *__restrict__ idx_n) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nbuf) return;
    SeekFooter F;
    const SeekVerdict v = seek_footer(src + src_off[s], src_len[s], F);
    int64_t r = 0;
    if (v == kSeekMalformed) r = ZLZ4_ERR_INVALID_STATE;
    else if (v == kSeekOk) r = F.nm > mem_cap[s] || idx_off[s + 1] > idx_cap ? (int64_t)ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL : (int64_t)F.nm;
    split_result[s] = r;
    idx_n[s] = r > 0 ? (int64_t)F.nb : (r < 0 ? r : (int64_t)ZLZ4_ERR_INVALID_STATE);
}

// The rows of every file that k_sk_head accepted, one row per thread, 256 rows a slice: a member row or an entry is read
// from the unaligned table, compared with its neighbour (seek_member_row, seek_entry_row) and written to the aligned
// output.  A slice that finds a row out of shape lowers the file's verdict with one atomic: no pass over the slices.
__global__ __launch_bounds__(256) void k_sk_rows(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                 const uint64_t *__restrict__ src_len, uint32_t nbuf, uint32_t gx,
                                                 zlz4f_member *__restrict__ member, const uint64_t *__restrict__ mem_off,
                                                 zlz4f_index_entry *__restrict__ index, const uint64_t *__restrict__ idx_off,
                                                 int64_t *split_result, int64_t *idx_n) {
    __shared__ int64_t verdict;
    const uint32_t tid = threadIdx.x;
    for (uint64_t u = blockIdx.x; u < (uint64_t)nbuf * gx; u += gridDim.x) {
        const uint32_t s = (uint32_t)(u / gx), j = (uint32_t)(u % gx);
        __syncthreads();
        // one read for the workgroup, so that it branches as one.  Another slice may be lowering the verdict meanwhile; a
        // stale positive value only costs this slice its rows' work, the atomic below decides.
        if (tid == 0) verdict = *(volatile int64_t *)&split_result[s];
        __syncthreads();
        if (verdict <= 0) continue;
        const uint8_t *f = src + src_off[s];
        const uint64_t n = src_len[s];
        SeekFooter F;
        bool bad = seek_footer(f, n, F) != kSeekOk;                            // (k_sk_head has accepted it)
        if (!bad) {
            zlz4f_member *mo = member + mem_off[s];
            zlz4f_index_entry *eo = index + idx_off[s];
            const uint64_t rows = F.nm + F.nb + 1u;
            for (uint64_t r = (uint64_t)j * kSkSlice + tid; r < rows; r += (uint64_t)gx * kSkSlice) {
                if (r < F.nm) {
                    zlz4f_member m;
                    if (!seek_member_row(f, n, F, r, m, RdAligned())) bad = true;
                    m.buf = s;
                    mo[r] = m;
                } else {
                    zlz4f_index_entry e;
                    if (!seek_entry_row(f, n, F, r - F.nm, e, RdAligned())) bad = true;
                    eo[r - F.nm] = e;
                }
            }
        }
        if (__syncthreads_or(bad ? 1 : 0) && tid == 0) {
            atomicMin(reinterpret_cast<long long *>(&split_result[s]), (long long)ZLZ4_ERR_INVALID_STATE);
            idx_n[s] = ZLZ4_ERR_INVALID_STATE;
        }
    }
}

// ------------------------------------------------------------------ concat
// one wavefront per file, 64 items a step: the first negative length in item order or the total against the capacity,
// then every item's place in the destination (~0: the file failed, nothing of it is copied)
__global__ __launch_bounds__(256) void k_sk_concat_plan(const int64_t *__restrict__ item_len, const uint64_t *__restrict__ item_first,
                                                        const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ dst_cap,
                                                        uint32_t nbuf, uint64_t *__restrict__ place, int64_t *__restrict__ result) {
    const uint32_t s = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (s >= nbuf) return;
    const uint64_t i0 = item_first[s], i1 = item_first[s + 1];
    unsigned long long sum = 0, bad = ~0ull;
    long long code = 0;
    for (uint64_t i = i0 + lane; i < i1; i += 64u) {
        const int64_t v = item_len[i];
        if (v < 0) { if (bad == ~0ull) { bad = i; code = v; } }
        else sum += (uint64_t)v;
    }
    unsigned long long first = bad;
    for (uint32_t d = 32u; d >= 1u; d >>= 1) {
        const unsigned long long o = __shfl_xor(first, (int)d);
        first = o < first ? o : first;
        sum += __shfl_xor(sum, (int)d);
    }
    int64_t out = (int64_t)sum;
    if (first != ~0ull) out = __shfl(code, (int)((first - i0) & 63u));          // (the lane that holds item `first`)
    else if (sum > dst_cap[s]) out = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
    if (lane == 0) result[s] = out;
    uint64_t run = dst_off[s];
    for (uint64_t base = i0; base < i1; base += 64u) {                // (wave-uniform trip count)
        const uint64_t i = base + lane;
        const unsigned long long c = i < i1 && out >= 0 ? (uint64_t)item_len[i] : 0u;
        unsigned long long incl = c;
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (i < i1) place[i] = out >= 0 ? run + (incl - c) : ~0ull;
        run += __shfl(incl, 63);
    }
}

// one workgroup per item: head bytes up to the destination's 8-byte boundary, aligned 8-byte stores funnelled from the
// source's aligned words, tail bytes
__global__ __launch_bounds__(256) void k_sk_concat_copy(const uint8_t *__restrict__ src, const uint64_t *__restrict__ item_off,
                                                        const int64_t *__restrict__ item_len, const uint64_t *__restrict__ place,
                                                        uint32_t nitems, uint8_t *__restrict__ dst) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < nitems; i += gridDim.x) {
        const uint64_t at = place[i];
        const int64_t len = item_len[i];
        if (at == ~0ull || len <= 0) continue;
        const uint64_t n = (uint64_t)len;
        const uint8_t *p = src + item_off[i];
        uint8_t *q = dst + at;
        uint64_t head = (8u - (reinterpret_cast<uintptr_t>(q) & 7u)) & 7u;
        if (head > n) head = n;
        const uint64_t words = (n - head) / 8u, tail = n - head - 8u * words;
        if (tid < head) q[tid] = p[tid];
        if (tid < tail) q[head + 8u * words + tid] = p[head + 8u * words + tid];
        uint64_t *body = reinterpret_cast<uint64_t *>(q + head);
        const RdAligned rd;
        for (uint64_t w = tid; w < words; w += 256u) body[w] = rd(p + head + 8u * w);
    }
}

}  // namespace

extern "C" {

size_t zlz4f_seek_table_bound(uint64_t nmembers, uint64_t nblocks) {
    uint64_t T;
    if (nmembers == ~0ull || !seek_table_bytes(nmembers + 1u, nblocks, T) || T - 8u > 0xFFFFFFFFull) return 0;
    return (size_t)T;
}

int32_t zlz4f_batch_append_seek_table(void *stream, uint8_t *d_buf, const uint64_t *d_buf_off, const uint64_t *d_buf_len,
                                      const uint64_t *d_buf_cap, uint32_t nbuf, const zlz4f_member *d_member,
                                      const uint64_t *d_mem_off, const int64_t *d_split_result,
                                      const zlz4f_index_entry *d_index, const uint64_t *d_idx_off, const int64_t *d_idx_n,
                                      int64_t *d_result) {
    if (nbuf == 0) return 0;
    if (!d_buf || !d_buf_off || !d_buf_len || !d_buf_cap || !d_member || !d_mem_off || !d_split_result || !d_index ||
        !d_idx_off || !d_idx_n || !d_result)
        return ZLZ4_ERR_INVALID_STATE;
    if (sk_misaligned(d_buf_off) || sk_misaligned(d_buf_len) || sk_misaligned(d_buf_cap) || sk_misaligned(d_member) ||
        sk_misaligned(d_mem_off) || sk_misaligned(d_split_result) || sk_misaligned(d_index) || sk_misaligned(d_idx_off) ||
        sk_misaligned(d_idx_n) || sk_misaligned(d_result))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    const uint32_t gx = sk_slices(nbuf);
    hipLaunchKernelGGL(k_sk_append, dim3(sk_grid(nbuf, gx)), dim3(256), 0, (hipStream_t)stream, d_buf, d_buf_off, d_buf_len,
                       d_buf_cap, nbuf, gx, d_member, d_mem_off, d_split_result, d_index, d_idx_off, d_idx_n, d_result);
    return zlz4_launch_status();
}

int32_t zlz4f_batch_load_seek_table(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                    uint32_t nbuf, uint64_t *d_count, uint64_t *d_totals, zlz4f_member *d_member,
                                    const uint64_t *d_mem_off, const uint64_t *d_mem_cap, int64_t *d_split_result,
                                    zlz4f_index_entry *d_index, uint64_t *d_idx_off, uint64_t idx_cap, int64_t *d_idx_n) {
    const bool record = d_member != nullptr;
    if (!d_totals || sk_misaligned(d_totals)) return ZLZ4_ERR_INVALID_STATE;
    if (nbuf && (!d_src || !d_src_off || !d_src_len || !d_count)) return ZLZ4_ERR_INVALID_STATE;
    if (record && (!d_idx_off || (nbuf && (!d_mem_off || !d_mem_cap || !d_split_result || !d_index || !d_idx_n))))
        return ZLZ4_ERR_INVALID_STATE;
    if (sk_misaligned(d_src_off) || sk_misaligned(d_src_len) || sk_misaligned(d_count) || sk_misaligned(d_member) ||
        (record && (sk_misaligned(d_mem_off) || sk_misaligned(d_mem_cap) || sk_misaligned(d_split_result) ||
                    sk_misaligned(d_index) || sk_misaligned(d_idx_off) || sk_misaligned(d_idx_n))))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_totals, 0, 16, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
    if (nbuf == 0) {
        if (record && hipMemsetAsync(d_idx_off, 0, 8, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
        return 0;
    }
    const uint32_t g = grid_of(nbuf, 64), gx = sk_slices(nbuf);
    hipLaunchKernelGGL(k_sk_count, dim3(g), dim3(64), 0, st, d_src, d_src_off, d_src_len, nbuf, d_count,
                       record ? d_idx_off : (uint64_t *)nullptr, reinterpret_cast<unsigned long long *>(d_totals));
    if (record) {
        hipLaunchKernelGGL(k_sk_scan, dim3(1), dim3(1024), 0, st, d_idx_off, nbuf);
        hipLaunchKernelGGL(k_sk_head, dim3(g), dim3(64), 0, st, d_src, d_src_off, d_src_len, nbuf, d_mem_cap, d_idx_off, idx_cap,
                           d_split_result, d_idx_n);
        hipLaunchKernelGGL(k_sk_rows, dim3(sk_grid(nbuf, gx)), dim3(256), 0, st, d_src, d_src_off, d_src_len, nbuf, gx, d_member,
                           d_mem_off, d_index, d_idx_off, d_split_result, d_idx_n);
    }
    return zlz4_launch_status();
}

size_t zlz4f_batch_concat_workspace(uint32_t nitems) { return ((size_t)nitems * 8u + 255u) & ~(size_t)255; }

int32_t zlz4f_batch_concat(void *stream, const uint8_t *d_src, const uint64_t *d_item_off, const int64_t *d_item_len,
                           const uint64_t *d_item_first, uint32_t nbuf, uint32_t nitems, uint8_t *d_dst,
                           const uint64_t *d_dst_off, const uint64_t *d_dst_cap, int64_t *d_result, void *d_workspace,
                           size_t workspace_bytes) {
    if (nbuf == 0) return 0;
    if (!d_item_first || !d_dst_off || !d_dst_cap || !d_result || (nitems && (!d_src || !d_item_off || !d_item_len || !d_dst)))
        return ZLZ4_ERR_INVALID_STATE;
    if (sk_misaligned(d_item_off) || sk_misaligned(d_item_len) || sk_misaligned(d_item_first) || sk_misaligned(d_dst_off) ||
        sk_misaligned(d_dst_cap) || sk_misaligned(d_result))
        return ZLZ4_ERR_INVALID_STATE;
    if (nitems && (!d_workspace || workspace_bytes < zlz4f_batch_concat_workspace(nitems) || sk_misaligned(d_workspace)))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    uint64_t *place = static_cast<uint64_t *>(d_workspace);
    hipLaunchKernelGGL(k_sk_concat_plan, dim3(grid_of(nbuf, 4)), dim3(256), 0, st, d_item_len, d_item_first, d_dst_off, d_dst_cap,
                       nbuf, place, d_result);
    if (nitems)
        hipLaunchKernelGGL(k_sk_concat_copy, dim3(grid_of(nitems, 1, 0x7FFFFFFFu)), dim3(256), 0, st, d_src, d_item_off, d_item_len,
                           place, nitems, d_dst);
    return zlz4_launch_status();
}

}  // extern "C"

// ====================================================================== one file in host memory
namespace {

// what both host calls stage: the file, one record whose fields are the arrays of a batch of one, and the tables
struct SkRec {
    uint64_t src_off, src_len, count, totals[4], mem_off, mem_cap, item_first[2], idx_off[2], dst_off, dst_cap, skip,
        plan_totals[2], tab_off, tab_cap, load_count, load_totals[2], dict_off;
    int64_t split_result, idx_n, rres, result;
    zlz4f_range range;
    uint32_t dict_len, pad;           // the dictionary of zlz4f_decompress_file_range_using_dict: its staged tail
};

// plan, range decode and the copy of exactly the wanted bytes: the tail of zlz4f_decompress_file_range over tables that
// are on the device already.  d_dict: the staged tail of the file's dictionary (r->dict_len bytes), else null.
int64_t sk_range_tail(DeviceCall &dc, SkRec *r, const uint8_t *s, const zlz4f_member *mem, const zlz4f_index_entry *index,
                      uint64_t idx_room, uint64_t a, uint64_t b, uint8_t *dst, size_t cap, const uint8_t *d_dict = nullptr) {
    hipStream_t st = dc.st;
    int32_t rc = zlz4f_batch_plan_frame_ranges(st, index, r->idx_off, &r->idx_n, 1, &r->range, 1, 0, &r->dst_off, &r->dst_cap,
                                               r->plan_totals);
    if (rc != 0) return rc;
    int64_t idx_n = 0;
    uint64_t plan[2] = {0, 0};
    if (hipMemcpyAsync(&idx_n, &r->idx_n, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(plan, r->plan_totals, 16, hipMemcpyDeviceToHost, st) != hipSuccess || !dc.sync())
        return ZLZ4_ERR_DEVICE;
    if (idx_n < 0) return idx_n;
    if ((uint64_t)idx_n >= idx_room) return ZLZ4_ERR_DEVICE;
    zlz4f_index_entry last = {0, 0};
    if (hipMemcpy(&last, index + idx_n, sizeof last, hipMemcpyDeviceToHost) != hipSuccess) return ZLZ4_ERR_DEVICE;
    const uint64_t S = last.dec, a1 = a < S ? a : S, b1 = b < S ? b : S;
    if (cap < b1 - a1) return ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
    if (plan[1] > 0xFFFFFFFFull) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    const uint32_t max_items = (uint32_t)plan[1];
    const size_t rws = d_dict ? zlz4f_batch_decompress_file_range_using_dict_workspace(1, max_items)
                              : zlz4f_batch_decompress_file_range_workspace(1, max_items);
    DevBuf d_rws(rws, &dc), d_dst((size_t)plan[0], &dc);
    if (!d_rws.p || !d_dst.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    dc.launched();
    rc = d_dict ? zlz4f_batch_decompress_file_range_using_dict(st, s, &r->src_off, &r->src_len, index, r->idx_off, &r->idx_n, 1,
                                                               mem, &r->mem_off, &r->split_result, &r->range,
                                                               d_dst.as<uint8_t>(), &r->dst_off, &r->dst_cap, &r->skip, &r->rres,
                                                               1, max_items, d_dict, &r->dict_off, &r->dict_len, 1, nullptr,
                                                               d_rws.p, rws)
                : zlz4f_batch_decompress_file_range(st, s, &r->src_off, &r->src_len, index, r->idx_off, &r->idx_n, 1, mem,
                                                    &r->mem_off, &r->split_result, &r->range, d_dst.as<uint8_t>(), &r->dst_off,
                                                    &r->dst_cap, &r->skip, &r->rres, 1, max_items, d_rws.p, rws);
    if (rc != 0) return rc;
    int64_t result = 0;
    uint64_t skip = 0;
    if (hipMemcpyAsync(&skip, &r->skip, 8, hipMemcpyDeviceToHost, st) != hipSuccess || !read_result(dc, &r->rres, result))
        return ZLZ4_ERR_DEVICE;
    if (result > 0 && ((uint64_t)result > cap || skip + (uint64_t)result > plan[0] ||
                       hipMemcpy(dst, d_dst.as<uint8_t>() + skip, (size_t)result, hipMemcpyDeviceToHost) != hipSuccess))
        return ZLZ4_ERR_DEVICE;
    return result;
}

}  // namespace

extern "C" {

// Split (count, record), index and append as a batch of one.  The append touches [n, n + T) alone, so the table is written
// to a buffer of its own: the staged buffer offset is -n, and offset + length is that buffer's first byte.
int64_t zlz4f_seek_table(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, uint32_t split_flags) {
    if (split_flags & ~ZLZ4F_SPLIT_LEGACY) return ZLZ4F_ERR_PARAMETER_INVALID;
    if ((!src && n) || (!dst && cap)) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    DevBuf d_src(n, &dc);
    Staged<SkRec> rec(&dc, 256);
    if (!d_src.p || !rec.d) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.src_len = n;
    rec.h.idx_off[1] = 1;                                              // (the file without a member: one entry { 0, 0 })
    dc.launched();
    if (!upload(d_src, src, n, st) || !rec.upload(st)) return ZLZ4_ERR_DEVICE;
    SkRec *r = rec.d;
    const uint8_t *s = d_src.as<uint8_t>();
    int32_t rc = zlz4f_batch_multiframe_split_ex(st, s, &r->src_off, &r->src_len, 1, &r->count, r->totals, nullptr, nullptr,
                                                 nullptr, nullptr, nullptr, nullptr, nullptr, split_flags, nullptr);
    if (rc != 0) return rc;
    uint64_t totals[4] = {0, 0, 0, 0};
    if (hipMemcpyAsync(totals, r->totals, 32, hipMemcpyDeviceToHost, st) != hipSuccess || !dc.sync()) return ZLZ4_ERR_DEVICE;
    if (totals[0] > 0xFFFFFFFFull || totals[1] > 0xFFFFFFFFull || totals[3] > 0xFFFFFFFFull) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    const size_t nitems = (size_t)totals[0];
    const uint64_t idx_cap = totals[1] + totals[3] + 1u;
    const size_t bound = zlz4f_seek_table_bound(nitems, idx_cap - 1u);
    if (bound == 0) return ZLZ4_ERR_UNSUPPORTED;
    const size_t iws = nitems ? zlz4f_batch_file_index_workspace(1, totals) : 0;
    DevBuf d_mem(nitems * sizeof(zlz4f_member), &dc), d_items(nitems * 24u, &dc), d_iws(iws, &dc),
        d_index((size_t)idx_cap * sizeof(zlz4f_index_entry), &dc), d_tab(bound, &dc);
    if (!d_mem.p || !d_items.p || !d_iws.p || !d_index.p || !d_tab.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.mem_cap = nitems;
    rec.h.tab_off = (uint64_t)0 - (uint64_t)n;
    rec.h.tab_cap = (uint64_t)n + (cap < bound ? cap : bound);
    dc.launched();
    if (hipMemcpyAsync(&r->mem_cap, &rec.h.mem_cap, 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(&r->tab_off, &rec.h.tab_off, 16, hipMemcpyHostToDevice, st) != hipSuccess)
        return ZLZ4_ERR_DEVICE;
    zlz4f_member *mem = d_mem.as<zlz4f_member>();
    zlz4f_index_entry *index = d_index.as<zlz4f_index_entry>();
    if (nitems) {
        uint64_t *item_off = d_items.as<uint64_t>(), *item_len = item_off + nitems, *leg_len = item_len + nitems;
        rc = zlz4f_batch_multiframe_split_ex(st, s, &r->src_off, &r->src_len, 1, &r->count, r->totals, mem, &r->mem_off,
                                             &r->mem_cap, r->item_first, item_off, item_len, &r->split_result, split_flags, leg_len);
        if (rc != 0) return rc;
        rc = zlz4f_batch_file_index(st, s, &r->src_off, &r->src_len, 1, mem, &r->mem_off, &r->split_result, r->item_first, item_off,
                                    item_len, leg_len, totals, index, r->idx_off, idx_cap, &r->idx_n, d_iws.p, iws);
        if (rc != 0) return rc;
    } else if (hipMemsetAsync(index, 0, sizeof(zlz4f_index_entry), st) != hipSuccess) return ZLZ4_ERR_DEVICE;
    rc = zlz4f_batch_append_seek_table(st, d_tab.as<uint8_t>(), &r->tab_off, &r->src_len, &r->tab_cap, 1, mem, &r->mem_off,
                                       &r->split_result, index, r->idx_off, &r->idx_n, &r->result);
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result)) return ZLZ4_ERR_DEVICE;
    if (result < 0) return result;
    const int64_t T = result - (int64_t)n;
    if (T <= 0 || (uint64_t)T > bound || (uint64_t)T > cap) return ZLZ4_ERR_DEVICE;        // (cannot happen)
    if (!copy_back(dst, cap, d_tab, T)) return ZLZ4_ERR_DEVICE;
    return T;
}

}  // extern "C"

namespace {

// zlz4f_decompress_file_range with ZLZ4F_RANGE_SEEK_TABLE, after the refusals: the tables are taken from the file's tail
// where the file ends in a well-formed seek table.  The whole file is staged either way.  tail: the D > 0 last bytes
// of the file's dictionary, else null.
int64_t sk_host_range(const uint8_t *src, size_t n, uint64_t a, uint64_t b, uint8_t *dst, size_t cap, uint32_t split_flags,
                      const uint8_t *tail, uint32_t D) {
    {
        hipStream_t st = nullptr;
        DeviceCall dc(st);
        DevBuf d_src(n, &dc);
        std::optional<DevBuf> d_dict;                                   // (the plain call keeps its allocations)
        if (tail) d_dict.emplace(D, &dc);
        Staged<SkRec> rec(&dc, 256);
        if (!d_src.p || !rec.d || (tail && !d_dict->p)) return ZLZ4F_ERR_ALLOCATION_FAILED;
        rec.h.src_len = n;
        rec.h.range.a = a; rec.h.range.b = b;
        rec.h.dict_len = D;
        dc.launched();
        if (!upload(d_src, src, n, st) || !rec.upload(st) || (tail && !upload(*d_dict, tail, D, st))) return ZLZ4_ERR_DEVICE;
        SkRec *r = rec.d;
        const uint8_t *s = d_src.as<uint8_t>();
        int32_t rc = zlz4f_batch_load_seek_table(st, s, &r->src_off, &r->src_len, 1, &r->load_count, r->load_totals, nullptr,
                                                 nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
        if (rc != 0) return rc;
        uint64_t lt[2] = {0, 0};
        if (hipMemcpyAsync(lt, r->load_totals, 16, hipMemcpyDeviceToHost, st) != hipSuccess || !dc.sync()) return ZLZ4_ERR_DEVICE;
        if (lt[0] != 0) {                                              // a footer in shape: the rows decide
            DevBuf d_mem((size_t)lt[0] * sizeof(zlz4f_member), &dc), d_index((size_t)lt[1] * sizeof(zlz4f_index_entry), &dc);
            if (!d_mem.p || !d_index.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
            rec.h.mem_cap = lt[0];
            dc.launched();
            if (hipMemcpyAsync(&r->mem_cap, &rec.h.mem_cap, 8, hipMemcpyHostToDevice, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
            zlz4f_member *mem = d_mem.as<zlz4f_member>();
            zlz4f_index_entry *index = d_index.as<zlz4f_index_entry>();
            rc = zlz4f_batch_load_seek_table(st, s, &r->src_off, &r->src_len, 1, &r->load_count, r->load_totals, mem, &r->mem_off,
                                             &r->mem_cap, &r->split_result, index, r->idx_off, lt[1], &r->idx_n);
            if (rc != 0) return rc;
            int64_t loaded = 0;
            if (!read_result(dc, &r->split_result, loaded)) return ZLZ4_ERR_DEVICE;
            if (loaded > 0)
                return sk_range_tail(dc, r, s, mem, index, lt[1], a, b, dst, cap, tail ? d_dict->as<uint8_t>() : nullptr);
        }
    }
    // no table, or one out of shape: the index is built
    return tail ? zlz4_host_file_range_dict(src, n, a, b, dst, cap, split_flags, tail, D)
                     : zlz4f_decompress_file_range(src, n, a, b, dst, cap, split_flags);
}

}  // namespace

extern "C" {

int64_t zlz4f_decompress_file_range_ex(const uint8_t *src, size_t n, uint64_t a, uint64_t b, uint8_t *dst, size_t cap,
                                       uint32_t split_flags, uint32_t range_flags) {
    if ((split_flags & ~ZLZ4F_SPLIT_LEGACY) || (range_flags & ~ZLZ4F_RANGE_SEEK_TABLE)) return ZLZ4F_ERR_PARAMETER_INVALID;
    if (range_flags == 0) return zlz4f_decompress_file_range(src, n, a, b, dst, cap, split_flags);
    if ((!src && n) || (!dst && cap) || a > b) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return sk_host_range(src, n, a, b, dst, cap, split_flags, nullptr, 0);
}

// The _ex call with a dictionary for the file: only the dictionary's last 64 KiB are staged.  dict_len == 0: the _ex call.
int64_t zlz4f_decompress_file_range_using_dict(const uint8_t *src, size_t n, uint64_t a, uint64_t b, uint8_t *dst, size_t cap,
                                               uint32_t split_flags, uint32_t range_flags, const uint8_t *dict,
                                               size_t dict_len) {
    if ((split_flags & ~ZLZ4F_SPLIT_LEGACY) || (range_flags & ~ZLZ4F_RANGE_SEEK_TABLE)) return ZLZ4F_ERR_PARAMETER_INVALID;
    if ((!src && n) || (!dst && cap) || (!dict && dict_len) || a > b) return ZLZ4_ERR_INVALID_STATE;
    if (dict_len == 0) return zlz4f_decompress_file_range_ex(src, n, a, b, dst, cap, split_flags, range_flags);
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    const uint32_t D = (uint32_t)dict_tail(dict_len);
    const uint8_t *tail = dict + (dict_len - D);
    return range_flags ? sk_host_range(src, n, a, b, dst, cap, split_flags, tail, D)
                       : zlz4_host_file_range_dict(src, n, a, b, dst, cap, split_flags, tail, D);
}

}  // extern "C"
