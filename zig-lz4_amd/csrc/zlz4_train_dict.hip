// zlz4_train_dict.hip -- dictionary training on the device: zlz4_batch_train_dict and the host
// call zlz4_train_dict.  No counterpart in the reference.
//
// The specification (the same text as include/zlz4_amd.h; the model is tools/pyref/zig_lz4_train_dict.py).  One group is
// a run of samples and yields one dictionary.  d in {4, 6, 8}, k in 16..1024 (k >= d), f in 10..24, m = k - d + 1; per
// group a capacity C <= 65536.
//   B      the group's samples back to back, S bytes (S <= 2^27); nd = S - d + 1; nd <= 0 or C == 0: the result is 0
//   h(p)   v = the d bytes at p, little endian; h = ((v << (64 - 8d)) * 0xCF1BBCDCB7A56463 mod 2^64) >> (64 - f)
//   freq   freq[x] = the number of p in [0, nd) with h(p) == x
//   epochs nseg = ceil(C / k), E = max(1, min(nseg, nd / (8k))), size = nd / E; epoch e = [e * size, (e + 1) * size), the
//          last one ends at nd
//   steps  at most T = 2 * nseg; tail = C, ep = 0, zero = 0; a step takes epoch ep as [b, e), finds the window start s in
//          [b, e) with the largest score(s) = sum of freq[h(p)] over p in [s, min(s + m, e)), each distinct hash value once
//          per window (lowest s on a tie), then ep = (ep + 1) % E; score 0: zero += 1, stop at zero == E; otherwise
//          zero = 0, seg = min(k, tail, S - s), tail -= seg, out[tail .. tail + seg) = B[s .. s + seg), freq[h(p)] = 0 for
//          p in [s, min(s + m, e)), stop at tail == 0
//   result L = C - tail, the dictionary is out[tail .. C) at the front of the group's slot
//
// Kernels.  Every launch carries all groups (the group is grid axis y); a group that is done returns at once.
//   k_train_sum / k_train_plan   S per group, the groups' places in the workspace, the refusals, the step state
//   k_train_pack                 the samples of a group back to back, 16 zero bytes behind them
//   k_train_count                h(p) for every position (kept: the hashes never change), freq by no-return atomic adds
//   k_train_reach                dist[p] = distance to the nearest q < p with h(q) == h(p) where that is <= m - 1, else 0:
//                                p counts in the window at s exactly when dist[p] == 0 or dist[p] > p - s, which is the
//                                "once per window" rule without a table per window.  Brute force over an LDS tile of
//                                hashes with a halo of m - 1.
//   per step k_train_score       w[p] = freq[h(p)] and dist[p] of a tile of the epoch in LDS, one lane per window start
//                                sums its <= m terms, the workgroup's (largest score, lowest s) goes into the group's
//                                winner word with one 64-bit atomicMax of score << 27 | (2^27 - 1 - (s - b))
//            k_train_commit      one workgroup per group: the winner's segment, the zeroed frequencies, the state
//   k_train_finish               out[tail .. C) to the slot's front, L or the code to the result
// The step boundary is the kernel boundary: no persistent kernel, no grid barrier, no flag to wait for, no read-back; the
// number of step launches comes from max_dict_cap and k alone.
#include <vector>

#include "zlz4_device.hpp"
#include "zlz4_host.hpp"
#include "zlz4_launch.hpp"

namespace zlz4 {
namespace {

constexpr uint32_t kTrainMaxDict = 65536u;
constexpr uint32_t kTrainMaxGroup = 1u << 27;
constexpr uint64_t kTrainPrime = 0xCF1BBCDCB7A56463ull;
constexpr uint32_t kPosBits = 27u, kPosMask = (1u << kPosBits) - 1u;
constexpr uint32_t kThreads = 256u;
constexpr uint32_t kHalo = 1024u;            // >= the largest m - 1 (k <= 1024, d >= 4: 1020)
constexpr uint32_t kReachTile = 2048u;       // positions per tile of k_train_reach
constexpr uint32_t kScoreTile = 1024u;       // window starts per tile of k_train_score
constexpr uint32_t kPad = 16u;               // bytes behind a group's samples (8 must be readable: a d-mer is loaded as 8)

struct TrainGroup {
    uint64_t base;           // where the group's bytes, hashes and distances start in their arrays (an element index)
    uint64_t winner;         // score << 27 | (2^27 - 1 - (s - b)) of the step under way, 0 between steps
    uint32_t S, nd, C, E, size, steps_left, tail, ep, zero, done;
    int32_t code;            // 0 or the group's refusal
    uint32_t reserved;
};
static_assert(sizeof(TrainGroup) == 64, "one group, one 64-byte record");

struct TrainParams { uint32_t d, k, f, m; };

// the regions of the workspace (byte offsets, every one a multiple of 16) for N elements of sample space
struct TrainLayout {
    size_t groups, out, freq, hash, dist, bytes, total;
    uint32_t out_stride;
};

inline bool train_params_ok(const zlz4_train_params *p) {
    return p && (p->d == 4u || p->d == 6u || p->d == 8u) && p->k >= 16u && p->k <= 1024u && p->k >= p->d && p->f >= 10u &&
           p->f <= 24u;
}

inline uint32_t train_cap(uint32_t max_dict_cap) { return max_dict_cap < kTrainMaxDict ? max_dict_cap : kTrainMaxDict; }

inline TrainLayout train_layout(uint32_t ngroups, uint64_t N, uint32_t max_dict_cap, uint32_t f) {
    TrainLayout L;
    L.out_stride = (train_cap(max_dict_cap) + 15u) & ~15u;
    L.groups = 0;
    L.out = L.groups + (size_t)ngroups * sizeof(TrainGroup);
    L.freq = L.out + (size_t)ngroups * L.out_stride;
    L.hash = L.freq + (size_t)ngroups * (sizeof(uint32_t) << f);
    L.dist = L.hash + N * 4u;
    L.bytes = L.dist + N * 2u;
    L.total = L.bytes + N;
    return L;
}

__device__ __forceinline__ uint64_t ld64(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }

__device__ __forceinline__ uint32_t train_hash(uint64_t v, uint32_t d, uint32_t f) {
    return (uint32_t)(((v << (64u - 8u * d)) * kTrainPrime) >> (64u - f));
}

// the sum of v over the workgroup's 256 threads, in every thread
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t *sh) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = kThreads / 2u; d > 0u; d >>= 1) {
        if (t < d) sh[t] += sh[t + d];
        __syncthreads();
    }
    return sh[0];
}

// S of every group into `base` (64 bits: the sum may not fit S), InvalidState for a run of samples that is none
__global__ __launch_bounds__(kThreads) void k_train_sum(const uint32_t *__restrict__ src_len, uint32_t nsamples,
                                                        const uint32_t *__restrict__ group_first,
                                                        TrainGroup *__restrict__ groups) {
    __shared__ uint64_t sh[kThreads];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    const uint32_t lo = group_first[g], hi = group_first[g + 1u];
    const bool bad = lo > hi || hi > nsamples;
    uint64_t s = 0;
    if (!bad)
        for (uint32_t i = lo + t; i < hi; i += kThreads) s += src_len[i];
    s = block_sum(s, sh);
    if (t == 0) {
        groups[g].base = s;
        groups[g].code = bad ? (int32_t)kErrInvalidState : 0;
    }
}

// One workgroup: the groups' places (an exclusive scan of S + kPad over the groups that take part) and their state.
__global__ __launch_bounds__(1024) void k_train_plan(TrainGroup *__restrict__ groups, uint32_t ngroups,
                                                     const uint32_t *__restrict__ dict_cap, uint64_t N, uint32_t max_cap,
                                                     TrainParams P) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (ngroups + 1023u) / 1024u;
    const uint64_t b0 = (uint64_t)t * chunk;
    const uint32_t lo = b0 < ngroups ? (uint32_t)b0 : ngroups;
    const uint32_t hi = b0 + chunk < ngroups ? (uint32_t)(b0 + chunk) : ngroups;
    auto valid = [&](uint32_t g) {
        return groups[g].code == 0 && groups[g].base <= kTrainMaxGroup && dict_cap[g] <= max_cap;
    };
    auto need = [&](uint32_t g) -> uint64_t { return valid(g) ? groups[g].base + kPad : 0ull; };
    uint64_t s = 0;
    for (uint32_t g = lo; g < hi; g++) s += need(g);
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - s;
    for (uint32_t g = lo; g < hi; g++) {
        const uint64_t n = need(g);
        const bool ok = n != 0 && run + n <= N;           // (a group the workspace has no room for is refused)
        TrainGroup G;
        G.base = run;
        G.winner = 0;
        G.S = ok ? (uint32_t)groups[g].base : 0u;
        G.nd = G.S >= P.d ? G.S - P.d + 1u : 0u;
        G.C = ok ? dict_cap[g] : 0u;
        const uint32_t nseg = (G.C + P.k - 1u) / P.k;
        const uint32_t by_len = G.nd / (8u * P.k);
        const uint32_t e = nseg < by_len ? nseg : by_len;
        G.E = e > 0u ? e : 1u;
        G.size = G.nd / G.E;
        G.steps_left = 2u * nseg;
        G.tail = G.C;
        G.ep = 0;
        G.zero = 0;
        G.done = (!ok || G.nd == 0u || G.C == 0u) ? 1u : 0u;
        G.code = ok ? 0 : (int32_t)kErrInvalidState;
        G.reserved = 0;
        groups[g] = G;
        run += n;
    }
}

// Block x of group g packs a contiguous share of the group's samples: the bytes in front of its share are summed first,
// then every sample is copied by the whole workgroup.  Block 0 also zeroes the kPad bytes behind the group.
__global__ __launch_bounds__(kThreads) void k_train_pack(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                         const uint32_t *__restrict__ src_len,
                                                         const uint32_t *__restrict__ group_first,
                                                         const TrainGroup *__restrict__ groups, uint8_t *__restrict__ bytes) {
    __shared__ uint64_t sh[kThreads];
    __shared__ uint64_t s_off[kThreads];
    __shared__ uint32_t s_len[kThreads];
    const uint32_t g = blockIdx.y, t = threadIdx.x;
    const TrainGroup G = groups[g];
    if (G.done) return;
    uint8_t *B = bytes + G.base;
    if (blockIdx.x == 0 && t < kPad) B[G.S + t] = 0;
    const uint32_t first = group_first[g], n = group_first[g + 1u] - first;
    const uint32_t per = (n + gridDim.x - 1u) / gridDim.x;
    const uint64_t a64 = (uint64_t)blockIdx.x * per;
    const uint32_t a = a64 < n ? (uint32_t)a64 : n;
    const uint32_t z = a64 + per < n ? (uint32_t)(a64 + per) : n;
    if (a >= z) return;
    uint64_t s = 0;
    for (uint32_t i = t; i < a; i += kThreads) s += src_len[first + i];
    uint64_t pos = block_sum(s, sh);
    for (uint32_t c = a; c < z; c += kThreads) {
        const uint32_t cnt = z - c < kThreads ? z - c : kThreads;
        __syncthreads();
        if (t < cnt) { s_off[t] = src_off[first + c + t]; s_len[t] = src_len[first + c + t]; }
        __syncthreads();
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t len = s_len[j];
            const uint8_t *from = src + s_off[j];
            for (uint32_t i = t; i < len; i += kThreads) B[pos + i] = from[i];     // (pos + len <= S: S is their sum)
            pos += len;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_train_count(const TrainGroup *__restrict__ groups, const uint8_t *__restrict__ bytes,
                                                          uint32_t *__restrict__ hash, uint32_t *__restrict__ freq,
                                                          TrainParams P) {
    const uint32_t g = blockIdx.y;
    const TrainGroup G = groups[g];
    if (G.done) return;
    const uint8_t *B = bytes + G.base;
    uint32_t *hs = hash + G.base;
    uint32_t *fq = freq + ((size_t)g << P.f);
    for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < G.nd; p += (uint64_t)gridDim.x * kThreads) {
        const uint32_t h = train_hash(ld64(B + p), P.d, P.f);        // (p + 8 <= S - d + 8 < S + kPad)
        hs[p] = h;
        atomicAdd(&fq[h], 1u);
    }
}

__global__ __launch_bounds__(kThreads) void k_train_reach(const TrainGroup *__restrict__ groups, const uint32_t *__restrict__ hash,
                                                          uint16_t *__restrict__ dist, TrainParams P) {
    __shared__ uint32_t sh[kReachTile + kHalo];
    const uint32_t g = blockIdx.y, t = threadIdx.x;
    const TrainGroup G = groups[g];
    if (G.done) return;
    const uint32_t *hs = hash + G.base;
    uint16_t *ds = dist + G.base;
    const uint32_t halo = P.m - 1u;                                  // <= 1020
    for (uint64_t p0 = (uint64_t)blockIdx.x * kReachTile; p0 < G.nd; p0 += (uint64_t)gridDim.x * kReachTile) {
        const uint32_t q0 = (uint32_t)p0;
        const uint32_t lo = q0 >= halo ? q0 - halo : 0u;
        const uint32_t hi = G.nd - q0 < kReachTile ? G.nd : q0 + kReachTile;
        __syncthreads();
        for (uint32_t i = t; i < hi - lo; i += kThreads) sh[i] = hs[lo + i];       // hi - lo <= kReachTile + halo
        __syncthreads();
        for (uint32_t i = q0 - lo + t; lo + i < hi; i += kThreads) {
            const uint32_t h = sh[i];
            const uint32_t back = i < halo ? i : halo;               // (i < halo only where lo == 0: i is the position)
            uint32_t dj = 0;
            for (uint32_t j = 1; j <= back; j++)
                if (sh[i - j] == h) { dj = j; break; }
            ds[lo + i] = (uint16_t)dj;
        }
    }
}

__device__ __forceinline__ void epoch_of(const TrainGroup &G, uint32_t &b, uint32_t &e) {
    b = G.ep * G.size;
    e = G.ep == G.E - 1u ? G.nd : b + G.size;
}

__global__ __launch_bounds__(kThreads) void k_train_score(TrainGroup *__restrict__ groups, const uint32_t *__restrict__ hash,
                                                          const uint16_t *__restrict__ dist, const uint32_t *__restrict__ freq,
                                                          TrainParams P) {
    __shared__ uint32_t w[kScoreTile + kHalo];
    __shared__ uint16_t dd[kScoreTile + kHalo];
    __shared__ uint64_t red[kThreads];
    const uint32_t g = blockIdx.y, t = threadIdx.x;
    const TrainGroup G = groups[g];
    if (G.done) return;
    uint32_t b, e;
    epoch_of(G, b, e);
    const uint32_t len = e - b;
    if ((uint64_t)blockIdx.x * kScoreTile >= len) return;
    const uint32_t *hs = hash + G.base;
    const uint16_t *ds = dist + G.base;
    const uint32_t *fq = freq + ((size_t)g << P.f);
    uint64_t best = 0;
    for (uint64_t t0 = (uint64_t)blockIdx.x * kScoreTile; t0 < len; t0 += (uint64_t)gridDim.x * kScoreTile) {
        const uint32_t s0 = b + (uint32_t)t0;
        const uint32_t want = kScoreTile + P.m - 1u;                 // <= kScoreTile + 1020
        const uint32_t cnt = e - s0 < want ? e - s0 : want;
        __syncthreads();
        for (uint32_t i = t; i < cnt; i += kThreads) {
            w[i] = fq[hs[s0 + i]];
            dd[i] = ds[s0 + i];
        }
        __syncthreads();
        for (uint32_t i = t; i < kScoreTile && s0 + i < e; i += kThreads) {
            const uint32_t left = e - (s0 + i);
            const uint32_t lim = left < P.m ? left : P.m;            // i + lim <= cnt
            uint64_t sum = 0;
            for (uint32_t j = 0; j < lim; j++) {
                const uint32_t dj = dd[i + j];
                if (dj == 0u || dj > j) sum += w[i + j];
            }
            const uint64_t key = (sum << kPosBits) | (uint64_t)(kPosMask - ((uint32_t)t0 + i));
            best = key > best ? key : best;
        }
    }
    __syncthreads();
    red[t] = best;
    __syncthreads();
    for (uint32_t d = kThreads / 2u; d > 0u; d >>= 1) {
        if (t < d) red[t] = red[t + d] > red[t] ? red[t + d] : red[t];
        __syncthreads();
    }
    if (t == 0) atomicMax((unsigned long long *)&groups[g].winner, (unsigned long long)red[0]);
}

__global__ __launch_bounds__(kThreads) void k_train_commit(TrainGroup *__restrict__ groups, const uint8_t *__restrict__ bytes,
                                                           const uint32_t *__restrict__ hash, uint32_t *__restrict__ freq,
                                                           uint8_t *__restrict__ out, uint32_t out_stride, TrainParams P) {
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    const TrainGroup G = groups[g];
    if (G.done) return;
    uint32_t b, e;
    epoch_of(G, b, e);
    const uint64_t score = G.winner >> kPosBits;
    const uint32_t s = b + (kPosMask - (uint32_t)(G.winner & kPosMask));
    uint32_t tail = G.tail;
    if (score != 0 && s < e) {                                       // (s < e always: a guard for the index below)
        const uint32_t rest = G.S - s;
        uint32_t seg = P.k < tail ? P.k : tail;
        seg = seg < rest ? seg : rest;
        tail -= seg;
        const uint8_t *from = bytes + G.base + s;
        uint8_t *to = out + (size_t)g * out_stride + tail;
        for (uint32_t i = t; i < seg; i += kThreads) to[i] = from[i];
        const uint32_t *hs = hash + G.base;
        uint32_t *fq = freq + ((size_t)g << P.f);
        const uint32_t lim = e - s < P.m ? e : s + P.m;
        for (uint32_t p = s + t; p < lim; p += kThreads) fq[hs[p]] = 0;
    }
    __syncthreads();                                                 // every thread holds G before it changes
    if (t == 0) {
        TrainGroup *W = &groups[g];
        const uint32_t left = G.steps_left - 1u;
        uint32_t done;
        if (score == 0) {
            W->zero = G.zero + 1u;
            done = G.zero + 1u == G.E;
        } else {
            W->zero = 0;
            W->tail = tail;
            done = tail == 0u;
        }
        W->ep = G.ep + 1u == G.E ? 0u : G.ep + 1u;
        W->steps_left = left;
        W->done = (done || left == 0u) ? 1u : 0u;
        W->winner = 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_train_finish(const TrainGroup *__restrict__ groups, const uint8_t *__restrict__ out,
                                                           uint32_t out_stride, uint8_t *__restrict__ dict,
                                                           const uint64_t *__restrict__ dict_off, int64_t *__restrict__ result) {
    const uint32_t g = blockIdx.y;
    const TrainGroup G = groups[g];
    const uint32_t L = G.C - G.tail;                                 // (0 for a refused group)
    const uint8_t *from = out + (size_t)g * out_stride + G.tail;
    uint8_t *to = dict + dict_off[g];
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < L; i += gridDim.x * kThreads) to[i] = from[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) result[g] = G.code < 0 ? (int64_t)G.code : (int64_t)L;
}

}  // namespace
}  // namespace zlz4

using namespace zlz4;

extern "C" size_t zlz4_batch_train_dict_workspace(uint32_t ngroups, uint64_t total_sample_bytes, uint32_t max_dict_cap,
                                                  const zlz4_train_params *params) {
    if (!train_params_ok(params) || total_sample_bytes > (1ull << 46)) return 0;
    const uint64_t N = ((total_sample_bytes + 15u) & ~15ull) + (uint64_t)kPad * ((uint64_t)ngroups + 1u);
    return train_layout(ngroups, N, max_dict_cap, params->f).total;
}

extern "C" int32_t zlz4_batch_train_dict(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_len,
                                         uint32_t nsamples, const uint32_t *d_group_first, uint32_t ngroups, uint8_t *d_dict,
                                         const uint64_t *d_dict_off, const uint32_t *d_dict_cap, int64_t *d_result,
                                         uint32_t max_dict_cap, const zlz4_train_params *params, void *d_workspace,
                                         size_t workspace_bytes) {
    if (ngroups == 0) return 0;
    if (!train_params_ok(params) || ngroups > 65535u) return ZLZ4_ERR_INVALID_STATE;      // (the group is grid axis y)
    if (!d_group_first || !d_dict_off || !d_dict_cap || !d_result || (!d_dict && max_dict_cap) ||
        (nsamples && (!d_src || !d_src_off || !d_src_len)))
        return ZLZ4_ERR_INVALID_STATE;
    if (((uintptr_t)d_src_off | (uintptr_t)d_dict_off | (uintptr_t)d_result) & 7u ||
        ((uintptr_t)d_src_len | (uintptr_t)d_group_first | (uintptr_t)d_dict_cap) & 3u)
        return ZLZ4_ERR_INVALID_STATE;
    const size_t fixed = zlz4_batch_train_dict_workspace(ngroups, 0, max_dict_cap, params);
    if (!d_workspace || ((uintptr_t)d_workspace & 15u) || workspace_bytes < fixed) return ZLZ4_ERR_INVALID_STATE;
    if (!zlz4host::device_ok()) return ZLZ4_ERR_DEVICE;

    // the sample space the workspace holds: what is left behind the fixed regions, 7 bytes per element
    const uint64_t N0 = (uint64_t)kPad * ((uint64_t)ngroups + 1u);
    const uint64_t N = N0 + (((uint64_t)(workspace_bytes - fixed) / 7u) & ~15ull);
    const TrainLayout L = train_layout(ngroups, N, max_dict_cap, params->f);
    uint8_t *ws = (uint8_t *)d_workspace;
    TrainGroup *groups = (TrainGroup *)(ws + L.groups);
    uint8_t *out = ws + L.out;
    uint32_t *freq = (uint32_t *)(ws + L.freq);
    uint32_t *hash = (uint32_t *)(ws + L.hash);
    uint16_t *dist = (uint16_t *)(ws + L.dist);
    uint8_t *bytes = ws + L.bytes;
    const TrainParams P{params->d, params->k, params->f, params->k - params->d + 1u};
    const uint32_t cap = train_cap(max_dict_cap);
    hipStream_t st = (hipStream_t)stream;

    if (hipMemsetAsync(freq, 0, L.hash - L.freq, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
    hipLaunchKernelGGL(k_train_sum, dim3(ngroups), dim3(kThreads), 0, st, d_src_len, nsamples, d_group_first, groups);
    hipLaunchKernelGGL(k_train_plan, dim3(1), dim3(1024), 0, st, groups, ngroups, d_dict_cap, N, cap, P);
    const uint32_t per_group = 16384u / ngroups ? 16384u / ngroups : 1u;     // workgroups of one group in a launch
    const uint32_t gp = grid_of(nsamples / ngroups / 16u + 1u, 1, per_group < 256u ? per_group : 256u);
    hipLaunchKernelGGL(k_train_pack, dim3(gp, ngroups), dim3(kThreads), 0, st, d_src, d_src_off, d_src_len, d_group_first, groups,
                       bytes);
    const uint32_t gx = grid_of(N, kReachTile, per_group);
    hipLaunchKernelGGL(k_train_count, dim3(gx, ngroups), dim3(kThreads), 0, st, groups, bytes, hash, freq, P);
    hipLaunchKernelGGL(k_train_reach, dim3(gx, ngroups), dim3(kThreads), 0, st, groups, hash, dist, P);
    const uint32_t steps = 2u * ((cap + P.k - 1u) / P.k);
    const uint32_t gs = grid_of(N, kScoreTile, per_group);
    for (uint32_t i = 0; i < steps; i++) {
        hipLaunchKernelGGL(k_train_score, dim3(gs, ngroups), dim3(kThreads), 0, st, groups, hash, dist, freq, P);
        hipLaunchKernelGGL(k_train_commit, dim3(ngroups), dim3(kThreads), 0, st, groups, bytes, hash, freq, out, L.out_stride, P);
    }
    hipLaunchKernelGGL(k_train_finish, dim3(grid_of(cap, 4u * kThreads), ngroups), dim3(kThreads), 0, st, groups, out,
                       L.out_stride, d_dict, d_dict_off, d_result);
    return zlz4_launch_status();
}

extern "C" int64_t zlz4_train_dict(const uint8_t *samples, const size_t *sample_sizes, uint32_t nsamples, uint8_t *dict,
                                   size_t dict_cap, const zlz4_train_params *params) {
    using namespace zlz4host;
    if (!train_params_ok(params)) return ZLZ4_ERR_INVALID_STATE;
    if ((nsamples && !sample_sizes) || (dict_cap && !dict)) return ZLZ4_ERR_INVALID_STATE;
    uint64_t total = 0;
    for (uint32_t i = 0; i < nsamples; i++) {
        if (sample_sizes[i] > kTrainMaxGroup) return ZLZ4_ERR_INVALID_STATE;
        total += sample_sizes[i];
    }
    if (dict_cap > kTrainMaxDict || total > kTrainMaxGroup || (total && !samples)) return ZLZ4_ERR_INVALID_STATE;
    if (total < params->d || dict_cap == 0) return 0;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;

    struct Rec { uint64_t dict_off; int64_t result; uint32_t first[2]; uint32_t cap; };
    std::vector<uint64_t> off(nsamples);
    std::vector<uint32_t> len(nsamples);
    uint64_t pos = 0;
    for (uint32_t i = 0; i < nsamples; i++) { off[i] = pos; len[i] = (uint32_t)sample_sizes[i]; pos += sample_sizes[i]; }
    const size_t ws = zlz4_batch_train_dict_workspace(1, total, (uint32_t)dict_cap, params);
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    DevBuf d_src((size_t)total, &dc), d_off((size_t)nsamples * 8u, &dc), d_len((size_t)nsamples * 4u, &dc);
    DevBuf d_dict(dict_cap, &dc), d_ws(ws, &dc);
    Staged<Rec> rec(&dc);
    if (!d_src.p || !d_off.p || !d_len.p || !d_dict.p || !d_ws.p || !rec.d) return ZLZ4_ERR_ALLOCATION_FAILED;
    rec.h.first[1] = nsamples; rec.h.cap = (uint32_t)dict_cap;
    dc.launched();
    if (!upload(d_src, samples, (size_t)total, st) || !upload(d_off, off.data(), (size_t)nsamples * 8u, st) ||
        !upload(d_len, len.data(), (size_t)nsamples * 4u, st) || !rec.upload(st))
        return ZLZ4_ERR_DEVICE;
    Rec *r = rec.d;
    const int32_t rc = zlz4_batch_train_dict(st, d_src.as<uint8_t>(), d_off.as<uint64_t>(), d_len.as<uint32_t>(), nsamples,
                                             r->first, 1, d_dict.as<uint8_t>(), &r->dict_off, &r->cap, &r->result,
                                             (uint32_t)dict_cap, params, d_ws.p, ws);
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result) || !copy_back(dict, dict_cap, d_dict, result)) return ZLZ4_ERR_DEVICE;
    return result;
}
