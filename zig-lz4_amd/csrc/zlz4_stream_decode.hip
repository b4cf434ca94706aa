// zlz4_stream_decode.hip -- StreamDecode.decompressSafeContinue over whole streams (src/lz4.zig:870-957).
//
// A call never reads a byte of the previous call's output: without a dictionary a match below lowPrefix is CorruptedData
// (:181-185) and every other match reads the current dst (:229-231).  The previous output matters only through its
// address and length, so every block of a stream can be decoded at once; what has to be resolved is each call's ENTRY
// state, which picks how the block is decoded -- its "key":
//   kKeyDict            decompressSafeUsingDict with the stream's dictionary (a pending setStreamDecode dictionary),
//   kKeyInvalid         a state with both a dictionary and a prefix (unreachable through the API): InvalidState,
//   lo (<= kBoundMax)   decompressGeneric with lowPrefix = dst + lo, no dictionary (lo = max(0, prefix - dst)); mode A
//                       (decompressSafe) is lo = 0.
// The entry state of call j is the stream's state S0 if no earlier call of its run succeeded, else the state left by
// the last earlier success p: (null, 0, dst_p, r_p) -- mode A after a 0-byte success, a bound after r_p > 0.
//
// Launch sequence (fixed): k_sd_plan<kSpec> guesses that every earlier call succeeded with
// r > 0 and the decoder runs every block; two rounds of k_sd_plan<kRedo> + decoder re-run the blocks whose true key
// (from the results so far) differs from the key they ran with; k_sd_plan<kCheck> flags the runs that still differ
// (or whose look-back ran past kLookback calls) and marks, per run, its last success and whether a success had a
// mode-B entry; k_sd_finish walks the flagged runs one call after another (one wavefront per run, re-decoding with
// decode_block_wave of zlz4_device.hpp where needed) and writes every run's final state.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zlz4_amd.h"
#include "zlz4_device.hpp"
#include "zlz4_launch.hpp"

namespace zlz4 {

constexpr uint64_t kKeyDict = 1ull << 32, kKeyInvalid = 2ull << 32;
constexpr uint32_t kLookback = 64;        // calls a k_sd_plan thread walks back before leaving its run to k_sd_finish
enum : uint32_t { kSpec = 0, kRedo = 1, kCheck = 2 };
enum : uint32_t { kRunUnresolved = 1, kRunHadB = 2 };

struct SdState { uint64_t dict, dict_len, prefix, prefix_len; };   // zlz4_stream_decode_t

struct SdWork {                            // carved out of the caller's workspace (zlz4_sd_workspace_bytes)
    uint64_t *key;                         // the key each block's current result was decoded with
    uint64_t *dict_addr;                   // the run's dictionary tail address (d_dict_off of the dict build, base 0)
    uint32_t *dl;                          // 2n: dictionary lengths, then the dict build's bounds (0 or kBoundSkip)
    uint32_t *bl;                          // 2n: unused, then the no-dict build's bounds
    uint32_t *run_last;                    // per run: 1 + the last successful call (0: none)
    uint32_t *run_flags;                   // per run: kRunUnresolved | kRunHadB
};

__device__ __forceinline__ uint64_t bound_of(uint64_t prefix, uint64_t dst) {
    if (prefix <= dst) return 0;
    const uint64_t d = prefix - dst;
    return d < kBoundMax ? d : kBoundMax;
}

// key of a call entered with state st at destination dst; *mode_b = the call takes branch B (:925-938)
__device__ __forceinline__ uint64_t key_of_state(const SdState &st, uint64_t dst, bool *mode_b) {
    *mode_b = !(st.prefix_len == 0 && st.dict_len == 0);              // :914
    if (!*mode_b) return 0;
    if (st.dict_len > 0 && st.prefix != 0) return kKeyInvalid;        // (restStart would underflow, :213)
    if (st.dict_len > 0 && st.dict != 0) return kKeyDict;             // prefix null: lowPrefix = dst (:921-927)
    return bound_of(st.prefix ? st.prefix : dst, dst);                // :921-924, no dictionary
}

__device__ __forceinline__ SdState load_state(const uint64_t *d_state, uint32_t s) {
    SdState st;
    st.dict = d_state[4 * s + 0]; st.dict_len = d_state[4 * s + 1];
    st.prefix = d_state[4 * s + 2]; st.prefix_len = d_state[4 * s + 3];
    return st;
}

// run holding call j: the largest s with run_start[s] <= j, or nstreams if j lies in no run
__device__ __forceinline__ uint32_t run_of(const uint32_t *run_start, uint32_t nstreams, uint32_t j) {
    if (nstreams == 0 || j < run_start[0] || j >= run_start[nstreams]) return nstreams;
    uint32_t a = 0, b = nstreams;                                      // run_start[a] <= j < run_start[b]
    while (b - a > 1u) {
        const uint32_t m = (a + b) >> 1;
        if (run_start[m] <= j) a = m; else b = m;
    }
    return a;
}

// One thread per call.  kSpec: the guessed key; kRedo: the true key from the current results, re-run if it changed;
// kCheck: no decoding, only the run flags, the last success and the mode-B mark.
template <uint32_t kMode>
__global__ __launch_bounds__(256) void k_sd_plan(uint8_t *d_out, const uint64_t *__restrict__ d_out_off,
                                                 const uint32_t *__restrict__ d_run_start,
                                                 const uint64_t *__restrict__ d_state, const int64_t *d_result,
                                                 uint32_t nblocks, uint32_t nstreams, SdWork w) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < nblocks;
    const uint32_t s = live ? run_of(d_run_start, nstreams, j) : nstreams;
    uint64_t key = kKeyInvalid;
    bool mode_b = false, resolved = true, ok = false;
    SdState st = {0, 0, 0, 0};
    if (live && s < nstreams) {
        const uint32_t rs = d_run_start[s];
        st = load_state(d_state, s);
        const uint64_t dst = (uint64_t)(uintptr_t)d_out + d_out_off[j];
        if (kMode == kSpec) {
            if (j == rs) key = key_of_state(st, dst, &mode_b);
            else key = bound_of((uint64_t)(uintptr_t)d_out + d_out_off[j - 1], dst);
        } else {
            uint32_t k = j, steps = 0;
            bool found = false;
            while (k > rs && steps < kLookback) {
                k--; steps++;
                if (d_result[k] >= 0) { found = true; break; }
            }
            if (found) {
                const int64_t rp = d_result[k];
                mode_b = rp > 0;                                      // a 0-byte prefix enters mode A (:914)
                key = rp > 0 ? bound_of((uint64_t)(uintptr_t)d_out + d_out_off[k], dst) : 0;
            } else if (k == rs) {
                key = key_of_state(st, dst, &mode_b);
            } else {
                resolved = false;                                     // k_sd_finish walks this run
            }
        }
    }
    if (kMode != kCheck) {
        if (!live) return;
        bool run = true;
        if (kMode == kRedo) run = resolved && key != w.key[j];
        if (run) {
            w.key[j] = key;
            const bool dict = key == kKeyDict;
            const uint32_t tail = dict ? (uint32_t)(st.dict_len < 65536u ? st.dict_len : 65536u) : 0u;
            w.dict_addr[j] = dict ? st.dict + st.dict_len - tail : 0;  // the reachable tail (offset <= 65535)
            w.dl[j] = tail;
            w.dl[nblocks + j] = dict ? 0u : kBoundSkip;
            w.bl[nblocks + j] = dict ? kBoundSkip : (key == kKeyInvalid ? kBoundInvalid : (uint32_t)key);
        } else {
            w.dl[nblocks + j] = kBoundSkip;
            w.bl[nblocks + j] = kBoundSkip;
        }
        return;
    }
    // kCheck (every lane reaches the ballot below)
    const bool in_run = live && s < nstreams;
    if (in_run && (!resolved || key != w.key[j])) atomicOr(&w.run_flags[s], (uint32_t)kRunUnresolved);
    ok = in_run && d_result[j] >= 0;
    if (ok) {
        const uint32_t re = d_run_start[s + 1];
        if (j + 1u == re || d_result[j + 1] < 0) atomicMax(&w.run_last[s], j + 1u);
    }
    // one atomic per stretch of mode-B successes of a run inside the wavefront
    const bool hb = ok && mode_b;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t m = ballot(hb);
    const uint32_t prev_s = shfl(s, lane ? lane - 1u : 0u);
    const bool prev_hb = lane && ((m >> (lane - 1u)) & 1ull);
    if (hb && !(prev_hb && prev_s == s)) atomicOr(&w.run_flags[s], (uint32_t)kRunHadB);
}

// One wavefront per run: the final state; a run flagged by k_sd_plan<kCheck> is first walked call by call with the
// reference's state machine, re-decoding every call whose true key differs from the one its result was decoded with.
__global__ __launch_bounds__(64) void k_sd_finish(const uint8_t *d_in, const uint64_t *__restrict__ d_in_off,
                                                  const uint32_t *__restrict__ d_in_len, uint8_t *d_out,
                                                  const uint64_t *__restrict__ d_out_off,
                                                  const uint32_t *__restrict__ d_out_cap,
                                                  const uint32_t *__restrict__ d_run_start, uint64_t *d_state,
                                                  int64_t *d_result, uint32_t nstreams, SdWork w) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (s >= nstreams) return;
    SdState st = load_state(d_state, s);
    const uint32_t flags = rfl(w.run_flags[s]);
    if (!(flags & kRunUnresolved)) {
        const uint32_t last = rfl(w.run_last[s]);
        if (last == 0) return;                                         // no success: the state is untouched (`try`)
        const uint32_t p = last - 1u;
        const bool had_b = flags & kRunHadB;
        st.dict = had_b ? 0 : st.dict;                                 // :936 (mode A keeps externalDict, :917-918)
        st.dict_len = 0;
        st.prefix = (uint64_t)(uintptr_t)d_out + d_out_off[p];
        st.prefix_len = (uint64_t)d_result[p];
    } else {
        const uint32_t rs = rfl(d_run_start[s]), re = rfl(d_run_start[s + 1]);
        for (uint32_t j0 = rs; j0 < re; j0 += 64u) {
            const uint32_t jl = j0 + lane;
            const int64_t rl = jl < re ? __builtin_nontemporal_load(&d_result[jl]) : 0;
            const uint64_t kl = jl < re ? w.key[jl] : 0;
            const uint32_t nj = re - j0 < 64u ? re - j0 : 64u;
            for (uint32_t i = 0; i < nj; i++) {
                const uint32_t j = j0 + i;
                const uint64_t dst = (uint64_t)(uintptr_t)d_out + d_out_off[j];
                bool mode_b;
                const uint64_t key = key_of_state(st, dst, &mode_b);
                int64_t r = (int64_t)(((uint64_t)rdlane((uint32_t)((uint64_t)rl >> 32), i) << 32) | rdlane((uint32_t)rl, i));
                const uint64_t kj = ((uint64_t)rdlane((uint32_t)(kl >> 32), i) << 32) | rdlane((uint32_t)kl, i);
                if (key != kj) {
                    if (key == kKeyInvalid) {
                        r = kErrInvalidState;
                    } else {
                        const uint8_t *src = d_in + d_in_off[j];
                        uint8_t *out = (uint8_t *)(uintptr_t)dst;
                        const uint32_t iend = rfl(d_in_len[j]), oend = rfl(d_out_cap[j]);
                        if (key == kKeyDict) {                        // lowPrefix = dst, the dictionary's reachable tail
                            const uint32_t dlen = (uint32_t)(st.dict_len < 65536u ? st.dict_len : 65536u);
                            r = decode_block_wave<true, true>(src, iend, out, oend, dlen, lane,
                                                              (const uint8_t *)(uintptr_t)(st.dict + st.dict_len), 0u);
                        } else {                                      // lowPrefix = dst + key, no dictionary
                            r = decode_block_wave<true, false, true>(src, iend, out, oend, 0u, lane, nullptr, 0u, (uint32_t)key);
                        }
                    }
                    if (lane == 0) { d_result[j] = r; w.key[j] = key; }
                }
                if (r >= 0) {                                          // :916-919 / :935-938; errors leave st (`try`)
                    if (mode_b) { st.dict = 0; st.dict_len = 0; }
                    st.prefix = dst;
                    st.prefix_len = (uint64_t)r;
                }
            }
        }
    }
    if (lane == 0) {
        d_state[4 * s + 0] = st.dict; d_state[4 * s + 1] = st.dict_len;
        d_state[4 * s + 2] = st.prefix; d_state[4 * s + 3] = st.prefix_len;
    }
}

__host__ __device__ constexpr size_t align16(size_t x) { return (x + 15u) & ~(size_t)15u; }

}  // namespace zlz4

extern "C" size_t zlz4_sd_workspace_bytes(uint32_t nblocks, uint32_t nstreams) {
    using zlz4::align16;
    const size_t n = nblocks;
    return align16(8 * n) * 2 + align16(8 * n) * 2 + align16(4 * (size_t)nstreams) * 2;
}

extern "C" int zlz4_launch_stream_decode(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                         const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                         const uint32_t *d_out_cap, const uint32_t *d_run_start, uint64_t *d_state,
                                         int64_t *d_result, uint32_t nblocks, uint32_t nstreams, void *d_workspace) {
    using namespace zlz4;
    if (nstreams == 0) return 0;
    const size_t n = nblocks;
    uint8_t *p = static_cast<uint8_t *>(d_workspace);
    SdWork w;
    w.key = reinterpret_cast<uint64_t *>(p); p += align16(8 * n);
    w.dict_addr = reinterpret_cast<uint64_t *>(p); p += align16(8 * n);
    w.dl = reinterpret_cast<uint32_t *>(p); p += align16(8 * n);
    w.bl = reinterpret_cast<uint32_t *>(p); p += align16(8 * n);
    w.run_last = reinterpret_cast<uint32_t *>(p); p += align16(4 * (size_t)nstreams);
    w.run_flags = reinterpret_cast<uint32_t *>(p);
    if (hipMemsetAsync(w.run_last, 0, align16(4 * (size_t)nstreams) * 2, stream) != hipSuccess) return ZLZ4_ERR_DEVICE;
    const uint32_t pgrid = (nblocks + 255u) / 256u;
    auto decode = [&]() {
        int rc = zlz4_launch_decompress_safe_bound(stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_result,
                                                   nblocks, nullptr, w.dict_addr, w.bl, 0);
        if (rc == 0)
            rc = zlz4_launch_decompress_safe_bound(stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_result,
                                                   nblocks, nullptr, w.dict_addr, w.dl, 1);
        return rc;
    };
    if (nblocks) {
        hipLaunchKernelGGL(k_sd_plan<kSpec>, dim3(pgrid), dim3(256), 0, stream, d_out, d_out_off, d_run_start, d_state,
                           d_result, nblocks, nstreams, w);
        if (int rc = zlz4_launch_status()) return rc;
        if (int rc = decode()) return rc;
        for (int round = 0; round < 2; round++) {
            hipLaunchKernelGGL(k_sd_plan<kRedo>, dim3(pgrid), dim3(256), 0, stream, d_out, d_out_off, d_run_start,
                               d_state, d_result, nblocks, nstreams, w);
            if (int rc = zlz4_launch_status()) return rc;
            if (int rc = decode()) return rc;
        }
        hipLaunchKernelGGL(k_sd_plan<kCheck>, dim3(pgrid), dim3(256), 0, stream, d_out, d_out_off, d_run_start, d_state,
                           d_result, nblocks, nstreams, w);
        if (int rc = zlz4_launch_status()) return rc;
    }
    hipLaunchKernelGGL(k_sd_finish, dim3(nstreams), dim3(64), 0, stream, d_in, d_in_off, d_in_len, d_out, d_out_off,
                       d_out_cap, d_run_start, d_state, d_result, nstreams, w);
    return zlz4_launch_status();
}
