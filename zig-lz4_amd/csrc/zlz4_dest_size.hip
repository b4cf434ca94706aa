// zlz4_dest_size.hip -- batch lz4.compressDestSize (reference src/lz4.zig:551-616) for gfx950.
//
// The reference binary-searches the largest prefix of src whose compressDefault output fits dst, one full compression
// per probe.  Here every block is compressed ONCE at full length (the unchanged k_compress_fast, into a workspace slot)
// and k_dest_size_plan derives the size of every probed prefix from that one stream (DESIGN.md section 4.5,
// tools/pyref/zig_lz4_dest_size.py):
//   compressDefault sees the input length only through mflimitPlusOne = srcSize - 12 and matchLimit = srcSize - 5
//   (:313-314).  With, per sequence j of the full stream, e_j = match end, f_j = the forwardIp of the attempt that
//   found the match (:327-333) and C_j = running max of max(f_j + 12, e_j + 13), compressDefault(src[:m]) shares the
//   first k(m) = #{j : C_j <= m} sequences with the full stream and ends with a short re-encoded tail:
//     case 1  f_{k+1} <= m - 12: sequence k+1 again, its match end cut to min(e, m - 5), then the last literals
//     case 2  otherwise: the last literals from e_k (e_0 = 0)
//   and every OutputTooSmall check of the reference fires exactly when that stream is longer than dst.len.
// fits(m) is not monotone in m, so the reference's probes are replayed one by one (the first one at m = cap, the
// `mid == N` and `low > N` exits included), never replaced by "largest prefix that fits".
//
// One wavefront per block, everything about the walk wave-uniform (SGPRs).  The stream is read through the decoder's
// 64-byte register window (lane i holds byte wbase + i, header bytes are pulled with v_readlane), with the next 64
// bytes loaded one window ahead.  The first walk leaves a checkpoint (running C, token offset, anchor) every G sequences
// in LDS; a probe counts the checkpoints with C <= m (ballot) and re-walks at most G sequences from the last one.  G is
// 64 for blocks up to 64 KiB (at most 13 110 sequences = 205 checkpoints) and grows with the block so that 256
// checkpoints always suffice (a sequence consumes at least 5 input bytes): 3 KiB of LDS per wavefront whatever
// max_in_len.  The walk is lazy: it only goes as far as the largest probe so far needs.
#include "zlz4_device.hpp"
#include "zlz4_launch.hpp"

namespace zlz4 {

constexpr uint32_t kCkMax = 256;     // checkpoints per wavefront
constexpr uint32_t kCkMinGap = 64;   // sequences between checkpoints (at least)
constexpr uint32_t kSlotPad = 128;   // bytes behind every stream slot: the window loads need no bounds test

// the step taken after the attempt that found a match `lit` (>= 1) bytes after its literal start a.  The search
// starts at s = a + 1 (:438-442, the first sequence at 1 = 0 + 1); attempt 0 visits s and steps 1, attempt t >= 1
// visits s + 1 + S(t) (S(t) = sum_{y < t} (y >> 6)) and steps t >> 6.  A revisit of the same position sees its own
// entry and fails `match < ip`, so the match is found at the first t with s + 1 + S(t) = p, i.e. D = p - s - 1 =
// S(64 q + r) = 32 q (q - 1) + q r, step q.
__device__ __forceinline__ uint32_t dsz_step(uint32_t lit) {
    if (lit == 1u) return 1u;
    if (lit == 2u) return 0u;
    const uint32_t D = lit - 2u;                                       // D = p - s - 1 = (a + lit) - (a + 1) - 1 >= 1
    uint32_t q = (uint32_t)__builtin_sqrtf((float)D * (1.0f / 32.0f)); // largest q >= 1 with 32 q (q - 1) <= D
    if (q < 1u) q = 1u;
    while (q > 1u && 32ull * q * (q - 1u) > D) q--;
    while (32ull * (q + 1u) * q <= D) q++;
    return q;
}

__device__ __forceinline__ uint32_t dsz_last_lits(uint32_t lit) { return lit ? 1u + ext_len_bytes(lit) + lit : 0u; }

// 64-byte register window over one stream, the next 64 bytes in flight
struct DszWindow {
    const uint8_t *s;
    uint32_t base, w0, w1;
    __device__ __forceinline__ void load(uint32_t pos, uint32_t lane) {
        base = pos;
        w0 = s[pos + lane];
        w1 = s[pos + 64u + lane];
    }
    __device__ __forceinline__ uint32_t byte(uint32_t x, uint32_t lane) {
        uint32_t k = x - base;
        if (k >= 64u) {
            if (k < 128u) {                                             // slide by one window
                base += 64u;
                w0 = w1;
                w1 = s[base + 64u + lane];
            } else {
                load(x, lane);
            }
            k = x - base;
        }
        return rdlane(w0, k);
    }
};

// one sequence of the full stream: token at O, literals [a, p), match [p, e), the next token at nxt
struct DszSeq {
    uint32_t O, a, lit, p, e, off, f, nxt;
    bool last;                                                          // the last-literals token
};

__device__ __forceinline__ DszSeq dsz_parse(DszWindow &win, uint32_t O, uint32_t a, uint32_t slen, uint32_t lane) {
    DszSeq s;
    s.O = O;
    s.a = a;
    const uint32_t tok = win.byte(O, lane);
    uint32_t q = O + 1u, lit = tok >> 4;
    if (lit == 15u) {
        uint32_t b;
        do { b = win.byte(q, lane); q++; lit += b; } while (b == 255u);
    }
    q += lit;
    s.lit = lit;
    s.p = a + lit;
    s.last = q >= slen;
    if (s.last) { s.e = s.p; s.off = 0; s.f = 0; s.nxt = q; return s; }
    s.off = win.byte(q, lane) | (win.byte(q + 1u, lane) << 8);
    q += 2u;
    uint32_t ml = tok & 15u;
    if (ml == 15u) {
        uint32_t b;
        do { b = win.byte(q, lane); q++; ml += b; } while (b == 255u);
    }
    s.e = s.p + ml + kMinMatch;
    s.f = s.p + dsz_step(lit);
    s.nxt = q;
    return s;
}

__device__ __forceinline__ uint32_t dsz_c(const DszSeq &s) {
    const uint32_t x = s.f + kMfLimit, y = s.e + kMfLimit + 1u;
    return x > y ? x : y;
}

// d_ws_res[i] / stream slot i (d_ws_stream + i * slot): the full-length compressDefault of block i
__global__ __launch_bounds__(64) void k_dest_size_plan(const uint8_t *__restrict__ d_in, const uint64_t *__restrict__ d_in_off,
                                                       const uint32_t *__restrict__ d_in_len, uint8_t *__restrict__ d_out,
                                                       const uint64_t *__restrict__ d_out_off, const uint32_t *__restrict__ d_out_cap,
                                                       int64_t *__restrict__ d_result, uint32_t *__restrict__ d_consumed,
                                                       uint32_t nblocks, uint32_t max_in_len,
                                                       const uint8_t *__restrict__ d_ws_stream, uint64_t slot,
                                                       const int64_t *__restrict__ d_ws_res) {
    __shared__ uint32_t ck_C[kCkMax], ck_O[kCkMax], ck_a[kCkMax];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t blk = rfl(blockIdx.x);
    if (blk >= nblocks) return;
    const uint32_t n = rfl(d_in_len[blk]);
    int64_t res = 0;
    uint32_t consumed = 0;
    const int64_t full = d_ws_res[blk];
    if (n > max_in_len) {
        res = kErrInvalidState;                                         // the batch precondition (include/zlz4_amd.h)
    } else if (full < 0) {
        res = full;                                                     // (cannot happen: the slot holds compressBound)
    } else if (n != 0) {                                                // :553-556
        const uint8_t *src = d_in + d_in_off[blk];
        uint8_t *dst = d_out + d_out_off[blk];
        const uint8_t *stream = d_ws_stream + (uint64_t)blk * slot;
        const uint32_t cap = rfl(d_out_cap[blk]);
        const uint32_t slen = (uint32_t)full;
        if ((uint64_t)cap >= (uint64_t)n + n / 255u + 16u) {            // :559-564 cap >= compressBound(n)
            copy_bytes(dst, stream, slen, lane);
            res = slen;
            consumed = n;
        } else {
            DszWindow win;
            win.s = stream;
            win.load(0, lane);
            // the lazy first walk: frontier state after fj sequences
            const uint32_t smax = n / 5u + 2u;
            const uint32_t gap = smax > kCkMax * kCkMinGap ? (smax + kCkMax - 1u) / kCkMax : kCkMinGap;
            uint32_t fO = 0, fa = 0, fC = 0, fj = 0, ncp = 0;
            bool fdone = false;
            // seq k+1 of the last probe and the anchor of its last literals (see `size`)
            DszSeq t;
            bool case1 = false;
            uint32_t anchor = 0, e2 = 0;
            auto size = [&](uint32_t m) -> uint32_t {
                if (m == 0u) return 0u;
                if (m < kMfLimit + 1u) return 1u + ext_len_bytes(m) + m;   // compressAsLiterals (:449-482)
                // extend the first walk until C > m: every checkpoint with C <= m exists
                while (!fdone && fC <= m) {
                    if (fj % gap == 0u && fj / gap < kCkMax) {          // (always: fewer than n / 5 sequences)
                        const uint32_t g = fj / gap;
                        if (lane == 0) { ck_C[g] = fC; ck_O[g] = fO; ck_a[g] = fa; }
                        ncp = g + 1u;
                    }
                    const DszSeq s = dsz_parse(win, fO, fa, slen, lane);
                    if (s.last) { fdone = true; break; }
                    const uint32_t c = dsz_c(s);
                    fC = c > fC ? c : fC;
                    fO = s.nxt; fa = s.e; fj++;
                }
                __syncthreads();                                        // (one wavefront: the checkpoint stores)
                // last checkpoint with C <= m (checkpoint 0 has C = 0)
                uint32_t cnt = 0;
                for (uint32_t r = 0; r < kCkMax; r += 64u) {
                    const uint32_t g = r + lane;
                    cnt += (uint32_t)__popcll(ballot(g < ncp && ck_C[g] <= m));
                }
                const uint32_t g = cnt - 1u;
                uint32_t O = rfl(ck_O[g]), a = rfl(ck_a[g]), C = rfl(ck_C[g]);
                for (;;) {                                              // at most `gap` sequences
                    t = dsz_parse(win, O, a, slen, lane);
                    if (t.last) break;
                    const uint32_t c = dsz_c(t);
                    C = c > C ? c : C;
                    if (C > m) break;
                    O = t.nxt; a = t.e;
                }
                case1 = !t.last && t.f + kMfLimit <= m;
                if (case1) {
                    e2 = t.e < m - kLastLiterals ? t.e : m - kLastLiterals;
                    anchor = e2;
                } else {
                    anchor = t.a;
                }
                uint32_t sz = t.O + dsz_last_lits(m - anchor);
                if (case1) sz += 1u + ext_len_bytes(t.lit) + t.lit + 2u + ext_len_bytes(e2 - t.p - kMinMatch);
                return sz;
            };
            // :567-612, probe for probe
            uint32_t low = 1, high = n, best = 0, best_c = 0;
            if (cap <= n) {
                const uint32_t sz = size(cap);
                if (sz <= cap) { best = cap; best_c = sz; low = cap + 1u; }
                else high = cap - 1u;
            }
            while (low <= high) {
                const uint32_t mid = low + (high - low) / 2u;
                if (mid == 0u || mid > n) break;
                const uint32_t sz = size(mid);
                if (sz <= cap) {
                    best = mid; best_c = sz;
                    if (mid == n) break;
                    low = mid + 1u;
                } else {
                    high = mid - 1u;
                }
                if (low > n) break;
            }
            res = best_c;
            consumed = best;
            // dst = compressDefault(src[:best]), exactly best_c bytes
            if (best >= kMfLimit + 1u) {
                (void)size(best);
                copy_bytes(dst, stream, t.O, lane);                     // the shared sequences
                uint32_t op = t.O;
                if (case1) {
                    const uint32_t ml = e2 - t.p - kMinMatch;
                    const uint32_t nl = ext_len_bytes(t.lit), nm = ext_len_bytes(ml);
                    if (lane == 0) dst[op] = (uint8_t)(((t.lit < 15u ? t.lit : 15u) << 4) | (ml < 15u ? ml : 15u));
                    if (t.lit >= 15u) write_ext_len(dst + op + 1u, t.lit, lane);
                    op += 1u + nl;
                    copy_bytes(dst + op, src + t.a, t.lit, lane);
                    op += t.lit;
                    if (lane == 0) { dst[op] = (uint8_t)t.off; dst[op + 1u] = (uint8_t)(t.off >> 8); }
                    op += 2u;
                    if (ml >= 15u) write_ext_len(dst + op, ml, lane);
                    op += nm;
                }
                anchor = case1 ? e2 : t.a;
                const uint32_t lit = best - anchor;                     // finishCompression (:484-519), lit >= 5
                if (lane == 0) dst[op] = (uint8_t)((lit < 15u ? lit : 15u) << 4);
                if (lit >= 15u) write_ext_len(dst + op + 1u, lit, lane);
                copy_bytes(dst + op + 1u + ext_len_bytes(lit), src + anchor, lit, lane);
            } else if (best > 0u) {                                     // compressAsLiterals, best <= 12
                if (lane == 0) dst[0] = (uint8_t)(best << 4);
                if (lane < best) dst[1u + lane] = src[lane];
            }
        }
    }
    if (lane == 0) {
        d_result[blk] = res;
        d_consumed[blk] = consumed;
    }
}

// the workspace slots the full-length compression writes into
__global__ void k_dest_size_prep(uint64_t *__restrict__ ws_off, uint32_t *__restrict__ ws_cap, uint64_t slot,
                                 uint32_t nblocks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblocks) return;
    ws_off[i] = (uint64_t)i * slot;
    ws_cap[i] = (uint32_t)(slot - kSlotPad);
}

}  // namespace zlz4

// Workspace layout: [result i64 x n][slot offset u64 x n][slot capacity u32 x n] (padded to 256 B) then n stream slots of
// compressBound(max_in_len) + kSlotPad bytes (rounded up to 256 B).
static uint64_t dsz_slot(uint32_t max_in_len) {
    const uint64_t bound = (uint64_t)max_in_len + max_in_len / 255u + 16u;
    return (bound + zlz4::kSlotPad + 255u) & ~255ull;
}

static uint64_t dsz_meta(uint32_t nblocks) { return ((uint64_t)nblocks * 20u + 255u) & ~255ull; }

extern "C" size_t zlz4_dest_size_workspace_bytes(uint32_t nblocks, uint32_t max_in_len) {
    if (nblocks == 0) return 0;
    return (size_t)(dsz_meta(nblocks) + (uint64_t)nblocks * dsz_slot(max_in_len));
}

extern "C" uint32_t zlz4_dest_size_slot_cap(uint32_t max_in_len) { return (uint32_t)(dsz_slot(max_in_len) - zlz4::kSlotPad); }

// d_slot_off / d_slot_cap: where the full-length compression of each block goes inside the workspace's stream area, and
// its capacity (zlz4_dest_size_slot_cap); NULL = this launcher writes them into the workspace's own table first (the
// single call stages them with its input instead)
extern "C" int zlz4_launch_compress_dest_size(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                              const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                              const uint32_t *d_out_cap, int64_t *d_result, uint32_t *d_consumed,
                                              uint32_t nblocks, uint32_t max_in_len, void *d_workspace,
                                              const uint64_t *d_slot_off, const uint32_t *d_slot_cap) {
    if (nblocks == 0) return 0;
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    int64_t *ws_res = reinterpret_cast<int64_t *>(ws);
    uint8_t *ws_stream = ws + dsz_meta(nblocks);
    const uint64_t slot = dsz_slot(max_in_len);
    if (!d_slot_off || !d_slot_cap) {
        uint64_t *ws_off = reinterpret_cast<uint64_t *>(ws + (uint64_t)nblocks * 8u);
        uint32_t *ws_cap = reinterpret_cast<uint32_t *>(ws + (uint64_t)nblocks * 16u);
        hipLaunchKernelGGL(zlz4::k_dest_size_prep, dim3((nblocks + 255u) / 256u), dim3(256), 0, stream, ws_off, ws_cap, slot,
                           nblocks);
        if (int rc = zlz4_launch_status()) return rc;
        d_slot_off = ws_off;
        d_slot_cap = ws_cap;
    }
    // (a) compressDefault of every whole block (a block longer than max_in_len gets InvalidState there and here)
    const int rc = zlz4_launch_compress_fast(stream, d_in, d_in_off, d_in_len, ws_stream, d_slot_off, d_slot_cap, ws_res,
                                             nblocks, max_in_len, 1);
    if (rc != 0) return rc;
    // (b) the search and the output of every block
    hipLaunchKernelGGL(zlz4::k_dest_size_plan, dim3(nblocks), dim3(64), 0, stream, d_in, d_in_off, d_in_len, d_out,
                       d_out_off, d_out_cap, d_result, d_consumed, nblocks, max_in_len, ws_stream, slot, ws_res);
    return zlz4_launch_status();
}
