// zlz4_device.hpp -- wave64 helpers shared by the gfx950 LZ4 kernels.
// One wavefront owns one independent LZ4 block; everything "scalar" about the
// block (ip, op, anchor, lengths) is wave-uniform and lives in SGPRs, the 64
// lanes are used for probing 64 hash positions at once, match-length
// extension (ballot + ffs) and byte copies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

// Experiment / A-B knobs exist only in the diagnostic builds (-DZLZ4_TUNING: `make tuning`,
// `make stamps`); the shipped library reads no environment variable.
#ifdef ZLZ4_TUNING
static inline const char *zlz4_tune_env(const char *name) { return getenv(name); }
#else
static inline const char *zlz4_tune_env(const char *) { return nullptr; }
#endif

namespace zlz4 {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kMinMatch = 4;        // src/lz4.zig:12
constexpr uint32_t kLastLiterals = 5;    // src/lz4.zig:14
constexpr uint32_t kMfLimit = 12;        // src/lz4.zig:15
constexpr uint32_t kMaxInput = 0x7E000000u;  // src/lz4.zig:23
constexpr uint32_t kMaxDist = 65535u;    // src/lz4.zig:24-25
constexpr uint32_t kHashMul = 2654435761u;   // src/lz4.zig:44

constexpr int64_t kErrOutputTooSmall = -1;   // lz4.Error order, src/lz4.zig:48-55
constexpr int64_t kErrInputTooLarge = -2;
constexpr int64_t kErrCorrupted = -3;
constexpr int64_t kErrInvalidState = -5;   // also: a batch block longer than the call's max_in_len (include/zlz4_amd.h)

// the per-block bound of the StreamDecode decoder builds (k_decompress_safe, kBound): lo <= kBoundMax is a bound, the
// other two values skip the block (kBoundSkip) or store InvalidState (kBoundInvalid)
constexpr uint32_t kBoundSkip = 0xFFFFFFFFu, kBoundInvalid = 0xFFFFFFFEu, kBoundMax = 0xFFFF0000u;

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t rdlane(uint32_t v, uint32_t l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
__device__ __forceinline__ uint32_t first_lane(uint64_t m) { return (uint32_t)__ffsll((long long)m) - 1u; }  // m != 0
// NOTE: call it from wave-uniform control flow only -- ds_bpermute reads 0 from lanes that are masked off.
__device__ __forceinline__ uint32_t shfl(uint32_t v, uint32_t src_lane) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src_lane << 2), (int)v);
}

// number of set bits of `mask` below this lane, popcount(mask & lanes_below), as v_mbcnt_lo + v_mbcnt_hi: no lanes_below
// operand, two instructions where the popcount form takes four
__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
// this lane's bit of the wave-uniform `mask`, (mask >> lane) & 1: the mask is used as the lane's condition as it stands
// (the inverse of a ballot), nothing is computed per lane
__device__ __forceinline__ bool in_mask(uint64_t mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }

// lane i reads lane i - 1 (lane 0 reads 0): DPP wave_shr:1, which crosses the 16-lane rows
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true);
}

// (a + kOff) & 0xFF in one instruction: SDWA keeps the low byte of the sum and pads the rest with zeros.  For ds_bpermute
// addresses (4 * lane index): in a byte they wrap modulo 64 lanes.  Only ds_bpermute may read the result (the compiler
// does not see the partial write inside the statement, so no VALU instruction should consume it right behind).
template <uint32_t kOff>
__device__ __forceinline__ uint32_t add_wrap_byte(uint32_t a) {
    static_assert(kOff <= 64u, "inline constant");
    uint32_t r;
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD"
        : "=v"(r) : "v"(a), "n"(kOff));
    return r;
}

// write the wave-uniform `val` into lane `l` (uniform) of `old` (v_cmp + v_cndmask; VALU has headroom here)
__device__ __forceinline__ uint32_t wrlane(uint32_t val, uint32_t l, uint32_t old) {
    return (__lane_id() == l) ? val : old;
}

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ u32x4 ld128(const uint8_t *p) { u32x4 v; __builtin_memcpy(&v, p, 16); return v; }
__device__ __forceinline__ void st128(uint8_t *p, u32x4 v) { __builtin_memcpy(p, &v, 16); }

// index of the first differing byte of two 16-byte vectors, 16 if equal
__device__ __forceinline__ uint32_t first_diff16(u32x4 a, u32x4 b) {
    const uint32_t x0 = a.x ^ b.x, x1 = a.y ^ b.y, x2 = a.z ^ b.z, x3 = a.w ^ b.w;
    if (x0) return (uint32_t)__builtin_ctz(x0) >> 3;
    if (x1) return 4u + ((uint32_t)__builtin_ctz(x1) >> 3);
    if (x2) return 8u + ((uint32_t)__builtin_ctz(x2) >> 3);
    if (x3) return 12u + ((uint32_t)__builtin_ctz(x3) >> 3);
    return 16u;
}

// the same with selects only (no divergent branches: for per-lane loops whose cost is scalar exec-mask handling)
__device__ __forceinline__ uint32_t first_diff16_sel(u32x4 a, u32x4 b) {
    const uint32_t x0 = a.x ^ b.x, x1 = a.y ^ b.y, x2 = a.z ^ b.z, x3 = a.w ^ b.w;
    const uint32_t lo = x0 ? x0 : x1, hi = x2 ? x2 : x3;
    const uint32_t blo = x0 ? 0u : 4u, bhi = x2 ? 8u : 12u;
    const bool in_lo = (x0 | x1) != 0;
    const uint32_t x = in_lo ? lo : hi;
    const uint32_t base = in_lo ? blo : bhi;
    return x ? base + ((uint32_t)__builtin_ctz(x) >> 3) : 16u;
}

// Wave-cooperative forward copy of n bytes (n wave-uniform).  Chunks of 1 KiB
// (16 B per lane, unaligned dwordx4) in increasing address order, then a byte
// tail.  Safe for dst/src in the same buffer when dst - src >= 1024 or the
// ranges do not overlap.
__device__ __forceinline__ void copy_bytes(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane) {
    uint32_t k = lane * 16u;
    for (; k + 16u <= n; k += 1024u) st128(dst + k, ld128(src + k));
    const uint32_t t0 = n & ~15u;
    if (t0 + lane < n && lane < 16u) dst[t0 + lane] = src[t0 + lane];
}

// inclusive prefix sum over the 64 lanes (DPP: Hillis-Steele inside each row of 16, then row broadcasts)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);    // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);    // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);    // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);    // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1, 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2, 3
    return x;
}

__device__ __forceinline__ uint64_t rfl64(uint64_t v) { return ((uint64_t)rfl((uint32_t)(v >> 32)) << 32) | rfl((uint32_t)v); }
__device__ __forceinline__ uint32_t byte_at(const uint8_t *p) { return rfl((uint32_t)*p); }   // wave-uniform address

// decompressGeneric (src/lz4.zig:89-251) of one block by one wavefront, straight from the reference's loop: the serial
// walk of the two decoders that cannot run a block per wavefront in parallel.  `out` is where the block's output starts,
// `hist` the bytes in front of it that a match may reach (<= 65536).  :181-192 with dict.len = hist: CorruptedData iff
// offset > op + hist; every other match is a copy to out + op, in the output from out + op - offset (overlap rule
// included), its byte stores following the general path of k_decompress_safe.
// kWrite false: the same walk without a byte written or read from the output (the size query).
// kDict: the `hist` bytes are the tail of T ++ (the `inframe` bytes directly in front of `out`), T an external buffer that
// ends at `tend`.  A match that starts more than `inframe` bytes in front of the block starts in T: its first bytes come
// from tend - a (a = offset - op - inframe), it may end there or run across T's end into the bytes that follow it, from
// where it is the in-output match at distance `offset`.
// kBound: `lo` is a floor inside the output: a match at op with offset o is CorruptedData unless op - o >= lo (:181-185
// without a dictionary; lo <= kBoundMax, so offset + lo cannot wrap).
// kPartial: prefix decoding (DESIGN.md sections 4.2e / 4.4f): oend is the number of bytes wanted and the sequence that would
// pass it is cut there instead of being OutputTooSmall.  The walk stops with op == oend as soon as that many bytes are out
// -- at the top of the loop, behind the literal copy, behind the match copy -- and nothing behind that point is read or
// validated.  The two OutputTooSmall exits become clamps of the length about to be copied (the T part of a dictionary match
// takes its share of the clamped length); every copy moves exactly the bytes asked for, so no store lands at or past
// out + oend.
// Callers:
//   k_bfl_decode (zlz4_frame_linked.hip, DESIGN.md sections 4.4c / 4.4d): block k of a linked frame at out = dst + pos,
//     inframe = min(pos, 65536); <kWrite> with hist = inframe, <kWrite, true> with T the frame's dictionary tail of D
//     bytes and hist = min(pos + D, 65536).
//   k_sd_finish (zlz4_stream_decode.hip): a call re-decoded with its true entry state;
//     <true, true> with a pending dictionary (lowPrefix = dst: inframe = 0, hist = its reachable length, tend = its end),
//     <true, false, true> with lowPrefix = dst + lo and no dictionary (hist = 0).
//   k_bfp_decode (zlz4_frame_linked.hip): the blocks of a frame up to the cut, <true, kDict, false,
//     true> with oend = the bytes still wanted.
template <bool kWrite, bool kDict = false, bool kBound = false, bool kPartial = false>
__device__ int64_t decode_block_wave(const uint8_t *src, uint32_t iend, uint8_t *out, uint32_t oend, uint32_t hist,
                                     uint32_t lane, const uint8_t *tend = nullptr, uint32_t inframe = 0, uint32_t lo = 0) {
    if (iend == 0 || oend == 0) return 0;                              // :97-98
    uint32_t ip = 0, op = 0;
    for (;;) {
        if (ip >= iend) break;                                         // :113
        if constexpr (kPartial) { if (op >= oend) break; }             // (prefix: every byte wanted is out)
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
            if constexpr (kPartial) {                                  // (prefix: the literals that fit; when they fill
                const uint32_t nl = lit < oend - op ? lit : oend - op; //  the output, nothing behind them is read)
                if (kWrite) copy_bytes(out + op, src + ip, nl, lane);
                ip += lit; op += nl;
                if (op >= oend) break;
            } else {
                if (lit > oend - op) return kErrOutputTooSmall;
                if (kWrite) copy_bytes(out + op, src + ip, lit, lane);
                ip += lit; op += lit;
            }
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
        if constexpr (kPartial) {
            if (ml > oend - op) ml = oend - op;                        // (prefix: the first oend - op >= 1 bytes)
        } else {
            if (ml > oend - op) return kErrOutputTooSmall;             // :174
        }
        if (offset > op && offset - op > hist) return kErrCorrupted;   // :181-192: in front of the history
        if constexpr (kBound) {
            if (offset + lo > op) return kErrCorrupted;                // :183-185: below lowPrefix, no dictionary
        }
        if (kWrite) {                                                  // :195-248: out[op + k] = out[op - offset + k]
            uint8_t *o = out + op;
            uint32_t n = ml;
            if constexpr (kDict) {
                if (offset > op + inframe) {                           // :199-225: the part that lies in T comes first
                    const uint32_t a = offset - op - inframe, n1 = a < n ? a : n;
                    copy_bytes(o, tend - a, n1, lane);
                    o += n1;
                    n -= n1;
                }
            }
            const uint8_t *m = o - offset;
            if (n == 0) {
                // (the match ended inside T)
            } else if (offset >= n || offset >= 1024u) {
                copy_bytes(o, m, n, lane);
            } else {
                // overlap (:235-241): what is made so far is copied again as a whole -- offset bytes, then 2 x, 4 x ... --
                // each copy disjoint from its source, and `made` a multiple of offset until the last one
                uint32_t made = 0;
                while (made < n) {
                    const uint32_t have = made + offset, left = n - made;
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

// number of extension bytes the LZ4 length code needs for a value v >= 15 (token nibble saturated)
__device__ __forceinline__ uint32_t ext_len_bytes(uint32_t v) { return v >= 15u ? 1u + (v - 15u) / 255u : 0u; }

// Wave-cooperative write of the 255-run length extension of value v (>= 15) at p:
// (v-15)/255 bytes of 255 followed by (v-15)%255.  src/lz4.zig:368-382, :416-429.
__device__ __forceinline__ void write_ext_len(uint8_t *p, uint32_t v, uint32_t lane) {
    const uint32_t rem = v - 15u;
    const uint32_t n255 = rem / 255u;
    for (uint32_t k = lane; k < n255; k += 64u) p[k] = 255;
    if (lane == 0) p[n255] = (uint8_t)(rem - n255 * 255u);
}

}  // namespace zlz4
