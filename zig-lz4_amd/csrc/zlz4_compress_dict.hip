// zlz4_compress_dict.hip -- LZ4 "fast" block compressor with an external dictionary for gfx950, one wavefront per block.
//
// zlz4_batch_compress_fast_using_dict (include/zlz4_amd.h).  No counterpart in the reference: its
// Stream.compressFastContinue reads every loaded table entry as a position in the current block (src/lz4.zig:656-659),
// so its blocks never refer to the dictionary.  This kernel runs the same loop, compressFastWithHashTable
// (src/lz4.zig:624-740), on the virtual buffer
//     V = tail ++ src          tail = the last D = min(dict_len, 65536) bytes of the dictionary
// with every position (table entries, ip, match, anchor) a position in V:
//   * the table starts as Stream.loadDict leaves it (:798-820): entry i for the 4-gram at tail[i], i.e. what
//     zlz4_batch_load_dict writes;
//   * anchor = D and ip = max(D, 1) at entry (:626-633 with the record starting at D);
//   * mflimitPlusOne = D + n - 12, matchLimit = D + n - 5 (:630-631);
//   * everything else is the reference's statement: validity `match > 0 and match < ip and match + 65535 >= ip and
//     rd32(V, match) == rd32(V, ip)` (:656-659), unconditional put (:661), skip schedule (:643-651), no backward
//     extension, forward extension V[ip] == V[match] up to matchLimit (:704-712, it may run from the dictionary into the
//     record and over itself), one put after a match (:732-736), offset = ip - match (:695), the OutputTooSmall tests.
// With D == 0 and a zero table this is compressFast.  A table that is not the dictionary's cannot break anything:
// `match < ip` bounds every read and the 4-byte compare vouches for every match.
//
// The 64-wide formulation of the serial probe loop is k_compress_fast's (header comment of zlz4_compress_fast.hip:
// data-independent probe schedule U(u), duplicate-hash groups by write / read-back plus ballot, first valid lane wins,
// later lanes restore their entries): its generic path, and its acceleration-1 window path without the input ring, the
// tags and the second-level guess (the generic path alone took 5.6x the time of k_compress_fast on 4 KiB records,
// profiles/r10_dict_compress.md).  Both carry over because only the meaning of a position changes: a position below D
// reads the tail, any other reads the record.  Probed positions are never below D, so the
// forward bytes and the literals always come from the record; only candidates and the match side of the extension can
// lie in the dictionary.  A candidate is gathered with ONE load from a per-lane 64-bit address (tail + p, or
// src - D + p); the lane whose read would straddle the dictionary's end (possible only in the extension, or with a
// foreign table) assembles it from bytes.
#include "zlz4_device.hpp"
#include "zlz4_launch.hpp"

namespace zlz4 {

namespace {

__device__ __forceinline__ uint32_t dc_hash4(uint32_t seq) { return (seq * kHashMul) >> 20; }   // src/lz4.zig:75-77

// S(x) = sum_{y < x} (y >> 6)
__device__ __forceinline__ uint32_t dc_skip_sum(uint32_t x) {
    const uint32_t q = x >> 6, r = x & 63u;
    return 32u * q * (q - 1u) + q * r;      // q == 0 -> 0
}

// literal-only sequence: compressAsLiterals (:449-482) and finishCompression (:484-519)
__device__ __forceinline__ int64_t dc_last_literals(uint8_t *dst, uint32_t dst_len, uint32_t op, const uint8_t *lit_src,
                                                    uint32_t lit, uint32_t lane) {
    if (lit == 0) return (int64_t)op;                                   // :488
    const uint32_t nle = ext_len_bytes(lit);
    if ((uint64_t)op + 1u + nle + lit > dst_len) return kErrOutputTooSmall;   // :491-514 / :454-477
    if (lane == 0) dst[op] = (uint8_t)((lit >= 15u ? 15u : lit) << 4);
    if (lit >= 15u) write_ext_len(dst + op + 1u, lit, lane);
    copy_bytes(dst + op + 1u + nle, lit_src, lit, lane);
    return (int64_t)(op + 1u + nle + lit);
}

// The two halves of V.  `srcv` = src - D, so that srcv + p is the record's byte for a position p >= D.
struct VBuf {
    const uint8_t *tail;
    const uint8_t *srcv;
    uint32_t D;
    uint32_t end;                                                       // D + n
    __device__ __forceinline__ const uint8_t *at(uint32_t p) const { return (p < D ? tail : srcv) + p; }
    __device__ __forceinline__ uint8_t byte(uint32_t p) const { return *at(p); }
    // k <= 16 bytes at p lie in one half
    __device__ __forceinline__ bool whole(uint32_t p, uint32_t k) const { return p >= D || p + k <= D; }
    // 16 bytes of V at p, p + 16 <= end; a read that straddles the dictionary's end is assembled from bytes
    __device__ __forceinline__ u32x4 ld128v(uint32_t p) const {
        if (whole(p, 16u)) return ld128(at(p));
        uint32_t w[4];
        for (uint32_t k = 0; k < 4u; k++)
            w[k] = (uint32_t)byte(p + 4u * k) | (uint32_t)byte(p + 4u * k + 1u) << 8 | (uint32_t)byte(p + 4u * k + 2u) << 16 |
                   (uint32_t)byte(p + 4u * k + 3u) << 24;
        return u32x4{w[0], w[1], w[2], w[3]};
    }
    // rd32(V, p), p + 4 <= end
    __device__ __forceinline__ uint32_t rd32(uint32_t p) const {
        if (whole(p, 4u)) return ld32(at(p));
        return (uint32_t)byte(p) | (uint32_t)byte(p + 1u) << 8 | (uint32_t)byte(p + 2u) << 16 | (uint32_t)byte(p + 3u) << 24;
    }
};

// Wave-cooperative forward extension (:704-712) in V: continues from `mlen` equal bytes after the 4 MINMATCH bytes,
// 16 B per lane, first mismatch or the matchLimit found with ballot + ffs.  The compare is split at the dictionary's
// end: a lane whose 16 match-side bytes lie in one half loads them at once, the one lane that straddles the end goes
// byte by byte (as do the lanes at the end of the record).  m_pos >= D: the forward side is always the record.
__device__ __forceinline__ uint32_t dc_extend_match(const VBuf &V, uint32_t m_pos, uint32_t m_cand, uint32_t mlen,
                                                    uint32_t match_limit, uint32_t lane) {
    const uint32_t ip0 = m_pos + kMinMatch, mt0 = m_cand + kMinMatch;
    for (;;) {
        const uint32_t p = ip0 + mlen + lane * 16u;         // first byte this lane compares
        uint32_t n = 0;                                     // how many bytes it may compare
        if (p < match_limit) n = (match_limit - p) < 16u ? (match_limit - p) : 16u;
        uint32_t d = 0;                                     // equal bytes found
        if (n > 0) {
            const uint32_t q = mt0 + mlen + lane * 16u;     // q < p
            if (p + 16u <= V.end && V.whole(q, 16u)) {
                d = first_diff16(ld128(V.srcv + p), ld128(V.at(q)));
                if (d > n) d = n;
            } else {
                while (d < n && V.srcv[p + d] == V.byte(q + d)) d++;
            }
        }
        const uint64_t stop = ballot(d < 16u);              // mismatch or limit inside this lane's chunk
        if (stop) {
            const uint32_t sl = first_lane(stop);
            return mlen + sl * 16u + rdlane(d, sl);
        }
        mlen += 1024u;
    }
}

}  // namespace

// T = uint16_t when every stored position fits 16 bits (max_dict_len + max_in_len <= 65547: every put is a position
// below D + n - 12), else uint32_t.  One wavefront per workgroup, the 4096-entry table in LDS: 8 KiB -> 20 wavefronts per
// CU, 16 KiB -> 10 (160 KiB of LDS per CU).
template <typename T>
__global__ __launch_bounds__(64) void k_compress_fast_dict(
    const uint8_t *d_in, const uint64_t *__restrict__ d_in_off, const uint32_t *__restrict__ d_in_len,
    uint8_t *__restrict__ d_out, const uint64_t *__restrict__ d_out_off, const uint32_t *__restrict__ d_out_cap,
    const uint8_t *d_dict, const uint64_t *__restrict__ d_dict_off, const uint32_t *__restrict__ d_dict_len,
    const uint32_t *__restrict__ d_table, const uint32_t *__restrict__ d_table_idx, int64_t *__restrict__ d_result,
    uint32_t nblocks, uint32_t max_in_len, uint32_t max_dict_len, uint32_t acceleration) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t blk = blockIdx.x;
    if (blk >= nblocks) return;
    // volatile, address space 3: lanes communicate through the table (see k_compress_fast)
    typedef __attribute__((address_space(3))) volatile T lds_entry;
    lds_entry *table = (lds_entry *)lds_raw;

    const uint8_t *src = d_in + d_in_off[blk];
    uint8_t *dst = d_out + d_out_off[blk];
    const uint32_t src_size = rfl(d_in_len[blk]);
    const uint32_t dst_len = rfl(d_out_cap[blk]);
    const uint32_t dict_len = rfl(d_dict_len[blk]);
    const uint32_t D = dict_len < 65536u ? dict_len : 65536u;           // :804

    int64_t res;
    if (src_size > kMaxInput) {                                         // :823
        res = kErrInputTooLarge;
    } else if (src_size > max_in_len || D > max_dict_len) {             // the table width was chosen from the two
        res = kErrInvalidState;
    } else if (src_size == 0) {                                         // :824
        res = 0;
    } else if (src_size < kMfLimit + 1u) {                              // :825-827
        res = dc_last_literals(dst, dst_len, 0, src, src_size, lane);
    } else {
        VBuf V;
        V.tail = D ? d_dict + d_dict_off[blk] + (dict_len - D) : src;   // :805 (D == 0: never read)
        V.srcv = src - D;
        V.D = D;
        V.end = D + src_size;
        const uint32_t L = V.end - kMfLimit;                            // mflimitPlusOne :630
        const uint32_t match_limit = V.end - kLastLiterals;             // :631
        {
            // the dictionary's table; an entry >= L cannot pass `match < ip` (ip <= L) and is loaded as empty, so every
            // loaded entry fits T
            const uint32_t tix = d_table_idx ? rfl(d_table_idx[blk]) : blk;
            const u32x4 *seed4 = reinterpret_cast<const u32x4 *>(d_table + (uint64_t)tix * 4096u);
            for (uint32_t k = lane; k < 1024u; k += 64u) {
                const u32x4 v = seed4[k];
                table[4u * k + 0u] = (T)(v.x < L ? v.x : 0u);
                table[4u * k + 1u] = (T)(v.y < L ? v.y : 0u);
                table[4u * k + 2u] = (T)(v.z < L ? v.z : 0u);
                table[4u * k + 3u] = (T)(v.w < L ? v.w : 0u);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        }
        const uint32_t accel = acceleration < 1u ? 1u : (acceleration > 65537u ? 65537u : acceleration);   // :636
        const uint32_t cbase = accel > 64u ? accel : 64u;
        const uint32_t s_cbase = dc_skip_sum(cbase);
        const uint64_t lane_bit = 1ull << lane;
        const uint64_t lanes_below = lane_bit - 1ull;

        uint32_t anchor = D, op = 0;                                    // :628
        uint32_t F0 = D > 1u ? D : 1u;                                  // :633 (position 0 of V is never probed)
        bool has_ins = false;    // pending put(anchor) of :732-736, folded into the next batch as lane 0
        bool failed = false;
        uint32_t guard = 0;      // every round of this loop consumes at least one input byte
        // forward bytes of the next window, loaded as soon as its anchor is known (before the emission and the table fix-up
        // of the current window)
        u32x4 fwd_pf = {0, 0, 0, 0};
        uint32_t pf_anchor = 0xFFFFFFFFu;
        while (F0 < L) {                                                // :635
            if (++guard > src_size) { failed = true; break; }           // unreachable; never spin on the GPU
            int32_t ub = has_ins ? -1 : 0;   // probe index of lane 0 (-1 = the pending put as a pseudo-probe)

            // =====================================================================================
            // Window path (acceleration 1, away from the end of the block), as in k_compress_fast: lane i <->
            // position anchor + i; every sequence that begins in these 64 positions is resolved from registers (16
            // forward bytes per lane, one table read / speculative put / read-back, one candidate gather), then one
            // short loop iteration per sequence.  Positions are positions in V: the window itself always lies in the
            // record, its candidates anywhere below.  It only starts behind a pending put(anchor) (lane 0, has_ins), so
            // the record's first search runs on the generic path: with a dictionary it PROBES position D, without one
            // (D == 0) position 0 is neither probed nor put.
            // =====================================================================================
            if (accel == 1u && F0 == anchor + 1u && has_ins && (uint64_t)anchor + 192u < L) {
              bool moved = false;           // the last window of the run advanced the anchor ...
              bool to_generic = false;      // ... or handed its search over to the generic path
              for (;;) {                    // consecutive windows: the next one starts without re-deriving the entry test
                const uint32_t A = anchor;
                const uint32_t pos = A + lane;
                const u32x4 fwd = pf_anchor == A ? fwd_pf : ld128(V.srcv + pos);     // (pos >= D: the record)
                const uint32_t prod = fwd.x * kHashMul;
                const uint32_t h = prod >> 20;                          // :653
                const uint32_t mine = (uint32_t)(T)pos;                 // my table entry
                const uint32_t old = table[h];                          // :654
                // pre-window candidates: the old table value passes `match > 0`, `match < ip` and the distance test
                // (:656-658); its bytes (dictionary or record) are gathered once for the whole window, right away, so
                // that the latency overlaps the speculative put / read-back below
                // (written mask by mask: see the note at `losers` below)
                const uint64_t okm = ballot(old > 0) & ballot(old < pos) & ballot(old + kMaxDist >= pos);
                const bool old_ok = in_mask(okm);
                u32x4 cold = {0, 0, 0, 0};
                if (old_ok) cold = V.ld128v(old);
                u32x4 f2 = {0, 0, 0, 0}, c2 = f2, f3 = f2, c3 = f2;
                table[h] = (T)mine;                                     // :661 (speculative)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                const uint32_t rb = table[h];
                // (a ballot is lowered to its compare only when its argument is one compare; a compound predicate goes
                //  through v_cndmask and v_cmp_ne again.  So compound predicates are scalar combinations of one-compare
                //  ballots, and a lane's own bit of such a mask is in_mask().)
                uint64_t losers = ballot(rb != mine);
                uint64_t grp = lane_bit;
                while (losers) {                                        // one round per duplicate-hash group
                    const uint32_t l = first_lane(losers);
                    const uint32_t hh = rdlane(h, l);
                    const uint64_t same = ballot(h == hh);
                    if (in_mask(same)) grp = same;
                    losers &= ~same;
                }

                // What a probe at lane i finds if its table slot still holds the pre-window value: validity
                // (:656-659), the first 12 bytes of forward extension (:704-712) and the offset.  For a lane
                // whose hash is unique in the window this does not depend on the parse at all.
                const uint64_t vom = okm & ballot(cold.x == fwd.x);
                const bool vo = in_mask(vom);
                uint32_t mlo;
                {
                    // selects only (a nested ?: chain compiles to exec-mask branches, i.e. scalar instructions)
                    const uint32_t x1 = fwd.y ^ cold.y, x2 = fwd.z ^ cold.z, x3 = fwd.w ^ cold.w;
                    const uint32_t xs = x1 ? x1 : (x2 ? x2 : x3);
                    const uint32_t xbase = x1 ? 0u : (x2 ? 4u : 8u);
                    mlo = xs ? xbase + ((uint32_t)__builtin_ctz(xs) >> 3) : 12u;
                }
                // second level: the few lanes whose 16 bytes all match compare 16 more (matches of 16..31 bytes are a
                // fifth of all sequences on text; without this each of them costs an exact step and its own emission)
                const bool need2 = in_mask(vom & ballot(mlo == 12u));
                if (need2) {                                  // (all loads in one round trip)
                    f2 = ld128(V.srcv + pos + 16u); f3 = ld128(V.srcv + pos + 32u);
                    c2 = V.ld128v(old + 16u); c3 = V.ld128v(old + 32u);
                }
                if (need2) {
                    const uint32_t d2 = first_diff16_sel(f2, c2);
                    mlo += d2 == 16u ? 16u + first_diff16_sel(f3, c3) : d2;
                }
                // a lane whose hash no EARLIER lane of the window shares reads the pre-window value whatever the parse does --
                // the only lane of its hash, or the first of a duplicate group (the first of a group would otherwise take
                // an exact step like the others, find no in-window candidate and fall back to the same registers)
                const uint64_t singm = ballot(lane_rank(grp) == 0u);   // (grp & lanes_below) == 0
                const uint64_t lt44 = ballot(mlo < 44u);
                const uint64_t cfast = vom & lt44;            // oldfast: the result against the pre-window value is complete in
                                                              // registers; usable if no in-window put precedes
                const uint64_t nsing = ~singm;
                const uint64_t slow = (nsing & ~cfast) | (vom & ~lt44);   // (!single && !oldfast) || (vo && mlo >= 44): exact step if reached
                // a search from lane i ends with the in-register match at the first fastm lane >= i iff that lane lies below the
                // first stopm lane >= i: cfast lies in fastm | stopm and slow in stopm, so nothing that can match comes first
                const uint64_t fastm = cfast & singm;
                const uint64_t stopm = slow | (cfast & nsing);
                // per lane i: J = first fastm lane >= i, S = first stopm lane >= i (64 = none)
                uint32_t J, S;
                {
                    const uint64_t mj = fastm >> lane, ms = stopm >> lane;
                    J = mj ? lane + (uint32_t)__builtin_ctzll(mj) : 64u;
                    S = ms ? lane + (uint32_t)__builtin_ctzll(ms) : 64u;
                }
                const uint32_t v_end = lane + kMinMatch + mlo;                          // anchor lane after a match at this lane
                uint32_t mlo_e = mlo, off_e = pos - old;                          // match length / offset the flush emits for a match lane
                // fast-run step of a search that starts at lane f, precomputed for every f: PK = j | ((v_end[j] + 1) << 6), the
                // match lane and the next probe lane, with bit 31 set if the step ends the window (v_end[j] >= 63), when
                // the search ends with the in-register match at j = J[f] (J[f] < S[f]), else ~0.
                // for the exact step: X = first lane >= f that can match at all (min(J, S), 64 = none); Q = the lane's own
                // nsing bit << 1 | what a probe finds against the pre-window value: valid | matched extension bytes << 2
                const uint32_t X = J < S ? J : S;
                const uint32_t Q = (mlo << 2) | (in_mask(nsing) ? 2u : 0u) | (vo ? 1u : 0u);
                uint32_t PK;
                {
                    const uint32_t ve_j = shfl(v_end, J & 63u);
                    const bool fastok = J < S;
                    PK = fastok ? (J | ((ve_j + 1u) << 6) | (ve_j >= 63u ? 0x80000000u : 0u)) : 0xFFFFFFFFu;
                }

                uint32_t f = 1;          // next lane to probe
                uint32_t a = 0;          // lane of the current anchor
                // lanes strictly inside a match that has been emitted (never put(), :732-736): every flush and every immediate
                // emission ORs in the lanes of its own matches.  Runs and immediate sequences are consecutive lane ranges and
                // a match's end lane is final once it is emitted, so no later event changes what an earlier one covered.
                uint64_t cov_acc = 0;
                bool continue_generic = false;
                // with less than 512 bytes of room left every sequence takes the exact step, which checks the capacity
                const bool tight = dst_len - op < 512u;
                uint32_t a0 = a;             // anchor lane at the start of the pending (unflushed) run; op stays where it was then
                uint64_t mm_run = 0;         // match lanes of the pending run
                // end lanes of the pending run's matches (those below 64), entered where mm_run gets its bit.  The matches of
                // a run are disjoint, ordered lane ranges, so the lanes strictly inside them are E_run - (mm_run << 1)
                // (mod 2^64): every match contributes 2^e - 2^(j+1) = lanes j+1 .. e-1, and a last match that ends at or past
                // lane 64 has no bit in E_run, so that the wrap carries its range up to lane 63.
                uint64_t E_run = 0;
                // lanes strictly inside a match so far, for an exact step: the emitted ones and those of the pending run
                auto covered_now = [&]() -> uint64_t { return cov_acc | (E_run - (mm_run << 1)); };
                // flush of the pending run: every offset from popcounts, three stores for all its sequences
                auto flush_run = [&]() {
                    const uint64_t covm = E_run - (mm_run << 1);        // strictly inside a match of this run
                    // first lane of my literal run: the nearest end lane of the run at or below me, else the run's anchor
                    // (a match that starts where the previous one ends finds that end at its own lane: no literals)
                    const uint64_t ends = (E_run | (1ull << a0) | 1ull) & (lanes_below | lane_bit);
                    const uint32_t pend = 63u - (uint32_t)__builtin_clzll(ends);
                    const bool is_m = in_mask(mm_run);
                    const uint32_t jlast = 63u - (uint32_t)__builtin_clzll(mm_run);
                    // literals: lanes from a0 up to the last match lane that are neither covered nor a match lane
                    const uint64_t litmask = ((1ull << jlast) - 1ull) & ~((1ull << a0) - 1ull) & ~(covm | mm_run);
                    const bool is_lit = in_mask(litmask);
                    const uint64_t extm = mm_run & ballot(mlo_e >= 15u);                // matches with one length-extension byte (:714-728)
                    // literal runs of 15..63 bytes carry one extension byte too (:673-687): a lane's sequence is the
                    // first match lane at or above it, its literal count that lane minus the start of the run
                    const uint64_t at_or_above = mm_run & ~lanes_below;
                    const uint32_t my_m = at_or_above ? (uint32_t)__builtin_ctzll(at_or_above) : lane;
                    const uint64_t ownm = ballot(my_m - pend >= 15u);
                    const uint32_t own_l = in_mask(ownm) ? 1u : 0u;
                    const uint64_t lextm = mm_run & ownm;
                    // (prefix popcounts as lane_rank: v_mbcnt_lo / _hi)
                    const uint32_t k = lane_rank(mm_run);                               // sequences completed before me
                    const uint32_t lb = lane_rank(litmask);                             // literal bytes before me
                    const uint32_t o1 = op + 3u * k + lb + 1u + lane_rank(extm) + lane_rank(lextm) + own_l;
                    if (is_lit) dst[o1] = (uint8_t)fwd.x;               // literals (:691)
                    if (is_m) {
                        const uint32_t lit_k = lane - pend;             // :668
                        uint8_t *tk = dst + (o1 - 1u - lit_k - own_l);
                        tk[0] = (uint8_t)(((lit_k < 15u ? lit_k : 15u) << 4) | (mlo_e < 15u ? mlo_e : 15u));   // token
                        if (own_l) tk[1] = (uint8_t)(lit_k - 15u);
                        const uint16_t off16 = (uint16_t)off_e;                          // :695
                        __builtin_memcpy(dst + o1, &off16, 2);
                        if (mlo_e >= 15u) dst[o1 + 2u] = (uint8_t)(mlo_e - 15u);         // < 255 (mlen < 270 in a run)
                    }
                    const uint32_t nm = (uint32_t)__popcll(mm_run);
                    op += 3u * nm + (uint32_t)__popcll(litmask) + (uint32_t)__popcll(extm) + (uint32_t)__popcll(lextm);
                    cov_acc |= covm;
                    mm_run = 0;
                    E_run = 0;
                };
                for (;;) {
                    // ---- fast run: a minimal scalar loop that only collects the match lanes.  A search that
                    //      starts at f ends at J[f] when no slow lane comes first, the lane's hash is unique in the
                    //      window (its probe reads the pre-window value whatever was put before) and the literal
                    //      run fits the token nibble. ----
                    if (mm_run == 0) a0 = a;
                    if (!tight && f < 64u) {
                        // hand-scheduled scalar loop (the compiler spends ~25 scalar instructions per trip on the
                        // boolean plumbing; the scalar unit is what bounds this kernel):
                        //   for (;;) { pk = PK[f]; if (pk < 0) break; f = pk >> 6; j = pk & 63;
                        //              mm_run |= 1 << j; a = f - 1; E_run |= 1 << a; }                (two trips per branch back)
                        // One exit test: bit 31 of pk is set in the sentinel and in the step that ends the window, so a trip
                        // that goes on has a < 63 and f < 64.
                        uint32_t t_pk, t_j;
#define ZLZ4_FAST_RUN_TRIP                                   \
                            "v_readlane_b32 %[pk], %[PK], %[f]\n\t" \
                            "s_cmp_lt_i32 %[pk], 0\n\t"      \
                            "s_cbranch_scc1 3f\n\t"          \
                            "s_lshr_b32 %[f], %[pk], 6\n\t"  \
                            "s_and_b32 %[j], %[pk], 63\n\t"  \
                            "s_bitset1_b64 %[mm], %[j]\n\t"  \
                            "s_sub_u32 %[a], %[f], 1\n\t"    \
                            "s_bitset1_b64 %[er], %[a]\n\t"
                        // (four scalar instructions lie between the write of f and the v_readlane that uses it as its lane
                        //  select: the ISA asks for four wait states there)
                        asm volatile(
                            "s_nop 3\n"
                            "1:\n\t"
                            ZLZ4_FAST_RUN_TRIP
                            ZLZ4_FAST_RUN_TRIP
                            "s_branch 1b\n"
                            "3:\n"
                            : [f] "+s"(f), [a] "+s"(a), [mm] "+s"(mm_run), [er] "+s"(E_run), [pk] "=&s"(t_pk), [j] "=&s"(t_j)
                            : [PK] "v"(PK)
                            : "scc");
#undef ZLZ4_FAST_RUN_TRIP
                        if (t_pk != 0xFFFFFFFFu) {
                            // the step that ends the window, consumed once: its end lane is 63 or beyond
                            mm_run |= 1ull << (t_pk & 63u);
                            f = (t_pk >> 6) & 127u;
                            a = f - 1u;
                            if (a == 63u) E_run |= 1ull << 63;
                        }
                    }
                    if (f >= 64u) {      // window done (a = last anchor lane, possibly >= 64)
                        if (a == 0u) continue_generic = true;    // every lane probed, no match
                        break;
                    }

                    // ---- exact step for the probe at the first lane >= f that can match at all ----
                    const uint32_t x = rdlane(X, f);
                    if (x >= 64u) {
                        if (a == 0u) continue_generic = true;   // the search goes on past the window -> generic batches
                        // else: restart a fresh window at the current anchor (its lanes > a are re-probed there)
                        break;
                    }
                    // earlier put()s of this window with the same hash (only lanes of duplicate-hash groups can have one):
                    // every lane below x that is not strictly inside a match has been put
                    const uint32_t q = rdlane(Q, x);
                    uint64_t pm = 0;
                    if (q & 2u) {
                        const uint64_t grp_x = (uint64_t)rdlane((uint32_t)grp, x) | ((uint64_t)rdlane((uint32_t)(grp >> 32), x) << 32);
                        pm = grp_x & ~covered_now() & ((1ull << x) - 1ull);
                    }
                    const uint32_t j = x;
                    const uint32_t m_pos = A + j;
                    uint32_t m_cand, mlen;
                    if (pm) {
                        // the probe reads the nearest earlier put of the window
                        const uint32_t pr = 63u - (uint32_t)__builtin_clzll(pm);
                        if (rdlane(fwd.x, pr) != rdlane(fwd.x, x)) { f = x + 1u; continue; }   // :659
                        m_cand = A + pr;
                        const uint64_t xa = ((uint64_t)(rdlane(fwd.z, j) ^ rdlane(fwd.z, pr)) << 32) | (rdlane(fwd.y, j) ^ rdlane(fwd.y, pr));
                        const uint32_t xb = rdlane(fwd.w, j) ^ rdlane(fwd.w, pr);
                        if (xa) mlen = (uint32_t)__builtin_ctzll(xa) >> 3;
                        else if (xb) mlen = 8u + ((uint32_t)__builtin_ctz(xb) >> 3);
                        else mlen = dc_extend_match(V, m_pos, m_cand, 12u, match_limit, lane);
                    } else {
                        // the probe reads the pre-window value: the vector code has already compared up to 48 bytes
                        if (!(q & 1u)) { f = x + 1u; continue; }      // probed, put, no match: next probe
                        mlen = q >> 2;
                        if (mlen < 44u && !tight) {
                            // mlo_e / off_e of lane j already describe this sequence: it just joins the run
                            mm_run |= 1ull << j;
                            a = j + kMinMatch + mlen;
                            if (a < 64u) E_run |= 1ull << a;
                            if (a >= 64u) break;                            // the next window inserts it as its lane 0
                            f = a + 1u;
                            continue;
                        }
                        m_cand = rdlane(old, x);
                        if (mlen >= 44u) mlen = dc_extend_match(V, m_pos, m_cand, 44u, match_limit, lane);
                    }
                    const uint32_t lit = j - a;
                    const uint32_t offset = m_pos - m_cand;
                    const uint32_t e = j + kMinMatch + mlen;                // lane of the new anchor (may be >= 64)
                    if (!tight && mlen < 270u) {
                        // simple sequence: joins the pending run, emitted by the flush
                        mlo_e = wrlane(mlen, j, mlo_e);
                        off_e = wrlane(offset, j, off_e);
                        mm_run |= 1ull << j;
                        if (e < 64u) E_run |= 1ull << e;
                        a = e;
                        if (e >= 64u) break;                                // the next window inserts it as its lane 0
                        f = e + 1u;
                        continue;
                    }
                    if (mm_run) flush_run();
                    // immediate emission (:668-728), literals = low bytes of lanes a..j-1
                    const uint32_t nle = ext_len_bytes(lit), nme = ext_len_bytes(mlen);
                    const uint64_t seq_end = (uint64_t)op + 1u + nle + lit + 2u + nme;
                    if (seq_end > dst_len) { failed = true; break; }
                    if (lane == 0)
                        dst[op] = (uint8_t)(((lit >= 15u ? 15u : lit) << 4) | (mlen >= 15u ? 15u : mlen));
                    if (lit >= 15u) write_ext_len(dst + op + 1u, lit, lane);
                    uint8_t *o = dst + op + 1u + nle;
                    if (lane >= a && lane < j) o[lane - a] = (uint8_t)fwd.x;
                    o += lit;
                    if (lane < 2u) o[lane] = (uint8_t)(offset >> (8u * lane));
                    if (mlen >= 15u) write_ext_len(o + 2u, mlen, lane);
                    op = (uint32_t)seq_end;
                    {
                        const uint64_t upto_e = e >= 64u ? ~0ull : (1ull << e) - 1ull;
                        cov_acc |= upto_e & ~((2ull << j) - 1ull);          // lanes j+1 .. e-1
                    }
                    a = e;
                    if (e >= 64u) break;                                    // the next window inserts it as its lane 0
                    f = e + 1u;
                }
                // (next_win implies everything the entry test above asks of the next round)
                const bool next_win = !continue_generic && !failed && a != 0u && (uint64_t)A + a + 192u < L;
                if (next_win) {
                    pf_anchor = A + a;
                    fwd_pf = ld128(V.srcv + pf_anchor + lane);
                }
                if (mm_run && !failed) flush_run();
                anchor = A + a;
                // lanes the serial loop put(): below the frontier and not strictly inside a match (no run is pending here)
                const uint32_t f_end = continue_generic ? 64u : (a >= 64u ? 64u : a + 1u);
                const uint64_t ins = ~cov_acc & (f_end >= 64u ? ~0ull : (1ull << f_end) - 1ull);
                if (failed) break;
                // ---- leave the table as the serial loop would have ----
                // One write per lane: the slot's final value depends only on gi, the group's lanes in `ins`.  None: every
                // written lane of the group puts the old value back (they all read it before any put, so equal addresses
                // carry equal values).  Else the last `ins` lane of the group stores its entry and the others write nothing.
                const uint64_t gi = grp & ins;
                const bool put_mine = in_mask(ins) && (gi & ~lanes_below & ~lane_bit) == 0;
                if (put_mine || gi == 0) table[h] = (T)(put_mine ? mine : old);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                moved = anchor != A;
                to_generic = continue_generic;
                if (next_win) {
                    has_ins = true;
                    F0 = anchor + 1u;
                    // (no guard here: next_win implies a != 0, so this window moved the anchor forward, and
                    //  A + a + 192 < L bounds the windows of one run; the outer loop's guard covers everything else)
                    continue;
                }
                break;
              }
                if (failed) break;
                if (!to_generic && moved) {
                    if (anchor < L) { has_ins = true; F0 = anchor + 1u; }
                    else { has_ins = false; F0 = L; }
                    continue;
                }
                // continue_generic: same search, next probe index 63 (lane 0 of the next batch is position F0 + 63).
                // (anchor == A without continue_generic cannot happen; if it ever did, the generic path below restarts
                //  the search from F0 -- the table then holds exactly the anchor's put -- and always makes progress.)
                if (to_generic) ub = 63;
            }

            // =====================================================================================
            // Generic path: any acceleration, the record's first search, block tail, searches longer than one window.
            // 64 probes of ONE search per step.
            // =====================================================================================
            bool found = false;
            uint32_t m_pos = 0, m_cand = 0, m_local = 0;
            bool m_local_done = false;
            for (;;) {
                const int32_t u = ub + (int32_t)lane;
                uint32_t pos, step_next;
                if (u <= 0) {
                    pos = (u < 0) ? F0 - 1u : F0;
                    step_next = accel;                  // u == 0: bail iff F0 + a > L  (:645-651, first iteration)
                } else if (u == 1) {
                    pos = F0 + accel;
                    step_next = accel >> 6;
                } else {
                    const uint32_t x = cbase + (uint32_t)u - 1u;
                    pos = F0 + accel + dc_skip_sum(x) - s_cbase;
                    step_next = x >> 6;
                }
                const bool is_probe = u >= 0;
                const bool bail = is_probe && ((uint64_t)pos + step_next > L);
                const uint64_t bail_mask = ballot(bail);
                // bail is monotone in u: everything from the first bailing lane on is out of the search
                const uint32_t nb = bail_mask ? first_lane(bail_mask) : 64u;
                const bool active = lane < nb;          // (the pseudo-probe exists only when has_ins: ub == -1)

                // forward data (pos >= D: the record): 16 B when they are inside the block, else the 4 hashed bytes only
                const bool have16 = active && (pos + 16u <= V.end);
                u32x4 fwd = {0, 0, 0, 0};
                if (have16) fwd = ld128(V.srcv + pos);
                else if (active) fwd.x = ld32(V.srcv + pos);
                const uint32_t h = dc_hash4(fwd.x);                     // :653
                const uint32_t mine = (uint32_t)(T)pos;

                // table read / speculative put / read-back
                uint32_t old = 0, rb = 0;
                if (active) {
                    old = table[h];                                     // :654
                    table[h] = (T)mine;                                 // :661 (speculative)
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                if (active) rb = table[h];
                // duplicate-hash groups inside the batch
                uint64_t losers = ballot(active && rb != mine);
                uint64_t grp = lane_bit;
                int32_t pred = -1;
                while (losers) {
                    const uint32_t l = first_lane(losers);
                    const uint32_t hh = rdlane(h, l);
                    const uint64_t same = ballot(active && h == hh);
                    if (active && h == hh) {
                        grp = same;
                        const uint64_t below = same & lanes_below;
                        pred = below ? 63 - (int32_t)__clzll((long long)below) : -1;
                    }
                    losers &= ~same;
                }
                const uint32_t pred_pos = shfl(pos, (uint32_t)(pred < 0 ? 0 : pred));
                const uint32_t cand = pred >= 0 ? pred_pos : old;

                // the four validity tests of :656-659
                bool valid = is_probe && active && cand > 0 && cand < pos && (cand + kMaxDist >= pos);
                u32x4 cnd = {0, 0, 0, 0};
                bool cnd16 = false;
                if (valid) {
                    cnd16 = have16 && V.whole(cand, 16u);
                    if (cnd16) cnd = ld128(V.at(cand)); else cnd.x = V.rd32(cand);
                    valid = cnd.x == fwd.x;
                }
                const uint64_t valid_mask = ballot(valid);

                if (valid_mask) {
                    // ---- match at lane wl (first valid probe, :663) ----
                    const uint32_t wl = first_lane(valid_mask);
                    // lanes after the winner never ran in the serial loop: undo their puts, then
                    // re-commit the last lane <= wl of every duplicate group
                    if (active && lane > wl) table[h] = (T)old;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    const uint64_t upto = (2ull << wl) - 1ull;   // lanes 0..wl
                    if (active && lane <= wl && ((grp & upto & ~lanes_below & ~lane_bit) == 0)) table[h] = (T)mine;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    // local extension: bytes 4..15 of the two 16-byte reads (:704-712)
                    uint32_t loc = 0;
                    bool loc_done = false;
                    if (lane == wl && cnd16) {
                        const uint32_t lim = match_limit - (pos + kMinMatch);   // bytes that may still be compared
                        u32x4 a = fwd, b = cnd;
                        a.x = 0; b.x = 0;
                        loc = first_diff16(a, b) - 4u;           // 0..12
                        if (loc >= lim) { loc = lim; loc_done = true; }
                        else if (loc < 12u) loc_done = true;
                    }
                    m_pos = rdlane(pos, wl);
                    m_cand = rdlane(cand, wl);
                    m_local = rdlane(loc, wl);
                    m_local_done = rdlane((uint32_t)loc_done, wl) != 0;
                    found = true;
                    break;
                }
                if (bail_mask) break;                                   // :649-651 -> finishCompression
                // no match in 64 probes: all puts stand; fix duplicate groups so the last lane's position is stored
                if (active && ((grp & ~lanes_below & ~lane_bit) == 0) && grp != lane_bit) table[h] = (T)mine;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                ub += 64;
            }
            if (!found) break;

            // ---------------- forward extension (:704-712) ----------------
            const uint32_t mlen = m_local_done ? m_local : dc_extend_match(V, m_pos, m_cand, m_local, match_limit, lane);

            // ---------------- emit the sequence (:668-728) ----------------
            const uint32_t lit = m_pos - anchor;                        // :668
            const uint32_t nle = ext_len_bytes(lit), nme = ext_len_bytes(mlen);
            const uint64_t seq_end = (uint64_t)op + 1u + nle + lit + 2u + nme;
            if (seq_end > dst_len) { failed = true; break; }            // :671-:724 (any of them)
            if (lane == 0)
                dst[op] = (uint8_t)(((lit >= 15u ? 15u : lit) << 4) | (mlen >= 15u ? 15u : mlen));
            if (lit >= 15u) write_ext_len(dst + op + 1u, lit, lane);
            uint8_t *o = dst + op + 1u + nle;
            copy_bytes(o, V.srcv + anchor, lit, lane);                  // :691 (anchor >= D: always the record)
            o += lit;
            const uint32_t offset = m_pos - m_cand;                     // :695
            if (lane < 2u) o[lane] = (uint8_t)(offset >> (8u * lane));  // :697
            if (mlen >= 15u) write_ext_len(o + 2u, mlen, lane);
            op = (uint32_t)seq_end;

            // ---------------- after the match (:730-736) ----------------
            const uint32_t end = m_pos + kMinMatch + mlen;
            anchor = end;
            if (end < L) { has_ins = true; F0 = end + 1u; }
            else { has_ins = false; F0 = L; }
        }
        res = failed ? kErrOutputTooSmall
                     : dc_last_literals(dst, dst_len, op, V.srcv + anchor, V.end - anchor, lane);   // :650, :739
    }
    if (lane == 0) d_result[blk] = res;
}

}  // namespace zlz4

extern "C" int zlz4_launch_compress_fast_using_dict(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                                    const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                                    const uint32_t *d_out_cap, const uint8_t *d_dict,
                                                    const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                                                    const uint32_t *d_table, const uint32_t *d_table_idx, int64_t *d_result,
                                                    uint32_t nblocks, uint32_t max_in_len, uint32_t max_dict_len,
                                                    uint32_t acceleration) {
    if (nblocks == 0) return 0;
    const uint32_t dmax = max_dict_len < 65536u ? max_dict_len : 65536u;
#define ZLZ4_LAUNCH_DICT(T)                                                                                              \
    hipLaunchKernelGGL((zlz4::k_compress_fast_dict<T>), dim3(nblocks), dim3(64), 4096 * sizeof(T), stream, d_in, d_in_off, \
                       d_in_len, d_out, d_out_off, d_out_cap, d_dict, d_dict_off, d_dict_len, d_table, d_table_idx,        \
                       d_result, nblocks, max_in_len, dmax, acceleration)
    // every stored position is below D + n - 12: 16-bit entries are exact while D + n <= 65547
    if ((uint64_t)dmax + max_in_len <= 65536u + 11u) ZLZ4_LAUNCH_DICT(uint16_t);
    else ZLZ4_LAUNCH_DICT(uint32_t);
#undef ZLZ4_LAUNCH_DICT
    return zlz4_launch_status();
}
