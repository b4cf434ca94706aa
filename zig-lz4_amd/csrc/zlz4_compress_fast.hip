// zlz4_compress_fast.hip -- LZ4 "fast" block compressor for gfx950, one wavefront per block.
//
// Replaces lz4.compressFast / lz4.compressDefault (reference src/lz4.zig:283-447,
// helpers :449-519).  Output is byte-identical to the Zig algorithm, including
// the quirks listed in SURVEY.md Appendix A.1:
//   Q1 position 0 is never inserted / never matchable (0 == empty)   :317, :345
//   Q2 the skip schedule  step = searchMatchNb >> 6  with searchMatchNb starting at
//      `acceleration`, and the bail-out test on the post-increment forwardIp      :322-338
//   Q3 probe = read table, 4 validity tests, unconditional put                     :342-350
//   Q4 no backward extension, Q5 forward extension up to srcSize-5               :401-413
//   Q6 after a match only the byte right after it is inserted                    :435-442
//
// How the serial probe loop becomes 64-wide without changing a byte
// -----------------------------------------------------------------
// A search that starts at F0 visits a position sequence that depends only on F0 and
// the acceleration a (not on data): with c = max(64, a) and S(x) = sum_{y<x} (y >> 6)
//     U(0) = F0                        bail iff F0 + a > L
//     U(1) = F0 + a                    bail iff U(1) + (a >> 6) > L
//     U(u) = F0 + a + S(c+u-1) - S(c)  bail iff U(u) + ((c+u-1) >> 6) > L      (u >= 2)
// (L = srcSize - 12).  The iterations in which the reference's step is 0 re-probe the
// same position, see match == ip, fail `match < ip` and re-put the same value: they
// change nothing and are skipped.  Lane i of a batch takes probe u = ub + i.  What a
// probe reads from the hash table is either the value from before the batch or the
// position of the nearest earlier lane of the batch with the same hash; those lanes
// are found with one LDS write/read-back (losers of the write race are members of a
// duplicate-hash group) plus one ballot per duplicate group.  The first valid lane
// wins (ballot + ffs); lanes after it put their old table value back, so the table
// ends up exactly as the serial loop would have left it.
#include <cstdlib>

#include "zlz4_device.hpp"
#include "zlz4_launch.hpp"

// Diagnostic build only (-DZLZ4_STAMPS): per-phase shader-cycle sums, see profiles/ notes.
#ifdef ZLZ4_STAMPS
__device__ unsigned long long g_zlz4_stamps[24];
#define STAMP_DECL unsigned long long st_acc[24] = {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0}; unsigned long long st_last = __builtin_amdgcn_s_memtime();
#define STAMP(i) do { unsigned long long st_now; __builtin_amdgcn_sched_barrier(0); \
                      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_now) :: "memory"); \
                      __builtin_amdgcn_sched_barrier(0); st_acc[i] += st_now - st_last; st_last = st_now; } while (0)
#define STAMP_COUNT(i) do { st_acc[i] += 1; } while (0)
#define STAMP_FLUSH do { if (lane == 0) for (int st_k = 0; st_k < 24; st_k++) atomicAdd(&g_zlz4_stamps[st_k], st_acc[st_k]); } while (0)
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_COUNT(i)
#define STAMP_FLUSH
#endif

namespace zlz4 {

__device__ __forceinline__ uint32_t hash4(uint32_t seq) { return (seq * kHashMul) >> 20; }   // src/lz4.zig:75-77

// S(x) = sum_{y < x} (y >> 6)
__device__ __forceinline__ uint32_t skip_sum(uint32_t x) {
    const uint32_t q = x >> 6, r = x & 63u;
    return 32u * q * (q - 1u) + q * r;      // q == 0 -> 0 (32*0*(-1) wraps to 0)
}

// literal-only sequence: compressAsLiterals (:449-482) and finishCompression (:484-519)
__device__ __forceinline__ int64_t emit_last_literals(uint8_t *dst, uint32_t dst_len, uint32_t op,
                                                       const uint8_t *lit_src, uint32_t lit, uint32_t lane) {
    if (lit == 0) return (int64_t)op;                                   // :488
    const uint32_t nle = ext_len_bytes(lit);
    if ((uint64_t)op + 1u + nle + lit > dst_len) return kErrOutputTooSmall;   // :491-514 / :454-477
    if (lane == 0) dst[op] = (uint8_t)((lit >= 15u ? 15u : lit) << 4);
    if (lit >= 15u) write_ext_len(dst + op + 1u, lit, lane);
    copy_bytes(dst + op + 1u + nle, lit_src, lit, lane);
    return (int64_t)(op + 1u + nle + lit);
}

// Wave-cooperative forward extension (:401-413): continues from `mlen` equal bytes after the 4 MINMATCH
// bytes, 16 B per lane (1 KiB per step), first mismatch or the srcSize-5 limit found with ballot + ffs.
__device__ __forceinline__ uint32_t extend_match(const uint8_t *__restrict__ src, uint32_t m_pos, uint32_t m_cand,
                                                 uint32_t mlen, uint32_t match_limit, uint32_t src_size,
                                                 uint32_t lane) {
    const uint32_t ip0 = m_pos + kMinMatch, mt0 = m_cand + kMinMatch;
    for (;;) {
        const uint32_t p = ip0 + mlen + lane * 16u;         // first byte this lane compares
        uint32_t n = 0;                                     // how many bytes it may compare
        if (p < match_limit) n = (match_limit - p) < 16u ? (match_limit - p) : 16u;
        uint32_t d = 0;                                     // equal bytes found
        if (n > 0) {
            const uint32_t q = mt0 + mlen + lane * 16u;
            if (p + 16u <= src_size) {
                d = first_diff16(ld128(src + p), ld128(src + q));
                if (d > n) d = n;
            } else {
                while (d < n && src[p + d] == src[q + d]) d++;
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

// T = uint16_t when every stored position fits 16 bits, else uint32_t.
// kTag: every table entry carries 8 more bits of the hashed sequence's product (bits 12..19; the index is bits 20..31),
// so a probe whose candidate cannot pass the 4-byte test of :348 is settled from LDS and never gathers the candidate's
// bytes from memory (on text more than half of all candidates are false: 4096 slots, 64 Ki positions).  A tag mismatch
// implies a 4-byte mismatch, so no decision changes.  1 = a separate u8 array beside the u16 table (12 KiB per
// wavefront), 2 = packed into bits 24..31 of a u32 entry (positions < 2^24), 0 = none.
//
// kSeed: Stream.compressFastContinue (src/lz4.zig:822-836).  compressFastWithHashTable (:624-748) is compressFast's
// loop with the table starting from the stream's state instead of zeros, so the only differences are here:
//   * block i starts from table d_table_in + idx[i] * 4096 (idx = d_table_idx, NULL = identity).  Every entry is read
//     as a position in the CURRENT block (:656-659), so an entry v >= L = srcSize - 12 cannot pass `match < ip`
//     (ip <= L) and is loaded as 0 (empty): no decision changes, and every loaded entry fits the u16 table and the
//     24-bit positions of the kTag == 2 table.  (No block ever refers to the dictionary: a loaded dictionary only
//     changes which in-block matches the greedy parse finds.)
//   * table values are no longer always earlier positions: the window path tests `old < pos` as well (the generic
//     path always did).
//   * the final table goes to d_table_out + i * 4096 (NULL = not written): out[h] = final[h] if it differs from what
//     was loaded, else the input value (re-read from memory).  A slot that differs was put by this block (a position
//     below srcSize); an equal one is untouched or a re-put of the same position; position 0 is never put (Q1).  So
//     entries this block could not use pass through unchanged.  Every exit that does not compress (InputTooLarge,
//     InvalidState, 0..12 bytes, OutputTooSmall) passes the whole input table through, as the reference returns
//     before its store (:823-827, :831).
// The launcher never picks kTag == 1 (its tag array is left uninitialised) for seeded calls; kTag == 2 entries get the
// tag of the current block's bytes at the loaded position.  d_table_in / d_table_out may be the same table (identity
// indexing): each lane reads an entry before it writes it.
template <typename T, int kTag, bool kSeed = false>
__global__ __launch_bounds__(256) void k_compress_fast(
    const uint8_t *__restrict__ d_in, const uint64_t *__restrict__ d_in_off,
    const uint32_t *__restrict__ d_in_len, uint8_t *__restrict__ d_out,
    const uint64_t *__restrict__ d_out_off, const uint32_t *__restrict__ d_out_cap,
    int64_t *__restrict__ d_result, uint32_t nblocks, uint32_t acceleration, uint32_t max_in_len,
    const uint32_t *d_table_in, const uint32_t *__restrict__ d_table_idx, uint32_t *d_table_out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_in_wg = threadIdx.x >> 6;
    const uint32_t blk = rfl(blockIdx.x * (blockDim.x >> 6) + wave_in_wg);
    if (blk >= nblocks) return;
    // HashTable, src/lz4.zig:263-277.  volatile: lanes communicate through it (write / read-back race
    // detection), so the compiler must neither forward stores to loads nor drop the re-reads.
    // (typed as address space 3: a generic `volatile T *` would compile to FLAT loads/stores with a full
    //  `s_waitcnt vmcnt(0)` each, i.e. every table access would also wait for the global gathers in flight)
    typedef __attribute__((address_space(3))) volatile T lds_entry;
    typedef __attribute__((address_space(3))) volatile uint8_t lds_tag;
    lds_entry *table = (lds_entry *)lds_raw + wave_in_wg * 4096u;
    // kTag == 1: the tag arrays follow the tables of all wavefronts of the workgroup (never initialised: an empty slot
    // is recognised by its position 0 before its tag is looked at)
    lds_tag *tags = (lds_tag *)lds_raw + (blockDim.x >> 6) * 4096u * (uint32_t)sizeof(T) + wave_in_wg * 4096u;
    constexpr uint32_t kPosMask = kTag == 2 ? 0x00FFFFFFu : 0xFFFFFFFFu;

    const uint8_t *src = d_in + d_in_off[blk];
    uint8_t *dst = d_out + d_out_off[blk];
    const uint32_t src_size = rfl(d_in_len[blk]);
    const uint32_t dst_len = rfl(d_out_cap[blk]);

    int64_t res;
    if (src_size > kMaxInput) {                                         // :296
        res = kErrInputTooLarge;
    } else if (src_size > max_in_len) {                                 // the table width was chosen from max_in_len
        res = kErrInvalidState;
    } else if (src_size == 0) {                                         // :299
        res = 0;
    } else if (src_size < kMfLimit + 1u) {                              // :302-304
        res = emit_last_literals(dst, dst_len, 0, src, src_size, lane);
    } else {
        if constexpr (kSeed) {
            // the stream's table (:830), entries >= L loaded as empty (see above)
            const uint32_t L = src_size - kMfLimit;
            const uint32_t tix = d_table_idx ? rfl(d_table_idx[blk]) : blk;
            const u32x4 *seed4 = reinterpret_cast<const u32x4 *>(d_table_in + (uint64_t)tix * 4096u);
            for (uint32_t k = lane; k < 1024u; k += 64u) {
                const u32x4 v = seed4[k];
                uint32_t e[4] = {v.x < L ? v.x : 0u, v.y < L ? v.y : 0u, v.z < L ? v.z : 0u, v.w < L ? v.w : 0u};
                if (kTag == 2) {
                    for (int q = 0; q < 4; q++)
                        if (e[q]) e[q] |= ((ld32(src + e[q]) * kHashMul) >> 12 & 0xFFu) << 24;   // v < L: in bounds
                }
                for (int q = 0; q < 4; q++) table[4u * k + q] = (T)e[q];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        } else {
        // HashTable.init(): zero fill (:266-268)
        {
            u32x4 z = {0, 0, 0, 0};
            u32x4 *t4 = reinterpret_cast<u32x4 *>(lds_raw) + wave_in_wg * (4096u * sizeof(T) / 16u);
            const uint32_t n16 = 4096u * sizeof(T) / 16u;
            for (uint32_t k = lane; k < n16; k += 64u) t4[k] = z;
        }
        }
        const uint32_t accel = acceleration < 1u ? 1u : (acceleration > 65537u ? 65537u : acceleration);   // :321
        const uint32_t cbase = accel > 64u ? accel : 64u;
        const uint32_t s_cbase = skip_sum(cbase);
        const uint32_t L = src_size - kMfLimit;                         // mflimitPlusOne :313
        const uint32_t match_limit = src_size - kLastLiterals;          // :314
        const uint64_t lane_bit = 1ull << lane;
        const uint64_t lanes_below = lane_bit - 1ull;

        uint32_t anchor = 0, op = 0;
        uint32_t F0 = 1;                                                // :317
        bool has_ins = false;    // pending put(anchor) of :438-441, folded into the next batch as lane 0
        bool failed = false;
        STAMP_DECL
        STAMP(0);   // table init

        // a window keeps going to its last lane (handing over to the next window earlier, once it holds a match, was
        // measured at every lane: 49 -> 55.6 ms, 64 -> 46.8 ms on configs[1]; any choice gives the same bytes)
        uint32_t guard = 0;      // every round of this loop consumes at least one input byte

        // Input ring of the window path: register k, lane l holds the dword at src + rbase + 256k + 4l (ring_q: at the end
        // of the block).  r0 and r1 cover [rbase, rbase + 512), r2 the next 256 bytes and is in flight.  A window
        // at A reads [A, A + 111) (16 forward bytes and 32 more for the second compare level, lanes 0..63); with
        // A - rbase < 256 that lies in r0 / r1, and it lies below src_size because the window path stops at A + 192 >= L.
        // The ring moves by 256 bytes when A - rbase reaches 256 (a window advances ~72 bytes, so r2 was issued three
        // or more windows earlier) and is reloaded when A has jumped further or the generic path ran in between.
        // (the 16 forward bytes of every window used to be a load of their own at its top: a trip through the CU's
        //  vector-memory address path behind the other wavefronts' gathers, on the chain that leads to the hash)
        // (the ring's offset lives in a VGPR, lane l = rbase + 4l, its own dword's offset: the scalar registers are full)
        // Only the u16 builds (blocks <= 65 547 bytes, 20 wavefronts per CU) have it.  The u32 builds run larger blocks
        // at as little as one wavefront per SIMD, where the permutes are latency that nothing overlaps: 1024 x 4 MiB
        // took 4.8 % longer with the ring (their second level is already fetched early, kGuess2 below).
        constexpr bool kRing = sizeof(T) == 2;
        uint32_t rpos = 0x80000000u + 4u * lane;                        // A - rbase >= 512 for every A: empty
        uint32_t r0 = 0, r1 = 0, r2 = 0;
        // lane's dword at q; a lane whose dword would reach past src_size reads the block's last dword instead (never
        // used: a window only reads below A + 111)
        // (the bound src_size - 4 is kept in a VGPR: as a loop invariant the compiler would give it a scalar register)
        uint32_t ring_lim = 0;
        if constexpr (kRing) asm volatile("v_mov_b32 %0, %1" : "=v"(ring_lim) : "s"(src_size - 4u));
        auto ring_q = [&](uint32_t q) -> uint32_t { return q < ring_lim ? q : ring_lim; };
        // The window's dwords come out of the ring in one hop.  The window register W of A used to be a permute of its
        // own: W[i] = lane (s0 + i) & 63 of sel, sel = lane >= s0 ? r0 : r1, s0 = (A - rbase) >> 2 -- the select depends on
        // the source lane only (lanes below s0 hold the dwords that wrapped into r1).  So the dword a lane wants,
        // W[jw + k], is sel[(s0 + jw + k) & 63]: the forward permutes read sel directly, and the window pays one
        // ds_bpermute and one dependent LDS wait less.  ring_sel moves or reloads the ring first and yields the snapshot
        // sel (a copy: it stays valid when the ring moves later) and ja, this lane's permute address of W[jw]:
        // 4 * ((s0 + jw) & 63), jw = ((A & 3) + lane) >> 2.
        auto ring_sel = [&](uint32_t A, uint32_t &ja) -> uint32_t {
            uint32_t rel = rfl(A - rpos);                               // A - rbase (lane 0)
            if (rel >= 256u) {
                // The ring's loads are issued by hand, move and reload in one statement: the compiler carries the ring
                // around the loop with copies, and waits for a load at the first copy of its register, i.e. at once.
                // Here r2 stays in its register until the next statement's wait (tools/check_compress_ring_asm.py
                // audits that no instruction reads, copies or spills it on any path before a wait that covers it).
                // A reload waits for r0 / r1 on the spot: where long matches make the anchor jump past the ring at
                // most windows (D-reptext) that wait is not hidden, and the ring costs 2.8 % there
                // (profiles/r06_compress_ring.md: the variants that hid it lost more elsewhere).
                const bool reload = rel >= 512u;
                const uint32_t nb = reload ? (A & ~127u) + 4u * lane : rpos + 256u;
                asm volatile("s_waitcnt vmcnt(0)\n\t"               // the previous r2
                             "s_cmpk_lt_u32 %[rel], 0x200\n\t"   // move
                             "s_cbranch_scc1 1f\n\t"
                             "global_load_dword %[r0], %[q0], %[src]\n\t"
                             "global_load_dword %[r1], %[q1], %[src]\n\t"
                             "s_waitcnt vmcnt(0)\n\t"
                             "s_branch 2f\n"
                             "1:\n\t"
                             "v_mov_b32 %[r0], %[r1]\n\t"
                             "v_mov_b32 %[r1], %[r2]\n"
                             "2:\n\t"
                             "global_load_dword %[r2], %[q2], %[src]"
                             : [r0] "+v"(r0), [r1] "+v"(r1), [r2] "+v"(r2)
                             : [rel] "s"(rel), [q0] "v"(ring_q(nb)), [q1] "v"(ring_q(nb + 256u)), [q2] "v"(ring_q(nb + 512u)),
                               [src] "s"(src)
                             : "scc", "memory");
                rpos = nb;
                rel = reload ? A & 127u : rel - 256u;
            }
            // (rel & ~3) = 4 s0 < 256 and ((A & 3) + lane) & ~3 = 4 jw <= 64: the byte keeps the lane index modulo 64
            ja = ((rel & ~3u) + (((A & 3u) + lane) & ~3u)) & 0xFFu;
            return lane >= (rel >> 2) ? r0 : r1;
        };
        // W[jw + K] of the snapshot (K <= 12).  The lane index is taken modulo 64 here, in the low byte of the address
        // (add_wrap_byte); nothing is left to what the instruction's offset field does past lane 63.
#define ZLZ4_SEL_DWORD(sel, ja, K) ((uint32_t)__builtin_amdgcn_ds_bpermute((int)add_wrap_byte<4u * (K)>(ja), (int)(sel)))
        // the 16 bytes at A + lane; hi4 = W[jw + 4], the last dword fetched, which the second compare level starts from
        auto ring_fwd = [&](uint32_t sel, uint32_t ja, uint32_t A, uint32_t &hi4) -> u32x4 {
            const uint32_t sh = (A + lane) & 3u;
            const uint32_t w0 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)ja, (int)sel);
            const uint32_t w1 = ZLZ4_SEL_DWORD(sel, ja, 1), w2 = ZLZ4_SEL_DWORD(sel, ja, 2), w3 = ZLZ4_SEL_DWORD(sel, ja, 3);
            hi4 = ZLZ4_SEL_DWORD(sel, ja, 4);
            return u32x4{__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                         __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(hi4, w3, sh)};
        };
        // bytes 16..47 at A + lane: dwords jw + 5 .. jw + 12 of the snapshot behind the kept hi4 (jw + 12 <= 28).  The
        // second level used to fetch W[jw + 4] again.
        auto ring_fwd2 = [&](uint32_t sel, uint32_t ja, uint32_t A, uint32_t hi4, u32x4 &f2, u32x4 &f3) {
            const uint32_t sh = (A + lane) & 3u;
            const uint32_t w5 = ZLZ4_SEL_DWORD(sel, ja, 5), w6 = ZLZ4_SEL_DWORD(sel, ja, 6), w7 = ZLZ4_SEL_DWORD(sel, ja, 7);
            const uint32_t w8 = ZLZ4_SEL_DWORD(sel, ja, 8), w9 = ZLZ4_SEL_DWORD(sel, ja, 9), w10 = ZLZ4_SEL_DWORD(sel, ja, 10);
            const uint32_t w11 = ZLZ4_SEL_DWORD(sel, ja, 11), w12 = ZLZ4_SEL_DWORD(sel, ja, 12);
            f2 = u32x4{__builtin_amdgcn_alignbyte(w5, hi4, sh), __builtin_amdgcn_alignbyte(w6, w5, sh),
                       __builtin_amdgcn_alignbyte(w7, w6, sh), __builtin_amdgcn_alignbyte(w8, w7, sh)};
            f3 = u32x4{__builtin_amdgcn_alignbyte(w9, w8, sh), __builtin_amdgcn_alignbyte(w10, w9, sh),
                       __builtin_amdgcn_alignbyte(w11, w10, sh), __builtin_amdgcn_alignbyte(w12, w11, sh)};
        };
#undef ZLZ4_SEL_DWORD
        // forward bytes of the next window, taken from the ring (u32: loaded) as soon as its anchor is known (before the
        // emission and the table fix-up of the current window, which hide the permutes)
        u32x4 fwd_pf = {0, 0, 0, 0};
        uint32_t sel_pf = 0, ja_pf = 0, hi4_pf = 0;                     // the snapshot the second level reads on
        uint32_t pf_anchor = 0xFFFFFFFFu;
        while (F0 < L) {                                                // :320
            if (++guard > src_size) { failed = true; break; }           // unreachable; never spin on the GPU
            int32_t ub = -1;      // probe index of lane 0 of the next generic batch (-1 = pending insert pseudo-probe)

            // =====================================================================================
            // Window path (acceleration 1, away from the end of the block): lane i <-> position
            // anchor + i.  Every search that starts inside the window probes consecutive positions
            // (the first 66 probes of a search have stride 1), so all sequences that begin in these
            // 64 positions are resolved from registers: 16 forward bytes per lane from the input ring
            // (u16; six ds_bpermute, no memory) or one 16-byte load (u32), one table read / speculative put /
            // read-back, one candidate gather -- then one short loop
            // iteration per sequence.  `ins` = lanes the serial loop would have put() so far; a lane's
            // table read is its nearest earlier `ins` lane with the same hash, else the pre-window
            // value.  At the end lanes not in `ins` put their old value back.
            // A window only starts behind a match: lane 0 is the anchor's pending put (has_ins), never a probe, and
            // every lane reads, puts and reads back its slot.  The block's first search, where position 0 is neither
            // probed nor put (Q1), runs on the generic path below (seeded builds too: they start with anchor 0 and
            // has_ins false like the others); its match sets has_ins, and every window of a run hands it on.
            // =====================================================================================
            if (accel == 1u && F0 == anchor + 1u && has_ins && (uint64_t)anchor + 192u < L) {
              bool moved = false;           // the last window of the run advanced the anchor ...
              bool to_generic = false;      // ... or handed its search over to the generic path
              for (;;) {                    // consecutive windows: the next one starts without re-deriving the entry test
                const uint32_t A = anchor;
                const uint32_t pos = A + lane;
                if (kRing && pf_anchor != A) {
                    sel_pf = ring_sel(A, ja_pf);
                    fwd_pf = ring_fwd(sel_pf, ja_pf, A, hi4_pf);
                }
                const uint32_t sel = sel_pf, ja = ja_pf, hi4 = hi4_pf;
                const u32x4 fwd = (kRing || pf_anchor == A) ? fwd_pf : ld128(src + pos);
                const uint32_t prod = fwd.x * kHashMul;
                const uint32_t h = prod >> 20;                          // :341
                const uint32_t tg = (prod >> 12) & 0xFFu;
                const uint32_t mine = kTag == 2 ? (pos | (tg << 24)) : (uint32_t)(T)pos;     // my table entry
                STAMP(1);
                STAMP_COUNT(16);
                uint32_t told = tg;
                const uint32_t old_e = table[h];                        // :342
                if (kTag == 1) told = tags[h];
                if (kTag == 2) told = old_e >> 24;
                const uint32_t old = old_e & kPosMask;
                // pre-window candidates: the old table value passes `match > 0`, `match < ip` (always, unless seeded) and
                // the distance test (:345-347); its bytes are gathered once for the whole window.  The gather is
                // issued right away so that its latency overlaps the speculative put / read-back below.
                // (written mask by mask: see the note at `losers` below)
                uint64_t okm = ballot(old > 0) & ballot(old + kMaxDist >= pos);
                if (kSeed) okm &= ballot(old < pos);
                if (kTag != 0) okm &= ballot(told == tg);
                const bool old_ok = in_mask(okm);
                u32x4 cold = {0, 0, 0, 0};
                if (old_ok) cold = ld128(src + old);
                // the second compare level (bytes 16..47, below) is a round trip of its own behind the first -- unless it is
                // asked for now: a lane whose candidate and the candidate twelve lanes on are twelve bytes apart sits at the
                // start of >= 16 matching bytes almost certainly, and fetches its 32 more bytes with the gather (a wrong
                // guess costs two loads; a lane that was not guessed fetches them when it knows, as before)
                // (blocks > 64 KiB only: few large blocks leave the chip to one wavefront per SIMD, where the round trip is
                //  what counts -- 1024 x 4 MiB 121.5 -> 118.9 ms; with 20 wavefronts per CU the extra requests cost more
                //  than the round trip, configs[1] 41.3 -> 41.6 ms, D-reptext 58.9 -> 60.3 ms)
                // (u16: the forward side, bytes 16..47 at pos, comes from the input ring when it is needed)
                constexpr bool kGuess2 = sizeof(T) == 4;
                const uint32_t old12 = kGuess2 ? shfl(old, (lane + 12u) & 63u) : 0u;
                const bool pred2 = kGuess2 && old_ok && lane < 52u && old12 == old + 12u;
                u32x4 f2 = {0, 0, 0, 0}, c2 = f2, f3 = f2, c3 = f2;
                if (pred2) {
                    if (!kRing) { f2 = ld128(src + pos + 16u); f3 = ld128(src + pos + 32u); }
                    c2 = ld128(src + old + 16u); c3 = ld128(src + old + 32u);
                }
                STAMP(3);
                table[h] = (T)mine;                                     // :350 (speculative)
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
                STAMP(2);

                // What a probe at lane i finds if its table slot still holds the pre-window value: validity
                // (:345-348), the first 12 bytes of forward extension (:401-413) and the offset.  For a lane
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
                const uint64_t need2m = vom & ballot(mlo == 12u);
                const bool need2 = in_mask(need2m);
                if (need2 && !pred2) {                        // (all loads in one round trip)
                    if (!kRing) { f2 = ld128(src + pos + 16u); f3 = ld128(src + pos + 32u); }
                    c2 = ld128(src + old + 16u); c3 = ld128(src + old + 32u);
                }
                if (kRing && need2m) ring_fwd2(sel, ja, A, hi4, f2, f3);   // (wave-uniform: the permutes read every lane)
                if (need2) {
                    const uint32_t d2 = first_diff16_sel(f2, c2);
                    mlo += d2 == 16u ? 16u + first_diff16_sel(f3, c3) : d2;
                }
                // a lane whose hash no EARLIER lane of the window shares reads the pre-window value whatever the parse does --
                // the only lane of its hash, or the first of a duplicate group (round 3: the first of a group used to take
                // an exact step like the others, which found no in-window candidate and fell back to the same registers;
                // 0.55 of the 0.72 exact steps per window on text were on duplicate-hash lanes, half of them first ones)
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

                STAMP(6);
                uint32_t f = 1;          // next lane to probe
                uint32_t a = 0;          // lane of the current anchor
                // lanes strictly inside a match that has been emitted (Q6: never put()): every flush and every immediate
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
                    STAMP(9); STAMP_COUNT(21);
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
                    const uint64_t extm = mm_run & ballot(mlo_e >= 15u);                // matches with one length-extension byte (:416-429)
                    // literal runs of 15..63 bytes carry one extension byte too (:368-382): a lane's sequence is the
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
                    if (is_lit) dst[o1] = (uint8_t)fwd.x;               // literals (:390)
                    if (is_m) {
                        const uint32_t lit_k = lane - pend;             // :360
                        uint8_t *tk = dst + (o1 - 1u - lit_k - own_l);
                        tk[0] = (uint8_t)(((lit_k < 15u ? lit_k : 15u) << 4) | (mlo_e < 15u ? mlo_e : 15u));   // token
                        if (own_l) tk[1] = (uint8_t)(lit_k - 15u);
                        const uint16_t off16 = (uint16_t)off_e;                          // :395
                        __builtin_memcpy(dst + o1, &off16, 2);
                        if (mlo_e >= 15u) dst[o1 + 2u] = (uint8_t)(mlo_e - 15u);         // < 255 (mlen < 270 in a run)
                    }
                    const uint32_t nm = (uint32_t)__popcll(mm_run);
                    op += 3u * nm + (uint32_t)__popcll(litmask) + (uint32_t)__popcll(extm) + (uint32_t)__popcll(lextm);
                    cov_acc |= covm;
                    mm_run = 0;
                    E_run = 0;
                    STAMP(10);
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
                    STAMP(8);
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
                        if (rdlane(fwd.x, pr) != rdlane(fwd.x, x)) { STAMP_COUNT(19); STAMP(9); f = x + 1u; continue; }   // :348
                        STAMP_COUNT(18);
                        m_cand = A + pr;
                        const uint64_t xa = ((uint64_t)(rdlane(fwd.z, j) ^ rdlane(fwd.z, pr)) << 32) | (rdlane(fwd.y, j) ^ rdlane(fwd.y, pr));
                        const uint32_t xb = rdlane(fwd.w, j) ^ rdlane(fwd.w, pr);
                        if (xa) mlen = (uint32_t)__builtin_ctzll(xa) >> 3;
                        else if (xb) mlen = 8u + ((uint32_t)__builtin_ctz(xb) >> 3);
                        else mlen = extend_match(src, m_pos, m_cand, 12u, match_limit, src_size, lane);
                    } else {
                        // the probe reads the pre-window value: the vector code has already compared up to 48 bytes
                        if (!(q & 1u)) { STAMP_COUNT(19); STAMP(9); f = x + 1u; continue; }      // probed, put, no match: next probe
                        STAMP_COUNT(18);
                        mlen = q >> 2;
                        if (mlen < 44u && !tight) {
                            // mlo_e / off_e of lane j already describe this sequence: it just joins the run
                            mm_run |= 1ull << j;
                            a = j + kMinMatch + mlen;
                            if (a < 64u) E_run |= 1ull << a;
                            STAMP(9);
                            if (a >= 64u) break;                            // the next window inserts it as its lane 0
                            f = a + 1u;
                            continue;
                        }
                        m_cand = rdlane(old, x);
                        if (mlen >= 44u) mlen = extend_match(src, m_pos, m_cand, 44u, match_limit, src_size, lane);
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
                        STAMP(9);
                        if (e >= 64u) break;                                // the next window inserts it as its lane 0
                        f = e + 1u;
                        continue;
                    }
                    if (mm_run) flush_run();
                    // immediate emission (:360-432), literals = low bytes of lanes a..j-1
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
                    if constexpr (kRing) {
                        sel_pf = ring_sel(pf_anchor, ja_pf);
                        fwd_pf = ring_fwd(sel_pf, ja_pf, pf_anchor, hi4_pf);
                    } else {
                        fwd_pf = ld128(src + pf_anchor + lane);
                    }
                }
                if (mm_run && !failed) flush_run();
                anchor = A + a;
                STAMP(4);
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
                if (put_mine || gi == 0) table[h] = (T)(put_mine ? mine : old_e);
                if (kTag == 1 && put_mine) tags[h] = (uint8_t)tg;       // (the speculative put left the old tag in place)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                STAMP(5);
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
            // Generic path: any acceleration, block tail, searches longer than one window.
            // 64 probes of ONE search per step.
            // =====================================================================================
            bool found = false, bailed = false;
            uint32_t m_pos = 0, m_cand = 0, m_local = 0;
            bool m_local_done = false;
            for (;;) {
                const int32_t u = ub + (int32_t)lane;
                uint32_t pos, step_next;
                if (u <= 0) {
                    pos = (u < 0) ? F0 - 1u : F0;
                    step_next = accel;                  // u == 0: bail iff F0 + a > L  (:331-335, first iteration)
                } else if (u == 1) {
                    pos = F0 + accel;
                    step_next = accel >> 6;
                } else {
                    const uint32_t x = cbase + (uint32_t)u - 1u;
                    pos = F0 + accel + skip_sum(x) - s_cbase;
                    step_next = x >> 6;
                }
                const bool is_probe = u >= 0;
                const bool bail = is_probe && ((uint64_t)pos + step_next > L);
                const uint64_t bail_mask = ballot(bail);
                // bail is monotone in u: everything from the first bailing lane on is out of the search
                const uint32_t nb = bail_mask ? first_lane(bail_mask) : 64u;
                const bool active = (lane < nb) && (is_probe || has_ins);

                // forward data: 16 B when they are inside the block, else the 4 hashed bytes only
                const bool have16 = active && (pos + 16u <= src_size);
                u32x4 fwd = {0, 0, 0, 0};
                if (have16) fwd = ld128(src + pos);
                else if (active) fwd.x = ld32(src + pos);
                const uint32_t prod = fwd.x * kHashMul;
                const uint32_t h = prod >> 20;                          // :341
                const uint32_t tg = (prod >> 12) & 0xFFu;
                const uint32_t mine = kTag == 2 ? (pos | (tg << 24)) : (uint32_t)(T)pos;

                // table read / speculative put / read-back
                uint32_t old_e = 0, rb = 0, told = tg;
                if (active) {
                    old_e = table[h];                                   // :342
                    if (kTag == 1) told = tags[h];
                    table[h] = (T)mine;                                 // :350 (speculative)
                }
                if (kTag == 2) told = old_e >> 24;
                const uint32_t old = old_e & kPosMask;
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

                // the four validity tests of :345-348
                bool valid = is_probe && active && cand > 0 && cand < pos && (cand + kMaxDist >= pos) &&
                             (kTag == 0 || pred >= 0 || told == tg);
                u32x4 cnd = {0, 0, 0, 0};
                if (valid) {
                    if (have16) cnd = ld128(src + cand); else cnd.x = ld32(src + cand);
                    valid = cnd.x == fwd.x;
                }
                const uint64_t valid_mask = ballot(valid);

                if (valid_mask) {
                    // ---- match at lane wl (first valid probe, :352) ----
                    const uint32_t wl = first_lane(valid_mask);
                    // lanes after the winner never ran in the serial loop: undo their puts, then
                    // re-commit the last lane <= wl of every duplicate group
                    if (active && lane > wl) table[h] = (T)old_e;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    const uint64_t upto = (2ull << wl) - 1ull;   // lanes 0..wl
                    if (active && lane <= wl && ((grp & upto & ~lanes_below & ~lane_bit) == 0)) {
                        table[h] = (T)mine;
                        if (kTag == 1) tags[h] = (uint8_t)tg;
                    }
                    // local extension: bytes 4..15 of the two 16-byte reads (:401-413)
                    uint32_t loc = 0;
                    bool loc_done = false;
                    if (lane == wl) {
                        const uint32_t lim = match_limit - (pos + kMinMatch);   // bytes that may still be compared
                        if (have16) {
                            u32x4 a = fwd, b = cnd;
                            a.x = 0; b.x = 0;
                            loc = first_diff16(a, b) - 4u;       // 0..12
                            if (loc >= lim) { loc = lim; loc_done = true; }
                            else if (loc < 12u) loc_done = true;
                        }
                    }
                    m_pos = rdlane(pos, wl);
                    m_cand = rdlane(cand, wl);
                    m_local = rdlane(loc, wl);
                    m_local_done = rdlane((uint32_t)loc_done, wl) != 0;
                    found = true;
                    break;
                }
                if (bail_mask) {                                        // :335-338 -> finishCompression
                    if constexpr (kSeed) {
                        // the final table is an output here: the last lane of every duplicate group holds the slot
                        if (active && ((grp & ~lanes_below & ~lane_bit) == 0) && grp != lane_bit) table[h] = (T)mine;
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    }
                    bailed = true; break;
                }
                // no match in 64 probes: all puts stand; fix duplicate groups so the last lane's position is stored
                if (active && ((grp & ~lanes_below & ~lane_bit) == 0)) {
                    if (grp != lane_bit) table[h] = (T)mine;
                    if (kTag == 1) tags[h] = (uint8_t)tg;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                ub += 64;
            }
            if (bailed || !found) break;
            STAMP_COUNT(20);

            // ---------------- forward extension (:401-413) ----------------
            const uint32_t mlen = m_local_done ? m_local
                                               : extend_match(src, m_pos, m_cand, m_local, match_limit, src_size, lane);

            // ---------------- emit the sequence (:360-432) ----------------
            const uint32_t lit = m_pos - anchor;                        // :360
            const uint32_t nle = ext_len_bytes(lit), nme = ext_len_bytes(mlen);
            const uint64_t seq_end = (uint64_t)op + 1u + nle + lit + 2u + nme;
            if (seq_end > dst_len) { failed = true; break; }            // :365-:427 (any of them)
            if (lane == 0)
                dst[op] = (uint8_t)(((lit >= 15u ? 15u : lit) << 4) | (mlen >= 15u ? 15u : mlen));
            if (lit >= 15u) write_ext_len(dst + op + 1u, lit, lane);
            uint8_t *o = dst + op + 1u + nle;
            copy_bytes(o, src + anchor, lit, lane);                     // :390
            o += lit;
            const uint32_t offset = m_pos - m_cand;                     // :395
            if (lane < 2u) o[lane] = (uint8_t)(offset >> (8u * lane));  // :397
            if (mlen >= 15u) write_ext_len(o + 2u, mlen, lane);
            op = (uint32_t)seq_end;

            // ---------------- after the match (:435-442) ----------------
            const uint32_t end = m_pos + kMinMatch + mlen;
            anchor = end;
            if (end < L) { has_ins = true; F0 = end + 1u; }
            else { has_ins = false; F0 = L; }
        }
        if constexpr (kRing) asm volatile("s_waitcnt vmcnt(0)" : "+v"(r2));   // (the ring's last load, before the wave can end)
        if constexpr (kSeed) {
            // a match that ends at L - 1 leaves its put(anchor) (:732-736) pending when the loop ends (F0 = L): the final
            // table is an output here, so it is applied
            if (!failed && has_ins && F0 >= L && lane == 0) {
                const uint32_t prod = ld32(src + anchor) * kHashMul;
                table[prod >> 20] = (T)(kTag == 2 ? (anchor | ((prod >> 12 & 0xFFu) << 24)) : anchor);
            }
        }
        res = failed ? kErrOutputTooSmall
                     : emit_last_literals(dst, dst_len, op, src + anchor, src_size - anchor, lane);   // :337, :446
        STAMP(7);   // tail
        STAMP_FLUSH;
    }
    if constexpr (kSeed) {
        // Stream.hashTable after the call (:830-833): merged where this block compressed, else the input table
        if (d_table_out) {
            const uint32_t tix = d_table_idx ? rfl(d_table_idx[blk]) : blk;
            const uint32_t *seed = d_table_in + (uint64_t)tix * 4096u;
            uint32_t *out = d_table_out + (uint64_t)blk * 4096u;
            const bool merged = src_size >= kMfLimit + 1u && src_size <= max_in_len && src_size <= kMaxInput && res >= 0;
            if (merged) {
                const uint32_t L = src_size - kMfLimit;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                for (uint32_t k = lane; k < 4096u; k += 64u) {
                    const uint32_t v = seed[k];
                    const uint32_t loaded = v < L ? v : 0u;
                    const uint32_t f = (uint32_t)table[k] & kPosMask;
                    out[k] = f != loaded ? f : v;
                }
            } else if (out != seed) {
                const u32x4 *s4 = reinterpret_cast<const u32x4 *>(seed);
                u32x4 *o4 = reinterpret_cast<u32x4 *>(out);
                for (uint32_t k = lane; k < 1024u; k += 64u) o4[k] = s4[k];
            }
        }
    }
    if (lane == 0) d_result[blk] = res;
}

// Stream.loadDict (src/lz4.zig:798-820), one workgroup per dictionary: the table of the last min(len, 64 KiB) bytes,
// table[hash4(rd32(tail + i))] = i for i in [0, dictSize - 5] (:810-815; a dictionary of 4 bytes or fewer hashes
// nothing).  "Last writer wins" is an LDS atomicMax per position (position 0 stores 0 = what the reference stores).  A
// lane whose right neighbour has the same hash leaves the slot to it (the neighbour's position is larger), so a run of
// one repeated byte, whose 64 Ki positions all share one slot, costs one atomic per wavefront instead of 64.
__global__ __launch_bounds__(256) void k_load_dict(const uint8_t *__restrict__ d_dict, const uint64_t *__restrict__ d_dict_off,
                                                   const uint32_t *__restrict__ d_dict_len, uint32_t *__restrict__ d_tables,
                                                   int64_t *__restrict__ d_result, uint32_t ndicts) {
    __shared__ uint32_t t[4096];
    const uint32_t d = blockIdx.x;
    if (d >= ndicts) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t len = d_dict_len[d];
    const uint32_t size = len < 65536u ? len : 65536u;                  // :804
    const uint8_t *tail = d_dict + d_dict_off[d] + (len - size);        // :805
    for (uint32_t k = threadIdx.x; k < 4096u; k += blockDim.x) t[k] = 0;   // resetFast (:799)
    __syncthreads();
    if (size >= kMinMatch) {                                            // :810
        const uint32_t n = size - kMinMatch;                            // :812  i < dictSize - MINMATCH
        for (uint32_t base = threadIdx.x - lane; base < n; base += blockDim.x) {   // wave-uniform trip count
            const uint32_t i = base + lane;
            const bool act = i < n;
            const uint32_t h = act ? hash4(ld32(tail + i)) : 0xFFFFFFFFu;  // :813
            const uint32_t hr = shfl(h, lane + 1u);                     // (lane 63 reads lane 0: ignored below)
            if (act && !(lane < 63u && hr == h)) atomicMax(&t[h], i);    // :814
        }
    }
    __syncthreads();
    uint32_t *out = d_tables + (uint64_t)d * 4096u;
    for (uint32_t k = threadIdx.x; k < 4096u; k += blockDim.x) out[k] = t[k];
    if (threadIdx.x == 0) d_result[d] = (int64_t)size;                  // :818
}

}  // namespace zlz4

extern "C" int zlz4_launch_compress_fast(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                         const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                         const uint32_t *d_out_cap, int64_t *d_result, uint32_t nblocks,
                                         uint32_t max_in_len, uint32_t acceleration) {
    if (nblocks == 0) return 0;
    // experiment knob: extra dynamic LDS per workgroup lowers the number of resident waves per CU
    static const uint32_t lds_pad = [] { const char *e = zlz4_tune_env("ZLZ4_TUNE_LDS_PAD"); return e ? (uint32_t)atoi(e) : 0u; }();
    // every position stored in the table is < srcSize - 12, so 16-bit entries are exact up to 65547-byte blocks
    static const uint32_t tune_wpw = [] { const char *e = zlz4_tune_env("ZLZ4_TUNE_WPW"); return e ? (uint32_t)atoi(e) : 0u; }();
    // tags (see k_compress_fast): free in a u32 entry (configs[4] shape 132.6 -> 125.9 ms); beside the u16 table they cost
    // LDS, 20 -> 13 wavefronts per CU, and lose (configs[1] 42.8 -> 54.0 ms; profiles/r03_fast_compress_tags.md), so
    // the u16 build carries them only when asked to (tuning build: ZLZ4_TUNE_TAG=1)
    static const int tune_tag = [] { const char *e = zlz4_tune_env("ZLZ4_TUNE_TAG"); return e ? atoi(e) : -1; }();
#define ZLZ4_LAUNCH_FAST(KERN, T, TAG, WPW, LDS)                                                                      \
    hipLaunchKernelGGL((zlz4::KERN<T, TAG>), dim3((nblocks + (WPW) - 1) / (WPW)), dim3(64 * (WPW)), (LDS),              \
                       stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_result, nblocks, acceleration,  \
                       max_in_len, nullptr, nullptr, nullptr)
    if (max_in_len <= 65536u + 11u) {
        // 8 KiB of table (+ 4 KiB of tags) per wavefront in LDS -> 20 (13) wavefronts per CU whatever the workgroup size;
        // one-wave workgroups measured 5 % faster than four-wave ones on MI355X (44.1 / 45.0 / 46.6 ms for 1 / 2 / 4 on
        // configs[1]): a finished block frees its slot at once instead of waiting for the slowest of four
        const uint32_t wpw = (tune_wpw == 2 || tune_wpw == 4) ? tune_wpw : 1;
        if (tune_tag > 0) ZLZ4_LAUNCH_FAST(k_compress_fast, uint16_t, 1, wpw, wpw * (4096 * sizeof(uint16_t) + 4096) + lds_pad);
        else ZLZ4_LAUNCH_FAST(k_compress_fast, uint16_t, 0, wpw, wpw * 4096 * sizeof(uint16_t) + lds_pad);
    } else {
        const uint32_t wpw = (tune_wpw == 2) ? 2 : 1;   // 16 KiB of LDS per wavefront -> 10 wavefronts per CU
        // positions below 2^24 leave the top byte of a u32 entry to the tag
        if (tune_tag != 0 && max_in_len <= (1u << 24)) ZLZ4_LAUNCH_FAST(k_compress_fast, uint32_t, 2, wpw, wpw * 4096 * sizeof(uint32_t) + lds_pad);
        else ZLZ4_LAUNCH_FAST(k_compress_fast, uint32_t, 0, wpw, wpw * 4096 * sizeof(uint32_t) + lds_pad);
    }
#undef ZLZ4_LAUNCH_FAST
    return zlz4_launch_status();
}

// Stream.compressFastContinue per block (see k_compress_fast, kSeed).  The same table widths as the launcher above, with
// the tag packed into u32 entries; never the u16 table with a separate tag array (kTag == 1).
extern "C" int zlz4_launch_compress_fast_continue(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                                  const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                                  const uint32_t *d_out_cap, const uint32_t *d_table_in,
                                                  const uint32_t *d_table_idx, uint32_t *d_table_out, int64_t *d_result,
                                                  uint32_t nblocks, uint32_t max_in_len, uint32_t acceleration) {
    if (nblocks == 0) return 0;
    static const int tune_tag = [] { const char *e = zlz4_tune_env("ZLZ4_TUNE_TAG"); return e ? atoi(e) : -1; }();
#define ZLZ4_LAUNCH_SEEDED(T, TAG)                                                                                      \
    hipLaunchKernelGGL((zlz4::k_compress_fast<T, TAG, true>), dim3(nblocks), dim3(64), 4096 * sizeof(T), stream, d_in,   \
                       d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_result, nblocks, acceleration, max_in_len,      \
                       d_table_in, d_table_idx, d_table_out)
    if (max_in_len <= 65536u + 11u) ZLZ4_LAUNCH_SEEDED(uint16_t, 0);
    else if (tune_tag != 0 && max_in_len <= (1u << 24)) ZLZ4_LAUNCH_SEEDED(uint32_t, 2);
    else ZLZ4_LAUNCH_SEEDED(uint32_t, 0);
#undef ZLZ4_LAUNCH_SEEDED
    return zlz4_launch_status();
}

extern "C" int zlz4_launch_load_dict(hipStream_t stream, const uint8_t *d_dict, const uint64_t *d_dict_off,
                                     const uint32_t *d_dict_len, uint32_t *d_tables, int64_t *d_result, uint32_t ndicts) {
    if (ndicts == 0) return 0;
    hipLaunchKernelGGL(zlz4::k_load_dict, dim3(ndicts), dim3(256), 0, stream, d_dict, d_dict_off, d_dict_len, d_tables,
                       d_result, ndicts);
    return zlz4_launch_status();
}

#ifdef ZLZ4_STAMPS
extern "C" int zlz4_debug_read_stamps(unsigned long long *out16, int reset) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_zlz4_stamps), 24 * sizeof(unsigned long long)) != hipSuccess) return ZLZ4_ERR_DEVICE;
    if (reset) {
        unsigned long long z[24] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_zlz4_stamps), z, sizeof z) != hipSuccess) return ZLZ4_ERR_DEVICE;
    }
    return 0;
}
#endif
