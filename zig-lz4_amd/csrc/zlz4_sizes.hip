// zlz4_sizes.hip -- decompressed-size queries for gfx950: what a decode WOULD return, with no output buffer.
//
// k_decompressed_size walks decompressGeneric (reference src/lz4.zig:89-251) one wavefront per block with the decision
// order and the exits of k_decompress_safe (zlz4_decompress.hip), into a destination of
// kSizeCap = 0xFFFFFFFF bytes (the library's per-block limit), and touches no output: a match is
// only TESTED (:154, :174, :181-192), never copied.  A dictionary takes part by its length alone: a match that reaches
// in front of the block is CorruptedData iff offset > op + min(dict_len, 65536) (:189-192), after the match's
// OutputTooSmall test (:174); no dictionary byte is read.
//
// The parse is the decoder's: tokens are taken in batches out of a streaming three-register window with the scalar walk
// over the token chain (the description is at k_decompress_safe; the window loads are hand-issued and awaited once per
// batch), everything a batch cannot take goes through the single-sequence paths.  Different from the decoder:
//   * a run of 255 length-extension bytes is consumed from the window with a ballot, 64 bytes per step, and 1 KiB per step
//     (16 bytes per lane) once a whole window was 255s -- the decoder walks it a byte at a time, which is slowest on the
//     most compressible data (a 64 KiB block of zeros is one token and 257 extension bytes);
//   * lengths are accumulated in 64 bits and compared in 64 bits, so op and kSizeCap - op are exact up to the limit (the
//     decoder saturates a length at 0xFFFF0000, which is only right below a capacity of that size).  An input has fewer
//     than 2^32 bytes, so a length stays below 2^40: nothing wraps.
//
// k_plan_outputs turns sizes into packed output slots (offset, capacity, total) on the device.
#include "zlz4_device.hpp"
#include "zlz4_launch.hpp"

namespace zlz4 {

namespace {

constexpr uint32_t kSizeCap = 0xFFFFFFFFu;

}  // namespace

__global__ __launch_bounds__(256) void k_decompressed_size(
    const uint8_t *__restrict__ d_in, const uint64_t *__restrict__ d_in_off, const uint32_t *__restrict__ d_in_len,
    const uint32_t *__restrict__ d_dict_len, int64_t *__restrict__ d_size, uint32_t nblocks) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t blk = rfl(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (blk >= nblocks) return;

    const uint8_t *src = d_in + d_in_off[blk];
    const uint32_t iend = rfl(d_in_len[blk]);   // src.len
    constexpr uint32_t oend = kSizeCap;         // dst.len
    uint32_t dlen = 0;                          // reachable dictionary length (offsets are <= 65535) :181-192
    if (d_dict_len) { const uint32_t dl = rfl(d_dict_len[blk]); dlen = dl < 65536u ? dl : 65536u; }

    int64_t res = 0;
    uint32_t ip = 0, op = 0;

    if (iend != 0) {                            // src/lz4.zig:97 (:98 never holds: dst.len is kSizeCap)
        // 64-byte register window over the compressed stream (single-sequence paths): lane i holds src[wbase + i]
        uint32_t wbase = 0;
        uint32_t w = (lane < iend) ? src[lane] : 0u;
        auto reload = [&](uint32_t pos) {
            wbase = pos;
            w = (pos + lane < iend) ? src[pos + lane] : 0u;
        };
        auto fetch = [&](uint32_t pos) -> uint32_t {   // caller guarantees pos < iend
            if (pos - wbase >= 64u) reload(pos);
            return rdlane(w, pos - wbase);
        };
        // :123-131 / :160-168: adds the extension bytes at ip to `acc` and moves ip behind the byte that ends the run;
        // false = the input ended first (:125 / :162).  Lanes at or behind iend hold 0, so they end a run like any byte
        // below 255 and the position decides.
        auto ext_run = [&](uint64_t &acc) -> bool {
            for (;;) {
                if (ip >= iend) return false;
                if (ip - wbase >= 64u) reload(ip);
                const uint32_t i0 = ip - wbase;
                const uint64_t stop = ballot(w != 255u) & (~0ull << i0);
                if (stop != 0) {
                    const uint32_t fl = first_lane(stop);
                    acc += 255ull * (fl - i0);
                    ip = wbase + fl;
                    if (ip >= iend) return false;
                    acc += rdlane(w, fl);
                    ip += 1u;
                    return true;
                }
                acc += 255ull * (64u - i0);
                ip = wbase + 64u;
                // a whole window of 255s: go on 16 bytes per lane while every byte of the next 1 KiB is 255
                while ((uint64_t)ip + 1024u <= iend) {
                    const u32x4 v = ld128(src + (ip + lane * 16u));
                    if (ballot((v.x & v.y & v.z & v.w) != 0xFFFFFFFFu) != 0) break;
                    acc += 255ull * 1024u;
                    ip += 1024u;
                }
            }
        };

        for (;;) {
            if (ip >= iend) break;                                  // :113
            // ---- batch path (k_decompress_safe's, without its copy side) ----
            if ((uint64_t)ip + 68u <= iend) {
              // X0 / X1 hold the dwords at xbase + lane and xbase + 64 + lane, X2 (xbase + 128 + lane) is a load in
              // flight, issued by hand and awaited once per batch; behind it goes a touch of the stream 1 KiB ahead as the
              // youngest vector-memory operation, so the batch's wait is vmcnt(1).  X2 / tdummy must not be touched
              // between issue and wait.  Every address is clamped into [0, iend - 4] (iend >= 68 here).
              auto woff = [&](uint32_t p) { const uint32_t a = p + lane; return a + 4u <= iend ? a : iend - 4u; };
              auto wload_async = [&](uint32_t p) {
                  uint32_t r;
                  asm volatile("global_load_dword %0, %1, %2" : "=v"(r) : "v"(woff(p)), "s"(src) : "memory");
                  return r;
              };
              uint32_t xbase = ip, tdummy = 0;
              uint32_t X0 = ld32(src + woff(xbase)), X1 = ld32(src + woff(xbase + 64u));
              uint32_t X2 = wload_async(xbase + 128u);
              asm volatile("s_waitcnt vmcnt(0)" : "+v"(X2), "+v"(X0), "+v"(X1));
              for (;;) {
                const uint32_t xi = ip - xbase + lane;
                const uint32_t xa = shfl(X0, xi & 63u), xb = shfl(X1, xi & 63u);
                const uint32_t w4 = xi < 64u ? xa : xb;             // lane i: src[ip + i .. ip + i + 3]
                const uint32_t b0 = w4 & 0xFFu, b1 = (w4 >> 8) & 0xFFu;
                uint32_t lit = b0 >> 4, hl = 1u;                    // :120
                bool cx = false;
                if (lit == 15u) { cx = (b1 == 255u); lit += b1; hl = 2u; }      // :123-131, one extension byte
                const uint32_t mpos = lane + hl + lit;              // window index of the offset
                const uint32_t mw = shfl(w4, mpos & 63u);           // offset (2 bytes) + first match-length extension byte
                const uint32_t off = mw & 0xFFFFu;                  // :150
                uint32_t mlc = b0 & 15u, slen = hl + lit + 2u;      // :157
                if (mlc == 15u) { const uint32_t e2 = (mw >> 16) & 0xFFu; cx = cx || (e2 == 255u); mlc += e2; slen += 1u; }   // :160-168
                const uint32_t ml = mlc + kMinMatch;                // :171, 4..273 here
                const uint32_t nxt = lane + slen;
                const bool ok = !cx && mpos <= 63u && nxt <= 64u && off != 0u;  // (:154 offset == 0 -> single path)
                const uint32_t ol = lit + ml;                       // output bytes of the sequence (<= 335)
                const uint32_t pkv = ok ? (nxt | (ol << 7)) : 0xFFFFFFFFu;      // sentinel: stops the walk
                const uint32_t room0 = oend - op;                   // :137, :174
                const uint32_t room = rfl(room0 < 4095u ? room0 : 4095u);
                // scalar walk over the token chain: R = mask of real token starts, T = output bytes, pos = window index of
                // the first token not taken (both forms are k_decompress_safe's)
                uint32_t pos, T, wa, wpk, wt;
                uint64_t R;
                const uint64_t okm = ballot(ok);
                const uint32_t pk2v = nxt | ((nxt < 64u && ((okm >> (nxt & 63u)) & 1ull)) ? 0x80u : 0u) | (ol << 8);
                if (room0 >= 7100u && (okm & 1ull)) {
                    asm volatile(
                        "s_mov_b64 %[R], 0\n\t"
                        "s_mov_b32 %[T], 0\n\t"
                        "s_mov_b32 %[A], 0\n\t"
                        "s_nop 3\n"
                        "1:\n\t"
                        "v_readlane_b32 %[pk], %[pkv], %[A]\n\t"
                        "s_and_b32 %[B], %[pk], 0x7f\n\t"
                        "s_bitset1_b64 %[R], %[A]\n\t"
                        "s_lshr_b32 %[t], %[pk], 8\n\t"
                        "s_add_u32 %[T], %[T], %[t]\n\t"
                        "s_bitcmp1_b32 %[pk], 7\n\t"
                        "s_cbranch_scc0 4f\n\t"
                        "v_readlane_b32 %[pk], %[pkv], %[B]\n\t"
                        "s_and_b32 %[A], %[pk], 0x7f\n\t"
                        "s_bitset1_b64 %[R], %[B]\n\t"
                        "s_lshr_b32 %[t], %[pk], 8\n\t"
                        "s_add_u32 %[T], %[T], %[t]\n\t"
                        "s_bitcmp1_b32 %[pk], 7\n\t"
                        "s_cbranch_scc1 1b\n\t"
                        "s_mov_b32 %[B], %[A]\n"
                        "4:\n"
                        : [R] "=&s"(R), [T] "=&s"(T), [A] "=&s"(wa), [B] "=&s"(pos), [pk] "=&s"(wpk), [t] "=&s"(wt)
                        : [pkv] "v"(pk2v)
                        : "scc");
                } else
                asm volatile(
                    "s_mov_b64 %[R], 0\n\t"
                    "s_mov_b32 %[T], 0\n\t"
                    "s_mov_b32 %[A], 0\n\t"
                    "s_nop 3\n"
                    "1:\n\t"
                    "v_readlane_b32 %[pk], %[pkv], %[A]\n\t"
                    "s_and_b32 %[B], %[pk], 0x7f\n\t"
                    "s_lshr_b32 %[t], %[pk], 7\n\t"
                    "s_add_u32 %[t], %[t], %[T]\n\t"
                    "s_cmp_gt_u32 %[t], %[room]\n\t"
                    "s_cbranch_scc1 3f\n\t"
                    "s_bitset1_b64 %[R], %[A]\n\t"
                    "s_mov_b32 %[T], %[t]\n\t"
                    "s_cmp_gt_u32 %[B], 63\n\t"
                    "s_cbranch_scc1 4f\n\t"
                    "v_readlane_b32 %[pk], %[pkv], %[B]\n\t"
                    "s_and_b32 %[A], %[pk], 0x7f\n\t"
                    "s_lshr_b32 %[t], %[pk], 7\n\t"
                    "s_add_u32 %[t], %[t], %[T]\n\t"
                    "s_cmp_gt_u32 %[t], %[room]\n\t"
                    "s_cbranch_scc1 4f\n\t"
                    "s_bitset1_b64 %[R], %[B]\n\t"
                    "s_mov_b32 %[T], %[t]\n\t"
                    "s_cmp_lt_u32 %[A], 64\n\t"
                    "s_cbranch_scc1 1b\n"
                    "3:\n\t"
                    "s_mov_b32 %[B], %[A]\n"
                    "4:\n"
                    : [R] "=&s"(R), [T] "=&s"(T), [A] "=&s"(wa), [B] "=&s"(pos), [pk] "=&s"(wpk), [t] "=&s"(wt)
                    : [pkv] "v"(pkv), [room] "s"(room)
                    : "scc");
                // :181-192 offset > op + dictionary: end the batch in front of the first such sequence (the single path
                // reports it).  op + T <= oend, so no sum below wraps.
                if (R != 0) {
                    const bool real0 = (R >> lane) & 1ull;
                    const uint32_t x = real0 ? ol : 0u;
                    const uint32_t relv = wave_incl_scan(x) - x;    // output offset of the sequence inside the batch
                    const uint32_t pr = op + relv + lit;
                    const uint64_t vm = ballot(real0 && off > pr && off - pr > dlen);
                    if (vm != 0) {
                        const uint32_t fb = first_lane(vm);
                        R &= (1ull << fb) - 1ull;
                        T = rdlane(relv, fb);
                        pos = fb;
                    }
                }
                // the one wait of a batch: the window load issued a batch ago (everything but the touch)
                asm volatile("s_waitcnt vmcnt(1)" : "+v"(X2), "+v"(tdummy));
                if (R == 0) break;                                  // the single-sequence paths take this one
                op += T;
                ip += pos;
                if ((uint64_t)ip + 68u > iend) break;
                {   // branch-free shift, one window load per batch, then the touch
                    const bool adv = ip - xbase >= 64u;
                    X0 = adv ? X1 : X0; X1 = adv ? X2 : X1; xbase += adv ? 64u : 0u;
                    X2 = wload_async(xbase + 128u);
                    const uint32_t ta = xbase + 128u + 1024u;
                    const uint32_t toff = ta < iend ? ta : iend - 1u;
                    asm volatile("global_load_ubyte %0, %1, %2" : "+v"(tdummy) : "v"(toff), "s"(src) : "memory");
                }
              }
              asm volatile("s_waitcnt vmcnt(0)" : "+v"(X2), "+v"(tdummy));
              if (ip >= iend) break;
            }
            // ---- fast path: the whole sequence header (token, <= 14 literals, offset) sits inside the window,
            //      no length extension bytes.  Same checks in the same order as the general path below. ----
            if (ip - wbase > 44u) reload(ip);                       // keep >= 20 window bytes ahead of the token
            {
                const uint32_t i0 = ip - wbase;
                const uint32_t token = rdlane(w, i0);               // :116
                const uint32_t lit = token >> 4, mlc = token & 15u; // :120, :157
                const uint32_t in_rem = iend - ip - 1u;             // bytes after the token
                if (lit != 15u && mlc != 15u && in_rem >= lit + 2u) {
                    // (in_rem >= lit + 2 : literals fit (:136) and the offset is present (:146, :149))
                    if (lit > oend - op) { res = kErrOutputTooSmall; break; }            // :137
                    op += lit;
                    const uint32_t offset = rdlane(w, i0 + 1u + lit) | (rdlane(w, i0 + 2u + lit) << 8);   // :150
                    ip += 3u + lit;
                    if (offset == 0) { res = kErrCorrupted; break; }                     // :154
                    const uint32_t ml = mlc + kMinMatch;                                 // :171 (4..18)
                    if (ml > oend - op) { res = kErrOutputTooSmall; break; }             // :174
                    if (offset > op && offset - op > dlen) { res = kErrCorrupted; break; }   // :181-192
                    op += ml;
                    continue;
                }
            }
            // ---- general path (length extensions, long literal runs, end of block, malformed input) ----
            const uint32_t token = fetch(ip);                       // :116
            ip += 1;
            uint64_t lit = token >> 4;                              // :120
            if (lit == 15u && !ext_run(lit)) { res = kErrCorrupted; break; }   // :123-131
            if (lit > 0) {                                          // :134
                if (lit > iend - ip) { res = kErrCorrupted; break; }        // :136
                if (lit > oend - op) { res = kErrOutputTooSmall; break; }   // :137
                ip += (uint32_t)lit;                                // (literals are skipped, the window follows lazily)
                op += (uint32_t)lit;
            }
            if (ip >= iend) break;                                  // :146
            if (iend - ip < 2u) { res = kErrCorrupted; break; }     // :149
            const uint32_t offset = fetch(ip) | (fetch(ip + 1u) << 8);   // :150
            ip += 2;
            if (offset == 0) { res = kErrCorrupted; break; }        // :154
            uint64_t ml = token & 15u;                              // :157
            if (ml == 15u && !ext_run(ml)) { res = kErrCorrupted; break; }     // :160-168
            ml += kMinMatch;                                        // :171
            if (ml > oend - op) { res = kErrOutputTooSmall; break; }   // :174
            if (offset > op && offset - op > dlen) { res = kErrCorrupted; break; }   // :181-192
            op += (uint32_t)ml;
        }
        if (res == 0) res = (int64_t)op;                            // :250
    }
    if (lane == 0) d_size[blk] = res;
}

// Packed output slots from sizes: slot i holds max(size[i], 0) bytes rounded up to `align` (a power of two, >= 1), its
// offset is the exclusive scan of the slot sizes, its capacity the size itself (0 for a failed block), total = the sum.
// One workgroup: thread t sums a contiguous run of blocks, the 1024 run sums are scanned in LDS, then every thread writes
// its run (k_bf_scan of the frame batch).
__global__ __launch_bounds__(1024) void k_plan_outputs(const int64_t *__restrict__ d_size, uint32_t n, uint64_t align,
                                                       uint64_t *__restrict__ d_out_off, uint32_t *__restrict__ d_out_cap,
                                                       uint64_t *__restrict__ d_total) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + 1023u) / 1024u;
    const uint64_t b0 = (uint64_t)t * chunk;
    const uint32_t lo = b0 < n ? (uint32_t)b0 : n;
    const uint32_t hi = b0 + chunk < n ? (uint32_t)(b0 + chunk) : n;
    auto slot = [&](int64_t s) -> uint64_t { return s > 0 ? ((uint64_t)s + (align - 1u)) & ~(align - 1u) : 0ull; };
    uint64_t s = 0;
    for (uint32_t i = lo; i < hi; i++) s += slot(d_size[i]);
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - s;
    for (uint32_t i = lo; i < hi; i++) {
        const int64_t sz = d_size[i];
        d_out_off[i] = run;
        d_out_cap[i] = sz > 0 ? (uint32_t)sz : 0u;      // (a size is at most 0xFFFFFFFF)
        run += slot(sz);
    }
    if (t == 1023u) *d_total = part[1023];
}

}  // namespace zlz4

// d_dict_len == nullptr: no dictionary
extern "C" int zlz4_launch_decompressed_size(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                             const uint32_t *d_in_len, const uint32_t *d_dict_len, int64_t *d_size,
                                             uint32_t nblocks) {
    if (nblocks == 0) return 0;
    const uint32_t waves_per_wg = 4;
    const uint32_t grid = (nblocks + waves_per_wg - 1) / waves_per_wg;
    hipLaunchKernelGGL(zlz4::k_decompressed_size, dim3(grid), dim3(64 * waves_per_wg), 0, stream, d_in, d_in_off, d_in_len,
                       d_dict_len, d_size, nblocks);
    return zlz4_launch_status();
}

// align: a power of two >= 1 (the caller checks).  n == 0 stores a total of 0.
extern "C" int zlz4_launch_plan_outputs(hipStream_t stream, const int64_t *d_size, uint32_t n, uint32_t align,
                                        uint64_t *d_out_off, uint32_t *d_out_cap, uint64_t *d_total) {
    hipLaunchKernelGGL(zlz4::k_plan_outputs, dim3(1), dim3(1024), 0, stream, d_size, n, (uint64_t)align, d_out_off,
                       d_out_cap, d_total);
    return zlz4_launch_status();
}
