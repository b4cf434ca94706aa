// zlz4_frame.hip -- LZ4 frame container (reference src/lz4f.zig) around the block kernels.
//
// compressFrame (src/lz4f.zig:354-446): the block loop carries no state from one block to the
// next, so every block is compressed by the batch kernel into a compressBound-sized slot; a
// one-wave plan kernel then does what the serial loop does with `dstPos` (stored-block decision
// :407-417, block header :418, optional block checksum :422-427) as a prefix sum, and a scatter
// kernel moves header + payload (+ checksum) of every block to its final place.  Frame header
// (:304-351), end mark (:433) and content checksum (:437-441) are written by a one-lane kernel.
//
// decompressFrame (src/lz4f.zig:541-638): the block chain is walked by one lane (each block header
// tells where the next one is), a size pass of the block decoder gives every block's decompressed
// size, a plan pass reproduces the serial `dstPos` accumulation including the order in which the
// reference would have hit an error, then all blocks are decoded / copied in parallel.
//
// XXH32 (std.hash.XxHash32 in the reference, standard XXH32 seed 0) is a strictly serial hash: one
// lane per block for block checksums, one lane for the content checksum (both are off by default,
// src/lz4f.zig:109,113).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <optional>

#include "../../include/zlz4_amd.h"
#include "zlz4_device.hpp"
#include "zlz4_frame_batch.hpp"
#include "zlz4_host.hpp"
#include "zlz4_launch.hpp"

using namespace zlz4host;

namespace {

const zlz4f_prefs kDefaultPrefs = {0, 0, 0, 0, 0, 0, 0};   // src/lz4f.zig:106-122 defaults

// BlockSizeID.toBlockSize, src/lz4f.zig:71-78
size_t block_size_of(uint32_t id) {
    switch (id) {
        case 5: return 256u * 1024;
        case 6: return 1024u * 1024;
        case 7: return 4u * 1024 * 1024;
        default: return 64u * 1024;
    }
}

// ------------------------------------------------------------------ frame header (host side, <= 19 bytes)
struct HeaderBytes { uint8_t b[20]; uint32_t n; };

// writeFrameHeader, src/lz4f.zig:304-351 (encodeFLG :152-184, encodeBD :224-232, headerChecksum :138-141) with
// `content_size` in place of p.content_size (the batch call can give every frame its own)
__host__ __device__ inline HeaderBytes encode_header_cs(const zlz4f_prefs &p, uint64_t content_size) {
    HeaderBytes h;
    for (uint32_t k = 0; k < sizeof h.b; k++) h.b[k] = 0;
    uint32_t pos = 0;
    const uint32_t magic = ZLZ4F_MAGICNUMBER;
    for (int k = 0; k < 4; k++) h.b[pos++] = (uint8_t)(magic >> (8 * k));
    uint8_t flg = 0x40;
    if (p.block_mode == 1) flg |= 0x20;
    if (p.block_checksum == 1) flg |= 0x10;
    if (content_size != 0) flg |= 0x08;
    if (p.content_checksum == 1) flg |= 0x04;
    if (p.dict_id != 0) flg |= 0x01;
    h.b[pos++] = flg;
    uint8_t bd = 4;
    if (p.block_size_id == 5) bd = 5; else if (p.block_size_id == 6) bd = 6; else if (p.block_size_id == 7) bd = 7;
    h.b[pos++] = (uint8_t)(bd << 4);
    if (content_size != 0) for (int k = 0; k < 8; k++) h.b[pos++] = (uint8_t)(content_size >> (8 * k));
    if (p.dict_id != 0) for (int k = 0; k < 4; k++) h.b[pos++] = (uint8_t)(p.dict_id >> (8 * k));
    h.b[pos] = (uint8_t)((xxh32(h.b + 4, pos - 4, 0) >> 8) & 0xFF);
    pos += 1;
    h.n = pos;
    return h;
}

HeaderBytes encode_header(const zlz4f_prefs &p) { return encode_header_cs(p, p.content_size); }

// ------------------------------------------------------------------ compress-side kernels
// block descriptors for the batch kernels: block i = src[i*bs, min(n, (i+1)*bs)) -> slot i
__global__ void k_frame_desc(uint64_t n, uint64_t bs, uint64_t slot, uint32_t nblocks, uint64_t *in_off,
                             uint32_t *in_len, uint64_t *out_off, uint32_t *out_cap) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nblocks; i += gridDim.x * blockDim.x) {
        const uint64_t o = (uint64_t)i * bs;
        in_off[i] = o;
        in_len[i] = (uint32_t)((n - o) < bs ? (n - o) : bs);
        out_off[i] = (uint64_t)i * slot;
        out_cap[i] = (uint32_t)slot;
    }
}

// plan[0] = total frame bytes, plan[1] = first failing block + 1 (0 = none), plan[2] = its error code
// One wavefront; 64 blocks per step with a shuffle prefix sum (the serial dstPos of src/lz4f.zig:379-430).
__global__ __launch_bounds__(64) void k_frame_plan(const int64_t *__restrict__ csize, const uint32_t *__restrict__ in_len,
                                                   uint32_t nblocks, uint32_t block_checksum, uint64_t start,
                                                   uint64_t *__restrict__ dst_off, uint32_t *__restrict__ hdr,
                                                   int64_t *__restrict__ plan) {
    const uint32_t lane = threadIdx.x;
    uint64_t pos = start;
    uint32_t bad = 0;
    int64_t bad_code = 0;
    for (uint32_t base = 0; base < nblocks; base += 64u) {
        const uint32_t i = base + lane;
        uint64_t bytes = 0;
        uint32_t h = 0;
        bool err = false;
        int64_t c = 0;
        if (i < nblocks) {
            c = csize[i];
            const uint32_t len = in_len[i];
            err = c < 0;
            const bool stored = !err && (uint64_t)c >= len;           // :407
            const uint32_t actual = stored ? len : (uint32_t)(err ? 0 : c);
            h = actual | (stored ? 0x80000000u : 0u);                 // :411-414
            bytes = 4u + (uint64_t)actual + (block_checksum ? 4u : 0u);
        }
        const uint64_t em = zlz4::ballot(err);
        if (em && !bad) {
            const uint32_t l = zlz4::first_lane(em);
            bad = base + l + 1u;
            bad_code = (int64_t)(int32_t)zlz4::rdlane((uint32_t)c, l);   // error codes are small negatives
        }
        uint64_t incl = bytes;                                        // inclusive scan over the 64 lanes
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t lo = __shfl_up((uint32_t)incl, d), hi = __shfl_up((uint32_t)(incl >> 32), d);
            if (lane >= d) incl += ((uint64_t)hi << 32) | lo;
        }
        if (i < nblocks) { dst_off[i] = pos + incl - bytes; hdr[i] = h; }
        const uint32_t tlo = zlz4::rdlane((uint32_t)incl, 63), thi = zlz4::rdlane((uint32_t)(incl >> 32), 63);
        pos += ((uint64_t)thi << 32) | tlo;
    }
    if (lane == 0) { plan[0] = (int64_t)pos; plan[1] = bad; plan[2] = bad_code; }
}

// one lane per block: XXH32 of the bytes that will be stored for the block (:422-427)
__global__ void k_block_xxh32(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                              const uint8_t *__restrict__ slots, const uint64_t *__restrict__ slot_off,
                              const uint32_t *__restrict__ hdr, uint32_t nblocks, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblocks) return;
    const BlockWord w = block_word(hdr[i]);
    out[i] = xxh32(w.stored ? src + src_off[i] : slots + slot_off[i], w.size, 0);
}

// one workgroup per block: header word, payload (compressed slot or raw source), optional checksum
__device__ __forceinline__ void scatter_block(uint32_t i, const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                              const uint8_t *__restrict__ slots, const uint64_t *__restrict__ slot_off,
                                              uint32_t h, const uint64_t *__restrict__ dst_off,
                                              const uint32_t *__restrict__ cks, uint32_t block_checksum,
                                              uint8_t *__restrict__ dst) {
    const uint32_t t = threadIdx.x;
    const BlockWord w = block_word(h);
    const uint32_t n = w.size;
    const uint8_t *p = w.stored ? src + src_off[i] : slots + slot_off[i];
    uint8_t *o = dst + dst_off[i];
    if (t < 4) o[t] = (uint8_t)(h >> (8u * t));                                   // :418
    o += 4;
    for (uint32_t k = t * 16u; k + 16u <= n; k += 256u * 16u) zlz4::st128(o + k, zlz4::ld128(p + k));
    const uint32_t t0 = n & ~15u;
    if (t < 16u && t0 + t < n) o[t0 + t] = p[t0 + t];
    if (block_checksum && t < 4) o[n + t] = (uint8_t)(cks[i] >> (8u * t));        // :425
}

__global__ __launch_bounds__(256) void k_frame_scatter(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                        const uint8_t *__restrict__ slots,
                                                        const uint64_t *__restrict__ slot_off,
                                                        const uint32_t *__restrict__ hdr,
                                                        const uint64_t *__restrict__ dst_off,
                                                        const uint32_t *__restrict__ cks, uint32_t block_checksum,
                                                        uint8_t *__restrict__ dst) {
    scatter_block(blockIdx.x, src, src_off, slots, slot_off, hdr[blockIdx.x], dst_off, cks, block_checksum, dst);
}

// one lane: frame header at dst[0..) (hb.n = 0: none), then -- for the segment that ends the frame -- the end mark and the
// optional content checksum at dst[plan[0]..)
__global__ void k_frame_head_tail(HeaderBytes hb, uint8_t *dst, const int64_t *plan, const uint8_t *src, uint64_t n,
                                  uint32_t tail, uint32_t content_checksum, int64_t *total_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (uint32_t k = 0; k < hb.n; k++) dst[k] = hb.b[k];
    uint64_t pos = (uint64_t)plan[0];
    if (tail) {
        for (int k = 0; k < 4; k++) dst[pos + k] = 0;                             // :433
        pos += 4;
        if (content_checksum) {
            const uint32_t c = xxh32(src, n, 0);                                  // :384-386, :437-441
            for (int k = 0; k < 4; k++) dst[pos + k] = (uint8_t)(c >> (8 * k));
            pos += 4;
        }
    }
    *total_out = (int64_t)pos;
}

// ------------------------------------------------------------------ decompress-side kernels
// walk[0] = number of data blocks, walk[1] = srcPos after the walk, walk[2] = pending error code (0 = none),
// walk[3] = header size or header error, walk[4] = FLG byte, walk[5] = block size
// The walk of src/lz4f.zig:563-600 without the payload work: block k's header position depends on all earlier block
// sizes, so this is a serial chain of 4-byte reads (one lane).  The frame header is parsed here too (:547), so that
// the host needs one read-back for header, block count and walk status.  Blocks beyond `max_blocks` are counted, not
// recorded (the caller then repeats the walk with a larger table).
// seg: bit 0 = the bytes start with a frame header; otherwise flg_in / bs_in describe the frame (a later rank's segment)
__global__ void k_frame_walk(const uint8_t *__restrict__ src, uint64_t src_len, uint32_t seg, uint32_t flg_in, uint64_t bs_in,
                             uint64_t *__restrict__ data_off, uint32_t *__restrict__ data_len,
                             uint32_t *__restrict__ flags, uint64_t *__restrict__ cks_off, uint64_t max_blocks,
                             int64_t *__restrict__ walk) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t src_pos = 0;
    uint32_t flg = flg_in;
    uint64_t bs = bs_in;
    walk[0] = 0; walk[1] = 0; walk[2] = 0; walk[3] = 0;
    if (seg & 1u) {
        const ParsedHeader ph = frame_header(src, src_len);                             // :547
        walk[3] = ph.size;
        if (ph.size < 0) { walk[4] = 0; walk[5] = 0; return; }
        src_pos = (uint64_t)ph.size;
        flg = ph.flg;
        bs = ph.block_size;
    }
    walk[4] = flg; walk[5] = (int64_t)bs;
    uint64_t nb;
    const bool bc = (flg & 0x10u) != 0;
    const ChainEnd end = chain_walk(src, src_len, bc, src_pos, ~0ull, nb, [&](uint64_t k, const ChainBlock &c) {
        if (k >= max_blocks) return;
        data_off[k] = c.off; data_len[k] = c.size; flags[k] = c.flags & (kBlkStored | kBlkNoCks); cks_off[k] = c.cks_off;
    });
    walk[0] = (int64_t)nb; walk[1] = (int64_t)src_pos; walk[2] = chain_error(end);
}

// one lane per block: verify the stored XXH32 of the block payload (:594-598); ok[i] = 1 / 0
__global__ void k_block_verify(const uint8_t *__restrict__ src, const uint64_t *__restrict__ data_off,
                               const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags,
                               const uint64_t *__restrict__ cks_off, uint32_t nblocks, uint32_t *__restrict__ ok) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblocks) return;
    if (flags[i] & 2u) { ok[i] = 2; return; }
    ok[i] = xxh32(src + data_off[i], data_len[i], 0) == zx_rd32(src + cks_off[i]) ? 1u : 0u;
}

// Serial dstPos accumulation of :602-621 with the reference's error order; one lane.
// dplan[0] = total output bytes, dplan[1] = error code (0 = none)
__global__ void k_dframe_plan(const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags,
                              const int64_t *__restrict__ sizes, const uint32_t *__restrict__ cks_ok,
                              uint32_t block_checksum, uint32_t nblocks, uint64_t dst_cap, int64_t walk_err,
                              uint64_t *__restrict__ out_off, uint32_t *__restrict__ out_cap, int64_t *__restrict__ dplan) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t pos = 0;
    int64_t err = 0;
    for (uint32_t i = 0; i < nblocks; i++) {
        if (block_checksum) {
            if (cks_ok[i] == 2u) { err = ZLZ4F_ERR_FRAME_SIZE_WRONG; break; }         // :591
            if (cks_ok[i] == 0u) { err = ZLZ4F_ERR_BLOCK_CHECKSUM_INVALID; break; }   // :596
        }
        const uint64_t rem = dst_cap - pos;
        uint64_t sz;
        if (flags[i] & 1u) {                                          // stored block :603-608
            sz = data_len[i];
            if (pos + sz > dst_cap) { err = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL; break; }
        } else {                                                      // :610 decompressSafe(blockData, dst[dstPos..])
            if (data_len[i] == 0 || rem == 0) sz = 0;                 // src/lz4.zig:97-98
            else {
                const int64_t s = sizes[i];
                if (s < 0 || (uint64_t)s > rem) { err = ZLZ4F_ERR_DECOMPRESSION_FAILED; break; }   // :611
                sz = (uint64_t)s;
            }
        }
        out_off[i] = pos;
        out_cap[i] = (uint32_t)sz;      // exact: the block decoders may chunk-write up to their capacity, never beyond
        pos += sz;
    }
    if (!err) err = walk_err;
    dplan[0] = (int64_t)pos; dplan[1] = err;
}

// Speculative layout: every frame compressFrame writes has blocks that decode to exactly block_size bytes, except the
// last one (:372-381), so block i can be decoded straight into dst + i * block_size with an exact capacity, without the
// size pass.  k_dframe_check then proves the guess from the decoder's results; any deviation (a foreign frame with
// short blocks, an error of any kind, a destination that is too small) sends the call to the exact two-pass plan.
__global__ void k_dframe_spec(const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags, uint32_t nblocks,
                              uint64_t bs, uint64_t dst_cap, uint64_t *__restrict__ out_off, uint32_t *__restrict__ out_cap,
                              uint32_t *__restrict__ dec_len) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nblocks; i += gridDim.x * blockDim.x) {
        const uint64_t o = (uint64_t)i * bs;
        out_off[i] = o < dst_cap ? o : dst_cap;
        out_cap[i] = o >= dst_cap ? 0u : (uint32_t)((dst_cap - o) < bs ? (dst_cap - o) : bs);
        dec_len[i] = (flags[i] & 1u) ? 0u : data_len[i];
    }
}

// dplan[0] = total output bytes, dplan[1] = error (stays 0 here), dplan[2] = 1 if the speculative layout is proven
__global__ __launch_bounds__(64) void k_dframe_check(const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags,
                                                     const int64_t *__restrict__ sizes, const uint32_t *__restrict__ cks_ok,
                                                     const uint32_t *__restrict__ out_cap, uint32_t block_checksum,
                                                     uint32_t nblocks, uint64_t bs, const int64_t *__restrict__ walk,
                                                     int64_t *__restrict__ dplan) {
    const uint32_t lane = threadIdx.x;
    bool ok = walk[2] == 0;
    uint64_t last = 0;
    for (uint32_t i = lane; i < nblocks; i += 64u) {
        if (block_checksum && cks_ok[i] != 1u) ok = false;
        uint64_t sz;
        if (flags[i] & 1u) { sz = data_len[i]; if (sz > out_cap[i]) ok = false; }
        else { const int64_t r = sizes[i]; if (r < 0 || data_len[i] == 0) ok = false; sz = r < 0 ? 0 : (uint64_t)r; }
        if (i + 1u < nblocks) { if (sz != bs) ok = false; }
        else last = sz;
    }
    const bool all_ok = zlz4::ballot(!ok) == 0;
    const uint32_t owner = nblocks ? (nblocks - 1u) & 63u : 0u;      // the lane that saw the last block
    const uint64_t last_sz = ((uint64_t)zlz4::rdlane((uint32_t)(last >> 32), owner) << 32) | zlz4::rdlane((uint32_t)last, owner);
    if (lane == 0) {
        dplan[0] = nblocks ? (int64_t)((uint64_t)(nblocks - 1u) * bs + last_sz) : 0;
        dplan[1] = 0;
        dplan[2] = all_ok ? 1 : 0;
    }
}

// one workgroup per block: raw copy of stored blocks (:607); compressed blocks are skipped here
__global__ __launch_bounds__(256) void k_copy_stored(const uint8_t *__restrict__ src, const uint64_t *__restrict__ data_off,
                                                      const uint32_t *__restrict__ data_len,
                                                      const uint32_t *__restrict__ flags,
                                                      const uint64_t *__restrict__ out_off, uint8_t *__restrict__ dst,
                                                      uint64_t dst_cap) {
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    if (!(flags[i] & 1u)) return;
    const uint32_t n = data_len[i];
    if (out_off[i] + n > dst_cap) return;               // (speculative layout: the check kernel reports it)
    const uint8_t *p = src + data_off[i];
    uint8_t *o = dst + out_off[i];
    for (uint32_t k = t * 16u; k + 16u <= n; k += 256u * 16u) zlz4::st128(o + k, zlz4::ld128(p + k));
    const uint32_t t0 = n & ~15u;
    if (t < 16u && t0 + t < n) o[t0 + t] = p[t0 + t];
}

// for the decoder batch call stored blocks become empty inputs (decoded size 0, nothing written)
__global__ void k_mask_stored(uint32_t *data_len_for_decode, const uint32_t *data_len, const uint32_t *flags,
                              uint32_t nblocks, uint64_t *zero_off, uint32_t *big_cap) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nblocks; i += gridDim.x * blockDim.x) {
        data_len_for_decode[i] = (flags[i] & 1u) ? 0u : data_len[i];
        if (zero_off) { zero_off[i] = 0; big_cap[i] = 0xFFFFFFFFu; }
    }
}

// content checksum over dst[0, total) with total read from the device (total_p[0]); only when no error is pending,
// and -- on the speculative path (need_proven) -- only when the layout guess has been proven: an unproven total can
// be anything a corrupted frame says (and XXH32 of gigabytes on one lane takes seconds)
__global__ void k_content_check(const uint8_t *dst, const int64_t *total_p, const uint8_t *stored, int64_t *dplan,
                                uint32_t need_proven, uint64_t dst_cap) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (dplan[1] != 0) return;
    if (need_proven && dplan[2] != 1) return;
    const uint64_t total = (uint64_t)total_p[0];
    if (total > dst_cap) return;
    if (xxh32(dst, total, 0) != zx_rd32(stored)) dplan[1] = ZLZ4F_ERR_CONTENT_CHECKSUM_INVALID;   // :631
}

__host__ __device__ inline int64_t map_block_error(int64_t e) {     // mapCompressionError, src/lz4f.zig:144-149
    if (e == ZLZ4_ERR_OUTPUT_TOO_SMALL) return ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
    if (e == ZLZ4_ERR_UNSUPPORTED || e == ZLZ4_ERR_DEVICE) return e;
    return ZLZ4F_ERR_GENERIC;
}

}  // namespace

extern "C" {

size_t zlz4f_compress_frame_bound(size_t src_size, const zlz4f_prefs *prefs) {   // src/lz4f.zig:274-301
    const zlz4f_prefs *p = prefs ? prefs : &kDefaultPrefs;
    const size_t block_size = block_size_of(p->block_size_id);
    const size_t num_blocks = (src_size + block_size - 1) / block_size;
    size_t per_block = 4 + zlz4_compress_bound(block_size);
    if (p->block_checksum == 1) per_block += 4;
    size_t result = 19 + num_blocks * per_block + 4;
    if (p->content_checksum == 1) result += 4;
    return result;
}

int64_t zlz4f_header_size(const uint8_t *src, size_t n) {   // src/lz4f.zig:451-480
    if (n < 5) return ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE;
    uint32_t magic;
    std::memcpy(&magic, src, 4);
    if (magic != ZLZ4F_MAGICNUMBER) {
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) return 8;
        return ZLZ4F_ERR_FRAME_TYPE_UNKNOWN;
    }
    const uint8_t flg = src[4];
    int64_t size = 7;
    if (flg & 0x08) size += 8;
    if (flg & 0x01) size += 4;
    return size;
}

}  // extern "C"

namespace {

constexpr uint32_t kSegFirst = 1u, kSegLast = 2u;

// src/lz4f.zig:354-446 on a device-resident source.  seg: kSegFirst = write the frame header (:369), kSegLast = write the
// end mark (:433) and the content checksum (:437-441); a whole frame has both.
int64_t compress_frame_impl(hipStream_t st, const uint8_t *d_src, size_t n, uint8_t *d_dst, size_t cap, const zlz4f_prefs &p,
                            uint32_t seg) {
    if (cap < zlz4f_compress_frame_bound(n, &p)) return ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;   // :363-366
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    HeaderBytes hb = encode_header(p);                                                     // :369
    if (!(seg & kSegFirst)) hb.n = 0;
    const size_t bs = block_size_of(p.block_size_id);                                      // :372
    const uint64_t nb64 = (n + bs - 1) / bs;
    if (nb64 > 0x7FFFFFFFull) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    const uint32_t nb = (uint32_t)nb64;
    // level routing :393-404; compressHC then normalises <2 -> 9, >12 -> 12 (src/lz4hc.zig:1445)
    int32_t hc_level = 0;
    if (p.compression_level > 0) {
        hc_level = p.compression_level < 2 ? 9 : (p.compression_level > 12 ? 12 : p.compression_level);
    }
    const uint32_t tail = (seg & kSegLast) ? 1u : 0u;
    const uint32_t content_checksum = (tail && p.content_checksum == 1) ? 1u : 0u;
    const uint64_t slot = (zlz4_compress_bound(bs) + 15) & ~15ull;
    DeviceCall fc(st);
    DevBuf d_plan(4 * sizeof(int64_t), &fc);
    if (!d_plan.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    int64_t total = 0;
    if (nb == 0) {
        int64_t plan0[3] = {(int64_t)hb.n, 0, 0};
        if (hipMemcpyAsync(d_plan.p, plan0, sizeof plan0, hipMemcpyHostToDevice, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
        fc.launched();
        hipLaunchKernelGGL(k_frame_head_tail, dim3(1), dim3(64), 0, st, hb, d_dst, d_plan.as<int64_t>(), d_src,
                           (uint64_t)n, tail, content_checksum, d_plan.as<int64_t>() + 3);
        if (hipMemcpyAsync(&total, d_plan.as<int64_t>() + 3, 8, hipMemcpyDeviceToHost, st) != hipSuccess || !fc.sync())
            return ZLZ4_ERR_DEVICE;
        return total;
    }
    DevBuf d_slots((uint64_t)nb * slot, &fc), d_u64((uint64_t)nb * 3 * sizeof(uint64_t), &fc),
        d_u32((uint64_t)nb * 4 * sizeof(uint32_t), &fc), d_res((uint64_t)nb * sizeof(int64_t), &fc);
    if (!d_slots.p || !d_u64.p || !d_u32.p || !d_res.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    const size_t wsb = hc_level ? zlz4_hc_workspace_bytes(nb, (uint32_t)bs) : 0;
    DevBuf d_ws(wsb, &fc);
    if (hc_level && !d_ws.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    uint64_t *in_off = d_u64.as<uint64_t>(), *out_off = in_off + nb, *dst_off = out_off + nb;
    uint32_t *in_len = d_u32.as<uint32_t>(), *out_cap = in_len + nb, *hdr = out_cap + nb, *cks = hdr + nb;
    fc.launched();
    hipLaunchKernelGGL(k_frame_desc, dim3((nb + 255) / 256 > 1024 ? 1024 : (nb + 255) / 256), dim3(256), 0, st, (uint64_t)n,
                       (uint64_t)bs, slot, nb, in_off, in_len, out_off, out_cap);
    int rc;
    if (hc_level == 0) {
        rc = zlz4_launch_compress_fast(st, d_src, in_off, in_len, d_slots.as<uint8_t>(), out_off, out_cap,
                                       d_res.as<int64_t>(), nb, (uint32_t)bs, 1);                        // :400-404
    } else {
        rc = zlz4_launch_compress_hc(st, d_src, in_off, in_len, d_slots.as<uint8_t>(), out_off, out_cap,
                                     d_res.as<int64_t>(), nb, (uint32_t)bs, hc_level, d_ws.p, wsb);      // :394-398
    }
    if (rc != 0) return rc;
    hipLaunchKernelGGL(k_frame_plan, dim3(1), dim3(64), 0, st, d_res.as<int64_t>(), in_len, nb,
                       p.block_checksum == 1 ? 1u : 0u, (uint64_t)hb.n, dst_off, hdr, d_plan.as<int64_t>());
    if (p.block_checksum == 1)
        hipLaunchKernelGGL(k_block_xxh32, dim3((nb + 63) / 64), dim3(64), 0, st, d_src, in_off, d_slots.as<uint8_t>(),
                           out_off, hdr, nb, cks);
    hipLaunchKernelGGL(k_frame_scatter, dim3(nb), dim3(256), 0, st, d_src, in_off, d_slots.as<uint8_t>(), out_off, hdr,
                       dst_off, cks, p.block_checksum == 1 ? 1u : 0u, d_dst);
    hipLaunchKernelGGL(k_frame_head_tail, dim3(1), dim3(64), 0, st, hb, d_dst, d_plan.as<int64_t>(), d_src, (uint64_t)n,
                       tail, content_checksum, d_plan.as<int64_t>() + 3);
    int64_t plan[4];
    if (hipMemcpyAsync(plan, d_plan.p, sizeof plan, hipMemcpyDeviceToHost, st) != hipSuccess || !fc.sync() ||
        hipGetLastError() != hipSuccess)
        return ZLZ4_ERR_DEVICE;
    if (plan[1] != 0) return map_block_error(plan[2]);                                                   // :398, :404
    return plan[3];
}

// src/lz4f.zig:541-638 on device-resident bytes.  seg & kSegFirst: the bytes start with the frame header (:547), else
// `p` describes the frame (block checksum flag, block size).  A whole frame has kSegFirst | kSegLast; without kSegLast
// the bytes are expected to end after a block (no end mark, no content checksum).
int64_t decompress_frame_impl(hipStream_t st, const uint8_t *d_src, size_t n, uint8_t *d_dst, size_t cap, const zlz4f_prefs &p,
                              uint32_t seg) {
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    DeviceCall fc(st);
    DevBuf d_walk(12 * sizeof(int64_t), &fc);
    if (!d_walk.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    int64_t *walk = d_walk.as<int64_t>(), *dplan = walk + 8;
    const uint32_t flg_in = 0x40u | (p.block_mode == 1 ? 0x20u : 0u) | (p.block_checksum == 1 ? 0x10u : 0u);
    const uint64_t bs_in = block_size_of(p.block_size_id);
    // the block table is sized for the blocks a frame of this length usually has; a frame of tiny blocks repeats the walk
    uint64_t table_cap = n / 1024 + 64;
    if (table_cap > n / 5 + 1) table_cap = n / 5 + 1;
    int64_t w[6];
    for (int attempt = 0;; attempt++) {
        DevBuf d_u64(table_cap * 3 * sizeof(uint64_t), &fc), d_u32(table_cap * 5 * sizeof(uint32_t), &fc),
            d_sz(table_cap * sizeof(int64_t), &fc);
        if (!d_u64.p || !d_u32.p || !d_sz.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
        uint64_t *data_off = d_u64.as<uint64_t>(), *cks_off = data_off + table_cap, *out_off = cks_off + table_cap;
        uint32_t *data_len = d_u32.as<uint32_t>(), *flags = data_len + table_cap, *cks_ok = flags + table_cap,
                 *out_cap = cks_ok + table_cap, *dec_len = out_cap + table_cap;
        fc.launched();
        hipLaunchKernelGGL(k_frame_walk, dim3(1), dim3(64), 0, st, d_src, (uint64_t)n, seg, flg_in, bs_in, data_off, data_len,
                           flags, cks_off, table_cap, walk);
        if (hipMemcpyAsync(w, walk, sizeof w, hipMemcpyDeviceToHost, st) != hipSuccess || !fc.sync()) return ZLZ4_ERR_DEVICE;
        if (w[3] < 0) return w[3];                                                                       // header error :547
        if (w[0] > 0x7FFFFFFFll) return ZLZ4F_ERR_FRAME_SIZE_WRONG;
        if ((uint64_t)w[0] > table_cap) {
            if (attempt) return ZLZ4_ERR_DEVICE;
            table_cap = (uint64_t)w[0];
            continue;
        }
        const uint32_t nb = (uint32_t)w[0];
        const uint64_t src_pos_end = (uint64_t)w[1];
        const int64_t walk_err = w[2];
        const uint32_t flg = (uint32_t)w[4];
        const uint64_t bs = (uint64_t)w[5];
        const uint32_t bc = (flg & 0x10) ? 1u : 0u, cc = ((seg & kSegLast) && (flg & 0x04)) ? 1u : 0u;
        int64_t plan_host[3] = {0, walk_err, 0};
        int64_t tot[2] = {0, 0};          // host source of an async copy: lives until the call's last synchronisation
        const uint32_t gridb = (nb + 255) / 256 > 1024 ? 1024 : (nb + 255) / 256;
        if (nb) {
            // speculative single pass: block i -> dst + i * block_size, proven afterwards
            fc.launched();
            if (bc) hipLaunchKernelGGL(k_block_verify, dim3((nb + 63) / 64), dim3(64), 0, st, d_src, data_off, data_len, flags,
                                       cks_off, nb, cks_ok);
            hipLaunchKernelGGL(k_dframe_spec, dim3(gridb), dim3(256), 0, st, data_len, flags, nb, bs, (uint64_t)cap, out_off,
                               out_cap, dec_len);
            int rc = zlz4_launch_decompress_safe(st, d_src, data_off, dec_len, d_dst, out_off, out_cap, d_sz.as<int64_t>(), nb);
            if (rc != 0) return rc;
            hipLaunchKernelGGL(k_copy_stored, dim3(nb), dim3(256), 0, st, d_src, data_off, data_len, flags, out_off, d_dst,
                               (uint64_t)cap);
            hipLaunchKernelGGL(k_dframe_check, dim3(1), dim3(64), 0, st, data_len, flags, d_sz.as<int64_t>(), cks_ok, out_cap, bc,
                               nb, bs, walk, dplan);
            if (cc && src_pos_end + 4 <= n)     // only meaningful when the guess holds; checked below
                hipLaunchKernelGGL(k_content_check, dim3(1), dim3(64), 0, st, d_dst, dplan, d_src + src_pos_end, dplan, 1u,
                                   (uint64_t)cap);
            if (hipMemcpyAsync(plan_host, dplan, sizeof plan_host, hipMemcpyDeviceToHost, st) != hipSuccess || !fc.sync())
                return ZLZ4_ERR_DEVICE;
            if (plan_host[2] == 1) {
                if (cc && src_pos_end + 4 > n) return ZLZ4F_ERR_FRAME_SIZE_WRONG;                        // :626
                if (hipGetLastError() != hipSuccess) return ZLZ4_ERR_DEVICE;
                return plan_host[1] != 0 ? plan_host[1] : plan_host[0];
            }
            // exact plan: size pass (unlimited capacity), the serial dstPos accumulation with the reference's error
            // order (:602-621), then decode + raw copies at the exact places
            DevBuf d_x64((uint64_t)nb * sizeof(uint64_t), &fc), d_x32((uint64_t)nb * sizeof(uint32_t), &fc);
            if (!d_x64.p || !d_x32.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
            uint64_t *zero_off = d_x64.as<uint64_t>();
            uint32_t *big_cap = d_x32.as<uint32_t>();
            fc.launched();
            hipLaunchKernelGGL(k_mask_stored, dim3(gridb), dim3(256), 0, st, dec_len, data_len, flags, nb, zero_off, big_cap);
            rc = zlz4_launch_decompress_sizes(st, d_src, data_off, dec_len, zero_off, big_cap, d_sz.as<int64_t>(), nb);
            if (rc != 0) return rc;
            hipLaunchKernelGGL(k_dframe_plan, dim3(1), dim3(64), 0, st, data_len, flags, d_sz.as<int64_t>(), cks_ok, bc, nb,
                               (uint64_t)cap, walk_err, out_off, out_cap, dplan);
            if (hipMemcpyAsync(plan_host, dplan, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess || !fc.sync())
                return ZLZ4_ERR_DEVICE;
            if (plan_host[1] != 0) return plan_host[1];
            fc.launched();
            rc = zlz4_launch_decompress_safe(st, d_src, data_off, dec_len, d_dst, out_off, out_cap, d_sz.as<int64_t>(), nb);
            if (rc != 0) return rc;
            hipLaunchKernelGGL(k_copy_stored, dim3(nb), dim3(256), 0, st, d_src, data_off, data_len, flags, out_off, d_dst,
                               (uint64_t)cap);
        } else if (walk_err != 0) {
            return walk_err;
        }
        if (cc) {                                                                                        // :625-635
            if (src_pos_end + 4 > n) { (void)fc.sync(); return ZLZ4F_ERR_FRAME_SIZE_WRONG; }
            tot[0] = plan_host[0];
            if (hipMemcpyAsync(dplan, tot, sizeof tot, hipMemcpyHostToDevice, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
            fc.launched();
            hipLaunchKernelGGL(k_content_check, dim3(1), dim3(64), 0, st, d_dst, dplan, d_src + src_pos_end, dplan, 0u,
                               (uint64_t)cap);
            if (hipMemcpyAsync(plan_host, dplan, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
        }
        if (!fc.sync() || hipGetLastError() != hipSuccess) return ZLZ4_ERR_DEVICE;
        if (plan_host[1] != 0) return plan_host[1];
        return plan_host[0];
    }
}

// The host-pointer frame calls: stage src, run device_call(d_src, d_dst) into a device destination of d_cap bytes, copy
// the first `result` bytes back.  A result <= 0 leaves dst unwritten.
template <typename Call>
int64_t host_frame_call(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t d_cap, Call device_call) {
    DevBuf d_src(n), d_dst(d_cap);
    if (!d_src.p || !d_dst.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    if (n && hipMemcpy(d_src.p, src, n, hipMemcpyHostToDevice) != hipSuccess) return ZLZ4_ERR_DEVICE;
    const int64_t r = device_call(d_src.as<uint8_t>(), d_dst.as<uint8_t>());
    if (!copy_back(dst, cap, d_dst, r)) return ZLZ4_ERR_DEVICE;
    return r;
}

}  // namespace

extern "C" {

int64_t zlz4f_compress_frame_device(void *stream_, const uint8_t *d_src, size_t n, uint8_t *d_dst, size_t cap,
                                    const zlz4f_prefs *prefs) {
    return compress_frame_impl((hipStream_t)stream_, d_src, n, d_dst, cap, prefs ? *prefs : kDefaultPrefs, kSegFirst | kSegLast);
}

// One rank's part of a frame whose blocks are spread over several GPUs (the block loop :379-430 carries no state)
int64_t zlz4f_compress_frame_segment_device(void *stream_, const uint8_t *d_src, size_t n, uint8_t *d_dst, size_t cap,
                                            const zlz4f_prefs *prefs, uint32_t segment_flags) {
    const zlz4f_prefs p = prefs ? *prefs : kDefaultPrefs;
    if (segment_flags & ~(kSegFirst | kSegLast)) return ZLZ4F_ERR_PARAMETER_INVALID;
    // XXH32 of the whole content is one serial chain over every rank's bytes: not available for a split frame
    if (p.content_checksum == 1 && segment_flags != (kSegFirst | kSegLast)) return ZLZ4_ERR_UNSUPPORTED;
    const size_t bs = block_size_of(p.block_size_id);
    if (!(segment_flags & kSegLast) && n % bs != 0) return ZLZ4F_ERR_PARAMETER_INVALID;   // only the last block may be short
    return compress_frame_impl((hipStream_t)stream_, d_src, n, d_dst, cap, p, segment_flags);
}

int64_t zlz4f_decompress_frame_device(void *stream_, const uint8_t *d_src, size_t n, uint8_t *d_dst, size_t cap) {
    return decompress_frame_impl((hipStream_t)stream_, d_src, n, d_dst, cap, kDefaultPrefs, kSegFirst | kSegLast);
}

int64_t zlz4f_decompress_frame_segment_device(void *stream_, const uint8_t *d_src, size_t n, uint8_t *d_dst, size_t cap,
                                              const zlz4f_prefs *prefs, uint32_t segment_flags) {
    const zlz4f_prefs p = prefs ? *prefs : kDefaultPrefs;
    if (segment_flags & ~(kSegFirst | kSegLast)) return ZLZ4F_ERR_PARAMETER_INVALID;
    if (p.content_checksum == 1 && segment_flags != (kSegFirst | kSegLast)) return ZLZ4_ERR_UNSUPPORTED;
    return decompress_frame_impl((hipStream_t)stream_, d_src, n, d_dst, cap, p, segment_flags);
}

// src/lz4f.zig:354-446, host pointers: stage -> device path -> copy the frame back
int64_t zlz4f_compress_frame(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const zlz4f_prefs *prefs) {
    const zlz4f_prefs p = prefs ? *prefs : kDefaultPrefs;
    const size_t bound = zlz4f_compress_frame_bound(n, &p);
    if (cap < bound) return ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;                                            // :363-366
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return host_frame_call(src, n, dst, cap, bound, [&](const uint8_t *d_src, uint8_t *d_dst) {
        return zlz4f_compress_frame_device(nullptr, d_src, n, d_dst, bound, &p);
    });
}

// src/lz4f.zig:541-638, host pointers
int64_t zlz4f_decompress_frame(const uint8_t *src, size_t n, uint8_t *dst, size_t cap) {
    const ParsedHeader ph = parse_header(src, n);      // header errors need no device
    if (ph.size < 0) return ph.size;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return host_frame_call(src, n, dst, cap, cap, [&](const uint8_t *d_src, uint8_t *d_dst) {
        return zlz4f_decompress_frame_device(nullptr, d_src, n, d_dst, cap);
    });
}

}  // extern "C"

// ====================================================================== batch frames: N independent frames per call
// zlz4f_batch_compress_frame / zlz4f_batch_decompress_frame (include/zlz4_amd.h).  Frame f's
// result is what compress_frame_impl / decompress_frame_impl return for it, but the whole batch is one fixed sequence of
// kernels on the caller's stream: no allocation, no read-back, no synchronisation (so it can be captured into a graph).
// The per-block work of every frame shares one block table of `max_blocks` entries: frame f owns the entries
// [base_f, base_f + nb_f), base = the exclusive scan of the block counts in frame order.  A frame with blocks whose range
// does not end at or below max_blocks gets ZLZ4_ERR_INVALID_STATE; every entry it would have owned, and every entry past
// the last block, has length 0.  Per-frame serial steps (header, chain walk, dstPos plan, XXH32 of the content) run one
// lane per frame; the block steps (compression, decoding, block checksums, copies) one entry per lane / wave / workgroup.
namespace {

// exclusive scan of fr[].nb into fr[].base: one workgroup, thread t sums a contiguous run of frames, the 1024 run sums are
// scanned in LDS, then every thread writes its run's bases
__global__ __launch_bounds__(1024) void k_bf_scan(BFrame *__restrict__ fr, uint32_t nframes) {
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

// ------------------------------------------------------------------ compress
// one lane per frame: block count and the frame's capacity check (compress_frame_impl's order: :363-366 first)
__global__ void k_bfc_count(const uint64_t *__restrict__ src_len, const uint64_t *__restrict__ dst_cap, uint32_t nframes,
                            uint64_t bs, uint64_t per_block, uint64_t fixed, BFrame *__restrict__ fr) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const uint64_t n = src_len[f];
    const uint64_t nb = n / bs + (n % bs != 0);
    BFrame F = {};
    F.nb = nb;
    F.status = dst_cap[f] < fixed + nb * per_block ? ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL
                                                    : (nb > 0x7FFFFFFFull ? ZLZ4F_ERR_SRC_SIZE_TOO_LARGE : 0);
    fr[f] = F;
}

// one lane per table entry: its frame (the last frame whose base is <= i: frames without blocks share the next frame's
// base), the block's source range and its workspace slot.  Entries of failed frames and unused entries get length 0.
__global__ void k_bfc_desc(const BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                           const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ src_len, uint64_t bs,
                           uint64_t slot, uint64_t *__restrict__ in_off, uint32_t *__restrict__ in_len,
                           uint64_t *__restrict__ out_off, uint32_t *__restrict__ out_cap, uint32_t *__restrict__ hdr) {
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
            const BFrame F = fr[f];
            const uint64_t k = i - F.base;
            if (k < F.nb && F.status == 0 && bf_fits(F, max_blocks)) {
                const uint64_t n = src_len[f], b = k * bs;
                len = (uint32_t)((n - b) < bs ? (n - b) : bs);
                o = src_off[f] + b;
            }
        }
        in_off[i] = o;
        in_len[i] = len;
        out_off[i] = (uint64_t)i * slot;
        out_cap[i] = (uint32_t)slot;
        hdr[i] = 0;
    }
}

__device__ __forceinline__ uint32_t bf_header_size(const zlz4f_prefs &p, uint64_t content_size) {   // :304-351
    return 7u + (content_size != 0 ? 8u : 0u) + (p.dict_id != 0 ? 4u : 0u);
}

// one wavefront per frame: k_frame_plan over the frame's entries, offsets absolute in dst; F.end = frame bytes in front
// of the end mark, F.err = the first failing block's code
__global__ __launch_bounds__(256) void k_bfc_plan(BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                                                  const int64_t *__restrict__ csize, const uint32_t *__restrict__ in_len,
                                                  uint32_t block_checksum, zlz4f_prefs p, uint32_t cs_from_len,
                                                  const uint64_t *__restrict__ src_len, const uint64_t *__restrict__ dst_off_f,
                                                  uint64_t *__restrict__ dst_off, uint32_t *__restrict__ hdr) {
    const uint32_t f = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (f >= nframes) return;
    const BFrame F = fr[f];
    if (F.status != 0 || F.nb == 0 || !bf_fits(F, max_blocks)) return;
    const uint32_t nb = (uint32_t)F.nb;
    const uint64_t start = bf_header_size(p, cs_from_len ? src_len[f] : p.content_size);
    uint64_t pos = dst_off_f[f] + start;
    uint32_t bad = 0;
    int64_t bad_code = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += 64u) {
        const uint32_t j = b0 + lane;
        const uint64_t i = F.base + j;
        uint64_t bytes = 0;
        uint32_t h = 0;
        bool err = false;
        int64_t c = 0;
        if (j < nb) {
            c = csize[i];
            const uint32_t len = in_len[i];
            err = c < 0;
            const bool stored = !err && (uint64_t)c >= len;           // :407
            const uint32_t actual = stored ? len : (uint32_t)(err ? 0 : c);
            h = actual | (stored ? 0x80000000u : 0u);                 // :411-414
            bytes = 4u + (uint64_t)actual + (block_checksum ? 4u : 0u);
        }
        const uint64_t em = zlz4::ballot(err);
        if (em && !bad) {
            const uint32_t l = zlz4::first_lane(em);
            bad = b0 + l + 1u;
            bad_code = (int64_t)(int32_t)zlz4::rdlane((uint32_t)c, l);
        }
        uint64_t incl = bytes;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t lo = __shfl_up((uint32_t)incl, d), hi = __shfl_up((uint32_t)(incl >> 32), d);
            if (lane >= d) incl += ((uint64_t)hi << 32) | lo;
        }
        if (j < nb) { dst_off[i] = pos + incl - bytes; hdr[i] = h; }
        const uint32_t tlo = zlz4::rdlane((uint32_t)incl, 63), thi = zlz4::rdlane((uint32_t)(incl >> 32), 63);
        pos += ((uint64_t)thi << 32) | tlo;
    }
    if (lane == 0) { fr[f].end = pos - dst_off_f[f]; fr[f].err = bad ? bad_code : 0; }
}

// one workgroup per entry; entries without a block (hdr 0: every real block has a non-empty payload) write nothing
__global__ __launch_bounds__(256) void k_bf_scatter(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                     const uint8_t *__restrict__ slots, const uint64_t *__restrict__ slot_off,
                                                     const uint32_t *__restrict__ hdr, const uint64_t *__restrict__ dst_off,
                                                     const uint32_t *__restrict__ cks, uint32_t block_checksum,
                                                     uint8_t *__restrict__ dst) {
    const uint32_t h = hdr[blockIdx.x];
    if (h == 0) return;
    scatter_block(blockIdx.x, src, src_off, slots, slot_off, h, dst_off, cks, block_checksum, dst);
}

// one lane per frame: the frame's status, or header (:369), end mark (:433), content checksum (:437-441) and its size
__global__ void k_bfc_head_tail(const BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks, zlz4f_prefs p,
                                uint32_t cs_from_len, const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                const uint64_t *__restrict__ src_len, uint8_t *__restrict__ dst,
                                const uint64_t *__restrict__ dst_off, int64_t *__restrict__ result) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const BFrame F = fr[f];
    if (F.status != 0) { result[f] = F.status; return; }
    if (!bf_fits(F, max_blocks)) { result[f] = ZLZ4_ERR_INVALID_STATE; return; }
    if (F.nb && F.err) { result[f] = map_block_error(F.err); return; }                   // :398, :404
    const uint64_t n = src_len[f];
    const HeaderBytes hb = encode_header_cs(p, cs_from_len ? n : p.content_size);
    uint8_t *o = dst + dst_off[f];
    for (uint32_t k = 0; k < hb.n; k++) o[k] = hb.b[k];
    uint64_t pos = F.nb ? F.end : hb.n;
    for (int k = 0; k < 4; k++) o[pos + k] = 0;
    pos += 4;
    if (p.content_checksum == 1) {
        const uint32_t c = xxh32(src + src_off[f], n, 0);
        for (int k = 0; k < 4; k++) o[pos + k] = (uint8_t)(c >> (8 * k));
        pos += 4;
    }
    result[f] = (int64_t)pos;
}

// ------------------------------------------------------------------ decompress
__global__ void k_bfd_init(uint32_t *__restrict__ data_len, uint32_t *__restrict__ flags, uint32_t *__restrict__ fidx,
                           uint32_t max_blocks) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        data_len[i] = 0; flags[i] = 0; fidx[i] = kNoFrame;
    }
}

// one lane per frame: the header parse (:547, frame_header) and the chain walk (:563-600, chain_walk) that k_frame_walk, the
// multiframe split and the host calls run too.  The first pass counts (kRecord false), the second records the blocks of
// every frame that fits the table at its base.
template <bool kRecord>
__global__ void k_bfd_walk(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                           const uint64_t *__restrict__ src_len, uint32_t nframes, uint32_t max_blocks,
                           BFrame *__restrict__ fr, uint64_t *__restrict__ data_off, uint32_t *__restrict__ data_len,
                           uint32_t *__restrict__ flags, uint64_t *__restrict__ cks_off, uint32_t *__restrict__ fidx) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const uint64_t so = src_off[f], n = src_len[f];
    const uint8_t *s = src + so;
    uint64_t pos, entry = 0;
    uint32_t flg;
    if (kRecord) {
        const BFrame F = fr[f];
        if (F.status < 0 || F.nb == 0 || !bf_fits(F, max_blocks)) return;
        pos = (uint64_t)F.status;
        flg = F.flg;
        entry = F.base;
    } else {
        const ParsedHeader ph = frame_header(s, n);
        BFrame F = {};
        F.status = ph.size;
        F.flg = ph.flg;
        F.bs = ph.block_size;
        if (ph.size < 0) { fr[f] = F; return; }
        fr[f] = F;
        pos = (uint64_t)ph.size;
        flg = ph.flg;
    }
    const uint64_t nb_max = kRecord ? fr[f].nb : ~0ull;               // (the record pass never leaves the frame's range)
    uint64_t nb;
    const ChainEnd end = chain_walk(s, n, (flg & 0x10u) != 0, pos, nb_max, nb, [&](uint64_t k, const ChainBlock &c) {
        if (!kRecord) return;
        const uint64_t i = entry + k;
        data_off[i] = so + c.off; data_len[i] = c.size; flags[i] = c.flags; cks_off[i] = so + c.cks_off; fidx[i] = f;
    });
    if (!kRecord) { fr[f].nb = nb; fr[f].end = pos; fr[f].err = chain_error(end); }
}

// one lane per entry of a frame whose FLG asks for block checksums: k_block_verify (:594-598)
__global__ void k_bfd_verify(const uint8_t *__restrict__ src, const uint64_t *__restrict__ data_off,
                             const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags,
                             const uint64_t *__restrict__ cks_off, uint32_t max_blocks, uint32_t *__restrict__ ok) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= max_blocks) return;
    const uint32_t fl = flags[i];
    if (fl & kBlkNoCks) { ok[i] = 2; return; }
    if (!(fl & kBlkCks)) return;
    ok[i] = xxh32(src + data_off[i], data_len[i], 0) == zx_rd32(src + cks_off[i]) ? 1u : 0u;
}

// k_dframe_spec per entry: block k of frame f -> dst_f + k * bs_f with the capacity left there (at most bs_f)
__global__ void k_bfd_spec(const BFrame *__restrict__ fr, const uint32_t *__restrict__ fidx,
                           const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags,
                           const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ dst_cap, uint32_t max_blocks,
                           uint64_t *__restrict__ out_off, uint32_t *__restrict__ out_cap, uint32_t *__restrict__ dec_len) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        const uint32_t f = fidx[i];
        if (f == kNoFrame) { out_off[i] = 0; out_cap[i] = 0; dec_len[i] = 0; continue; }
        const uint64_t bs = fr[f].bs, o = (i - fr[f].base) * bs, cap = dst_cap[f];
        out_off[i] = dst_off[f] + (o < cap ? o : cap);
        out_cap[i] = o >= cap ? 0u : (uint32_t)((cap - o) < bs ? (cap - o) : bs);
        dec_len[i] = (flags[i] & kBlkStored) ? 0u : data_len[i];
    }
}

// one workgroup per entry: raw copy of a stored block (:607) that fits its entry's capacity
__global__ __launch_bounds__(256) void k_bf_copy_stored(const uint8_t *__restrict__ src, const uint64_t *__restrict__ data_off,
                                                         const uint32_t *__restrict__ data_len,
                                                         const uint32_t *__restrict__ flags,
                                                         const uint64_t *__restrict__ out_off,
                                                         const uint32_t *__restrict__ out_cap, uint8_t *__restrict__ dst) {
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    if (!(flags[i] & kBlkStored)) return;
    const uint32_t n = data_len[i];
    if (n > out_cap[i]) return;                         // (speculative layout: the check kernel reports it)
    const uint8_t *p = src + data_off[i];
    uint8_t *o = dst + out_off[i];
    for (uint32_t k = t * 16u; k + 16u <= n; k += 256u * 16u) zlz4::st128(o + k, zlz4::ld128(p + k));
    const uint32_t t0 = n & ~15u;
    if (t < 16u && t0 + t < n) o[t0 + t] = p[t0 + t];
}

// one wavefront per frame: k_dframe_check over the frame's entries -> F.proven, F.total
__global__ __launch_bounds__(256) void k_bfd_check(BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                                                   const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags,
                                                   const int64_t *__restrict__ sizes, const uint32_t *__restrict__ cks_ok,
                                                   const uint32_t *__restrict__ out_cap) {
    const uint32_t f = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (f >= nframes) return;
    const BFrame F = fr[f];
    if (F.status < 0 || F.nb == 0 || !bf_fits(F, max_blocks)) return;
    const bool bc = (F.flg & 0x10u) != 0;
    bool ok = F.err == 0;
    uint64_t last = 0;
    for (uint64_t j = lane; j < F.nb; j += 64u) {
        const uint64_t i = F.base + j;
        if (bc && cks_ok[i] != 1u) ok = false;
        uint64_t sz;
        if (flags[i] & kBlkStored) { sz = data_len[i]; if (sz > out_cap[i]) ok = false; }
        else { const int64_t r = sizes[i]; if (r < 0 || data_len[i] == 0) ok = false; sz = r < 0 ? 0 : (uint64_t)r; }
        if (j + 1u < F.nb) { if (sz != F.bs) ok = false; }
        else last = sz;
    }
    const bool all_ok = zlz4::ballot(!ok) == 0;
    const uint32_t owner = (uint32_t)((F.nb - 1u) & 63u);
    const uint64_t last_sz = ((uint64_t)zlz4::rdlane((uint32_t)(last >> 32), owner) << 32) | zlz4::rdlane((uint32_t)last, owner);
    if (lane == 0) {
        fr[f].proven = all_ok ? 1u : 0u;
        fr[f].total = (F.nb - 1u) * F.bs + last_sz;
    }
}

// exact path, per entry: only the blocks of frames that fit the table and are not proven take part (stored blocks as
// empty inputs); everything else has length and capacity 0
__global__ void k_bfd_mask(const BFrame *__restrict__ fr, const uint32_t *__restrict__ fidx,
                           const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags, uint32_t max_blocks,
                           uint64_t *__restrict__ x_off, uint32_t *__restrict__ x_cap, uint32_t *__restrict__ x_len) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        const uint32_t f = fidx[i];
        const bool cand = f != kNoFrame && !fr[f].proven;
        x_len[i] = cand && !(flags[i] & kBlkStored) ? data_len[i] : 0u;
        x_off[i] = 0;
        x_cap[i] = cand ? 0xFFFFFFFFu : 0u;
    }
}

// exact path, one lane per unproven frame: k_dframe_plan (:602-621, the reference's error order) -> exact offsets and
// capacities; a frame with an error decodes nothing
__global__ void k_bfd_plan(BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                           const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags,
                           const int64_t *__restrict__ sizes, const uint32_t *__restrict__ cks_ok,
                           const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ dst_cap,
                           uint64_t *__restrict__ x_off, uint32_t *__restrict__ x_cap, uint32_t *__restrict__ x_len) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const BFrame F = fr[f];
    if (F.status < 0 || !bf_fits(F, max_blocks) || F.proven) return;
    const bool bc = (F.flg & 0x10u) != 0;
    const uint64_t cap = dst_cap[f];
    uint64_t pos = 0;
    int64_t err = 0;
    for (uint64_t j = 0; j < F.nb; j++) {
        const uint64_t i = F.base + j;
        if (bc) {
            if (cks_ok[i] == 2u) { err = ZLZ4F_ERR_FRAME_SIZE_WRONG; break; }          // :591
            if (cks_ok[i] == 0u) { err = ZLZ4F_ERR_BLOCK_CHECKSUM_INVALID; break; }    // :596
        }
        const uint64_t rem = cap - pos;
        uint64_t sz;
        if (flags[i] & kBlkStored) {                                  // stored block :603-608
            sz = data_len[i];
            if (pos + sz > cap) { err = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL; break; }
        } else {                                                      // :610
            if (data_len[i] == 0 || rem == 0) sz = 0;                 // src/lz4.zig:97-98
            else {
                const int64_t s = sizes[i];
                if (s < 0 || (uint64_t)s > rem) { err = ZLZ4F_ERR_DECOMPRESSION_FAILED; break; }   // :611
                sz = (uint64_t)s;
            }
        }
        x_off[i] = dst_off[f] + pos;
        x_cap[i] = (uint32_t)sz;
        pos += sz;
    }
    if (!err) err = F.err;
    if (err)
        for (uint64_t j = 0; j < F.nb; j++) { x_cap[F.base + j] = 0; x_len[F.base + j] = 0; }
    fr[f].total = pos;
    fr[f].err = err;
}

// one lane per frame: the status, or the content checksum check (:625-635) and the decoded size
__global__ void k_bfd_finish(const BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                             const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                             const uint64_t *__restrict__ src_len, const uint8_t *__restrict__ dst,
                             const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ dst_cap,
                             int64_t *__restrict__ result) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const BFrame F = fr[f];
    if (F.status < 0) { result[f] = F.status; return; }                                // :547
    if (!bf_fits(F, max_blocks)) { result[f] = ZLZ4_ERR_INVALID_STATE; return; }
    if (F.err) { result[f] = F.err; return; }              // (a proven frame has no error: its walk ended cleanly)
    if (F.flg & 0x04u) {
        if (F.end + 4 > src_len[f]) { result[f] = ZLZ4F_ERR_FRAME_SIZE_WRONG; return; }            // :626
        if (F.total > dst_cap[f] ||
            xxh32(dst + dst_off[f], F.total, 0) != zx_rd32(src + src_off[f] + F.end)) {             // :631
            result[f] = ZLZ4F_ERR_CONTENT_CHECKSUM_INVALID;
            return;
        }
    }
    result[f] = (int64_t)F.total;
}

// ------------------------------------------------------------------ decompressed-size query
// per entry: the size kernel's input length (a stored block is not decoded: length 0)
__global__ void k_bfq_len(const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags, uint32_t max_blocks,
                          uint32_t *__restrict__ dec_len) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x)
        dec_len[i] = (flags[i] & kBlkStored) ? 0u : data_len[i];
}

// one wavefront per frame: k_bfd_plan and k_bfd_finish for a destination that is never too small, without the content
// checksum (it needs the decoded bytes).  The first failing block decides (:591, :596, :611), then the walk's error, then
// the missing content-checksum word (:626); otherwise the sum of the block sizes (a stored block counts its data).
__global__ __launch_bounds__(256) void k_bfq_total(const BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                                                   const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags,
                                                   const int64_t *__restrict__ sizes, const uint32_t *__restrict__ cks_ok,
                                                   const uint64_t *__restrict__ src_len, int64_t *__restrict__ result) {
    const uint32_t f = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (f >= nframes) return;
    const BFrame F = fr[f];
    int64_t out;
    if (F.status < 0) out = F.status;                                                  // :547
    else if (!bf_fits(F, max_blocks)) out = ZLZ4_ERR_INVALID_STATE;
    else {
        const bool bc = (F.flg & 0x10u) != 0;
        unsigned long long sum = 0, bad = ~0ull;                      // bad = this lane's first failing block
        int32_t code = 0;
        for (uint64_t j = lane; j < F.nb && bad == ~0ull; j += 64u) {
            const uint64_t i = F.base + j;
            int32_t err = 0;
            uint64_t sz = 0;
            if (bc && cks_ok[i] == 2u) err = ZLZ4F_ERR_FRAME_SIZE_WRONG;               // :591
            else if (bc && cks_ok[i] == 0u) err = ZLZ4F_ERR_BLOCK_CHECKSUM_INVALID;    // :596
            else if (flags[i] & kBlkStored) sz = data_len[i];                          // :603-608
            else if (data_len[i] != 0) {                                               // :610 (src/lz4.zig:97)
                const int64_t s = sizes[i];
                if (s < 0) err = ZLZ4F_ERR_DECOMPRESSION_FAILED;                       // :611
                else sz = (uint64_t)s;
            }
            if (err) { bad = j; code = err; } else sum += sz;
        }
        unsigned long long first = bad;
        for (uint32_t d = 32u; d >= 1u; d >>= 1) {
            const unsigned long long o = __shfl_xor(first, (int)d), t = __shfl_xor(sum, (int)d);
            first = o < first ? o : first;
            sum += t;
        }
        int64_t err = 0;
        if (first != ~0ull) err = (int64_t)(int32_t)zlz4::rdlane((uint32_t)code, zlz4::first_lane(zlz4::ballot(bad == first)));
        if (!err) err = F.err;
        if (err) out = err;
        else if ((F.flg & 0x04u) && F.end + 4 > src_len[f]) out = ZLZ4F_ERR_FRAME_SIZE_WRONG;   // :626
        else out = (int64_t)sum;
    }
    if (lane == 0) result[f] = out;
}

// ------------------------------------------------------------------ workspace layout (Region, Carver: zlz4_frame_batch.hpp)
int32_t bf_hc_level(const zlz4f_prefs &p) {   // compress_frame_impl's routing (:393-404, src/lz4hc.zig:1445)
    if (p.compression_level <= 0) return 0;
    return p.compression_level < 2 ? 9 : (p.compression_level > 12 ? 12 : p.compression_level);
}

uint64_t bf_slot(size_t bs) { return (zlz4_compress_bound(bs) + 15) & ~15ull; }

// what every compress call starts with: the frame records, the block table (`m` entries) and a compressBound slot per entry
struct CompressCore {
    Region<BFrame> frames;
    Region<uint64_t> in_off, out_off, dst_off;
    Region<uint32_t> in_len, out_cap, hdr, cks;
    Region<int64_t> csize;
    Region<uint8_t> slots;
    void carve(Carver &c, uint32_t nframes, size_t m, size_t bs) {
        c.take(nframes, frames);
        c.take(m, in_off, out_off, dst_off, in_len, out_cap, hdr, cks, csize);
        c.take(m * bf_slot(bs), slots);
    }
};

// linked blocks at the fast level: a loadDict table per entry, where the entry's dictionary lies
// in the input, and what loadDict reports
struct LinkedFastTail {
    Region<uint32_t> tables, len;
    Region<uint64_t> off;
    Region<int64_t> dict_size;
    void carve(Carver &c, size_t m) { c.take(m * ZLZ4_STREAM_TABLE_ENTRIES, tables); c.take(m, off, len, dict_size); }
};

// linked blocks at the HC levels 3..9: the V descriptors of zlz4_launch_compress_hc_linked (v_pair = { v_len, start })
struct LinkedHcTail {
    Region<uint64_t> v_off;
    Region<uint32_t> v_pair, v_len;
    void carve(Carver &c, size_t m) { c.take(m, v_off); c.take(m * 2, v_pair); c.take(m, v_len); }
};

bool bf_hc_linked(const zlz4f_prefs &p, uint32_t batch_flags) {
    const int32_t lv = bf_hc_level(p);
    return (batch_flags & ZLZ4F_BATCH_LINK_BLOCKS) && lv >= 3 && lv <= 9;
}

// zlz4f_batch_compress_frame / _ex.  hc: the workspace of the HC launcher the call uses (empty at the fast level);
// ZLZ4F_BATCH_LINK_BLOCKS adds the trailer of its level.
struct BfcLayout {
    CompressCore c;
    Region<uint8_t> hc;
    LinkedFastTail lf;
    LinkedHcTail lh;
    size_t bytes = 0;
};

BfcLayout bfc_layout(uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs &p, uint32_t batch_flags = 0,
                     void *ws = nullptr) {
    const size_t bs = block_size_of(p.block_size_id), m = max_blocks;
    BfcLayout L;
    Carver c{static_cast<uint8_t *>(ws)};
    L.c.carve(c, nframes, m, bs);
    if (bf_hc_linked(p, batch_flags)) {
        c.take(zlz4_hc_linked_workspace_bytes(max_blocks, (uint32_t)bs), L.hc);
        L.lh.carve(c, m);
    } else {
        c.take(bf_hc_level(p) ? zlz4_hc_workspace_bytes(max_blocks, (uint32_t)bs) : 0, L.hc);
        if (batch_flags & ZLZ4F_BATCH_LINK_BLOCKS) L.lf.carve(c, m);
    }
    L.bytes = c.bytes;
    return L;
}

// The decode-side calls, zlz4f_batch_decompress_frame and (query) zlz4f_batch_frame_decompressed_size, share one layout.
struct BfdLayout {
    // the block table both walk the frames into (walk_err: ZLZ4F_DECODE_LINKED, one per frame)
    Region<BFrame> frames;
    Region<uint64_t> data_off, cks_off;
    Region<uint32_t> data_len, flags, fidx, cks_ok, dec_len;
    Region<int64_t> sizes, walk_err;
    // decode only: where the blocks go, speculative (out_) and exact (x_)
    Region<uint64_t> out_off, x_off;
    Region<uint32_t> out_cap, x_cap, x_len;
    // the dictionary of the _using_dict calls per frame (fd_) and per entry (e_); the query reads no dictionary byte and
    // has the lengths alone
    Region<uint64_t> fd_end, e_off;
    Region<uint32_t> fd_len, e_len;
    size_t bytes = 0;
};

constexpr bool kDecode = false, kQuery = true;

BfdLayout bfd_layout(uint32_t nframes, uint32_t max_blocks, uint32_t decode_flags, bool dict, bool query,
                     void *ws = nullptr) {
    const size_t m = max_blocks;
    BfdLayout L;
    Carver c{static_cast<uint8_t *>(ws)};
    c.take(nframes, L.frames);
    c.take(m, L.data_off, L.cks_off);
    if (!query) c.take(m, L.out_off, L.x_off);
    c.take(m, L.data_len, L.flags, L.fidx, L.cks_ok);
    if (!query) c.take(m, L.out_cap);
    c.take(m, L.dec_len);
    if (!query) c.take(m, L.x_cap, L.x_len);
    c.take(m, L.sizes);
    if (decode_flags & ZLZ4F_DECODE_LINKED) c.take(nframes, L.walk_err);
    if (dict && !query) c.take(nframes, L.fd_end);
    if (dict) c.take(nframes, L.fd_len);
    if (dict && !query) c.take(m, L.e_off);
    if (dict) c.take(m, L.e_len);
    L.bytes = c.bytes;
    return L;
}

// ------------------------------------------------------------------ arguments
// the caller's per-frame arrays (include/zlz4_amd.h); the size query and the dictID call have no destination
struct BfArrays {
    const uint8_t *src; const uint64_t *src_off, *src_len;
    uint8_t *dst; const uint64_t *dst_off, *dst_cap;
    int64_t *result; uint32_t nframes, max_blocks;
};

// the dictionary arguments of the _using_dict calls; a null BfDict * is a call without them
struct BfDict { const uint8_t *dict; const uint64_t *off; const uint32_t *len; uint32_t n; const uint32_t *idx; };

inline bool bf_misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// Every refusal of a device array or of the workspace answers ZLZ4_ERR_INVALID_STATE.  Which of them an entry point makes,
// and where among its other refusals (flags, no device, nframes == 0) they stand, differs from call to call and is what
// callers see: each entry point names its own set here and keeps its own order.
enum : uint32_t {
    kArgSrc = 1u,          // d_src, d_src_off, d_src_len and the result array are not null
    kArgDst = 2u,          // d_dst, d_dst_off, d_dst_cap are not null
    kArgDictLen = 4u,      // with ndicts != 0: d_dict_len is not null
    kArgDictOff = 8u,      //                   d_dict_off is not null
    kArgDictBytes = 16u,   //                   d_dict is not null (when max_dict_len != 0)
    kArgAligned = 32u,     // the 64-bit arrays are 8-aligned, the dictionary's 32-bit arrays 4-aligned
    kArgWs = 64u,          // the workspace is not null and holds `need` bytes
    kArgWs16 = 128u,       // the workspace is 16-aligned
};

bool bf_args_refused(uint32_t want, const BfArrays &a, const BfDict *dd = nullptr, uint32_t max_dict_len = 0,
                     const void *ws = nullptr, size_t ws_bytes = 0, size_t need = 0) {
    if ((want & kArgSrc) && (!a.src || !a.src_off || !a.src_len || !a.result)) return true;
    if ((want & kArgDst) && (!a.dst || !a.dst_off || !a.dst_cap)) return true;
    if (dd && dd->n && (((want & kArgDictLen) && !dd->len) || ((want & kArgDictOff) && !dd->off) ||
                        ((want & kArgDictBytes) && max_dict_len && !dd->dict)))
        return true;
    if ((want & kArgAligned) &&
        (bf_misaligned(a.src_off, 8) || bf_misaligned(a.src_len, 8) || bf_misaligned(a.dst_off, 8) ||
         bf_misaligned(a.dst_cap, 8) || bf_misaligned(a.result, 8) ||
         (dd && (bf_misaligned(dd->off, 8) || bf_misaligned(dd->len, 4) || bf_misaligned(dd->idx, 4)))))
        return true;
    if ((want & kArgWs) && (!ws || ws_bytes < need)) return true;
    return (want & kArgWs16) && bf_misaligned(ws, 16);
}

inline uint32_t bf_grid(uint64_t items, uint32_t threads, uint32_t cap = 0xFFFFFFFFu) {
    const uint64_t g = (items + threads - 1) / threads;
    return g == 0 ? 1u : (g > cap ? cap : (uint32_t)g);
}

}  // namespace

extern "C" {

size_t zlz4f_batch_compress_frame_workspace(uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs *prefs) {
    return bfc_layout(nframes, max_blocks, prefs ? *prefs : kDefaultPrefs).bytes;
}

size_t zlz4f_batch_compress_frame_workspace_ex(uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs *prefs,
                                               uint32_t batch_flags) {
    return bfc_layout(nframes, max_blocks, prefs ? *prefs : kDefaultPrefs, batch_flags).bytes;
}

size_t zlz4f_batch_decompress_frame_workspace(uint32_t nframes, uint32_t max_blocks) {
    return bfd_layout(nframes, max_blocks, 0, false, kDecode).bytes;
}

size_t zlz4f_batch_decompress_frame_workspace_ex(uint32_t nframes, uint32_t max_blocks, uint32_t decode_flags) {
    return bfd_layout(nframes, max_blocks, decode_flags, false, kDecode).bytes;
}

}  // extern "C"

namespace {

// ------------------------------------------------------------------ compress: the launch sequences both calls share
// Open: block count and capacity check per frame, the dictionary call's preconditions (dd; the one early return), the
// scan, and -- with a table -- the block descriptors.
int32_t bfc_open(hipStream_t st, const BfArrays &a, const zlz4f_prefs &p, const CompressCore &C, const BfDict *dd = nullptr,
                 uint64_t max_src_len = 0, uint32_t max_dict_len = 0) {
    const size_t bs = block_size_of(p.block_size_id);
    const uint64_t per_block = 4 + zlz4_compress_bound(bs) + (p.block_checksum == 1 ? 4 : 0);   // zlz4f_compress_frame_bound
    const uint64_t fixed = 19 + 4 + (p.content_checksum == 1 ? 4 : 0);
    hipLaunchKernelGGL(k_bfc_count, dim3(bf_grid(a.nframes, 256)), dim3(256), 0, st, a.src_len, a.dst_cap, a.nframes,
                       (uint64_t)bs, per_block, fixed, C.frames);
    if (dd && zlz4_launch_bfcd_pre(st, C.frames, a.nframes, a.src_len, dd->len, dd->n, dd->idx, max_src_len, max_dict_len) != 0)
        return ZLZ4_ERR_DEVICE;
    hipLaunchKernelGGL(k_bf_scan, dim3(1), dim3(1024), 0, st, C.frames, a.nframes);
    if (a.max_blocks)
        hipLaunchKernelGGL(k_bfc_desc, dim3(bf_grid(a.max_blocks, 256, 4096)), dim3(256), 0, st, C.frames, a.nframes,
                           a.max_blocks, a.src_off, a.src_len, (uint64_t)bs, bf_slot(bs), C.in_off, C.in_len, C.out_off,
                           C.out_cap, C.hdr);
    return 0;
}

// Close: with a table the dstPos plan per frame, the block checksums and the scatter; then header, end mark, content
// checksum and result of every frame.
int32_t bfc_close(hipStream_t st, const BfArrays &a, const zlz4f_prefs &p, uint32_t cs_from_len, const CompressCore &C) {
    const uint32_t bc = p.block_checksum == 1 ? 1u : 0u;
    if (a.max_blocks) {
        hipLaunchKernelGGL(k_bfc_plan, dim3(bf_grid(a.nframes, 4)), dim3(256), 0, st, C.frames, a.nframes, a.max_blocks,
                           C.csize, C.in_len, bc, p, cs_from_len, a.src_len, a.dst_off, C.dst_off, C.hdr);
        if (bc)
            hipLaunchKernelGGL(k_block_xxh32, dim3(bf_grid(a.max_blocks, 64)), dim3(64), 0, st, a.src, C.in_off, C.slots,
                               C.out_off, C.hdr, a.max_blocks, C.cks);
        hipLaunchKernelGGL(k_bf_scatter, dim3(a.max_blocks), dim3(256), 0, st, a.src, C.in_off, C.slots, C.out_off, C.hdr,
                           C.dst_off, C.cks, bc, a.dst);
    }
    hipLaunchKernelGGL(k_bfc_head_tail, dim3(bf_grid(a.nframes, 64)), dim3(64), 0, st, C.frames, a.nframes, a.max_blocks, p,
                       cs_from_len, a.src, a.src_off, a.src_len, a.dst, a.dst_off, a.result);
    return hipGetLastError() == hipSuccess ? 0 : ZLZ4_ERR_DEVICE;
}

// Linked blocks at the fast level: the entries with len[i] != 0 against the 64 KiB of input in front of them.  Descriptors,
// one loadDict table per entry, then the dictionary compressor over the table (block 0 of a frame has an empty dictionary:
// compressDefault's bytes).  Answers the first failing launcher's code.
int bfc_linked_fast(hipStream_t st, const BfArrays &a, const CompressCore &C, const LinkedFastTail &T, const uint32_t *len,
                    int64_t *csize, size_t bs) {
    int rc = zlz4_launch_bfl_dict_desc(st, C.frames, a.nframes, a.max_blocks, a.src_off, C.in_off, len, T.off, T.len);
    if (rc == 0) rc = zlz4_launch_load_dict(st, a.src, T.off, T.len, T.tables, T.dict_size, a.max_blocks);
    if (rc == 0)
        rc = zlz4_launch_compress_fast_using_dict(st, a.src, C.in_off, len, C.slots, C.out_off, C.out_cap, a.src, T.off, T.len,
                                                  T.tables, nullptr, csize, a.max_blocks, (uint32_t)bs, 65536u, 1);
    return rc;
}

// Linked blocks at the levels 3..9: block k is compressHCUsingDict against the same 64 KiB; V_k = tail ++ block lies
// contiguous in d_src, so the descriptors point the HC kernels at the input itself (no staged copy, no loadDict table).
int bfc_linked_hc(hipStream_t st, const BfArrays &a, const CompressCore &C, const LinkedHcTail &T, const Region<uint8_t> &hc,
                  const uint32_t *len, int64_t *csize, size_t bs, int32_t level) {
    int rc = zlz4_launch_bfl_hc_desc(st, C.frames, a.nframes, a.max_blocks, a.src_off, C.in_off, len, T.v_off, T.v_len,
                                     T.v_pair);
    if (rc == 0)
        rc = zlz4_launch_compress_hc_linked(st, a.src, T.v_off, T.v_len, T.v_pair, C.slots, C.out_off, C.out_cap, csize,
                                            a.max_blocks, (uint32_t)bs, level, hc, hc.bytes);
    return rc;
}

// the refusals of both compress calls that need no device, in their order.  ex: zlz4f_batch_compress_frame_ex, which links
// blocks at the HC levels 3..9 (the levels zlz4_batch_compress_hc_using_dict takes); the plain call refuses every HC level.
int32_t bfc_refusal(const zlz4f_prefs &p, uint32_t batch_flags, bool ex) {
    if (batch_flags & ~(ZLZ4F_BATCH_CONTENT_SIZE | ZLZ4F_BATCH_LINK_BLOCKS)) return ZLZ4F_ERR_PARAMETER_INVALID;
    const bool link = (batch_flags & ZLZ4F_BATCH_LINK_BLOCKS) != 0;
    if ((batch_flags & ZLZ4F_BATCH_CONTENT_SIZE) && p.content_size != 0) return ZLZ4F_ERR_PARAMETER_INVALID;
    if (link && p.block_mode != 0) return ZLZ4F_ERR_PARAMETER_INVALID;     // FLG must declare what the blocks are
    if (link && bf_hc_level(p) > 0 && !(ex && bf_hc_linked(p, batch_flags))) return ZLZ4_ERR_UNSUPPORTED;
    return 0;
}

// The compressors answer their own code on the paths without links; a failing launcher of a linked path is a DeviceError.
int32_t batch_compress_frame_impl(void *stream_, const BfArrays &a, const zlz4f_prefs *prefs, uint32_t batch_flags,
                                  void *ws, size_t workspace_bytes, bool ex) {
    const zlz4f_prefs p = prefs ? *prefs : kDefaultPrefs;
    const int32_t refused = bfc_refusal(p, batch_flags, ex);
    if (refused != 0) return refused;
    const uint32_t cs_from_len = (batch_flags & ZLZ4F_BATCH_CONTENT_SIZE) ? 1u : 0u;
    const bool link = (batch_flags & ZLZ4F_BATCH_LINK_BLOCKS) != 0;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    const BfcLayout L = bfc_layout(a.nframes, a.max_blocks, p, batch_flags, ws);
    if (a.nframes == 0) return 0;
    if (bf_args_refused(kArgWs | (ex ? kArgWs16 : 0u), a, nullptr, 0, ws, workspace_bytes, L.bytes))
        return ZLZ4_ERR_INVALID_STATE;
    hipStream_t st = (hipStream_t)stream_;
    const CompressCore &C = L.c;
    const size_t bs = block_size_of(p.block_size_id);
    const int32_t hc_level = bf_hc_level(p);
    (void)bfc_open(st, a, p, C);             // (its one failure is the dictionary call's)
    if (a.max_blocks) {
        int rc;
        if (link) {
            rc = hc_level != 0 ? bfc_linked_hc(st, a, C, L.lh, L.hc, C.in_len, C.csize, bs, hc_level)
                               : bfc_linked_fast(st, a, C, L.lf, C.in_len, C.csize, bs);
            if (rc != 0) rc = ZLZ4_ERR_DEVICE;
        } else if (hc_level == 0)
            rc = zlz4_launch_compress_fast(st, a.src, C.in_off, C.in_len, C.slots, C.out_off, C.out_cap, C.csize, a.max_blocks,
                                           (uint32_t)bs, 1);                                               // :400-404
        else
            rc = zlz4_launch_compress_hc(st, a.src, C.in_off, C.in_len, C.slots, C.out_off, C.out_cap, C.csize, a.max_blocks,
                                         (uint32_t)bs, hc_level, L.hc, L.hc.bytes);                        // :394-398
        if (rc != 0) return rc;
    }
    return bfc_close(st, a, p, cs_from_len, C);
}

// ------------------------------------------------------------------ dictionary frames, compress
// Launch B (the linked path of section 4.4c for the blocks k >= 1) is needed when FLG declares linked blocks and a frame
// can have a second block.
bool bfcd_link_b(const zlz4f_prefs &p, uint64_t max_src_len) {
    return p.block_mode != 1 && !(max_src_len != 0 && max_src_len <= block_size_of(p.block_size_id));
}

// the _ex calls at the HC levels zlz4_batch_compress_hc_using_dict takes; every other level is
// the plain call's business
bool bfcd_hc(const zlz4f_prefs &p, bool ex) {
    const int32_t lv = bf_hc_level(p);
    return ex && lv >= 3 && lv <= 9;
}

// what the dictionary compressor of launch A is given as its max_in_len
uint32_t bfcd_in_max(size_t bs, uint64_t max_src_len) {
    return max_src_len != 0 && max_src_len < bs ? (uint32_t)max_src_len : (uint32_t)bs;
}

// zlz4f_batch_compress_frame_using_dict / _ex.  d_tables, d_sizes: loadDict over the ndicts dictionaries (fast level only).
// len_a ... a_tix: launch A's lengths and dictionary descriptors.  With launch B: len_b, the linked trailer of the level and
// B's results.  hc (bfcd_hc) is ONE region, the larger of zlz4_hc_dict_workspace_bytes (launch A) and
// zlz4_hc_linked_workspace_bytes (launch B): both launchers join their side stream into the caller's before they return,
// so launch B's first memset is ordered behind all of launch A's work.
struct BfcdLayout {
    CompressCore c;
    Region<uint32_t> d_tables, len_a, a_len, a_tix, len_b;
    Region<uint64_t> a_off;
    Region<int64_t> d_sizes, csize_b;
    Region<uint8_t> hc;
    LinkedFastTail lf;
    LinkedHcTail lh;
    size_t bytes = 0;
};

BfcdLayout bfcd_layout(uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs &p, uint32_t ndicts, uint64_t max_src_len,
                       uint32_t max_dict_len = 0, bool hc = false, void *ws = nullptr) {
    const size_t bs = block_size_of(p.block_size_id), m = max_blocks;
    const bool link_b = bfcd_link_b(p, max_src_len);
    BfcdLayout L;
    Carver c{static_cast<uint8_t *>(ws)};
    L.c.carve(c, nframes, m, bs);
    if (!hc) { c.take((size_t)ndicts * ZLZ4_STREAM_TABLE_ENTRIES, L.d_tables); c.take(ndicts, L.d_sizes); }
    c.take(m, L.len_a, L.a_off, L.a_len, L.a_tix);
    if (hc) {
        const size_t scratch_a = zlz4_hc_dict_workspace_bytes(max_blocks, bfcd_in_max(bs, max_src_len), max_dict_len);
        const size_t scratch_b = link_b ? zlz4_hc_linked_workspace_bytes(max_blocks, (uint32_t)bs) : 0;
        c.take(scratch_a > scratch_b ? scratch_a : scratch_b, L.hc);
    }
    if (link_b) {
        c.take(m, L.len_b);
        if (hc) L.lh.carve(c, m); else L.lf.carve(c, m);
        c.take(m, L.csize_b);
    }
    L.bytes = c.bytes;
    return L;
}

// the refusals that need no device, in their order: parameter errors, then the levels the call does not serve (the plain
// call: every HC level; ex, the _ex calls: 2 and 10..12, which zlz4_batch_compress_hc_using_dict refuses)
int32_t bfcd_refusal(const zlz4f_prefs &p, uint32_t batch_flags, bool ex = false) {
    if (batch_flags & ~ZLZ4F_BATCH_CONTENT_SIZE) return ZLZ4F_ERR_PARAMETER_INVALID;   // block_mode says "linked"
    if ((batch_flags & ZLZ4F_BATCH_CONTENT_SIZE) && p.content_size != 0) return ZLZ4F_ERR_PARAMETER_INVALID;
    if (bf_hc_level(p) > 0 && !bfcd_hc(p, ex)) return ZLZ4_ERR_UNSUPPORTED;
    return 0;
}

// batch_compress_frame_impl at the fast level with a dictionary per frame.  The ndicts dictionaries are hashed once
// (zlz4_launch_load_dict over them, never per frame); launch A compresses every block of an independent frame and block 0
// of a linked one against the frame's dictionary where it lies in d_dict, launch B the blocks k >= 1 of a linked frame
// against the input in front of them where it lies in d_src (section 4.4c).  The two launches run over complementary
// length arrays into the same slots; k_bfcd_merge takes B's results for B's entries only.
// ex at levels 3..9 (the _ex calls, section 4.4e): the same two launches with the HC compressors.  Launch A is
// zlz4_launch_compress_hc_dict over len_a / a_off / a_len (an entry that takes no part has record and dictionary length 0:
// nothing staged, result 0), launch B zlz4_launch_compress_hc_linked over the V descriptors k_bfl_hc_desc derives from
// len_b (block 0 and the empty entries get an empty V).  No loadDict table is built.
// Every failing launcher is a DeviceError here.
int32_t batch_compress_frame_dict_impl(void *stream_, const BfArrays &a, const zlz4f_prefs *prefs, uint32_t batch_flags,
                                       const BfDict &dd, uint64_t max_src_len, uint32_t max_dict_len, void *ws,
                                       size_t workspace_bytes, bool ex) {
    const zlz4f_prefs p = prefs ? *prefs : kDefaultPrefs;
    const int32_t refused = bfcd_refusal(p, batch_flags, ex);
    if (refused != 0) return refused;
    const uint32_t cs_from_len = (batch_flags & ZLZ4F_BATCH_CONTENT_SIZE) ? 1u : 0u;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    const bool hc = bfcd_hc(p, ex);
    const BfcdLayout L = bfcd_layout(a.nframes, a.max_blocks, p, dd.n, max_src_len, max_dict_len, hc, ws);
    if (a.nframes == 0) return 0;
    if (bf_args_refused(kArgSrc | kArgDst | kArgDictLen | kArgDictOff | kArgDictBytes | kArgAligned | kArgWs | kArgWs16, a, &dd,
                        max_dict_len, ws, workspace_bytes, L.bytes))
        return ZLZ4_ERR_INVALID_STATE;
    hipStream_t st = (hipStream_t)stream_;
    const CompressCore &C = L.c;
    const bool link_b = bfcd_link_b(p, max_src_len);
    const size_t bs = block_size_of(p.block_size_id);
    if (bfc_open(st, a, p, C, &dd, max_src_len, max_dict_len) != 0) return ZLZ4_ERR_DEVICE;
    if (a.max_blocks) {
        // (without launch B every frame has one block at most: all entries are launch A's, len_b does not exist)
        int rc = zlz4_launch_bfcd_desc(st, C.frames, a.nframes, a.max_blocks, link_b, dd.off, dd.len, dd.idx, C.in_len, L.len_a,
                                       L.len_b, L.a_off, L.a_len, L.a_tix);
        const uint32_t in_max = bfcd_in_max(bs, max_src_len);
        if (hc) {
            if (rc == 0)
                rc = zlz4_launch_compress_hc_dict(st, a.src, C.in_off, L.len_a, C.slots, C.out_off, C.out_cap, dd.dict, L.a_off,
                                                  L.a_len, C.csize, a.max_blocks, in_max, max_dict_len, bf_hc_level(p), L.hc,
                                                  L.hc.bytes);
            if (rc == 0 && link_b) rc = bfc_linked_hc(st, a, C, L.lh, L.hc, L.len_b, L.csize_b, bs, bf_hc_level(p));
        } else {
            if (rc == 0 && dd.n) rc = zlz4_launch_load_dict(st, dd.dict, dd.off, dd.len, L.d_tables, L.d_sizes, dd.n);
            if (rc == 0)
                rc = zlz4_launch_compress_fast_using_dict(st, a.src, C.in_off, L.len_a, C.slots, C.out_off, C.out_cap, dd.dict,
                                                          L.a_off, L.a_len, L.d_tables, L.a_tix, C.csize, a.max_blocks, in_max,
                                                          max_dict_len, 1);
            if (rc == 0 && link_b) rc = bfc_linked_fast(st, a, C, L.lf, L.len_b, L.csize_b, bs);
        }
        if (rc == 0 && link_b) rc = zlz4_launch_bfcd_merge(st, L.len_b, L.csize_b, C.csize, a.max_blocks);
        if (rc != 0) return ZLZ4_ERR_DEVICE;
    }
    return bfc_close(st, a, p, cs_from_len, C);
}

// One frame through zlz4f_batch_compress_frame_ex or, with a dictionary of dict_len bytes at d_dict, through
// zlz4f_batch_compress_frame_using_dict (ex: .._using_dict_ex); device pointers: a batch of one with max_blocks =
// ceil(n / bs), a staged record and a workspace from the device cache; synchronises `st` (as single_frame_ex of the
// decode side)
struct OneDict { const uint8_t *d_dict; uint32_t dict_len; bool ex; };

int64_t single_compress_frame(hipStream_t st, const uint8_t *d_src, size_t n, uint8_t *d_dst, size_t cap, const zlz4f_prefs &p,
                              uint32_t batch_flags, const OneDict *dict = nullptr) {
    const size_t bs = block_size_of(p.block_size_id);
    const uint64_t nb = (uint64_t)n / bs + (n % bs != 0);
    if (nb > 0x7FFFFFFFull) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    const uint32_t max_blocks = (uint32_t)nb;
    DeviceCall dc(st);
    const size_t ws = dict ? bfcd_layout(1, max_blocks, p, 1, n, dict->dict_len, bfcd_hc(p, dict->ex)).bytes
                           : bfc_layout(1, max_blocks, p, batch_flags).bytes;
    struct Rec { FrameRec f; uint64_t dict_off; uint32_t dict_len; };
    Staged<Rec> rec(&dc);
    DevBuf d_ws(ws, &dc);
    if (!rec.d || !d_ws.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.f.src_len = n; rec.h.f.dst_cap = cap; rec.h.dict_len = dict ? dict->dict_len : 0;
    dc.launched();
    if (!rec.upload(st, dict ? sizeof(Rec) : sizeof(FrameRec))) return ZLZ4_ERR_DEVICE;   // (the dictionary fields follow f)
    FrameRec *r = &rec.d->f;
    const BfArrays a = {d_src, &r->src_off, &r->src_len, d_dst, &r->dst_off, &r->dst_cap, &r->result, 1, max_blocks};
    int32_t rc;
    if (dict) {
        const BfDict dd = {dict->d_dict, &rec.d->dict_off, &rec.d->dict_len, 1u, nullptr};
        rc = batch_compress_frame_dict_impl(st, a, &p, 0, dd, n, dict->dict_len, d_ws.p, ws, dict->ex);
    } else {
        rc = batch_compress_frame_impl(st, a, &p, batch_flags, d_ws.p, ws, true);
    }
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result)) return ZLZ4_ERR_DEVICE;
    return result;
}

// the last 64 KiB of a host dictionary on the device, for the call that then runs with it
template <typename Call> int64_t with_dict_tail(const uint8_t *dict, size_t dict_len, Call call) {
    const size_t D = dict_tail(dict_len);
    DevBuf d_dict(D);
    if (!d_dict.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    if (D && hipMemcpy(d_dict.p, dict + (dict_len - D), D, hipMemcpyHostToDevice) != hipSuccess) return ZLZ4_ERR_DEVICE;
    return call(d_dict.as<uint8_t>(), (uint32_t)D);
}

}  // namespace

extern "C" {

int32_t zlz4f_batch_compress_frame(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                   uint8_t *d_dst, const uint64_t *d_dst_off, const uint64_t *d_dst_cap, int64_t *d_result,
                                   uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs *prefs, uint32_t batch_flags,
                                   void *d_workspace, size_t workspace_bytes) {
    const BfArrays a = {d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_result, nframes, max_blocks};
    return batch_compress_frame_impl(stream, a, prefs, batch_flags, d_workspace, workspace_bytes, false);
}

// zlz4f_batch_compress_frame, and ZLZ4F_BATCH_LINK_BLOCKS at the HC levels 3..9
int32_t zlz4f_batch_compress_frame_ex(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                      uint8_t *d_dst, const uint64_t *d_dst_off, const uint64_t *d_dst_cap, int64_t *d_result,
                                      uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs *prefs, uint32_t batch_flags,
                                      void *d_workspace, size_t workspace_bytes) {
    const BfArrays a = {d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_result, nframes, max_blocks};
    return batch_compress_frame_impl(stream, a, prefs, batch_flags, d_workspace, workspace_bytes, true);
}

// one frame through zlz4f_batch_compress_frame_ex (the result is the batch call's for that frame); synchronises `stream`
int64_t zlz4f_compress_frame_device_ex(void *stream, const uint8_t *d_src, size_t n, uint8_t *d_dst, size_t cap,
                                       const zlz4f_prefs *prefs, uint32_t batch_flags) {
    const zlz4f_prefs p = prefs ? *prefs : kDefaultPrefs;
    const int32_t refused = bfc_refusal(p, batch_flags, true);
    if (refused != 0) return refused;
    if ((!d_src && n) || (!d_dst && cap)) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return single_compress_frame((hipStream_t)stream, d_src, n, d_dst, cap, p, batch_flags);
}

// host pointers: stage -> the device call -> copy the frame back
int64_t zlz4f_compress_frame_ex(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const zlz4f_prefs *prefs,
                                uint32_t batch_flags) {
    const zlz4f_prefs p = prefs ? *prefs : kDefaultPrefs;
    const int32_t refused = bfc_refusal(p, batch_flags, true);
    if (refused != 0) return refused;
    if ((!src && n) || (!dst && cap)) return ZLZ4_ERR_INVALID_STATE;
    const size_t bound = zlz4f_compress_frame_bound(n, &p);
    if (cap < bound) return ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;                                            // :363-366
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return host_frame_call(src, n, dst, cap, bound, [&](const uint8_t *d_src, uint8_t *d_dst) {
        return single_compress_frame(nullptr, d_src, n, d_dst, bound, p, batch_flags);
    });
}

}  // extern "C"

namespace {

// ------------------------------------------------------------------ decode: what both decode-side calls share
// with a dictionary the block decoders take a descriptor per entry
int bfd_decode_safe(hipStream_t st, const BfArrays &a, const BfDict *dd, const BfdLayout &L, const uint32_t *len,
                    const uint64_t *off, const uint32_t *cap) {
    return dd ? zlz4_launch_decompress_safe_using_dict(st, a.src, L.data_off, len, a.dst, off, cap, L.sizes, a.max_blocks,
                                                       dd->dict, L.e_off, L.e_len)
              : zlz4_launch_decompress_safe(st, a.src, L.data_off, len, a.dst, off, cap, L.sizes, a.max_blocks);
}

int bfd_decode_sizes(hipStream_t st, const BfArrays &a, const BfDict *dd, const BfdLayout &L, const uint32_t *len,
                     const uint64_t *off, const uint32_t *cap) {
    return dd ? zlz4_launch_decompress_sizes_using_dict(st, a.src, L.data_off, len, off, cap, L.sizes, a.max_blocks, L.e_off,
                                                        L.e_len)
              : zlz4_launch_decompress_sizes(st, a.src, L.data_off, len, off, cap, L.sizes, a.max_blocks);
}

// the entries of the frames k_bfl_decode takes leave a length / capacity array (ZLZ4F_DECODE_LINKED only)
int bfd_mask_serial(hipStream_t st, const BfDict *dd, const BfdLayout &L, uint32_t max_blocks, uint32_t *cap, uint32_t *len) {
    return (dd ? zlz4_launch_bfdd_mask : zlz4_launch_bfl_mask)(st, L.frames, L.fidx, max_blocks, cap, len);
}

// The prelude: clear the table, count every frame's blocks, (dictionary) the frame's dictionary, scan, (linked) keep the
// walk's error, and -- with a table -- record the blocks, (dictionary) the entry's dictionary, verify the block checksums.
// The size query has no fd_end / e_off and passes no dictionary offsets.  0 or ZLZ4_ERR_DEVICE.
int32_t bfd_prelude(hipStream_t st, const BfArrays &a, bool linked, const BfDict *dd, const BfdLayout &L) {
    const uint32_t gf = bf_grid(a.nframes, 256), gb = bf_grid(a.max_blocks, 256, 4096);
    if (a.max_blocks) hipLaunchKernelGGL(k_bfd_init, dim3(gb), dim3(256), 0, st, L.data_len, L.flags, L.fidx, a.max_blocks);
    hipLaunchKernelGGL(k_bfd_walk<false>, dim3(gf), dim3(256), 0, st, a.src, a.src_off, a.src_len, a.nframes, a.max_blocks,
                       L.frames, L.data_off, L.data_len, L.flags, L.cks_off, L.fidx);
    if (dd && zlz4_launch_bfdd_frame(st, L.frames, a.nframes, L.fd_end ? dd->off : nullptr, dd->len, dd->n, dd->idx, L.fd_end,
                                     L.fd_len) != 0)
        return ZLZ4_ERR_DEVICE;
    hipLaunchKernelGGL(k_bf_scan, dim3(1), dim3(1024), 0, st, L.frames, a.nframes);
    if (linked && zlz4_launch_bfl_save(st, L.frames, a.nframes, L.walk_err) != 0) return ZLZ4_ERR_DEVICE;
    if (a.max_blocks) {
        hipLaunchKernelGGL(k_bfd_walk<true>, dim3(gf), dim3(256), 0, st, a.src, a.src_off, a.src_len, a.nframes, a.max_blocks,
                           L.frames, L.data_off, L.data_len, L.flags, L.cks_off, L.fidx);
        if (dd && zlz4_launch_bfdd_entry(st, L.frames, L.fidx, a.max_blocks, L.fd_end, L.fd_len, L.e_off, L.e_len) != 0)
            return ZLZ4_ERR_DEVICE;
        hipLaunchKernelGGL(k_bfd_verify, dim3(bf_grid(a.max_blocks, 64)), dim3(64), 0, st, a.src, L.data_off, L.data_len,
                           L.flags, L.cks_off, a.max_blocks, L.cks_ok);
    }
    return 0;
}

// The frames that are decoded in block order by one wavefront each: with a dictionary the linked-declared frames of several
// blocks (with the external tail), else -- ZLZ4F_DECODE_LINKED -- the linked-declared ones.  write: decode into a.dst and
// leave F.total / F.err; else the size query, whose results go to a.result.
int32_t bfd_serial(hipStream_t st, int write, const BfArrays &a, bool linked, const BfDict *dd, const BfdLayout &L) {
    int64_t *d_size = write ? nullptr : a.result;
    if (dd)
        return zlz4_launch_bfl_decode_dict(st, write, L.frames, a.nframes, a.max_blocks, a.src, L.data_off, L.data_len, L.flags,
                                           L.cks_ok, L.walk_err, a.dst, a.dst_off, a.dst_cap, a.src_len, d_size,
                                           write ? dd->dict : nullptr, L.fd_end, L.fd_len);
    if (!linked) return 0;
    return zlz4_launch_bfl_decode(st, write, L.frames, a.nframes, a.max_blocks, a.src, L.data_off, L.data_len, L.flags, L.cks_ok,
                                  L.walk_err, a.dst, a.dst_off, a.dst_cap, a.src_len, d_size);
}

// decode_flags 0: zlz4f_batch_decompress_frame.  ZLZ4F_DECODE_LINKED: the frames whose FLG declares linked blocks leave the
// parallel decodes (bfd_mask_serial after each kernel that fills a length / capacity array) and are decoded in block order
// by k_bfl_decode, which leaves F.total / F.err for k_bfd_finish; the sequence of launches stays fixed.
// Dictionary frames (dd): the linked-declared frames of several blocks go through k_bfl_decode with
// the external tail, the others stay on the parallel decodes, which get a dictionary descriptor per entry.
int32_t batch_decompress_frame_impl(void *stream_, const BfArrays &a, uint32_t decode_flags, void *ws, size_t workspace_bytes,
                                    const BfDict *dd = nullptr) {
    if (decode_flags & ~ZLZ4F_DECODE_LINKED) return ZLZ4F_ERR_PARAMETER_INVALID;
    const bool linked = (decode_flags & ZLZ4F_DECODE_LINKED) != 0;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    const BfdLayout L = bfd_layout(a.nframes, a.max_blocks, decode_flags, dd != nullptr, kDecode, ws);
    if (a.nframes == 0) return 0;
    if (bf_args_refused(kArgWs | (dd ? kArgSrc | kArgDst | kArgDictLen | kArgDictOff | kArgAligned | kArgWs16 : 0u), a, dd, 0, ws,
                        workspace_bytes, L.bytes))
        return ZLZ4_ERR_INVALID_STATE;
    hipStream_t st = (hipStream_t)stream_;
    const uint32_t gf = bf_grid(a.nframes, 256), gb = bf_grid(a.max_blocks, 256, 4096), mb = a.max_blocks;
    if (bfd_prelude(st, a, linked, dd, L) != 0) return ZLZ4_ERR_DEVICE;
    if (mb) {
        // speculative layout, proven per frame
        hipLaunchKernelGGL(k_bfd_spec, dim3(gb), dim3(256), 0, st, L.frames, L.fidx, L.data_len, L.flags, a.dst_off, a.dst_cap,
                           mb, L.out_off, L.out_cap, L.dec_len);
        if (linked && bfd_mask_serial(st, dd, L, mb, L.out_cap, L.dec_len) != 0) return ZLZ4_ERR_DEVICE;
        if (bfd_decode_safe(st, a, dd, L, L.dec_len, L.out_off, L.out_cap) != 0) return ZLZ4_ERR_DEVICE;
        hipLaunchKernelGGL(k_bf_copy_stored, dim3(mb), dim3(256), 0, st, a.src, L.data_off, L.data_len, L.flags, L.out_off,
                           L.out_cap, a.dst);
        hipLaunchKernelGGL(k_bfd_check, dim3(bf_grid(a.nframes, 4)), dim3(256), 0, st, L.frames, a.nframes, mb, L.data_len,
                           L.flags, L.sizes, L.cks_ok, L.out_cap);
        // exact path for the frames whose layout was not proven (always enqueued: the sequence does not depend on data)
        hipLaunchKernelGGL(k_bfd_mask, dim3(gb), dim3(256), 0, st, L.frames, L.fidx, L.data_len, L.flags, mb, L.x_off, L.x_cap,
                           L.x_len);
        if (linked && bfd_mask_serial(st, dd, L, mb, L.x_cap, L.x_len) != 0) return ZLZ4_ERR_DEVICE;
        if (bfd_decode_sizes(st, a, dd, L, L.x_len, L.x_off, L.x_cap) != 0) return ZLZ4_ERR_DEVICE;
    }
    hipLaunchKernelGGL(k_bfd_plan, dim3(gf), dim3(256), 0, st, L.frames, a.nframes, mb, L.data_len, L.flags, L.sizes, L.cks_ok,
                       a.dst_off, a.dst_cap, L.x_off, L.x_cap, L.x_len);
    if (mb) {
        // (k_bfd_plan laid out the unproven frames, a linked one among them from sizes that mean nothing: masked again)
        if (linked && bfd_mask_serial(st, dd, L, mb, L.x_cap, L.x_len) != 0) return ZLZ4_ERR_DEVICE;
        if (bfd_decode_safe(st, a, dd, L, L.x_len, L.x_off, L.x_cap) != 0) return ZLZ4_ERR_DEVICE;
        hipLaunchKernelGGL(k_bf_copy_stored, dim3(mb), dim3(256), 0, st, a.src, L.data_off, L.data_len, L.flags, L.x_off,
                           L.x_cap, a.dst);
    }
    if (bfd_serial(st, 1, a, linked, dd, L) != 0) return ZLZ4_ERR_DEVICE;
    hipLaunchKernelGGL(k_bfd_finish, dim3(gf), dim3(256), 0, st, L.frames, a.nframes, mb, a.src, a.src_off, a.src_len, a.dst,
                       a.dst_off, a.dst_cap, a.result);
    return hipGetLastError() == hipSuccess ? 0 : ZLZ4_ERR_DEVICE;
}

// The prelude of zlz4f_batch_decompress_frame, then the size kernel over the block table and the per-frame total; nothing
// but a.result (d_size) and the workspace is written.  ZLZ4F_DECODE_LINKED: the entries of the linked-declared frames are
// masked out of the size kernel and k_bfl_decode<false> replaces their results.  No device is the LAST refusal here.
int32_t batch_frame_decompressed_size_impl(void *stream_, const BfArrays &a, uint32_t decode_flags, void *ws,
                                           size_t workspace_bytes, const BfDict *dd = nullptr) {
    if (decode_flags & ~ZLZ4F_DECODE_LINKED) return ZLZ4F_ERR_PARAMETER_INVALID;
    const bool linked = (decode_flags & ZLZ4F_DECODE_LINKED) != 0;
    if (a.nframes == 0) return 0;
    const BfdLayout L = bfd_layout(a.nframes, a.max_blocks, decode_flags, dd != nullptr, kQuery, ws);
    if (bf_args_refused(kArgSrc | kArgWs | kArgWs16 | (dd ? kArgDictLen | kArgAligned : 0u), a, dd, 0, ws, workspace_bytes,
                        L.bytes))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream_;
    const uint32_t mb = a.max_blocks;
    if (bfd_prelude(st, a, linked, dd, L) != 0) return ZLZ4_ERR_DEVICE;
    if (mb) {
        hipLaunchKernelGGL(k_bfq_len, dim3(bf_grid(mb, 256, 4096)), dim3(256), 0, st, L.data_len, L.flags, mb, L.dec_len);
        if (linked && bfd_mask_serial(st, dd, L, mb, nullptr, L.dec_len) != 0) return ZLZ4_ERR_DEVICE;
        if (zlz4_launch_decompressed_size(st, a.src, L.data_off, L.dec_len, L.e_len, L.sizes, mb) != 0) return ZLZ4_ERR_DEVICE;
    }
    hipLaunchKernelGGL(k_bfq_total, dim3(bf_grid(a.nframes, 4)), dim3(256), 0, st, L.frames, a.nframes, mb, L.data_len, L.flags,
                       L.sizes, L.cks_ok, a.src_len, a.result);
    if (bfd_serial(st, 0, a, linked, dd, L) != 0) return ZLZ4_ERR_DEVICE;
    return hipGetLastError() == hipSuccess ? 0 : ZLZ4_ERR_DEVICE;
}

// One frame through the batch calls, device pointers: a counting walk finds the table size (read back), then the frame
// is a batch of one.  d_dst == nullptr with want_size: the size query.
// with_dict: the _using_dict calls with one dictionary of dict_len bytes at d_dict (the size query needs no bytes).
int64_t single_frame_ex(hipStream_t st, const uint8_t *d_src, size_t n, uint8_t *d_dst, size_t cap, uint32_t decode_flags,
                        bool want_size, bool with_dict = false, const uint8_t *d_dict = nullptr, uint32_t dict_len = 0) {
    if (decode_flags & ~ZLZ4F_DECODE_LINKED) return ZLZ4F_ERR_PARAMETER_INVALID;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    DeviceCall dc(st);
    struct Rec { FrameRec f; uint64_t dict_off; uint32_t dict_len; uint32_t pad[3]; BFrame fr; };
    Staged<Rec> rec(&dc, 256);
    if (!rec.d) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.f.src_len = n; rec.h.f.dst_cap = cap; rec.h.dict_len = dict_len;
    dc.launched();
    if (!rec.upload(st)) return ZLZ4_ERR_DEVICE;
    FrameRec *r = &rec.d->f;
    BFrame *p_fr = &rec.d->fr;
    hipLaunchKernelGGL(k_bfd_walk<false>, dim3(1), dim3(256), 0, st, d_src, &r->src_off, &r->src_len, 1u, 0u, p_fr, nullptr,
                       nullptr, nullptr, nullptr, nullptr);
    BFrame F;
    if (hipMemcpyAsync(&F, p_fr, sizeof F, hipMemcpyDeviceToHost, st) != hipSuccess || !dc.sync()) return ZLZ4_ERR_DEVICE;
    if (F.status < 0) return F.status;
    if (F.nb > 0x7FFFFFFFull) return ZLZ4F_ERR_FRAME_SIZE_WRONG;
    const uint32_t max_blocks = (uint32_t)F.nb;
    const size_t ws = bfd_layout(1, max_blocks, decode_flags, with_dict, want_size).bytes;
    DevBuf d_ws(ws, &dc);
    if (!d_ws.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    dc.launched();
    const BfDict one = {d_dict, &rec.d->dict_off, &rec.d->dict_len, 1u, nullptr};
    const BfDict *dd = with_dict ? &one : nullptr;
    const BfArrays a = {d_src, &r->src_off, &r->src_len, want_size ? nullptr : d_dst, want_size ? nullptr : &r->dst_off,
                        want_size ? nullptr : &r->dst_cap, &r->result, 1, max_blocks};
    const int32_t rc = want_size ? batch_frame_decompressed_size_impl(st, a, decode_flags, d_ws.p, ws, dd)
                                 : batch_decompress_frame_impl(st, a, decode_flags, d_ws.p, ws, dd);
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result)) return ZLZ4_ERR_DEVICE;
    return result;
}

}  // namespace

extern "C" {

int32_t zlz4f_batch_decompress_frame(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                     const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                     const uint64_t *d_dst_cap, int64_t *d_result, uint32_t nframes, uint32_t max_blocks,
                                     void *d_workspace, size_t workspace_bytes) {
    const BfArrays a = {d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_result, nframes, max_blocks};
    return batch_decompress_frame_impl(stream, a, 0, d_workspace, workspace_bytes);
}

int32_t zlz4f_batch_decompress_frame_ex(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                        const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                        const uint64_t *d_dst_cap, int64_t *d_result, uint32_t nframes, uint32_t max_blocks,
                                        uint32_t decode_flags, void *d_workspace, size_t workspace_bytes) {
    const BfArrays a = {d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_result, nframes, max_blocks};
    return batch_decompress_frame_impl(stream, a, decode_flags, d_workspace, workspace_bytes);
}

size_t zlz4f_batch_frame_decompressed_size_workspace(uint32_t nframes, uint32_t max_blocks) {
    return bfd_layout(nframes, max_blocks, 0, false, kQuery).bytes;
}

size_t zlz4f_batch_frame_decompressed_size_workspace_ex(uint32_t nframes, uint32_t max_blocks, uint32_t decode_flags) {
    return bfd_layout(nframes, max_blocks, decode_flags, false, kQuery).bytes;
}

int32_t zlz4f_batch_frame_decompressed_size(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                            const uint64_t *d_src_len, int64_t *d_size, uint32_t nframes,
                                            uint32_t max_blocks, void *d_workspace, size_t workspace_bytes) {
    const BfArrays a = {d_src, d_src_off, d_src_len, nullptr, nullptr, nullptr, d_size, nframes, max_blocks};
    return batch_frame_decompressed_size_impl(stream, a, 0, d_workspace, workspace_bytes);
}

int32_t zlz4f_batch_frame_decompressed_size_ex(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                               const uint64_t *d_src_len, int64_t *d_size, uint32_t nframes,
                                               uint32_t max_blocks, uint32_t decode_flags, void *d_workspace,
                                               size_t workspace_bytes) {
    const BfArrays a = {d_src, d_src_off, d_src_len, nullptr, nullptr, nullptr, d_size, nframes, max_blocks};
    return batch_frame_decompressed_size_impl(stream, a, decode_flags, d_workspace, workspace_bytes);
}

// one frame through zlz4f_batch_decompress_frame_ex / zlz4f_batch_frame_decompressed_size_ex (the result is the batch
// call's for that frame); synchronises `stream`
int64_t zlz4f_decompress_frame_device_ex(void *stream, const uint8_t *d_src, size_t n, uint8_t *d_dst, size_t cap,
                                         uint32_t decode_flags) {
    return single_frame_ex((hipStream_t)stream, d_src, n, d_dst, cap, decode_flags, false);
}

int64_t zlz4f_decompress_frame_ex(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, uint32_t decode_flags) {
    if (decode_flags & ~ZLZ4F_DECODE_LINKED) return ZLZ4F_ERR_PARAMETER_INVALID;
    if ((!src && n) || (!dst && cap)) return ZLZ4_ERR_INVALID_STATE;
    const ParsedHeader ph = parse_header(src, n);      // header errors need no device
    if (ph.size < 0) return ph.size;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return host_frame_call(src, n, dst, cap, cap, [&](const uint8_t *d_src, uint8_t *d_dst) {
        return single_frame_ex(nullptr, d_src, n, d_dst, cap, decode_flags, false);
    });
}

int64_t zlz4f_frame_decompressed_size_ex(const uint8_t *src, size_t n, uint32_t decode_flags) {
    if (decode_flags & ~ZLZ4F_DECODE_LINKED) return ZLZ4F_ERR_PARAMETER_INVALID;
    if (!src && n) return ZLZ4_ERR_INVALID_STATE;
    const ParsedHeader ph = parse_header(src, n);
    if (ph.size < 0) return ph.size;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    DevBuf d_src(n);
    if (!d_src.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    if (hipMemcpy(d_src.p, src, n, hipMemcpyHostToDevice) != hipSuccess) return ZLZ4_ERR_DEVICE;
    return single_frame_ex(nullptr, d_src.as<uint8_t>(), n, nullptr, 0, decode_flags, true);
}

// what zlz4f_decompress_frame returns into a destination that is large enough (the content checksum aside), host
// pointers: the frame is staged and queried as a batch of one; the block count for the table comes from a host walk of
// the chain (chain_blocks)
int64_t zlz4f_frame_decompressed_size(const uint8_t *src, size_t n) {
    if (!src && n) return ZLZ4_ERR_INVALID_STATE;
    const ParsedHeader ph = parse_header(src, n);      // header errors need no device
    if (ph.size < 0) return ph.size;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    const uint64_t nb = chain_blocks(src, n, ph);
    if (nb > 0xFFFFFFFFull) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    const uint32_t max_blocks = (uint32_t)nb;
    const size_t ws = zlz4f_batch_frame_decompressed_size_workspace(1, max_blocks);
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    DevBuf d_src(n, &dc);
    Staged<FrameRec> rec(&dc);
    DevBuf d_ws(ws, &dc);
    if (!d_src.p || !rec.d || !d_ws.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.src_len = n;
    dc.launched();
    if (!upload(d_src, src, n, st) || !rec.upload(st)) return ZLZ4_ERR_DEVICE;
    FrameRec *r = rec.d;
    const int32_t rc = zlz4f_batch_frame_decompressed_size(st, d_src.as<uint8_t>(), &r->src_off, &r->src_len, &r->result, 1,
                                                           max_blocks, d_ws.p, ws);
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result)) return ZLZ4_ERR_DEVICE;
    return result;
}

}  // extern "C"

// ====================================================================== dictionary frames
namespace {

// one lane per frame: the header's dictID (0 when the frame carries none), or the header's error
__global__ void k_bf_dict_id(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                             const uint64_t *__restrict__ src_len, uint32_t nframes, int64_t *__restrict__ dict_id) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const uint8_t *s = src + src_off[f];
    const ParsedHeader ph = frame_header(s, src_len[f]);
    if (ph.size < 0) { dict_id[f] = ph.size; return; }
    dict_id[f] = (ph.flg & 0x01u) ? (int64_t)zx_rd32(s + 6 + ((ph.flg & 0x08u) ? 8 : 0)) : 0;   // (inside the header)
}

// the host-pointer call of both entry points: the refusals are host arithmetic and come before the device check
int64_t host_compress_frame_dict(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const zlz4f_prefs *prefs,
                                 const uint8_t *dict, size_t dict_len, bool ex) {
    const zlz4f_prefs p = prefs ? *prefs : kDefaultPrefs;
    const int32_t refused = bfcd_refusal(p, 0, ex);
    if (refused != 0) return refused;
    if ((!src && n) || (!dst && cap) || (!dict && dict_len)) return ZLZ4_ERR_INVALID_STATE;
    const size_t bound = zlz4f_compress_frame_bound(n, &p);
    if (cap < bound) return ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;                                            // :363-366
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return with_dict_tail(dict, dict_len, [&](const uint8_t *d_dict, uint32_t D) {
        return host_frame_call(src, n, dst, cap, bound, [&](const uint8_t *d_src, uint8_t *d_dst) {
            const OneDict one = {d_dict, D, ex};
            return single_compress_frame(nullptr, d_src, n, d_dst, bound, p, 0, &one);
        });
    });
}

}  // namespace

extern "C" {

size_t zlz4f_batch_compress_frame_using_dict_workspace(uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs *prefs,
                                                       uint32_t batch_flags, uint32_t ndicts, uint64_t max_src_len,
                                                       uint32_t max_dict_len) {
    (void)batch_flags; (void)max_dict_len;
    return bfcd_layout(nframes, max_blocks, prefs ? *prefs : kDefaultPrefs, ndicts, max_src_len).bytes;
}

int32_t zlz4f_batch_compress_frame_using_dict(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                              const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                              const uint64_t *d_dst_cap, int64_t *d_result, uint32_t nframes,
                                              uint32_t max_blocks, const zlz4f_prefs *prefs, uint32_t batch_flags,
                                              const uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                                              uint32_t ndicts, const uint32_t *d_dict_idx, uint64_t max_src_len,
                                              uint32_t max_dict_len, void *d_workspace, size_t workspace_bytes) {
    const BfArrays a = {d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_result, nframes, max_blocks};
    const BfDict dd = {d_dict, d_dict_off, d_dict_len, ndicts, d_dict_idx};
    return batch_compress_frame_dict_impl(stream, a, prefs, batch_flags, dd, max_src_len, max_dict_len, d_workspace,
                                          workspace_bytes, false);
}

// the same, and the HC levels 3..9
size_t zlz4f_batch_compress_frame_using_dict_workspace_ex(uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs *prefs,
                                                          uint32_t batch_flags, uint32_t ndicts, uint64_t max_src_len,
                                                          uint32_t max_dict_len) {
    (void)batch_flags;
    const zlz4f_prefs p = prefs ? *prefs : kDefaultPrefs;
    return bfcd_layout(nframes, max_blocks, p, ndicts, max_src_len, max_dict_len, bfcd_hc(p, true)).bytes;
}

int32_t zlz4f_batch_compress_frame_using_dict_ex(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                                 const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                                 const uint64_t *d_dst_cap, int64_t *d_result, uint32_t nframes,
                                                 uint32_t max_blocks, const zlz4f_prefs *prefs, uint32_t batch_flags,
                                                 const uint8_t *d_dict, const uint64_t *d_dict_off,
                                                 const uint32_t *d_dict_len, uint32_t ndicts, const uint32_t *d_dict_idx,
                                                 uint64_t max_src_len, uint32_t max_dict_len, void *d_workspace,
                                                 size_t workspace_bytes) {
    const BfArrays a = {d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_result, nframes, max_blocks};
    const BfDict dd = {d_dict, d_dict_off, d_dict_len, ndicts, d_dict_idx};
    return batch_compress_frame_dict_impl(stream, a, prefs, batch_flags, dd, max_src_len, max_dict_len, d_workspace,
                                          workspace_bytes, true);
}

size_t zlz4f_batch_decompress_frame_using_dict_workspace(uint32_t nframes, uint32_t max_blocks) {
    return bfd_layout(nframes, max_blocks, ZLZ4F_DECODE_LINKED, true, kDecode).bytes;
}

int32_t zlz4f_batch_decompress_frame_using_dict(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                                const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                                const uint64_t *d_dst_cap, int64_t *d_result, uint32_t nframes,
                                                uint32_t max_blocks, const uint8_t *d_dict, const uint64_t *d_dict_off,
                                                const uint32_t *d_dict_len, uint32_t ndicts, const uint32_t *d_dict_idx,
                                                void *d_workspace, size_t workspace_bytes) {
    const BfArrays a = {d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_result, nframes, max_blocks};
    const BfDict dd = {d_dict, d_dict_off, d_dict_len, ndicts, d_dict_idx};
    return batch_decompress_frame_impl(stream, a, ZLZ4F_DECODE_LINKED, d_workspace, workspace_bytes, &dd);
}

size_t zlz4f_batch_frame_decompressed_size_using_dict_workspace(uint32_t nframes, uint32_t max_blocks) {
    return bfd_layout(nframes, max_blocks, ZLZ4F_DECODE_LINKED, true, kQuery).bytes;
}

int32_t zlz4f_batch_frame_decompressed_size_using_dict(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                                       const uint64_t *d_src_len, int64_t *d_size, uint32_t nframes,
                                                       uint32_t max_blocks, const uint32_t *d_dict_len, uint32_t ndicts,
                                                       const uint32_t *d_dict_idx, void *d_workspace,
                                                       size_t workspace_bytes) {
    const BfArrays a = {d_src, d_src_off, d_src_len, nullptr, nullptr, nullptr, d_size, nframes, max_blocks};
    const BfDict dd = {nullptr, nullptr, d_dict_len, ndicts, d_dict_idx};
    return batch_frame_decompressed_size_impl(stream, a, ZLZ4F_DECODE_LINKED, d_workspace, workspace_bytes, &dd);
}

int32_t zlz4f_batch_frame_dict_id(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                  int64_t *d_dict_id, uint32_t nframes) {
    if (nframes == 0) return 0;
    const BfArrays a = {d_src, d_src_off, d_src_len, nullptr, nullptr, nullptr, d_dict_id, nframes, 0};
    if (bf_args_refused(kArgSrc | kArgAligned, a)) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipLaunchKernelGGL(k_bf_dict_id, dim3(bf_grid(nframes, 256)), dim3(256), 0, (hipStream_t)stream, d_src, d_src_off,
                       d_src_len, nframes, d_dict_id);
    return hipGetLastError() == hipSuccess ? 0 : ZLZ4_ERR_DEVICE;
}

// host pointers: the frame, the dictionary's tail and a batch of one (zlz4f_compress_frame_ex)
int64_t zlz4f_compress_frame_using_dict(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const zlz4f_prefs *prefs,
                                        const uint8_t *dict, size_t dict_len) {
    return host_compress_frame_dict(src, n, dst, cap, prefs, dict, dict_len, false);
}

int64_t zlz4f_compress_frame_using_dict_ex(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const zlz4f_prefs *prefs,
                                           const uint8_t *dict, size_t dict_len) {
    return host_compress_frame_dict(src, n, dst, cap, prefs, dict, dict_len, true);
}

int64_t zlz4f_decompress_frame_using_dict(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const uint8_t *dict,
                                          size_t dict_len) {
    if ((!src && n) || (!dst && cap) || (!dict && dict_len)) return ZLZ4_ERR_INVALID_STATE;
    const ParsedHeader ph = parse_header(src, n);      // header errors need no device
    if (ph.size < 0) return ph.size;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return with_dict_tail(dict, dict_len, [&](const uint8_t *d_dict, uint32_t D) {
        return host_frame_call(src, n, dst, cap, cap, [&](const uint8_t *d_src, uint8_t *d_dst) {
            return single_frame_ex(nullptr, d_src, n, d_dst, cap, ZLZ4F_DECODE_LINKED, false, true, d_dict, D);
        });
    });
}

// ---- frame prefix decoding (include/zlz4_amd.h): d_dst_cap[f] = bytes wanted = slot size; one
// launch of k_bfp_decode, no workspace.  The plain call is the dictionary call without dictionaries.
int32_t zlz4f_batch_decompress_frame_prefix_using_dict(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                                       const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                                       const uint64_t *d_dst_cap, int64_t *d_result, uint32_t nframes,
                                                       const uint8_t *d_dict, const uint64_t *d_dict_off,
                                                       const uint32_t *d_dict_len, uint32_t ndicts,
                                                       const uint32_t *d_dict_idx) {
    if (nframes == 0) return 0;
    const BfArrays a = {d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_result, nframes, 0};
    const BfDict dd = {d_dict, d_dict_off, d_dict_len, ndicts, d_dict_idx};
    // (d_dict may be null: every dictionary empty)
    if (bf_args_refused(kArgSrc | kArgDst | kArgDictLen | kArgDictOff | kArgAligned, a, &dd)) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_bfp_decode_dict((hipStream_t)stream, d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_result,
                                       nframes, d_dict, d_dict_off, d_dict_len, ndicts, d_dict_idx);
}

int32_t zlz4f_batch_decompress_frame_prefix(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                            const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                            const uint64_t *d_dst_cap, int64_t *d_result, uint32_t nframes) {
    return zlz4f_batch_decompress_frame_prefix_using_dict(stream, d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap,
                                                          d_result, nframes, nullptr, nullptr, nullptr, 0, nullptr);
}

// host pointers: the frame, the dictionary's tail and a batch of one.  dst_cap == 0 needs no destination.
int64_t zlz4f_decompress_frame_prefix_using_dict(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const uint8_t *dict,
                                                 size_t dict_len) {
    if ((!src && n) || (!dst && cap) || (!dict && dict_len)) return ZLZ4_ERR_INVALID_STATE;
    const ParsedHeader ph = parse_header(src, n);      // header errors need no device
    if (ph.size < 0) return ph.size;
    if (cap == 0) return 0;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return with_dict_tail(dict, dict_len, [&](const uint8_t *d_dict, uint32_t D) {
        return host_frame_call(src, n, dst, cap, cap, [&](const uint8_t *d_src, uint8_t *d_dst) -> int64_t {
            hipStream_t st = nullptr;
            DeviceCall dc(st);
            struct Rec { FrameRec f; uint64_t dict_off; uint32_t dict_len; };
            Staged<Rec> rec(&dc);
            if (!rec.d) return ZLZ4F_ERR_ALLOCATION_FAILED;
            rec.h.f.src_len = n; rec.h.f.dst_cap = cap; rec.h.dict_len = D;
            dc.launched();
            if (!rec.upload(st)) return ZLZ4_ERR_DEVICE;
            FrameRec *r = &rec.d->f;
            const int32_t rc = zlz4f_batch_decompress_frame_prefix_using_dict(st, d_src, &r->src_off, &r->src_len, d_dst,
                                                                              &r->dst_off, &r->dst_cap, &r->result, 1, d_dict,
                                                                              &rec.d->dict_off, &rec.d->dict_len, D ? 1u : 0u,
                                                                              nullptr);
            if (rc != 0) return rc;
            int64_t result = 0;
            if (!read_result(dc, &r->result, result)) return ZLZ4_ERR_DEVICE;
            return result;
        });
    });
}

int64_t zlz4f_decompress_frame_prefix(const uint8_t *src, size_t n, uint8_t *dst, size_t cap) {
    return zlz4f_decompress_frame_prefix_using_dict(src, n, dst, cap, nullptr, 0);
}

int64_t zlz4f_frame_decompressed_size_using_dict(const uint8_t *src, size_t n, size_t dict_len) {
    if (!src && n) return ZLZ4_ERR_INVALID_STATE;
    const ParsedHeader ph = parse_header(src, n);
    if (ph.size < 0) return ph.size;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    DevBuf d_src(n);
    if (!d_src.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    if (hipMemcpy(d_src.p, src, n, hipMemcpyHostToDevice) != hipSuccess) return ZLZ4_ERR_DEVICE;
    return single_frame_ex(nullptr, d_src.as<uint8_t>(), n, nullptr, 0, ZLZ4F_DECODE_LINKED, true, true, nullptr,
                           (uint32_t)dict_tail(dict_len));
}

}  // extern "C"

// ====================================================================== frame index and range decoding
// zlz4f_batch_frame_index keeps what the size query computes and drops -- the per-block decoded sizes -- as a table of
// (position, decoded offset) per block; zlz4f_batch_decompress_frame_range decodes the blocks that overlap [a, b) through
// the block decoders, one item (= one block of one range) per wavefront.  The index is the caller's data: k_bfr_range and
// k_bfr_expand check every entry they use against the frame before a position becomes an address.
namespace {

// k_bfq_total's status of frame F (n bytes long) over the same entries in the same order; wave-uniform, 0 = no error
__device__ inline int64_t bfi_status(const BFrame &F, uint32_t max_blocks, uint32_t lane, const uint32_t *__restrict__ data_len,
                                     const uint32_t *__restrict__ flags, const int64_t *__restrict__ sizes,
                                     const uint32_t *__restrict__ cks_ok, uint64_t n) {
    if (F.status < 0) return F.status;                                                 // :547
    if (!bf_fits(F, max_blocks)) return ZLZ4_ERR_INVALID_STATE;
    int64_t out = 0;
    const bool bc = (F.flg & 0x10u) != 0;
    unsigned long long bad = ~0ull;                                   // this lane's first failing block
    int32_t code = 0;
    for (uint64_t j = lane; j < F.nb && bad == ~0ull; j += 64u) {
        const uint64_t i = F.base + j;
        int32_t err = 0;
        if (bc && cks_ok[i] == 2u) err = ZLZ4F_ERR_FRAME_SIZE_WRONG;                   // :591
        else if (bc && cks_ok[i] == 0u) err = ZLZ4F_ERR_BLOCK_CHECKSUM_INVALID;        // :596
        else if (!(flags[i] & kBlkStored) && data_len[i] != 0 && sizes[i] < 0) err = ZLZ4F_ERR_DECOMPRESSION_FAILED;   // :611
        if (err) { bad = j; code = err; }
    }
    unsigned long long first = bad;
    for (uint32_t d = 32u; d >= 1u; d >>= 1) {
        const unsigned long long o = __shfl_xor(first, (int)d);
        first = o < first ? o : first;
    }
    if (first != ~0ull) out = (int64_t)(int32_t)zlz4::rdlane((uint32_t)code, zlz4::first_lane(zlz4::ballot(bad == first)));
    if (!out) out = F.err;
    if (!out && (F.flg & 0x04u) && F.end + 4 > n) out = ZLZ4F_ERR_FRAME_SIZE_WRONG;    // :626
    return out;
}

// The index entries of frame F's nb blocks, 64 per step with a shuffle prefix sum of their sizes (k_frame_plan's scan):
// entry j = { the block's header word, counted from the byte `so` of d_src; run + the sizes in front of it }.  e == nullptr
// writes nothing.  run advances by the frame's decoded size; -> where the chain ended (head for a frame without blocks).
__device__ inline uint64_t bfi_entries(const BFrame &F, uint32_t lane, const uint64_t *__restrict__ data_off,
                                       const uint32_t *__restrict__ data_len, const uint32_t *__restrict__ flags,
                                       const int64_t *__restrict__ sizes, uint64_t so, uint64_t head,
                                       zlz4f_index_entry *__restrict__ e, uint64_t &run) {
    uint64_t end_pos = head;                                          // (no block: the chain ends behind the header)
    for (uint64_t b0 = 0; b0 < F.nb; b0 += 64u) {
        const uint64_t j = b0 + lane, i = F.base + j;
        uint64_t sz = 0;
        if (j < F.nb) sz = (flags[i] & kBlkStored) ? data_len[i] : (data_len[i] != 0 ? (uint64_t)sizes[i] : 0u);
        uint64_t incl = sz;                                           // inclusive scan over the 64 lanes
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t lo = __shfl_up((uint32_t)incl, d), hi = __shfl_up((uint32_t)(incl >> 32), d);
            if (lane >= d) incl += ((uint64_t)hi << 32) | lo;
        }
        if (j < F.nb) {
            if (e) {
                zlz4f_index_entry E;
                E.pos = data_off[i] - so - 4u;
                E.dec = run + incl - sz;
                e[j] = E;
            }
            if (j + 1u == F.nb) end_pos = data_off[i] - so + data_len[i] + ((flags[i] & kBlkCks) ? 4u : 0u);
        }
        run += ((uint64_t)zlz4::rdlane((uint32_t)(incl >> 32), 63) << 32) | zlz4::rdlane((uint32_t)incl, 63);
    }
    const uint32_t owner = F.nb ? (uint32_t)((F.nb - 1u) & 63u) : 0u;                  // the lane that saw the last block
    return ((uint64_t)zlz4::rdlane((uint32_t)(end_pos >> 32), owner) << 32) | zlz4::rdlane((uint32_t)end_pos, owner);
}

// one wavefront per frame: the status, then -- no error -- the nb + 1 index entries
__global__ __launch_bounds__(256) void k_bfi_index(const BFrame *__restrict__ fr, uint32_t nframes, uint32_t max_blocks,
                                                   const uint64_t *__restrict__ data_off, const uint32_t *__restrict__ data_len,
                                                   const uint32_t *__restrict__ flags, const int64_t *__restrict__ sizes,
                                                   const uint32_t *__restrict__ cks_ok, const uint64_t *__restrict__ src_off,
                                                   const uint64_t *__restrict__ src_len, zlz4f_index_entry *__restrict__ index,
                                                   const uint64_t *__restrict__ idx_off, const uint64_t *__restrict__ idx_cap,
                                                   int64_t *__restrict__ result) {
    const uint32_t f = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (f >= nframes) return;
    const BFrame F = fr[f];
    int64_t out = bfi_status(F, max_blocks, lane, data_len, flags, sizes, cks_ok, src_len[f]);
    if (!out && F.nb + 1u > idx_cap[f]) out = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
    if (out) { if (lane == 0) result[f] = out; return; }
    zlz4f_index_entry *e = index + idx_off[f];
    uint64_t run = 0;
    const uint64_t end_pos = bfi_entries(F, lane, data_off, data_len, flags, sizes, src_off[f], (uint64_t)F.status, e, run);
    if (lane == 0) {
        zlz4f_index_entry E;
        E.pos = end_pos;
        E.dec = run;
        e[F.nb] = E;
        result[f] = (int64_t)F.nb;
    }
}

// ------------------------------------------------------------------ ranges
// what k_bfr_range leaves per range.  status < 0: the range's result; else n items (n == 0: the empty range, result 0)
struct BRange {
    uint64_t n;         // items = k1 - k0 + 1
    uint64_t base;      // first item (exclusive scan of n)
    uint64_t k0;        // first block
    uint64_t a, b;      // a', b'
    uint64_t d0;        // dec[k0] (the empty range: a')
    int64_t status;
    uint32_t bc;        // FLG 0x10 of the frame's header
    uint32_t pad;
};

__device__ __forceinline__ bool bfr_fits(const BRange &G, uint32_t max_items) { return G.n == 0 || G.base + G.n <= max_items; }

// the block that holds decoded byte t: the last entry k of 0..nb with dec[k] <= t (bisection for the first entry above t).
// ~0 when entry 0 is already above t.  On a sorted index with t < dec[nb] the block is < nb and does not decode to nothing.
__host__ __device__ inline uint64_t bfr_block_of(const zlz4f_index_entry *e, uint64_t nb, uint64_t t) {
    uint64_t lo = 0, hi = nb + 1u;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (e[mid].dec <= t) lo = mid + 1u; else hi = mid;
    }
    return lo - 1u;
}

// a', b', k0, k1 of range R from the index alone; false = nothing to decode (frame / a > b / index status / a' == b') or
// the entries found are no blocks (an index that is not sorted)
struct BfrSpan { uint64_t a, b, k0, k1; };
__device__ inline bool bfr_span(const zlz4f_range &R, const zlz4f_index_entry *__restrict__ index,
                                const uint64_t *__restrict__ idx_off, const int64_t *__restrict__ idx_n, uint32_t nframes,
                                BfrSpan &s, const zlz4f_index_entry *&e, uint64_t &nb) {
    s = BfrSpan{0, 0, 0, 0};
    if (R.frame >= nframes || R.a > R.b || idx_n[R.frame] < 0) return false;
    nb = (uint64_t)idx_n[R.frame];
    e = index + idx_off[R.frame];
    const uint64_t S = e[nb].dec;
    s.a = R.a < S ? R.a : S;
    s.b = R.b < S ? R.b : S;
    if (s.a == s.b) return false;
    s.k0 = bfr_block_of(e, nb, s.a);
    s.k1 = bfr_block_of(e, nb, s.b - 1u);
    return s.k0 < nb && s.k1 < nb && s.k0 <= s.k1 && e[s.k0].dec <= s.a;
}

// exclusive scan of one value per thread over the one workgroup of 1024 threads (k_bf_scan's LDS scan); -> the sum in
// front of thread t, `total` = the sum of all
__device__ inline uint64_t bfr_wg_scan(uint64_t s, uint64_t *part, uint64_t &total) {
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

// plan, one lane per range: dst_cap[r] = the slot size; dst_off[r] holds the item count until k_bfr_plan_scan replaces it
__global__ void k_bfr_plan(const zlz4f_index_entry *__restrict__ index, const uint64_t *__restrict__ idx_off,
                           const int64_t *__restrict__ idx_n, uint32_t nframes, const zlz4f_range *__restrict__ range,
                           uint32_t nranges, uint64_t *__restrict__ dst_off, uint64_t *__restrict__ dst_cap) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nranges) return;
    BfrSpan s;
    const zlz4f_index_entry *e = nullptr;
    uint64_t nb = 0;
    const bool ok = bfr_span(range[r], index, idx_off, idx_n, nframes, s, e, nb);
    dst_cap[r] = ok ? s.b - e[s.k0].dec : 0u;
    dst_off[r] = ok ? s.k1 - s.k0 + 1u : 0u;
}

// one workgroup: dst_off = the exclusive scan of the slot sizes rounded up to `align`; totals = { arena bytes, items }
__global__ __launch_bounds__(1024) void k_bfr_plan_scan(uint32_t nranges, uint64_t align, uint64_t *__restrict__ dst_off,
                                                        const uint64_t *__restrict__ dst_cap, uint64_t *__restrict__ totals) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (nranges + 1023u) / 1024u;
    const uint64_t b0 = (uint64_t)t * chunk;
    const uint32_t lo = b0 < nranges ? (uint32_t)b0 : nranges;
    const uint32_t hi = b0 + chunk < nranges ? (uint32_t)(b0 + chunk) : nranges;
    auto slot = [&](uint64_t c) -> uint64_t { return (c + (align - 1u)) & ~(align - 1u); };
    uint64_t bytes = 0, items = 0;
    for (uint32_t r = lo; r < hi; r++) { bytes += slot(dst_cap[r]); items += dst_off[r]; }
    uint64_t tot_bytes, tot_items;
    uint64_t run = bfr_wg_scan(bytes, part, tot_bytes);
    (void)bfr_wg_scan(items, part, tot_items);
    for (uint32_t r = lo; r < hi; r++) { dst_off[r] = run; run += slot(dst_cap[r]); }
    if (t == 0) { totals[0] = tot_bytes; totals[1] = tot_items; }
}

// decode step 1, one wavefront per range: statuses 1-3 of include/zlz4_amd.h and the item count.  Everything up to the
// chain check depends on the range alone (wave-uniform); the lanes share the pairs (k, k + 1) of the chain.
__global__ __launch_bounds__(256) void k_bfr_range(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                   const uint64_t *__restrict__ src_len,
                                                   const zlz4f_index_entry *__restrict__ index,
                                                   const uint64_t *__restrict__ idx_off, const int64_t *__restrict__ idx_n,
                                                   uint32_t nframes, const zlz4f_range *__restrict__ range,
                                                   const uint64_t *__restrict__ dst_cap, uint32_t nranges,
                                                   BRange *__restrict__ rg) {
    const uint32_t r = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (r >= nranges) return;
    const zlz4f_range R = range[r];
    BRange G = {};
    int64_t st = 0;
    if (R.frame >= nframes || R.a > R.b || R.reserved != 0) st = ZLZ4_ERR_INVALID_STATE;
    else if (idx_n[R.frame] < 0) st = idx_n[R.frame];
    else {
        const uint64_t n = src_len[R.frame];
        const uint8_t *s = src + src_off[R.frame];
        const ParsedHeader ph = parse_header(s, n < 19u ? (size_t)n : 19u);    // (reads the bytes it is given, no more)
        if (ph.size < 0) st = ph.size;
        else {
            BfrSpan sp;
            const zlz4f_index_entry *e = nullptr;
            uint64_t nb = 0;
            const bool found = bfr_span(R, index, idx_off, idx_n, nframes, sp, e, nb);
            G.a = sp.a; G.b = sp.b; G.d0 = sp.a;
            G.bc = (ph.flg & 0x10u) ? 1u : 0u;
            if (e[0].pos != (uint64_t)ph.size) st = ZLZ4_ERR_INVALID_STATE;
            else if (sp.a != sp.b) {
                bool bad = !found;
                if (found) {
                    for (uint64_t k = sp.k0 + lane; k <= sp.k1; k += 64u) {
                        const zlz4f_index_entry E = e[k], N = e[k + 1u];
                        if (N.pos <= E.pos || E.pos > n || n - E.pos < 4u || N.pos > n || N.dec < E.dec ||
                            N.dec - E.dec > ph.block_size)
                            bad = true;
                    }
                    if (e[sp.k1].dec >= sp.b || e[sp.k1 + 1u].dec < sp.b) bad = true;
                }
                if (zlz4::ballot(bad) != 0) st = ZLZ4_ERR_INVALID_STATE;
                else if (dst_cap[r] < sp.b - e[sp.k0].dec) st = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
                else { G.n = sp.k1 - sp.k0 + 1u; G.k0 = sp.k0; G.d0 = e[sp.k0].dec; }
            }
        }
    }
    G.status = st;
    if (lane == 0) rg[r] = G;
}

// k_bf_scan over the ranges' item counts
__global__ __launch_bounds__(1024) void k_bfr_scan(BRange *__restrict__ rg, uint32_t nranges) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (nranges + 1023u) / 1024u;
    const uint64_t b0 = (uint64_t)t * chunk;
    const uint32_t lo = b0 < nranges ? (uint32_t)b0 : nranges;
    const uint32_t hi = b0 + chunk < nranges ? (uint32_t)(b0 + chunk) : nranges;
    uint64_t s = 0, total;
    for (uint32_t r = lo; r < hi; r++) s += rg[r].n;
    uint64_t run = bfr_wg_scan(s, part, total);
    for (uint32_t r = lo; r < hi; r++) { rg[r].base = run; run += rg[r].n; }
}

// per-item error marks of k_bfr_expand, in the order k_bfr_finish reports them around the block checksum
constexpr uint32_t kItemChain = 1u, kItemStored = 2u;

// the item tables: what the block decoders, k_bfd_verify and the copy read.  A length of 0 keeps an item out of a launch.
struct BfrTables {
    uint64_t *data_off, *cks_off, *out_off;
    uint32_t *data_len, *flags, *f_len, *f_cap, *p_len, *p_cap, *c_len, *ierr;
};

// decode step 3, one lane per item: its range (the last whose base is <= i, as k_bfc_desc), block k = k0 + (i - base), the
// chain check of that block against the frame, and the item's row in every table.  k_bfr_range has checked that the header
// word and everything up to pos[k + 1] lie inside the frame; the block's data is only used when it ends at pos[k + 1].
__global__ void k_bfr_expand(const BRange *__restrict__ rg, uint32_t nranges, uint32_t max_items,
                             const zlz4f_range *__restrict__ range, const uint8_t *__restrict__ src,
                             const uint64_t *__restrict__ src_off, const zlz4f_index_entry *__restrict__ index,
                             const uint64_t *__restrict__ idx_off, const uint64_t *__restrict__ dst_off, BfrTables T) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_items; i += gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = nranges;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (rg[mid].base <= i) lo = mid + 1u; else hi = mid;
        }
        uint64_t d_off = 0, c_off = 0, o_off = 0;
        uint32_t d_len = 0, fl = 0, f_len = 0, f_cap = 0, p_len = 0, p_cap = 0, c_len = 0, ierr = 0;
        if (lo > 0) {
            const uint32_t r = lo - 1u;
            const BRange G = rg[r];
            const uint64_t j = i - G.base;
            if (j < G.n && G.status == 0 && bfr_fits(G, max_items)) {
                const uint32_t f = range[r].frame;
                const zlz4f_index_entry *e = index + idx_off[f];
                const uint64_t k = G.k0 + j;
                const zlz4f_index_entry E = e[k], N = e[k + 1u];
                const uint64_t so = src_off[f];
                const BlockWord w = block_word(zx_rd32(src + so + E.pos));
                const uint32_t sz = w.size;
                if (w.end_mark || E.pos + 4u + sz + (G.bc ? 4u : 0u) != N.pos) ierr = kItemChain;  // (the end mark is no block)
                else {
                    const uint32_t step = (uint32_t)(N.dec - E.dec);             // <= the block size (k_bfr_range)
                    const uint64_t left = G.b - E.dec;                           // > 0: dec[k] <= dec[k1] < b'
                    const uint32_t want = left < step ? (uint32_t)left : step;
                    d_off = so + E.pos + 4u;
                    d_len = sz;
                    o_off = dst_off[r] + (E.dec - G.d0);
                    if (G.bc) { fl |= kBlkCks; c_off = d_off + sz; }
                    if (w.stored) {
                        fl |= kBlkStored;
                        if (sz != step) ierr = kItemStored; else c_len = want;
                    } else if (want == step) { f_len = sz; f_cap = step; }
                    else { p_len = sz; p_cap = want; }
                }
            }
        }
        T.data_off[i] = d_off; T.cks_off[i] = c_off; T.out_off[i] = o_off;
        T.data_len[i] = d_len; T.flags[i] = fl; T.f_len[i] = f_len; T.f_cap[i] = f_cap; T.p_len[i] = p_len;
        T.p_cap[i] = p_cap; T.c_len[i] = c_len; T.ierr[i] = ierr;
    }
}

// decode step 6, one workgroup per item: the wanted part of a stored block
__global__ __launch_bounds__(256) void k_bfr_copy(const uint8_t *__restrict__ src, const uint64_t *__restrict__ data_off,
                                                   const uint32_t *__restrict__ c_len, const uint64_t *__restrict__ out_off,
                                                   uint8_t *__restrict__ dst) {
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    const uint32_t n = c_len[i];
    if (n == 0) return;
    const uint8_t *p = src + data_off[i];
    uint8_t *o = dst + out_off[i];
    for (uint32_t k = t * 16u; k + 16u <= n; k += 256u * 16u) zlz4::st128(o + k, zlz4::ld128(p + k));
    const uint32_t t0 = n & ~15u;
    if (t < 16u && t0 + t < n) o[t0 + t] = p[t0 + t];
}

// decode step 7, one wavefront per range: the first failing item in block order (a min-reduction by index), else b' - a'
__global__ __launch_bounds__(256) void k_bfr_finish(const BRange *__restrict__ rg, uint32_t nranges, uint32_t max_items,
                                                    BfrTables T, const uint32_t *__restrict__ cks_ok,
                                                    const int64_t *__restrict__ sizes_f, const int64_t *__restrict__ sizes_p,
                                                    uint64_t *__restrict__ skip, int64_t *__restrict__ result) {
    const uint32_t r = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (r >= nranges) return;
    const BRange G = rg[r];
    int64_t out = G.status;
    if (!out && !bfr_fits(G, max_items)) out = ZLZ4_ERR_INVALID_STATE;
    if (!out) {
        unsigned long long bad = ~0ull;
        int32_t code = 0;
        for (uint64_t j = lane; j < G.n && bad == ~0ull; j += 64u) {
            const uint64_t i = G.base + j;
            int32_t err = 0;
            if (T.ierr[i] == kItemChain) err = ZLZ4_ERR_INVALID_STATE;
            else if ((T.flags[i] & kBlkCks) && cks_ok[i] != 1u) err = ZLZ4F_ERR_BLOCK_CHECKSUM_INVALID;
            else if (T.ierr[i] == kItemStored) err = ZLZ4_ERR_INVALID_STATE;
            else if (T.f_len[i] != 0 && sizes_f[i] != (int64_t)T.f_cap[i]) err = ZLZ4F_ERR_DECOMPRESSION_FAILED;
            else if (T.p_len[i] != 0 && sizes_p[i] != (int64_t)T.p_cap[i]) err = ZLZ4F_ERR_DECOMPRESSION_FAILED;
            if (err) { bad = j; code = err; }
        }
        unsigned long long first = bad;
        for (uint32_t d = 32u; d >= 1u; d >>= 1) {
            const unsigned long long o = __shfl_xor(first, (int)d);
            first = o < first ? o : first;
        }
        if (first != ~0ull) out = (int64_t)(int32_t)zlz4::rdlane((uint32_t)code, zlz4::first_lane(zlz4::ballot(bad == first)));
    }
    if (lane == 0) {
        result[r] = out ? out : (int64_t)(G.b - G.a);
        skip[r] = out ? 0u : G.a - G.d0;
    }
}

// the range decode's workspace: the range records, the item tables, the decoders' results
struct BfrLayout {
    Region<BRange> ranges;
    Region<uint64_t> data_off, cks_off, out_off;
    Region<uint32_t> data_len, flags, cks_ok, f_len, f_cap, p_len, p_cap, c_len, ierr;
    Region<int64_t> sizes_f, sizes_p;
    // the items' dictionary descriptors (the file range call with dictionaries)
    Region<uint64_t> e_off;
    Region<uint32_t> e_len;
    size_t bytes = 0;
};

BfrLayout bfr_layout(uint32_t nranges, uint32_t max_items, void *ws = nullptr, bool dict = false) {
    const size_t m = max_items;
    BfrLayout L;
    Carver c{static_cast<uint8_t *>(ws)};
    c.take(nranges, L.ranges);
    c.take(m, L.data_off, L.cks_off, L.out_off);
    c.take(m, L.data_len, L.flags, L.cks_ok, L.f_len, L.f_cap, L.p_len, L.p_cap, L.c_len, L.ierr);
    c.take(m, L.sizes_f, L.sizes_p);
    if (dict) { c.take(m, L.e_off); c.take(m, L.e_len); }
    L.bytes = c.bytes;
    return L;
}

}  // namespace

extern "C" {

size_t zlz4f_batch_frame_index_workspace(uint32_t nframes, uint32_t max_blocks) {
    return bfd_layout(nframes, max_blocks, 0, false, kQuery).bytes;
}

// the size query's launch sequence with k_bfi_index in k_bfq_total's place; its refusals, then the device
int32_t zlz4f_batch_frame_index(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                zlz4f_index_entry *d_index, const uint64_t *d_idx_off, const uint64_t *d_idx_cap,
                                int64_t *d_result, uint32_t nframes, uint32_t max_blocks, void *d_workspace,
                                size_t workspace_bytes) {
    if (nframes == 0) return 0;
    const BfArrays a = {d_src, d_src_off, d_src_len, nullptr, nullptr, nullptr, d_result, nframes, max_blocks};
    const BfdLayout L = bfd_layout(nframes, max_blocks, 0, false, kQuery, d_workspace);
    if (!d_index || !d_idx_off || !d_idx_cap || bf_misaligned(d_index, 8) || bf_misaligned(d_idx_off, 8) ||
        bf_misaligned(d_idx_cap, 8) || bf_args_refused(kArgSrc | kArgWs | kArgWs16, a, nullptr, 0, d_workspace, workspace_bytes, L.bytes))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (bfd_prelude(st, a, false, nullptr, L) != 0) return ZLZ4_ERR_DEVICE;
    if (max_blocks) {
        hipLaunchKernelGGL(k_bfq_len, dim3(bf_grid(max_blocks, 256, 4096)), dim3(256), 0, st, L.data_len, L.flags, max_blocks,
                           L.dec_len);
        if (zlz4_launch_decompressed_size(st, d_src, L.data_off, L.dec_len, nullptr, L.sizes, max_blocks) != 0)
            return ZLZ4_ERR_DEVICE;
    }
    hipLaunchKernelGGL(k_bfi_index, dim3(bf_grid(nframes, 4)), dim3(256), 0, st, L.frames, nframes, max_blocks, L.data_off,
                       L.data_len, L.flags, L.sizes, L.cks_ok, d_src_off, d_src_len, d_index, d_idx_off, d_idx_cap, d_result);
    return hipGetLastError() == hipSuccess ? 0 : ZLZ4_ERR_DEVICE;
}

int32_t zlz4f_batch_plan_frame_ranges(void *stream, const zlz4f_index_entry *d_index, const uint64_t *d_idx_off,
                                      const int64_t *d_idx_n, uint32_t nframes, const zlz4f_range *d_range, uint32_t nranges,
                                      uint32_t align, uint64_t *d_dst_off, uint64_t *d_dst_cap, uint64_t *d_totals) {
    if (align > 4096u || (align & (align - 1u))) return ZLZ4_ERR_INVALID_STATE;      // 0, 1 or a power of two up to 4096
    if (!d_totals || bf_misaligned(d_totals, 8)) return ZLZ4_ERR_INVALID_STATE;
    if (nranges && (!d_range || !d_dst_off || !d_dst_cap || (nframes && (!d_index || !d_idx_off || !d_idx_n)))) return ZLZ4_ERR_INVALID_STATE;
    if (bf_misaligned(d_index, 8) || bf_misaligned(d_idx_off, 8) || bf_misaligned(d_idx_n, 8) || bf_misaligned(d_range, 8) ||
        bf_misaligned(d_dst_off, 8) || bf_misaligned(d_dst_cap, 8))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (nranges)
        hipLaunchKernelGGL(k_bfr_plan, dim3(bf_grid(nranges, 256)), dim3(256), 0, st, d_index, d_idx_off, d_idx_n, nframes,
                           d_range, nranges, d_dst_off, d_dst_cap);
    hipLaunchKernelGGL(k_bfr_plan_scan, dim3(1), dim3(1024), 0, st, nranges, (uint64_t)(align ? align : 1u), d_dst_off,
                       d_dst_cap, d_totals);
    return hipGetLastError() == hipSuccess ? 0 : ZLZ4_ERR_DEVICE;
}

size_t zlz4f_batch_decompress_frame_range_workspace(uint32_t nranges, uint32_t max_items) {
    return bfr_layout(nranges, max_items).bytes;
}

int32_t zlz4f_batch_decompress_frame_range(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                           const uint64_t *d_src_len, const zlz4f_index_entry *d_index,
                                           const uint64_t *d_idx_off, const int64_t *d_idx_n, uint32_t nframes,
                                           const zlz4f_range *d_range, uint8_t *d_dst, const uint64_t *d_dst_off,
                                           const uint64_t *d_dst_cap, uint64_t *d_skip, int64_t *d_result, uint32_t nranges,
                                           uint32_t max_items, void *d_workspace, size_t workspace_bytes) {
    if (nranges == 0) return 0;
    const BfrLayout L = bfr_layout(nranges, max_items, d_workspace);
    if (!d_range || !d_dst_off || !d_dst_cap || !d_skip || !d_result || (max_items && !d_dst) ||
        (nframes && (!d_src || !d_src_off || !d_src_len || !d_index || !d_idx_off || !d_idx_n)))
        return ZLZ4_ERR_INVALID_STATE;
    if (bf_misaligned(d_src_off, 8) || bf_misaligned(d_src_len, 8) || bf_misaligned(d_index, 8) || bf_misaligned(d_idx_off, 8) ||
        bf_misaligned(d_idx_n, 8) || bf_misaligned(d_range, 8) || bf_misaligned(d_dst_off, 8) || bf_misaligned(d_dst_cap, 8) ||
        bf_misaligned(d_skip, 8) || bf_misaligned(d_result, 8))
        return ZLZ4_ERR_INVALID_STATE;
    if (!d_workspace || workspace_bytes < L.bytes || bf_misaligned(d_workspace, 16)) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t m = max_items, gr = bf_grid(nranges, 4);
    const BfrTables T = {L.data_off, L.cks_off, L.out_off, L.data_len, L.flags, L.f_len, L.f_cap, L.p_len, L.p_cap, L.c_len, L.ierr};
    hipLaunchKernelGGL(k_bfr_range, dim3(gr), dim3(256), 0, st, d_src, d_src_off, d_src_len, d_index, d_idx_off, d_idx_n, nframes,
                       d_range, d_dst_cap, nranges, L.ranges);
    hipLaunchKernelGGL(k_bfr_scan, dim3(1), dim3(1024), 0, st, L.ranges, nranges);
    if (m) {
        hipLaunchKernelGGL(k_bfr_expand, dim3(bf_grid(m, 256, 4096)), dim3(256), 0, st, L.ranges, nranges, m, d_range, d_src,
                           d_src_off, d_index, d_idx_off, d_dst_off, T);
        hipLaunchKernelGGL(k_bfd_verify, dim3(bf_grid(m, 64)), dim3(64), 0, st, d_src, L.data_off, L.data_len, L.flags,
                           L.cks_off, m, L.cks_ok);
        if (zlz4_launch_decompress_safe(st, d_src, L.data_off, L.f_len, d_dst, L.out_off, L.f_cap, L.sizes_f, m) != 0 ||
            zlz4_launch_decompress_safe_prefix(st, d_src, L.data_off, L.p_len, d_dst, L.out_off, L.p_cap, L.sizes_p, m) != 0)
            return ZLZ4_ERR_DEVICE;
        hipLaunchKernelGGL(k_bfr_copy, dim3(m), dim3(256), 0, st, d_src, L.data_off, L.c_len, L.out_off, d_dst);
    }
    hipLaunchKernelGGL(k_bfr_finish, dim3(gr), dim3(256), 0, st, L.ranges, nranges, m, T, L.cks_ok, L.sizes_f, L.sizes_p, d_skip,
                       d_result);
    return hipGetLastError() == hipSuccess ? 0 : ZLZ4_ERR_DEVICE;
}

// One frame from host memory: the index, the plan and the range decode as a batch of one.  The index is built on every call.
int64_t zlz4f_decompress_frame_range(const uint8_t *src, size_t n, uint64_t a, uint64_t b, uint8_t *dst, size_t cap) {
    if ((!src && n) || (!dst && cap)) return ZLZ4_ERR_INVALID_STATE;
    const ParsedHeader ph = parse_header(src, n);      // header errors need no device
    if (ph.size < 0) return ph.size;
    if (a > b) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    const uint64_t nb = chain_blocks(src, n, ph);        // the block count for the table
    if (nb >= 0xFFFFFFFFull) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    const uint32_t max_blocks = (uint32_t)nb;
    const size_t iws = zlz4f_batch_frame_index_workspace(1, max_blocks);
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    struct Rec {
        FrameRec f; uint64_t idx_off, idx_cap, dst_off, dst_cap, skip, totals[2]; int64_t rres; zlz4f_range range;
    };
    DevBuf d_src(n, &dc), d_iws(iws, &dc), d_index((nb + 1) * sizeof(zlz4f_index_entry), &dc);
    Staged<Rec> rec(&dc, 256);
    if (!d_src.p || !d_iws.p || !d_index.p || !rec.d) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.f.src_len = n; rec.h.idx_cap = nb + 1;
    rec.h.range.a = a; rec.h.range.b = b;
    dc.launched();
    if (!upload(d_src, src, n, st) || !rec.upload(st)) return ZLZ4_ERR_DEVICE;
    Rec *r = rec.d;
    zlz4f_index_entry *index = d_index.as<zlz4f_index_entry>();
    int32_t rc = zlz4f_batch_frame_index(st, d_src.as<uint8_t>(), &r->f.src_off, &r->f.src_len, index, &r->idx_off, &r->idx_cap,
                                         &r->f.result, 1, max_blocks, d_iws.p, iws);
    if (rc != 0) return rc;
    rc = zlz4f_batch_plan_frame_ranges(st, index, &r->idx_off, &r->f.result, 1, &r->range, 1, 0, &r->dst_off, &r->dst_cap,
                                       r->totals);
    if (rc != 0) return rc;
    // one read-back: the index status, the slot and item count, and S (entry nb: the walk above is the index call's)
    int64_t idx_n = 0;
    uint64_t totals[2] = {0, 0};
    zlz4f_index_entry last = {0, 0};
    if (hipMemcpyAsync(&idx_n, &r->f.result, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(totals, r->totals, 16, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&last, index + nb, sizeof last, hipMemcpyDeviceToHost, st) != hipSuccess || !dc.sync())
        return ZLZ4_ERR_DEVICE;
    if (idx_n < 0) return idx_n;
    if ((uint64_t)idx_n != nb) return ZLZ4_ERR_DEVICE;           // (both counts are chain_walk's, here and in k_bfd_walk)
    const uint64_t S = last.dec, a1 = a < S ? a : S, b1 = b < S ? b : S;
    if (cap < b1 - a1) return ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
    if (totals[1] > 0xFFFFFFFFull) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    const uint32_t max_items = (uint32_t)totals[1];
    const size_t rws = zlz4f_batch_decompress_frame_range_workspace(1, max_items);
    DevBuf d_rws(rws, &dc), d_dst(totals[0], &dc);
    if (!d_rws.p || !d_dst.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    dc.launched();
    rc = zlz4f_batch_decompress_frame_range(st, d_src.as<uint8_t>(), &r->f.src_off, &r->f.src_len, index, &r->idx_off,
                                            &r->f.result, 1, &r->range, d_dst.as<uint8_t>(), &r->dst_off, &r->dst_cap, &r->skip,
                                            &r->rres, 1, max_items, d_rws.p, rws);
    if (rc != 0) return rc;
    int64_t result = 0;
    uint64_t skip = 0;
    if (hipMemcpyAsync(&skip, &r->skip, 8, hipMemcpyDeviceToHost, st) != hipSuccess || !read_result(dc, &r->rres, result))
        return ZLZ4_ERR_DEVICE;
    if (result > 0 && ((uint64_t)result > cap || skip + (uint64_t)result > totals[0] ||
                       hipMemcpy(dst, d_dst.as<uint8_t>() + skip, (size_t)result, hipMemcpyDeviceToHost) != hipSuccess))
        return ZLZ4_ERR_DEVICE;
    return result;
}

}  // extern "C"

// ====================================================================== file index and range decoding
// A FILE is a multiframe buffer as the record-mode split delimits it: frame, skippable and legacy members.  The file index
// is the frame index across members -- one run of (position in the buffer, offset in the file's content) per block, in
// member order -- and the file range decode is the frame range decode whose items each look up their own member: a
// range may cross members, so block checksums, stored blocks and the block size bound change from item to item.
namespace {

// what the index keeps per item for a legacy member (an item of another kind has nb 0 and is never read)
struct FfLeg {
    uint64_t nb;        // blocks of the chain
    uint64_t base;      // first entry of the legacy block table (exclusive scan of nb)
    int64_t status;     // legacy_walk's verdict
    uint64_t pad;
};

// one lane per item, k_lf_walk's two passes over (item_off, leg_len): count, then record the blocks at the item's base
template <bool kRecord>
__global__ __launch_bounds__(64) void k_ff_leg_walk(const uint8_t *__restrict__ src, const uint64_t *__restrict__ item_off,
                                                    const uint64_t *__restrict__ leg_len, uint32_t nitems, uint32_t leg_blocks,
                                                    FfLeg *__restrict__ lg, uint64_t *__restrict__ data_off,
                                                    uint32_t *__restrict__ data_len) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems) return;
    const uint64_t so = item_off[i], n = leg_len[i];
    uint64_t nb = 0, end = 0;
    if (kRecord) {
        const FfLeg G = lg[i];
        if (G.nb != 0 && G.base + G.nb <= leg_blocks)
            (void)legacy_walk(src + so, n, G.nb, nb, end, [&](uint64_t k, uint64_t off, uint32_t size) {
                data_off[G.base + k] = so + off;                      // (the record pass never leaves the item's range)
                data_len[G.base + k] = size;
            });
    } else {
        FfLeg G = {};
        if (n != 0) {                                                 // (length 0: the item of a member that is not legacy)
            G.status = legacy_walk(src + so, n, ~0ull, nb, end, [](uint64_t, uint64_t, uint32_t) {});
            G.nb = nb;
        }
        lg[i] = G;
    }
}

// k_bf_scan over the legacy records
__global__ __launch_bounds__(1024) void k_ff_leg_scan(FfLeg *__restrict__ lg, uint32_t nitems) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (nitems + 1023u) / 1024u;
    const uint64_t b0 = (uint64_t)t * chunk;
    const uint32_t lo = b0 < nitems ? (uint32_t)b0 : nitems;
    const uint32_t hi = b0 + chunk < nitems ? (uint32_t)(b0 + chunk) : nitems;
    uint64_t s = 0, total;
    for (uint32_t i = lo; i < hi; i++) s += lg[i].nb;
    uint64_t run = bfr_wg_scan(s, part, total);
    for (uint32_t i = lo; i < hi; i++) { lg[i].base = run; run += lg[i].nb; }
}

// one wavefront per buffer: its room in the index = the blocks of its items' chains, as the walks counted them, plus one
__global__ __launch_bounds__(256) void k_ff_room(const BFrame *__restrict__ fr, const FfLeg *__restrict__ lg,
                                                 const uint64_t *__restrict__ item_first, uint32_t nbuf,
                                                 uint64_t *__restrict__ room) {
    const uint32_t s = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (s >= nbuf) return;
    const uint64_t i0 = item_first[s], i1 = item_first[s + 1];
    unsigned long long sum = 0;
    for (uint64_t i = i0 + lane; i < i1; i += 64u) sum += fr[i].nb + (lg ? lg[i].nb : 0u);
    for (uint32_t d = 32u; d >= 1u; d >>= 1) sum += __shfl_xor(sum, (int)d);
    if (lane == 0) room[s] = sum + 1u;
}

// one workgroup: out[0..n] = the exclusive scan of in[0..n), out[n] = the total
__global__ __launch_bounds__(1024) void k_ff_scan(const uint64_t *__restrict__ in, uint32_t n, uint64_t *__restrict__ out) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + 1023u) / 1024u;
    const uint64_t b0 = (uint64_t)t * chunk;
    const uint32_t lo = b0 < n ? (uint32_t)b0 : n;
    const uint32_t hi = b0 + chunk < n ? (uint32_t)(b0 + chunk) : n;
    uint64_t s = 0, total;
    for (uint32_t i = lo; i < hi; i++) s += in[i];
    uint64_t run = bfr_wg_scan(s, part, total);
    for (uint32_t i = lo; i < hi; i++) { out[i] = run; run += in[i]; }
    if (t == 0) out[n] = total;
}

// the tables the fold reads: the frame size query's over the items, and the legacy walk's
struct FfTables {
    const BFrame *fr;
    const uint64_t *data_off;
    const uint32_t *data_len, *flags, *cks_ok;
    const int64_t *sizes;
    const FfLeg *lg;                  // null: the split found no legacy member
    const uint64_t *leg_off;
    const int64_t *leg_sizes;
    uint32_t max_blocks, leg_blocks;
};

// The fold, one wavefront per buffer: k_mf_finish's verdict over the members in member order -- the first member that is
// not OK decides -- while the decoded base `run`, the block count `kb` and the position base (the buffer's offset in d_src)
// carry from member to member and every block's entry is written rebased: pos counts from the buffer's first byte, dec
// from the file's first content byte.  Members and blocks are taken 64 at a step (blocks) or one at a time (members), so
// neither count is bounded by the wavefront.  A buffer whose room does not fit idx_cap writes nothing.
__global__ __launch_bounds__(256) void k_ff_fold(FfTables T, const zlz4f_member *__restrict__ member,
                                                 const uint64_t *__restrict__ mem_off, const int64_t *__restrict__ split_result,
                                                 const uint64_t *__restrict__ item_first, const uint64_t *__restrict__ item_len,
                                                 const uint64_t *__restrict__ src_off, uint32_t nbuf,
                                                 zlz4f_index_entry *__restrict__ index, const uint64_t *__restrict__ idx_off,
                                                 uint64_t idx_cap, int64_t *__restrict__ result) {
    const uint32_t s = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (s >= nbuf) return;
    const int64_t sr = split_result[s];
    if (sr < 0) { if (lane == 0) result[s] = sr; return; }
    const uint64_t i0 = item_first[s], cnt = item_first[s + 1] - i0, so = src_off[s];
    const uint64_t room = idx_off[s + 1] - idx_off[s];
    const bool fits = idx_off[s + 1] <= idx_cap;
    zlz4f_index_entry *e = fits ? index + idx_off[s] : nullptr;
    const zlz4f_member *m = member + mem_off[s];
    int64_t out = 0;
    uint64_t kb = 0, run = 0, end_pos = 0;
    for (uint64_t k = 0; k < cnt && !out; k++) {                      // (wave-uniform)
        const zlz4f_member M = m[k];
        const uint32_t kind = M.kind & 0xFFu;
        const uint64_t i = i0 + k;
        if (kind == ZLZ4F_MEMBER_FRAME) {
            const BFrame F = T.fr[i];
            out = bfi_status(F, T.max_blocks, lane, T.data_len, T.flags, T.sizes, T.cks_ok, item_len[i]);
            if (!out && kb + F.nb + 1u > room) out = ZLZ4_ERR_INVALID_STATE;           // (tables that are not this split's)
            if (out) break;
            end_pos = bfi_entries(F, lane, T.data_off, T.data_len, T.flags, T.sizes, so, M.pos + (uint64_t)F.status,
                                  e ? e + kb : nullptr, run);
            kb += F.nb;
        } else if (kind == ZLZ4F_MEMBER_LEGACY) {
            if (!T.lg) { out = ZLZ4_ERR_INVALID_STATE; break; }
            const FfLeg G = T.lg[i];
            if ((G.nb != 0 && G.base + G.nb > T.leg_blocks) || kb + G.nb + 1u > room) { out = ZLZ4_ERR_INVALID_STATE; break; }
            for (uint64_t b0 = 0; b0 < G.nb; b0 += 64u) {              // (wave-uniform trip count)
                const uint64_t j = b0 + lane, ii = G.base + j;
                const int64_t sz = j < G.nb ? T.leg_sizes[ii] : 0;
                if (zlz4::ballot(sz < 0 || sz > (int64_t)ZLZ4F_LEGACY_BLOCK_SIZE) != 0) {
                    out = ZLZ4F_ERR_DECOMPRESSION_FAILED;              // (a bad block stands in front of what ended the walk)
                    break;
                }
                const uint32_t incl = zlz4::wave_incl_scan((uint32_t)sz);              // (64 blocks stay below 2^32)
                if (e && j < G.nb) {
                    zlz4f_index_entry E;
                    E.pos = T.leg_off[ii] - so - 4u;
                    E.dec = run + (incl - (uint32_t)sz);
                    e[kb + j] = E;
                }
                run += zlz4::rdlane(incl, 63);
            }
            if (!out) out = G.status;
            if (out) break;
            kb += G.nb;
            end_pos = M.pos + M.len;
        } else if (kind == ZLZ4F_MEMBER_SKIPPABLE_TRUNCATED) {
            out = M.len < 8 ? ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE : ZLZ4F_ERR_FRAME_SIZE_WRONG;
        }
    }
    if (!out && !fits) out = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
    if (lane == 0) {
        if (!out) {
            zlz4f_index_entry E;
            E.pos = end_pos;
            E.dec = run;
            e[kb] = E;
        }
        result[s] = out ? out : (int64_t)kb;
    }
}

// ------------------------------------------------------------------ file ranges
// what an item takes from its member
struct FfMem {
    uint64_t end;       // the member's end inside the buffer
    uint64_t first;     // the end of the member's header: where the word of its block 0 stands
    uint32_t bound;     // the most a block decodes to
    bool bc, legacy;    // block checksums (FLG 0x10); a legacy member: size words, no stored bit
    bool linked;        // a frame member whose FLG declares linked blocks (0x20 clear)
};

// The member of buffer (s, n bytes; cnt members at m) that holds position pos, by bisection for the last member that
// starts at or in front of pos.  false: pos is no place for a block word -- no such member, a member that is neither a
// frame nor a legacy frame, that leaves the buffer or whose header is none, a position inside the header, or fewer than 4
// bytes up to the member's end.  Reads the member table and the member's header, nothing else.
__device__ inline bool ff_member_of(const zlz4f_member *__restrict__ m, uint64_t cnt, const uint8_t *__restrict__ s, uint64_t n,
                                    uint64_t pos, FfMem &out) {
    uint64_t lo = 0, hi = cnt;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (m[mid].pos <= pos) lo = mid + 1u; else hi = mid;
    }
    if (lo == 0) return false;
    const zlz4f_member M = m[lo - 1u];
    if (M.len > n || M.pos > n - M.len) return false;
    const uint32_t kind = M.kind & 0xFFu;
    uint64_t first;
    if (kind == ZLZ4F_MEMBER_FRAME) {
        const ParsedHeader ph = frame_header(s + M.pos, M.len);
        if (ph.size < 0) return false;
        first = M.pos + (uint64_t)ph.size;
        out.bound = (uint32_t)ph.block_size;
        out.bc = (ph.flg & 0x10u) != 0;
        out.legacy = false;
        out.linked = (ph.flg & 0x20u) == 0;
    } else if (kind == ZLZ4F_MEMBER_LEGACY) {
        if (M.len < 4 || zx_rd32(s + M.pos) != ZLZ4F_LEGACY_MAGICNUMBER) return false;
        first = M.pos + 4u;
        out.bound = ZLZ4F_LEGACY_BLOCK_SIZE;
        out.bc = false;
        out.legacy = true;
        out.linked = false;
    } else return false;
    out.end = M.pos + M.len;
    out.first = first;
    return pos >= first && pos <= out.end && out.end - pos >= 4u;
}

// A FILE has at most one dictionary: buffer s uses dictionary dd.idx[s], dictionary 0 for a null
// index.  false: the buffer names none.  T = the last D = min(len, 65536) bytes of the dictionary.
__device__ __forceinline__ bool ff_dict_of(const BfDict &dd, uint32_t s, uint32_t &D, uint64_t &t_off) {
    const uint32_t d = dd.idx ? dd.idx[s] : 0u;
    D = 0; t_off = 0;
    if (d >= dd.n) return false;
    const uint32_t len = dd.len[d];
    D = len < 65536u ? len : 65536u;
    if (dd.off) t_off = dd.off[d] + (len - D);
    return true;
}

// the buffer that holds item i: the last s < nbuf with item_first[s] <= i (buffers without items share their first)
__device__ __forceinline__ uint32_t ff_buffer_of(const uint64_t *__restrict__ item_first, uint32_t nbuf, uint64_t i) {
    uint32_t lo = 0, hi = nbuf;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (item_first[mid] <= i) lo = mid + 1u; else hi = mid;
    }
    return lo ? lo - 1u : 0u;
}

// k_bfr_range for files: the same statuses in the same order, with the chain check of every pair (k, k + 1) made against
// the member that holds pos[k].  Nothing but the tables is read for a range with a' == b'.  kDict: a range whose file names
// no dictionary is refused with the first statuses.
template <bool kDict>
__device__ __forceinline__ void ffr_range(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                          const uint64_t *__restrict__ src_len, const zlz4f_index_entry *__restrict__ index,
                                          const uint64_t *__restrict__ idx_off, const int64_t *__restrict__ idx_n,
                                          uint32_t nbuf, const zlz4f_member *__restrict__ member,
                                          const uint64_t *__restrict__ mem_off, const int64_t *__restrict__ split_result,
                                          const zlz4f_range *__restrict__ range, const uint64_t *__restrict__ dst_cap,
                                          uint32_t nranges, BRange *__restrict__ rg, const BfDict &dd) {
    const uint32_t r = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (r >= nranges) return;
    const zlz4f_range R = range[r];
    BRange G = {};
    int64_t st = 0;
    uint32_t D;
    uint64_t t_off;
    if (R.frame >= nbuf || R.a > R.b || R.reserved != 0 || (kDict && !ff_dict_of(dd, R.frame, D, t_off)))
        st = ZLZ4_ERR_INVALID_STATE;
    else if (idx_n[R.frame] < 0) st = idx_n[R.frame];
    else {
        BfrSpan sp;
        const zlz4f_index_entry *e = nullptr;
        uint64_t nb = 0;
        const bool found = bfr_span(R, index, idx_off, idx_n, nbuf, sp, e, nb);
        G.a = sp.a; G.b = sp.b; G.d0 = sp.a;
        if (sp.a != sp.b) {
            const int64_t cnt = split_result[R.frame];
            bool bad = !found || cnt <= 0;                            // (no member table: not this file's index)
            if (!bad) {
                const uint64_t n = src_len[R.frame];
                const uint8_t *s = src + src_off[R.frame];
                const zlz4f_member *m = member + mem_off[R.frame];
                for (uint64_t k = sp.k0 + lane; k <= sp.k1; k += 64u) {
                    const zlz4f_index_entry E = e[k], N = e[k + 1u];
                    FfMem fm;
                    if (!ff_member_of(m, (uint64_t)cnt, s, n, E.pos, fm) || N.pos <= E.pos || N.dec < E.dec ||
                        N.dec - E.dec > fm.bound)
                        bad = true;
                }
                if (e[sp.k1].dec >= sp.b || e[sp.k1 + 1u].dec < sp.b) bad = true;
            }
            if (zlz4::ballot(bad) != 0) st = ZLZ4_ERR_INVALID_STATE;
            else if (dst_cap[r] < sp.b - e[sp.k0].dec) st = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
            else { G.n = sp.k1 - sp.k0 + 1u; G.k0 = sp.k0; G.d0 = e[sp.k0].dec; }
        }
    }
    G.status = st;
    if (lane == 0) rg[r] = G;
}

__global__ __launch_bounds__(256) void k_ffr_range(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                   const uint64_t *__restrict__ src_len,
                                                   const zlz4f_index_entry *__restrict__ index,
                                                   const uint64_t *__restrict__ idx_off, const int64_t *__restrict__ idx_n,
                                                   uint32_t nbuf, const zlz4f_member *__restrict__ member,
                                                   const uint64_t *__restrict__ mem_off, const int64_t *__restrict__ split_result,
                                                   const zlz4f_range *__restrict__ range, const uint64_t *__restrict__ dst_cap,
                                                   uint32_t nranges, BRange *__restrict__ rg) {
    ffr_range<false>(src, src_off, src_len, index, idx_off, idx_n, nbuf, member, mem_off, split_result, range, dst_cap, nranges,
                     rg, BfDict{});
}

__global__ __launch_bounds__(256) void k_ffr_range_dict(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                        const uint64_t *__restrict__ src_len,
                                                        const zlz4f_index_entry *__restrict__ index,
                                                        const uint64_t *__restrict__ idx_off, const int64_t *__restrict__ idx_n,
                                                        uint32_t nbuf, const zlz4f_member *__restrict__ member,
                                                        const uint64_t *__restrict__ mem_off,
                                                        const int64_t *__restrict__ split_result,
                                                        const zlz4f_range *__restrict__ range,
                                                        const uint64_t *__restrict__ dst_cap, uint32_t nranges,
                                                        BRange *__restrict__ rg, BfDict dd) {
    ffr_range<true>(src, src_off, src_len, index, idx_off, idx_n, nbuf, member, mem_off, split_result, range, dst_cap, nranges,
                    rg, dd);
}

// k_bfr_expand for files, one lane per item: the item's member again (k_ffr_range has accepted it), the block word as that
// member reads it -- a frame's header word, or a legacy size word that is neither 0 nor above the bound -- and where the
// block has to end: at pos[k + 1] when that lies in the same member, else on the frame member's end mark or, for a chain
// without one and for a legacy member, at the member's end.  The block's bytes are used only when all of that holds.
// kDict: the item's dictionary descriptor (e_off, e_len) -- T of its file where the block sees it: every block of a frame
// member that declares independent blocks, block 0 (the word at the header's end) of one that declares linked blocks, no
// block of a legacy member; length 0 elsewhere.
template <bool kDict>
__device__ __forceinline__ void ffr_expand(const BRange *__restrict__ rg, uint32_t nranges, uint32_t max_items,
                                           const zlz4f_range *__restrict__ range, const uint8_t *__restrict__ src,
                                           const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ src_len,
                                           const zlz4f_index_entry *__restrict__ index, const uint64_t *__restrict__ idx_off,
                                           const zlz4f_member *__restrict__ member, const uint64_t *__restrict__ mem_off,
                                           const int64_t *__restrict__ split_result, const uint64_t *__restrict__ dst_off,
                                           const BfrTables &T, const BfDict &dd, uint64_t *__restrict__ e_off,
                                           uint32_t *__restrict__ e_len) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_items; i += gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = nranges;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (rg[mid].base <= i) lo = mid + 1u; else hi = mid;
        }
        uint64_t d_off = 0, c_off = 0, o_off = 0, x_off = 0;
        uint32_t d_len = 0, fl = 0, f_len = 0, f_cap = 0, p_len = 0, p_cap = 0, c_len = 0, ierr = 0, x_len = 0;
        if (lo > 0) {
            const uint32_t r = lo - 1u;
            const BRange G = rg[r];
            const uint64_t j = i - G.base;
            if (j < G.n && G.status == 0 && bfr_fits(G, max_items)) {
                const uint32_t f = range[r].frame;
                const zlz4f_index_entry *e = index + idx_off[f];
                const uint64_t k = G.k0 + j;
                const zlz4f_index_entry E = e[k], N = e[k + 1u];
                const uint64_t so = src_off[f];
                const uint8_t *s = src + so;
                const int64_t cnt = split_result[f];
                FfMem fm;
                bool ok = cnt > 0 && ff_member_of(member + mem_off[f], (uint64_t)cnt, s, src_len[f], E.pos, fm);
                uint32_t sz = 0;
                bool stored = false;
                if (ok) {
                    const uint32_t word = zx_rd32(s + E.pos);
                    if (fm.legacy) { sz = word; ok = word != 0 && word <= ZLZ4F_LEGACY_BLOCK_BOUND; }
                    else { const BlockWord w = block_word(word); sz = w.size; stored = w.stored; ok = !w.end_mark; }
                }
                if (ok) {
                    const uint64_t q = E.pos + 4u + sz + (fm.bc ? 4u : 0u);             // where the block ends
                    if (q > fm.end) ok = false;
                    else if (N.pos <= fm.end) ok = q == N.pos;                           // k + 1 in the same member
                    else if (fm.legacy) ok = q == fm.end;
                    else ok = q == fm.end || (fm.end - q >= 4u && zx_rd32(s + q) == 0u);
                }
                if (!ok) ierr = kItemChain;
                else {
                    const uint32_t step = (uint32_t)(N.dec - E.dec);             // <= the member's bound (k_ffr_range)
                    const uint64_t left = G.b - E.dec;                           // > 0: dec[k] <= dec[k1] < b'
                    const uint32_t want = left < step ? (uint32_t)left : step;
                    d_off = so + E.pos + 4u;
                    d_len = sz;
                    o_off = dst_off[r] + (E.dec - G.d0);
                    if (fm.bc) { fl |= kBlkCks; c_off = d_off + sz; }
                    if (stored) {
                        fl |= kBlkStored;
                        if (sz != step) ierr = kItemStored; else c_len = want;
                    } else if (want == step) { f_len = sz; f_cap = step; }
                    else { p_len = sz; p_cap = want; }
                    if (kDict && !fm.legacy && (!fm.linked || E.pos == fm.first)) (void)ff_dict_of(dd, f, x_len, x_off);
                }
            }
        }
        T.data_off[i] = d_off; T.cks_off[i] = c_off; T.out_off[i] = o_off;
        T.data_len[i] = d_len; T.flags[i] = fl; T.f_len[i] = f_len; T.f_cap[i] = f_cap; T.p_len[i] = p_len;
        T.p_cap[i] = p_cap; T.c_len[i] = c_len; T.ierr[i] = ierr;
        if (kDict) { e_off[i] = x_off; e_len[i] = x_len; }
    }
}

__global__ void k_ffr_expand(const BRange *__restrict__ rg, uint32_t nranges, uint32_t max_items,
                             const zlz4f_range *__restrict__ range, const uint8_t *__restrict__ src,
                             const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ src_len,
                             const zlz4f_index_entry *__restrict__ index, const uint64_t *__restrict__ idx_off,
                             const zlz4f_member *__restrict__ member, const uint64_t *__restrict__ mem_off,
                             const int64_t *__restrict__ split_result, const uint64_t *__restrict__ dst_off, BfrTables T) {
    ffr_expand<false>(rg, nranges, max_items, range, src, src_off, src_len, index, idx_off, member, mem_off, split_result, dst_off,
                      T, BfDict{}, nullptr, nullptr);
}

__global__ void k_ffr_expand_dict(const BRange *__restrict__ rg, uint32_t nranges, uint32_t max_items,
                                  const zlz4f_range *__restrict__ range, const uint8_t *__restrict__ src,
                                  const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ src_len,
                                  const zlz4f_index_entry *__restrict__ index, const uint64_t *__restrict__ idx_off,
                                  const zlz4f_member *__restrict__ member, const uint64_t *__restrict__ mem_off,
                                  const int64_t *__restrict__ split_result, const uint64_t *__restrict__ dst_off, BfrTables T,
                                  BfDict dd, uint64_t *__restrict__ e_off, uint32_t *__restrict__ e_len) {
    ffr_expand<true>(rg, nranges, max_items, range, src, src_off, src_len, index, idx_off, member, mem_off, split_result, dst_off,
                     T, dd, e_off, e_len);
}

// ------------------------------------------------------------------ the dictionary forms
// the index, one lane per table entry: the dictionary length the size pass gives the entry's block -- D of its file where
// the block sees T (every block of an independent-declared member, block 0 of a linked-declared one), else 0
__global__ void k_ffd_entry_len(const BFrame *__restrict__ fr, const uint32_t *__restrict__ fidx, uint32_t max_blocks,
                                const uint64_t *__restrict__ item_first, uint32_t nbuf, BfDict dd,
                                uint32_t *__restrict__ e_len) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < max_blocks; i += gridDim.x * blockDim.x) {
        const uint32_t f = fidx[i];
        uint32_t D = 0;
        uint64_t t_off;
        if (f != kNoFrame) {
            const BFrame F = fr[f];
            if ((F.flg & 0x20u) || i == F.base) (void)ff_dict_of(dd, ff_buffer_of(item_first, nbuf, f), D, t_off);
        }
        e_len[i] = D;
    }
}

// the index, one lane per buffer, behind the fold: a file that names no dictionary is InvalidState in front of every other
// status of the file, the split's included (its room stays: the room is the walks' count alone)
__global__ void k_ffd_refuse(BfDict dd, uint32_t nbuf, int64_t *__restrict__ result) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t D;
    uint64_t t_off;
    if (s < nbuf && !ff_dict_of(dd, s, D, t_off)) result[s] = ZLZ4_ERR_INVALID_STATE;
}

// one lane per item: the dictionary index of its buffer, carried through unchanged
__global__ void k_ffd_item_dicts(const uint64_t *__restrict__ item_first, uint32_t nbuf, uint32_t nitems,
                                 const uint32_t *__restrict__ dict_idx, uint32_t *__restrict__ item_dict_idx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nitems) item_dict_idx[i] = dict_idx ? dict_idx[ff_buffer_of(item_first, nbuf, i)] : 0u;
}

// the file index's workspace: the frame size query's over the items, then the legacy walk's records and block table and
// the rooms; with dictionaries the entries' dictionary lengths behind them
struct FfLayout {
    BfdLayout q;
    Region<FfLeg> leg;
    Region<uint64_t> leg_off, room;
    Region<uint32_t> leg_len, e_len;
    Region<int64_t> leg_sizes;
    size_t bytes = 0;
};

FfLayout ff_layout(uint32_t nbuf, uint32_t nitems, uint32_t max_blocks, uint32_t leg_blocks, void *ws = nullptr,
                   bool dict = false) {
    FfLayout L;
    L.q = bfd_layout(nitems, max_blocks, 0, false, kQuery, ws);
    Carver c{static_cast<uint8_t *>(ws), L.q.bytes};
    c.take(nitems, L.leg);
    c.take(leg_blocks, L.leg_off, L.leg_len, L.leg_sizes);
    c.take(nbuf, L.room);
    if (dict) c.take(max_blocks, L.e_len);
    L.bytes = c.bytes;
    return L;
}

// the split's four totals as the 32-bit counts the kernels take; false: a null pointer or a count that is none
bool ff_totals(const uint64_t *t, uint32_t &nitems, uint32_t &max_blocks, uint32_t &leg_blocks) {
    if (!t || t[0] > 0xFFFFFFFFull || t[1] > 0xFFFFFFFFull || t[3] > 0xFFFFFFFFull) return false;
    nitems = (uint32_t)t[0]; max_blocks = (uint32_t)t[1]; leg_blocks = (uint32_t)t[3];
    return true;
}

// the dictionary arrays of a file call's _using_dict form are refused as the dictionary frame calls refuse theirs: with
// ndicts != 0 a null length array (`bytes`: or a null offset array), and a misaligned array
bool ff_dict_refused(const BfDict &dd, bool bytes) {
    if (dd.n && (!dd.len || (bytes && !dd.off))) return true;
    return bf_misaligned(dd.off, 8) || bf_misaligned(dd.len, 4) || bf_misaligned(dd.idx, 4);
}

// The frame size query's launch sequence over the items up to its fold, the legacy walk and size kernel over the same
// items where the split found legacy members, the rooms and their scan, the fold.  The sequence depends on the totals alone.
// dd (zlz4f_batch_file_index_using_dict): the size kernel gets a dictionary length per table entry, and the files that name
// no dictionary are refused behind the fold.
int32_t ff_index_impl(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len, uint32_t nbuf,
                      const zlz4f_member *d_member, const uint64_t *d_mem_off, const int64_t *d_split_result,
                      const uint64_t *d_item_first, const uint64_t *d_item_off, const uint64_t *d_item_len,
                      const uint64_t *d_leg_len, const uint64_t *split_totals, zlz4f_index_entry *d_index, uint64_t *d_idx_off,
                      uint64_t idx_cap, int64_t *d_result, void *d_workspace, size_t workspace_bytes,
                      const BfDict *dd = nullptr) {
    if (nbuf == 0) return 0;
    uint32_t nitems, mb, lb;
    if (!ff_totals(split_totals, nitems, mb, lb)) return ZLZ4_ERR_INVALID_STATE;
    const bool legacy = split_totals[2] != 0;
    if (!d_src || !d_src_off || !d_src_len || !d_mem_off || !d_split_result || !d_item_first || !d_index || !d_idx_off ||
        !d_result || (nitems && (!d_member || !d_item_off || !d_item_len)) || (legacy && !d_leg_len))
        return ZLZ4_ERR_INVALID_STATE;
    if (bf_misaligned(d_src_off, 8) || bf_misaligned(d_src_len, 8) || bf_misaligned(d_member, 8) || bf_misaligned(d_mem_off, 8) ||
        bf_misaligned(d_split_result, 8) || bf_misaligned(d_item_first, 8) || bf_misaligned(d_item_off, 8) ||
        bf_misaligned(d_item_len, 8) || bf_misaligned(d_leg_len, 8) || bf_misaligned(d_index, 8) || bf_misaligned(d_idx_off, 8) ||
        bf_misaligned(d_result, 8) || (dd && ff_dict_refused(*dd, false)))
        return ZLZ4_ERR_INVALID_STATE;
    const FfLayout L = ff_layout(nbuf, nitems, mb, lb, d_workspace, dd != nullptr);
    if (!d_workspace || workspace_bytes < L.bytes || bf_misaligned(d_workspace, 16)) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const BfArrays a = {d_src, d_item_off, d_item_len, nullptr, nullptr, nullptr, nullptr, nitems, mb};
    if (bfd_prelude(st, a, false, nullptr, L.q) != 0) return ZLZ4_ERR_DEVICE;
    if (mb) {
        hipLaunchKernelGGL(k_bfq_len, dim3(bf_grid(mb, 256, 4096)), dim3(256), 0, st, L.q.data_len, L.q.flags, mb, L.q.dec_len);
        if (dd)
            hipLaunchKernelGGL(k_ffd_entry_len, dim3(bf_grid(mb, 256, 4096)), dim3(256), 0, st, L.q.frames.p, L.q.fidx.p, mb,
                               d_item_first, nbuf, *dd, L.e_len.p);
        if (zlz4_launch_decompressed_size(st, d_src, L.q.data_off, L.q.dec_len, dd ? L.e_len.p : nullptr, L.q.sizes, mb) != 0)
            return ZLZ4_ERR_DEVICE;
    }
    if (legacy) {
        const uint32_t gi = bf_grid(nitems, 64);
        hipLaunchKernelGGL(k_ff_leg_walk<false>, dim3(gi), dim3(64), 0, st, d_src, d_item_off, d_leg_len, nitems, lb, L.leg.p,
                           (uint64_t *)nullptr, (uint32_t *)nullptr);
        hipLaunchKernelGGL(k_ff_leg_scan, dim3(1), dim3(1024), 0, st, L.leg.p, nitems);
        if (lb) {
            if (hipMemsetAsync(L.leg_len.p, 0, (size_t)lb * 4u, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
            hipLaunchKernelGGL(k_ff_leg_walk<true>, dim3(gi), dim3(64), 0, st, d_src, d_item_off, d_leg_len, nitems, lb, L.leg.p,
                               L.leg_off.p, L.leg_len.p);
            if (zlz4_launch_decompressed_size(st, d_src, L.leg_off, L.leg_len, nullptr, L.leg_sizes, lb) != 0)
                return ZLZ4_ERR_DEVICE;
        }
    }
    const FfLeg *lg = legacy ? L.leg.p : nullptr;
    const uint32_t gs = bf_grid(nbuf, 4);
    hipLaunchKernelGGL(k_ff_room, dim3(gs), dim3(256), 0, st, L.q.frames.p, lg, d_item_first, nbuf, L.room.p);
    hipLaunchKernelGGL(k_ff_scan, dim3(1), dim3(1024), 0, st, L.room.p, nbuf, d_idx_off);
    const FfTables T = {L.q.frames, L.q.data_off, L.q.data_len, L.q.flags, L.q.cks_ok, L.q.sizes, lg, L.leg_off, L.leg_sizes, mb, lb};
    hipLaunchKernelGGL(k_ff_fold, dim3(gs), dim3(256), 0, st, T, d_member, d_mem_off, d_split_result, d_item_first, d_item_len,
                       d_src_off, nbuf, d_index, d_idx_off, idx_cap, d_result);
    if (dd) hipLaunchKernelGGL(k_ffd_refuse, dim3(bf_grid(nbuf, 256)), dim3(256), 0, st, *dd, nbuf, d_result);
    return hipGetLastError() == hipSuccess ? 0 : ZLZ4_ERR_DEVICE;
}

// zlz4f_batch_decompress_frame_range's launch sequence with k_ffr_range and k_ffr_expand in the places of k_bfr_range and
// k_bfr_expand; scan, checksums, decoders, copy and finish are that call's.  dd
// (zlz4f_batch_decompress_file_range_using_dict): the _dict kernels, which also write every item's dictionary descriptor,
// and the block decoders that take one.
int32_t ff_range_impl(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                      const zlz4f_index_entry *d_index, const uint64_t *d_idx_off, const int64_t *d_idx_n, uint32_t nbuf,
                      const zlz4f_member *d_member, const uint64_t *d_mem_off, const int64_t *d_split_result,
                      const zlz4f_range *d_range, uint8_t *d_dst, const uint64_t *d_dst_off, const uint64_t *d_dst_cap,
                      uint64_t *d_skip, int64_t *d_result, uint32_t nranges, uint32_t max_items, void *d_workspace,
                      size_t workspace_bytes, const BfDict *dd = nullptr) {
    if (nranges == 0) return 0;
    const BfrLayout L = bfr_layout(nranges, max_items, d_workspace, dd != nullptr);
    if (!d_range || !d_dst_off || !d_dst_cap || !d_skip || !d_result || (max_items && !d_dst) ||
        (nbuf && (!d_src || !d_src_off || !d_src_len || !d_index || !d_idx_off || !d_idx_n || !d_member || !d_mem_off ||
                  !d_split_result)))
        return ZLZ4_ERR_INVALID_STATE;
    if (bf_misaligned(d_src_off, 8) || bf_misaligned(d_src_len, 8) || bf_misaligned(d_index, 8) || bf_misaligned(d_idx_off, 8) ||
        bf_misaligned(d_idx_n, 8) || bf_misaligned(d_member, 8) || bf_misaligned(d_mem_off, 8) ||
        bf_misaligned(d_split_result, 8) || bf_misaligned(d_range, 8) || bf_misaligned(d_dst_off, 8) ||
        bf_misaligned(d_dst_cap, 8) || bf_misaligned(d_skip, 8) || bf_misaligned(d_result, 8) ||
        (dd && ff_dict_refused(*dd, true)))
        return ZLZ4_ERR_INVALID_STATE;
    if (!d_workspace || workspace_bytes < L.bytes || bf_misaligned(d_workspace, 16)) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t m = max_items, gr = bf_grid(nranges, 4);
    const BfrTables T = {L.data_off, L.cks_off, L.out_off, L.data_len, L.flags, L.f_len, L.f_cap, L.p_len, L.p_cap, L.c_len, L.ierr};
    if (dd)
        hipLaunchKernelGGL(k_ffr_range_dict, dim3(gr), dim3(256), 0, st, d_src, d_src_off, d_src_len, d_index, d_idx_off, d_idx_n,
                           nbuf, d_member, d_mem_off, d_split_result, d_range, d_dst_cap, nranges, L.ranges, *dd);
    else
        hipLaunchKernelGGL(k_ffr_range, dim3(gr), dim3(256), 0, st, d_src, d_src_off, d_src_len, d_index, d_idx_off, d_idx_n, nbuf,
                           d_member, d_mem_off, d_split_result, d_range, d_dst_cap, nranges, L.ranges);
    hipLaunchKernelGGL(k_bfr_scan, dim3(1), dim3(1024), 0, st, L.ranges, nranges);
    if (m) {
        if (dd)
            hipLaunchKernelGGL(k_ffr_expand_dict, dim3(bf_grid(m, 256, 4096)), dim3(256), 0, st, L.ranges, nranges, m, d_range,
                               d_src, d_src_off, d_src_len, d_index, d_idx_off, d_member, d_mem_off, d_split_result, d_dst_off, T,
                               *dd, L.e_off.p, L.e_len.p);
        else
            hipLaunchKernelGGL(k_ffr_expand, dim3(bf_grid(m, 256, 4096)), dim3(256), 0, st, L.ranges, nranges, m, d_range, d_src,
                               d_src_off, d_src_len, d_index, d_idx_off, d_member, d_mem_off, d_split_result, d_dst_off, T);
        hipLaunchKernelGGL(k_bfd_verify, dim3(bf_grid(m, 64)), dim3(64), 0, st, d_src, L.data_off, L.data_len, L.flags,
                           L.cks_off, m, L.cks_ok);
        if (dd ? zlz4_launch_decompress_safe_using_dict(st, d_src, L.data_off, L.f_len, d_dst, L.out_off, L.f_cap, L.sizes_f, m,
                                                        dd->dict, L.e_off, L.e_len) != 0 ||
                     zlz4_launch_decompress_safe_prefix_using_dict(st, d_src, L.data_off, L.p_len, d_dst, L.out_off, L.p_cap,
                                                                   L.sizes_p, m, dd->dict, L.e_off, L.e_len) != 0
               : zlz4_launch_decompress_safe(st, d_src, L.data_off, L.f_len, d_dst, L.out_off, L.f_cap, L.sizes_f, m) != 0 ||
                     zlz4_launch_decompress_safe_prefix(st, d_src, L.data_off, L.p_len, d_dst, L.out_off, L.p_cap, L.sizes_p,
                                                        m) != 0)
            return ZLZ4_ERR_DEVICE;
        hipLaunchKernelGGL(k_bfr_copy, dim3(m), dim3(256), 0, st, d_src, L.data_off, L.c_len, L.out_off, d_dst);
    }
    hipLaunchKernelGGL(k_bfr_finish, dim3(gr), dim3(256), 0, st, L.ranges, nranges, m, T, L.cks_ok, L.sizes_f, L.sizes_p, d_skip,
                       d_result);
    return hipGetLastError() == hipSuccess ? 0 : ZLZ4_ERR_DEVICE;
}

}  // namespace

extern "C" {

size_t zlz4f_batch_file_index_workspace(uint32_t nbuf, const uint64_t *split_totals) {
    uint32_t nitems, mb, lb;
    return ff_totals(split_totals, nitems, mb, lb) ? ff_layout(nbuf, nitems, mb, lb).bytes : 0;
}

int32_t zlz4f_batch_file_index(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                               uint32_t nbuf, const zlz4f_member *d_member, const uint64_t *d_mem_off,
                               const int64_t *d_split_result, const uint64_t *d_item_first, const uint64_t *d_item_off,
                               const uint64_t *d_item_len, const uint64_t *d_leg_len, const uint64_t *split_totals,
                               zlz4f_index_entry *d_index, uint64_t *d_idx_off, uint64_t idx_cap, int64_t *d_result,
                               void *d_workspace, size_t workspace_bytes) {
    return ff_index_impl(stream, d_src, d_src_off, d_src_len, nbuf, d_member, d_mem_off, d_split_result, d_item_first, d_item_off,
                         d_item_len, d_leg_len, split_totals, d_index, d_idx_off, idx_cap, d_result, d_workspace, workspace_bytes);
}

size_t zlz4f_batch_decompress_file_range_workspace(uint32_t nranges, uint32_t max_items) {
    return bfr_layout(nranges, max_items).bytes;
}

int32_t zlz4f_batch_decompress_file_range(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                          const uint64_t *d_src_len, const zlz4f_index_entry *d_index,
                                          const uint64_t *d_idx_off, const int64_t *d_idx_n, uint32_t nbuf,
                                          const zlz4f_member *d_member, const uint64_t *d_mem_off,
                                          const int64_t *d_split_result, const zlz4f_range *d_range, uint8_t *d_dst,
                                          const uint64_t *d_dst_off, const uint64_t *d_dst_cap, uint64_t *d_skip,
                                          int64_t *d_result, uint32_t nranges, uint32_t max_items, void *d_workspace,
                                          size_t workspace_bytes) {
    return ff_range_impl(stream, d_src, d_src_off, d_src_len, d_index, d_idx_off, d_idx_n, nbuf, d_member, d_mem_off,
                         d_split_result, d_range, d_dst, d_dst_off, d_dst_cap, d_skip, d_result, nranges, max_items, d_workspace,
                         workspace_bytes);
}

// ---- the dictionary forms: a FILE has at most one dictionary, d_dict_idx has nbuf entries
size_t zlz4f_batch_file_index_using_dict_workspace(uint32_t nbuf, const uint64_t *split_totals) {
    uint32_t nitems, mb, lb;
    return ff_totals(split_totals, nitems, mb, lb) ? ff_layout(nbuf, nitems, mb, lb, nullptr, true).bytes : 0;
}

int32_t zlz4f_batch_file_index_using_dict(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                          const uint64_t *d_src_len, uint32_t nbuf, const zlz4f_member *d_member,
                                          const uint64_t *d_mem_off, const int64_t *d_split_result,
                                          const uint64_t *d_item_first, const uint64_t *d_item_off, const uint64_t *d_item_len,
                                          const uint64_t *d_leg_len, const uint64_t *split_totals, zlz4f_index_entry *d_index,
                                          uint64_t *d_idx_off, uint64_t idx_cap, int64_t *d_result, const uint32_t *d_dict_len,
                                          uint32_t ndicts, const uint32_t *d_dict_idx, void *d_workspace,
                                          size_t workspace_bytes) {
    const BfDict dd = {nullptr, nullptr, d_dict_len, ndicts, d_dict_idx};
    return ff_index_impl(stream, d_src, d_src_off, d_src_len, nbuf, d_member, d_mem_off, d_split_result, d_item_first, d_item_off,
                         d_item_len, d_leg_len, split_totals, d_index, d_idx_off, idx_cap, d_result, d_workspace, workspace_bytes,
                         &dd);
}

size_t zlz4f_batch_decompress_file_range_using_dict_workspace(uint32_t nranges, uint32_t max_items) {
    return bfr_layout(nranges, max_items, nullptr, true).bytes;
}

int32_t zlz4f_batch_decompress_file_range_using_dict(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                                     const uint64_t *d_src_len, const zlz4f_index_entry *d_index,
                                                     const uint64_t *d_idx_off, const int64_t *d_idx_n, uint32_t nbuf,
                                                     const zlz4f_member *d_member, const uint64_t *d_mem_off,
                                                     const int64_t *d_split_result, const zlz4f_range *d_range, uint8_t *d_dst,
                                                     const uint64_t *d_dst_off, const uint64_t *d_dst_cap, uint64_t *d_skip,
                                                     int64_t *d_result, uint32_t nranges, uint32_t max_items,
                                                     const uint8_t *d_dict, const uint64_t *d_dict_off,
                                                     const uint32_t *d_dict_len, uint32_t ndicts, const uint32_t *d_dict_idx,
                                                     void *d_workspace, size_t workspace_bytes) {
    const BfDict dd = {d_dict, d_dict_off, d_dict_len, ndicts, d_dict_idx};
    return ff_range_impl(stream, d_src, d_src_off, d_src_len, d_index, d_idx_off, d_idx_n, nbuf, d_member, d_mem_off,
                         d_split_result, d_range, d_dst, d_dst_off, d_dst_cap, d_skip, d_result, nranges, max_items, d_workspace,
                         workspace_bytes, &dd);
}

// One launch, one lane per item.  nbuf == 0 or nitems == 0 returns 0.
int32_t zlz4f_batch_multiframe_item_dicts(void *stream, const uint64_t *d_item_first, uint32_t nbuf, uint32_t nitems,
                                          const uint32_t *d_dict_idx, uint32_t *d_item_dict_idx) {
    if (nbuf == 0 || nitems == 0) return 0;
    if (!d_item_first || !d_item_dict_idx || bf_misaligned(d_item_first, 8) || bf_misaligned(d_dict_idx, 4) ||
        bf_misaligned(d_item_dict_idx, 4))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    hipLaunchKernelGGL(k_ffd_item_dicts, dim3(bf_grid(nitems, 256)), dim3(256), 0, (hipStream_t)stream, d_item_first, nbuf, nitems,
                       d_dict_idx, d_item_dict_idx);
    return hipGetLastError() == hipSuccess ? 0 : ZLZ4_ERR_DEVICE;
}

}  // extern "C"

namespace {

// One file from host memory: split (count, record), index, plan and range as a batch of one.  The index is built on every
// call.  d_dict: the staged tail T of the file's dictionary, D bytes (zlz4f_decompress_file_range_using_dict), else null.
int64_t ff_host_range(const uint8_t *src, size_t n, uint64_t a, uint64_t b, uint8_t *dst, size_t cap, uint32_t split_flags,
                      const uint8_t *tail, uint32_t D) {
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    struct Rec {
        uint64_t src_off, src_len, count, totals[4], mem_off, mem_cap, item_first[2], idx_off[2], dst_off, dst_cap, skip,
            plan_totals[2], dict_off;
        int64_t split_result, idx_n, rres;
        zlz4f_range range;
        uint32_t dict_len, pad;
    };
    DevBuf d_src(n, &dc);
    std::optional<DevBuf> d_dict;                                       // (the plain call keeps its allocations)
    if (tail) d_dict.emplace(D, &dc);
    Staged<Rec> rec(&dc, 256);
    if (!d_src.p || !rec.d || (tail && !d_dict->p)) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.src_len = n;
    rec.h.range.a = a; rec.h.range.b = b;
    rec.h.dict_len = D;
    dc.launched();
    if (!upload(d_src, src, n, st) || !rec.upload(st) || (tail && !upload(*d_dict, tail, D, st))) return ZLZ4_ERR_DEVICE;
    Rec *r = rec.d;
    const uint8_t *s = d_src.as<uint8_t>();
    int32_t rc = zlz4f_batch_multiframe_split_ex(st, s, &r->src_off, &r->src_len, 1, &r->count, r->totals, nullptr, nullptr,
                                                 nullptr, nullptr, nullptr, nullptr, nullptr, split_flags, nullptr);
    if (rc != 0) return rc;
    uint64_t totals[4] = {0, 0, 0, 0};
    if (hipMemcpyAsync(totals, r->totals, 32, hipMemcpyDeviceToHost, st) != hipSuccess || !dc.sync()) return ZLZ4_ERR_DEVICE;
    if (totals[0] == 0) return 0;                                      // the empty file: S == 0
    if (totals[0] > 0xFFFFFFFFull || totals[1] > 0xFFFFFFFFull || totals[3] > 0xFFFFFFFFull) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    const size_t nitems = (size_t)totals[0];
    const uint64_t idx_cap = totals[1] + totals[3] + 1u;
    const BfDict dd = {tail ? d_dict->as<uint8_t>() : nullptr, &r->dict_off, &r->dict_len, 1, nullptr};
    const BfDict *ddp = tail ? &dd : nullptr;
    const size_t iws = ff_layout(1, (uint32_t)totals[0], (uint32_t)totals[1], (uint32_t)totals[3], nullptr, ddp != nullptr).bytes;
    DevBuf d_mem(nitems * sizeof(zlz4f_member), &dc), d_items(nitems * 24u, &dc), d_iws(iws, &dc),
        d_index((size_t)idx_cap * sizeof(zlz4f_index_entry), &dc);
    if (!d_mem.p || !d_items.p || !d_iws.p || !d_index.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    rec.h.mem_cap = nitems;
    dc.launched();
    if (hipMemcpyAsync(&r->mem_cap, &rec.h.mem_cap, 8, hipMemcpyHostToDevice, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
    zlz4f_member *mem = d_mem.as<zlz4f_member>();
    uint64_t *item_off = d_items.as<uint64_t>(), *item_len = item_off + nitems, *leg_len = item_len + nitems;
    zlz4f_index_entry *index = d_index.as<zlz4f_index_entry>();
    rc = zlz4f_batch_multiframe_split_ex(st, s, &r->src_off, &r->src_len, 1, &r->count, r->totals, mem, &r->mem_off, &r->mem_cap,
                                         r->item_first, item_off, item_len, &r->split_result, split_flags, leg_len);
    if (rc != 0) return rc;
    rc = ff_index_impl(st, s, &r->src_off, &r->src_len, 1, mem, &r->mem_off, &r->split_result, r->item_first, item_off, item_len,
                       leg_len, totals, index, r->idx_off, idx_cap, &r->idx_n, d_iws.p, iws, ddp);
    if (rc != 0) return rc;
    rc = zlz4f_batch_plan_frame_ranges(st, index, r->idx_off, &r->idx_n, 1, &r->range, 1, 0, &r->dst_off, &r->dst_cap,
                                       r->plan_totals);
    if (rc != 0) return rc;
    int64_t idx_n = 0;
    uint64_t plan[2] = {0, 0};
    if (hipMemcpyAsync(&idx_n, &r->idx_n, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(plan, r->plan_totals, 16, hipMemcpyDeviceToHost, st) != hipSuccess || !dc.sync())
        return ZLZ4_ERR_DEVICE;
    if (idx_n < 0) return idx_n;
    if ((uint64_t)idx_n >= idx_cap) return ZLZ4_ERR_DEVICE;          // (the fold's count is the walks', as the totals are)
    zlz4f_index_entry last = {0, 0};
    if (hipMemcpy(&last, index + idx_n, sizeof last, hipMemcpyDeviceToHost) != hipSuccess) return ZLZ4_ERR_DEVICE;
    const uint64_t S = last.dec, a1 = a < S ? a : S, b1 = b < S ? b : S;
    if (cap < b1 - a1) return ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL;
    if (plan[1] > 0xFFFFFFFFull) return ZLZ4F_ERR_SRC_SIZE_TOO_LARGE;
    const uint32_t max_items = (uint32_t)plan[1];
    const size_t rws = bfr_layout(1, max_items, nullptr, ddp != nullptr).bytes;
    DevBuf d_rws(rws, &dc), d_dst((size_t)plan[0], &dc);
    if (!d_rws.p || !d_dst.p) return ZLZ4F_ERR_ALLOCATION_FAILED;
    dc.launched();
    rc = ff_range_impl(st, s, &r->src_off, &r->src_len, index, r->idx_off, &r->idx_n, 1, mem, &r->mem_off, &r->split_result,
                       &r->range, d_dst.as<uint8_t>(), &r->dst_off, &r->dst_cap, &r->skip, &r->rres, 1, max_items, d_rws.p, rws,
                       ddp);
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

int64_t zlz4f_decompress_file_range(const uint8_t *src, size_t n, uint64_t a, uint64_t b, uint8_t *dst, size_t cap,
                                    uint32_t split_flags) {
    if (split_flags & ~ZLZ4F_SPLIT_LEGACY) return ZLZ4F_ERR_PARAMETER_INVALID;
    if ((!src && n) || (!dst && cap) || a > b) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return ff_host_range(src, n, a, b, dst, cap, split_flags, nullptr, 0);
}

// zlz4f_decompress_file_range with the D > 0 bytes of a dictionary's tail: what zlz4f_decompress_file_range_using_dict
// (zlz4_frame_seek.hip), which has made the refusals, runs where the file's seek table is not used
int64_t zlz4_host_file_range_dict(const uint8_t *src, size_t n, uint64_t a, uint64_t b, uint8_t *dst, size_t cap,
                                  uint32_t split_flags, const uint8_t *tail, uint32_t D) {
    return ff_host_range(src, n, a, b, dst, cap, split_flags, tail, D);
}

}  // extern "C"
