// zlz4_capi.hip -- the C ABI declared in include/zlz4_amd.h.
//
// Host side of the MI355X LZ4 codec: validates arguments the way the reference
// entry points do (src/lz4.zig, src/lz4hc.zig, src/lz4f.zig -- cited per function),
// stages host buffers, and enqueues the gfx950 kernels.  There is no CPU codec in
// here: without a usable HIP device every compute call returns ZLZ4_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/zlz4_amd.h"
#include "zlz4_host.hpp"
#include "zlz4_launch.hpp"

using namespace zlz4host;

namespace {

enum class Op { Fast, Hc, Decompress, DecompressDict, DecompressBound, DecompressPrefix, DecompressPrefixDict };

// One block, host pointers: stage -> kernel -> copy back.  Op::DecompressDict stages the tail of `dict` (dict_tail,
// zlz4_host.hpp).  Op::DecompressBound decodes with the StreamDecode bound `bound` (k_decompress_safe, kBound).
// Op::DecompressPrefix / DecompressPrefixDict: the prefix decoder (kPartial), dst_cap bytes wanted; the second stages the
// dictionary's tail like Op::DecompressDict.
int64_t run_single(Op op, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, uint32_t accel,
                   int32_t level, const uint8_t *dict = nullptr, size_t dict_len = 0, uint32_t bound = 0) {
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    if (src_len > 0xFFFFFFFFull)
        return op == Op::Decompress || op == Op::DecompressPrefix || op == Op::DecompressPrefixDict ? ZLZ4_ERR_CORRUPTED_DATA
                                                                                                  : ZLZ4_ERR_INPUT_TOO_LARGE;
    const uint32_t cap32 = clamp_cap32(dst_cap), len32 = (uint32_t)src_len;

    // scratch from the parked-buffer cache (zlz4_host.hpp): a caller that loops over single blocks does not pay a
    // hipMalloc / hipFree pair per call
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    const size_t ws = op == Op::Hc ? zlz4_hc_workspace_bytes(1, len32) : 0;
    const size_t dtail = op == Op::DecompressDict || op == Op::DecompressPrefixDict ? dict_tail(dict_len) : 0;
    DevBuf d_in(src_len, &dc), d_out(cap32, &dc);
    Staged<BlockRec> rec(&dc);
    DevBuf d_ws(ws, &dc), d_dict(dtail, &dc);
    if (!d_in.p || !d_out.p || !rec.d || !d_ws.p || !d_dict.p) return ZLZ4_ERR_ALLOCATION_FAILED;
    rec.h.in_len = len32; rec.h.out_cap = cap32; rec.h.dict_len = (uint32_t)dtail; rec.h.bound = bound;
    dc.launched();
    if (!upload(d_in, src, src_len, st) || !upload(d_dict, dict + (dict_len - dtail), dtail, st) || !rec.upload(st))
        return ZLZ4_ERR_DEVICE;
    BlockRec *r = rec.d;
    const uint8_t *in = d_in.as<uint8_t>();
    uint8_t *out = d_out.as<uint8_t>();
    int rc;
    if (op == Op::Fast) {
        rc = zlz4_launch_compress_fast(st, in, &r->in_off, &r->in_len, out, &r->out_off, &r->out_cap, &r->result, 1, len32,
                                       accel);
    } else if (op == Op::Hc) {
        rc = zlz4_launch_compress_hc(st, in, &r->in_off, &r->in_len, out, &r->out_off, &r->out_cap, &r->result, 1, len32,
                                     level, d_ws.p, ws);
    } else if (op == Op::Decompress) {
        rc = zlz4_launch_decompress_safe(st, in, &r->in_off, &r->in_len, out, &r->out_off, &r->out_cap, &r->result, 1);
    } else if (op == Op::DecompressBound) {
        rc = zlz4_launch_decompress_safe_bound(st, in, &r->in_off, &r->in_len, out, &r->out_off, &r->out_cap, &r->result, 1,
                                               nullptr, &r->dict_off, &r->dict_len, 0);
    } else if (op == Op::DecompressPrefix) {
        rc = zlz4_launch_decompress_safe_prefix(st, in, &r->in_off, &r->in_len, out, &r->out_off, &r->out_cap, &r->result, 1);
    } else if (op == Op::DecompressPrefixDict) {
        rc = zlz4_launch_decompress_safe_prefix_using_dict(st, in, &r->in_off, &r->in_len, out, &r->out_off, &r->out_cap,
                                                           &r->result, 1, d_dict.as<uint8_t>(), &r->dict_off, &r->dict_len);
    } else {
        rc = zlz4_launch_decompress_safe_using_dict(st, in, &r->in_off, &r->in_len, out, &r->out_off, &r->out_cap,
                                                    &r->result, 1, d_dict.as<uint8_t>(), &r->dict_off, &r->dict_len);
    }
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result) || !copy_back(dst, dst_cap, d_out, result)) return ZLZ4_ERR_DEVICE;
    return result;
}

// decompressGeneric with targetOutputSize == 0 and a non-empty dst (src/lz4.zig:111-174): no byte can be produced, the
// result is decided by the first sequence header alone -- nothing to run on the device.  Every exit comes before the
// match-source tests (:181-192), so it holds with and without a dictionary.
int64_t partial_target_zero(const uint8_t *src, size_t n) {
    size_t ip = 0;
    const uint8_t token = src[ip++];
    size_t lit = token >> 4;
    if (lit == 15) {
        for (;;) {
            if (ip >= n) return ZLZ4_ERR_CORRUPTED_DATA;            // :125
            const uint8_t s = src[ip++];
            lit += s;
            if (s != 255) break;
        }
    }
    if (lit > 0) {
        if (ip + lit > n) return ZLZ4_ERR_CORRUPTED_DATA;           // :136
        return ZLZ4_ERR_OUTPUT_TOO_SMALL;                           // :137 (op + lit > 0)
    }
    if (ip >= n) return 0;                                          // :146
    if (ip + 2 > n) return ZLZ4_ERR_CORRUPTED_DATA;                 // :149
    if ((src[ip] | (src[ip + 1] << 8)) == 0) return ZLZ4_ERR_CORRUPTED_DATA;   // :154
    ip += 2;
    if ((token & 15) == 15) {
        for (;;) {
            if (ip >= n) return ZLZ4_ERR_CORRUPTED_DATA;            // :162
            if (src[ip++] != 255) break;
        }
    }
    return ZLZ4_ERR_OUTPUT_TOO_SMALL;                               // :174 (op + matchLength > 0)
}

// Stream.loadDict / compressFastContinue on a HOST table of 4096 u32: the table is staged with the data, the kernel
// updates it in place on the device, and it is copied back.  src == nullptr: loadDict of `dict` (its tail is staged);
// else compressFastContinue of src[0..src_len).
int64_t run_stream_single(uint32_t *table, const uint8_t *dict, size_t dict_len, const uint8_t *src, size_t src_len,
                          uint8_t *dst, size_t dst_cap, uint32_t accel) {
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    const bool load = src == nullptr;
    const size_t in_len = load ? dict_tail(dict_len) : src_len;
    const uint8_t *in = load ? dict + (dict_len - in_len) : src;
    const uint32_t cap32 = clamp_cap32(dst_cap);
    const size_t tbytes = ZLZ4_STREAM_TABLE_ENTRIES * sizeof(uint32_t);
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    DevBuf d_in(in_len, &dc), d_out(load ? 0 : cap32, &dc);
    Staged<BlockRec> rec(&dc);
    DevBuf d_tab(tbytes, &dc);
    if (!d_in.p || !d_out.p || !rec.d || !d_tab.p) return ZLZ4_ERR_ALLOCATION_FAILED;
    rec.h.in_len = (uint32_t)in_len; rec.h.out_cap = cap32;
    dc.launched();
    if (!upload(d_in, in, in_len, st) || !(load || upload(d_tab, table, tbytes, st)) || !rec.upload(st))
        return ZLZ4_ERR_DEVICE;
    BlockRec *r = rec.d;
    int rc;
    if (load) {
        rc = zlz4_launch_load_dict(st, d_in.as<uint8_t>(), &r->in_off, &r->in_len, d_tab.as<uint32_t>(), &r->result, 1);
    } else {
        rc = zlz4_launch_compress_fast_continue(st, d_in.as<uint8_t>(), &r->in_off, &r->in_len, d_out.as<uint8_t>(),
                                                &r->out_off, &r->out_cap, d_tab.as<uint32_t>(), nullptr,
                                                d_tab.as<uint32_t>(), &r->result, 1, (uint32_t)in_len, accel);
    }
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result)) return ZLZ4_ERR_DEVICE;
    if (!load && !copy_back(dst, dst_cap, d_out, result)) return ZLZ4_ERR_DEVICE;
    // the table is the reference's after the call on every exit (unchanged ones included)
    if (hipMemcpy(table, d_tab.p, tbytes, hipMemcpyDeviceToHost) != hipSuccess) return ZLZ4_ERR_DEVICE;
    return result;
}

// zlz4_compress_fast_using_dict for 1 <= src_len <= ZLZ4_MAX_INPUT_SIZE: the record and the tail of the dictionary are
// staged, k_load_dict builds the dictionary's table on the device and the batch kernel (zlz4_compress_dict.hip) runs on
// one block.
int64_t run_dict_compress_single(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, const uint8_t *dict,
                                 size_t dict_len, uint32_t accel) {
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    const uint32_t cap32 = clamp_cap32(dst_cap), len32 = (uint32_t)src_len;
    const size_t dtail = dict_tail(dict_len);
    const size_t tbytes = ZLZ4_STREAM_TABLE_ENTRIES * sizeof(uint32_t);
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    DevBuf d_in(src_len, &dc), d_out(cap32, &dc);
    Staged<BlockRec> rec(&dc);
    DevBuf d_dict(dtail, &dc), d_tab(tbytes, &dc);
    if (!d_in.p || !d_out.p || !rec.d || !d_dict.p || !d_tab.p) return ZLZ4_ERR_ALLOCATION_FAILED;
    rec.h.in_len = len32; rec.h.out_cap = cap32; rec.h.dict_len = (uint32_t)dtail;
    dc.launched();
    if (!upload(d_in, src, src_len, st) || !upload(d_dict, dict + (dict_len - dtail), dtail, st) || !rec.upload(st))
        return ZLZ4_ERR_DEVICE;
    BlockRec *r = rec.d;
    int rc = zlz4_launch_load_dict(st, d_dict.as<uint8_t>(), &r->dict_off, &r->dict_len, d_tab.as<uint32_t>(), &r->dict_size, 1);
    if (rc != 0) return rc;
    rc = zlz4_launch_compress_fast_using_dict(st, d_in.as<uint8_t>(), &r->in_off, &r->in_len, d_out.as<uint8_t>(), &r->out_off,
                                              &r->out_cap, d_dict.as<uint8_t>(), &r->dict_off, &r->dict_len,
                                              d_tab.as<uint32_t>(), nullptr, &r->result, 1, len32, (uint32_t)dtail, accel);
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result) || !copy_back(dst, dst_cap, d_out, result)) return ZLZ4_ERR_DEVICE;
    return result;
}

// zlz4_compress_hc_using_dict for 1 <= src_len <= ZLZ4_MAX_INPUT_SIZE and a level of 3..9: the record and the tail of the
// dictionary are staged and the batch pipeline runs on one block.
int64_t run_hc_dict_single(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, const uint8_t *dict,
                           size_t dict_len, int32_t level) {
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    const uint32_t cap32 = clamp_cap32(dst_cap), len32 = (uint32_t)src_len;
    const size_t dtail = dict_tail(dict_len);
    const size_t ws = zlz4_hc_dict_workspace_bytes(1, len32, (uint32_t)dtail);
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    DevBuf d_in(src_len, &dc), d_out(cap32, &dc);
    Staged<BlockRec> rec(&dc);
    DevBuf d_dict(dtail, &dc), d_ws(ws, &dc);
    if (!d_in.p || !d_out.p || !rec.d || !d_dict.p || !d_ws.p) return ZLZ4_ERR_ALLOCATION_FAILED;
    rec.h.in_len = len32; rec.h.out_cap = cap32; rec.h.dict_len = (uint32_t)dtail;
    dc.launched();
    if (!upload(d_in, src, src_len, st) || !upload(d_dict, dict + (dict_len - dtail), dtail, st) || !rec.upload(st))
        return ZLZ4_ERR_DEVICE;
    BlockRec *r = rec.d;
    const int rc = zlz4_launch_compress_hc_dict(st, d_in.as<uint8_t>(), &r->in_off, &r->in_len, d_out.as<uint8_t>(), &r->out_off,
                                                &r->out_cap, d_dict.as<uint8_t>(), &r->dict_off, &r->dict_len, &r->result, 1,
                                                len32, (uint32_t)dtail, level, d_ws.p, ws);
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result) || !copy_back(dst, dst_cap, d_out, result)) return ZLZ4_ERR_DEVICE;
    return result;
}

// the level compressHC runs (src/lz4hc.zig:1446-1452), or 0 where the dictionary call has none: 2 (lz4mid) and 10..12
int32_t hc_dict_level(int32_t level) {
    if (level < 2) level = ZLZ4HC_CLEVEL_DEFAULT;
    if (level > ZLZ4HC_CLEVEL_MAX) level = ZLZ4HC_CLEVEL_MAX;
    return level >= 3 && level <= 9 ? level : 0;
}

// compressDestSize's search branch (src/lz4.zig:567-615) for 1 <= *src_size <= ZLZ4_MAX_INPUT_SIZE and dst_cap below
// compressBound: the batch pipeline (zlz4_dest_size.hip) as a batch of one.  One upload (descriptors + input), two
// launches, one read-back (output slot + results): the device does the whole search.
int64_t dest_size_batch_of_one(const uint8_t *src, uint8_t *dst, size_t cap, size_t *src_size) {
    const uint32_t n = (uint32_t)*src_size;
    const uint32_t cap32 = (uint32_t)cap;                     // < compressBound(n) <= 2^31
    struct Rec {
        uint64_t in_off, out_off, slot_off; int64_t result; uint32_t in_len, out_cap, slot_cap, consumed;
    };
    const size_t out_bytes = ((size_t)cap32 + 15u) & ~(size_t)15u;   // [out | record | input]
    const size_t rec_bytes = (sizeof(Rec) + 15u) & ~(size_t)15u;
    const size_t ws_bytes = zlz4_dest_size_workspace_bytes(1, n);
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    DevBuf d_buf(out_bytes + rec_bytes + n, &dc), d_ws(ws_bytes, &dc);
    if (!d_buf.p || !d_ws.p) return ZLZ4_ERR_ALLOCATION_FAILED;
    std::vector<uint8_t> h(rec_bytes + n);
    Rec m;
    std::memset(&m, 0, sizeof m);
    m.in_off = rec_bytes;                                     // relative to the record
    m.in_len = n;
    m.out_off = 0;
    m.out_cap = cap32;
    m.slot_off = 0;
    m.slot_cap = zlz4_dest_size_slot_cap(n);
    std::memcpy(h.data(), &m, sizeof m);
    std::memcpy(h.data() + rec_bytes, src, n);
    uint8_t *dm = d_buf.as<uint8_t>() + out_bytes;
    Rec *r = reinterpret_cast<Rec *>(dm);
    dc.launched();
    if (hipMemcpyAsync(dm, h.data(), h.size(), hipMemcpyHostToDevice, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
    const int rc = zlz4_launch_compress_dest_size(st, dm, &r->in_off, &r->in_len, d_buf.as<uint8_t>(), &r->out_off, &r->out_cap,
                                                  &r->result, &r->consumed, 1, n, d_ws.p, &r->slot_off, &r->slot_cap);
    if (rc != 0) return rc;
    std::vector<uint8_t> back(out_bytes + sizeof(Rec));
    if (hipMemcpyAsync(back.data(), d_buf.p, back.size(), hipMemcpyDeviceToHost, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
    if (!dc.sync()) return ZLZ4_ERR_DEVICE;
    std::memcpy(&m, back.data() + out_bytes, sizeof m);
    if (m.result < 0) return m.result;
    if ((uint64_t)m.result > cap || m.consumed > n) return ZLZ4_ERR_DEVICE;   // cannot happen; never overrun the caller
    if (m.result > 0) std::memcpy(dst, back.data(), (size_t)m.result);
    *src_size = m.consumed;
    return m.result;
}

// src/lz4hc.zig:1445 + :1464-1466 level normalisation, strategy table :72-86
int32_t normalise_hc_level(int32_t level) {
    if (level < ZLZ4HC_CLEVEL_MIN) level = ZLZ4HC_CLEVEL_DEFAULT;
    if (level > ZLZ4HC_CLEVEL_MAX) level = ZLZ4HC_CLEVEL_MAX;
    return level;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- introspection
int32_t zlz4_device_check(void) { return device_ok() ? 0 : ZLZ4_ERR_DEVICE; }

const char *zlz4_version_string(void) { return "zlz4-amd 0.1.0 (gfx950)"; }

const char *zlz4_error_name(int64_t code) {
    switch (code) {
        case ZLZ4_ERR_OUTPUT_TOO_SMALL: return "OutputTooSmall";
        case ZLZ4_ERR_INPUT_TOO_LARGE: return "InputTooLarge";
        case ZLZ4_ERR_CORRUPTED_DATA: return "CorruptedData";
        case ZLZ4_ERR_DECOMPRESSION_FAILED: return "DecompressionFailed";
        case ZLZ4_ERR_INVALID_STATE: return "InvalidState";
        case ZLZ4_ERR_ALLOCATION_FAILED: return "AllocationFailed";
        case ZLZ4_ERR_DEVICE: return "DeviceError";
        case ZLZ4_ERR_UNSUPPORTED: return "Unsupported";
        case ZLZ4_ERR_VERIFY: return "VerifyFailed";
        case ZLZ4F_ERR_GENERIC: return "Generic";
        case ZLZ4F_ERR_MAX_BLOCK_SIZE_INVALID: return "MaxBlockSizeInvalid";
        case ZLZ4F_ERR_BLOCK_MODE_INVALID: return "BlockModeInvalid";
        case ZLZ4F_ERR_PARAMETER_INVALID: return "ParameterInvalid";
        case ZLZ4F_ERR_COMPRESSION_LEVEL_INVALID: return "CompressionLevelInvalid";
        case ZLZ4F_ERR_HEADER_VERSION_WRONG: return "HeaderVersionWrong";
        case ZLZ4F_ERR_BLOCK_CHECKSUM_INVALID: return "BlockChecksumInvalid";
        case ZLZ4F_ERR_RESERVED_FLAG_SET: return "ReservedFlagSet";
        case ZLZ4F_ERR_ALLOCATION_FAILED: return "AllocationFailed";
        case ZLZ4F_ERR_SRC_SIZE_TOO_LARGE: return "SrcSizeTooLarge";
        case ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL: return "DstMaxSizeTooSmall";
        case ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE: return "FrameHeaderIncomplete";
        case ZLZ4F_ERR_FRAME_TYPE_UNKNOWN: return "FrameTypeUnknown";
        case ZLZ4F_ERR_FRAME_SIZE_WRONG: return "FrameSizeWrong";
        case ZLZ4F_ERR_SRC_PTR_WRONG: return "SrcPtrWrong";
        case ZLZ4F_ERR_DECOMPRESSION_FAILED: return "DecompressionFailed";
        case ZLZ4F_ERR_HEADER_CHECKSUM_INVALID: return "HeaderChecksumInvalid";
        case ZLZ4F_ERR_CONTENT_CHECKSUM_INVALID: return "ContentChecksumInvalid";
        default: return code >= 0 ? "ok" : "unknown";
    }
}

// ---------------------------------------------------------------- single buffer, host pointers
size_t zlz4_compress_bound(size_t n) {                      // src/lz4.zig:80-83
    if (n > ZLZ4_MAX_INPUT_SIZE) return 0;
    return n + (n / 255) + 16;
}

int64_t zlz4_compress_fast(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, uint32_t accel) {
    if (n > ZLZ4_MAX_INPUT_SIZE) return ZLZ4_ERR_INPUT_TOO_LARGE;   // src/lz4.zig:296
    if (n == 0) return 0;                                           // :299
    return run_single(Op::Fast, src, n, dst, cap, accel, 0);
}

int64_t zlz4_compress_default(const uint8_t *src, size_t n, uint8_t *dst, size_t cap) {   // src/lz4.zig:283-285
    return zlz4_compress_fast(src, n, dst, cap, 1);
}

int64_t zlz4_compress_hc(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, int32_t level) {
    if (n > ZLZ4_MAX_INPUT_SIZE) return ZLZ4_ERR_INPUT_TOO_LARGE;   // src/lz4hc.zig:1442
    if (n == 0) return 0;                                           // :1443
    if (cap == 0) return ZLZ4_ERR_OUTPUT_TOO_SMALL;                 // :1461
    level = normalise_hc_level(level);                              // 2 lz4mid, 3-9 lz4hc, 10-12 lz4opt (:72-86)
    return run_single(Op::Hc, src, n, dst, cap, 0, level);
}

int64_t zlz4_decompress_safe(const uint8_t *src, size_t n, uint8_t *dst, size_t cap) {
    if (n == 0) return 0;                                           // src/lz4.zig:97
    if (cap == 0) return 0;                                         // :98
    return run_single(Op::Decompress, src, n, dst, cap, 0, 0);
}

int64_t zlz4_decompress_safe_partial(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t target) {
    if (n == 0) return 0;                                           // src/lz4.zig:97
    if (cap == 0) return 0;                                         // :98
    if (target > cap) return ZLZ4_ERR_OUTPUT_TOO_SMALL;             // :99
    if (target > 0) return run_single(Op::Decompress, src, n, dst, target, 0, 0);   // oend = targetOutputSize (:109)
    return partial_target_zero(src, n);
}

int64_t zlz4_decompress_safe_using_dict(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const uint8_t *dict,
                                        size_t dict_len) {                   // src/lz4.zig:960-962
    if (n == 0) return 0;                                           // :97
    if (cap == 0) return 0;                                         // :98
    if (!dict && dict_len) return ZLZ4_ERR_INVALID_STATE;
    return run_single(Op::DecompressDict, src, n, dst, cap, 0, 0, dict, dict_len);
}

int64_t zlz4_decompress_safe_partial_using_dict(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t target,
                                                const uint8_t *dict, size_t dict_len) {   // src/lz4.zig:967-969
    if (n == 0) return 0;                                           // :97
    if (cap == 0) return 0;                                         // :98
    if (target > cap) return ZLZ4_ERR_OUTPUT_TOO_SMALL;             // :99
    if (!dict && dict_len) return ZLZ4_ERR_INVALID_STATE;
    if (target > 0) return run_single(Op::DecompressDict, src, n, dst, target, 0, 0, dict, dict_len);
    return partial_target_zero(src, n);
}

// prefix decoding (include/zlz4_amd.h): dst_cap is the number of bytes wanted and the size of dst
int64_t zlz4_decompress_safe_prefix(const uint8_t *src, size_t n, uint8_t *dst, size_t cap) {
    if (n == 0) return 0;                                           // src/lz4.zig:97
    if (cap == 0) return 0;                                         // :98
    return run_single(Op::DecompressPrefix, src, n, dst, cap, 0, 0);
}

int64_t zlz4_decompress_safe_prefix_using_dict(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const uint8_t *dict,
                                               size_t dict_len) {
    if (n == 0) return 0;                                           // :97
    if (cap == 0) return 0;                                         // :98
    if (!dict && dict_len) return ZLZ4_ERR_INVALID_STATE;
    return run_single(Op::DecompressPrefixDict, src, n, dst, cap, 0, 0, dict, dict_len);
}

void zlz4_stream_decode_init(zlz4_stream_decode_t *sd) {          // src/lz4.zig:893-901
    if (sd) *sd = zlz4_stream_decode_t{0, 0, 0, 0};
}

void zlz4_set_stream_decode(zlz4_stream_decode_t *sd, const uint8_t *dict, size_t dict_len) {   // :904-909
    if (!sd) return;
    sd->dict = (uint64_t)(uintptr_t)dict;
    sd->dict_len = dict ? (uint64_t)dict_len : 0;
    sd->prefix = 0;
    sd->prefix_len = 0;
}

int64_t zlz4_decompress_safe_continue(zlz4_stream_decode_t *sd, const uint8_t *src, size_t n, uint8_t *dst,
                                      size_t cap) {                 // :912-939
    if (!sd) return ZLZ4_ERR_INVALID_STATE;
    const uint64_t d = (uint64_t)(uintptr_t)dst;
    if (sd->prefix_len == 0 && sd->dict_len == 0) {                 // :914-921
        const int64_t r = zlz4_decompress_safe(src, n, dst, cap);
        if (r >= 0) { sd->prefix = d; sd->prefix_len = (uint64_t)r; }
        return r;
    }
    if (sd->dict_len > 0 && sd->prefix != 0) return ZLZ4_ERR_INVALID_STATE;   // (restStart would underflow, :213)
    int64_t r;
    if (sd->dict_len > 0 && sd->dict != 0) {                        // prefix null: lowPrefix = dst (:924-930)
        r = zlz4_decompress_safe_using_dict(src, n, dst, cap, (const uint8_t *)(uintptr_t)sd->dict, (size_t)sd->dict_len);
    } else {
        // lowPrefix = prefix (or dst), no dictionary: matches below it are CorruptedData (:181-185)
        const uint64_t low = sd->prefix ? sd->prefix : d;
        const uint64_t lo = low > d ? low - d : 0;
        if (lo == 0) r = zlz4_decompress_safe(src, n, dst, cap);
        else if (n == 0 || cap == 0) r = 0;                         // :97-98
        else r = run_single(Op::DecompressBound, src, n, dst, cap, 0, 0, nullptr, 0,
                            lo < 0xFFFF0000ull ? (uint32_t)lo : 0xFFFF0000u);
    }
    if (r >= 0) { sd->dict = 0; sd->dict_len = 0; sd->prefix = d; sd->prefix_len = (uint64_t)r; }   // :933-938
    return r;
}

// what decompressSafe / decompressSafeUsingDict would return into 0xFFFFFFFF bytes: the size kernel on one staged block
int64_t zlz4_decompressed_size(const uint8_t *src, size_t n, size_t dict_len) {
    if (n == 0) return 0;                                           // src/lz4.zig:97
    if (!src) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    if (n > 0xFFFFFFFFull) return ZLZ4_ERR_CORRUPTED_DATA;          // (as zlz4_decompress_safe)
    hipStream_t st = nullptr;
    DeviceCall dc(st);
    DevBuf d_in(n, &dc);
    Staged<BlockRec> rec(&dc);
    if (!d_in.p || !rec.d) return ZLZ4_ERR_ALLOCATION_FAILED;
    rec.h.in_len = (uint32_t)n; rec.h.dict_len = (uint32_t)dict_tail(dict_len);
    dc.launched();
    if (!upload(d_in, src, n, st) || !rec.upload(st)) return ZLZ4_ERR_DEVICE;
    BlockRec *r = rec.d;
    const int rc = zlz4_launch_decompressed_size(st, d_in.as<uint8_t>(), &r->in_off, &r->in_len, &r->dict_len, &r->result, 1);
    if (rc != 0) return rc;
    int64_t result = 0;
    if (!read_result(dc, &r->result, result)) return ZLZ4_ERR_DEVICE;
    return result;
}

size_t zlz4_decoder_ring_buffer_size(size_t max_block_size) {        // :954-957
    return max_block_size == 0 ? 0 : 65536 + 14 + max_block_size;
}

int64_t zlz4_stream_load_dict(uint32_t *table, const uint8_t *dict, size_t dict_len) {   // src/lz4.zig:798-820
    if (!table || (!dict && dict_len)) return ZLZ4_ERR_INVALID_STATE;
    return run_stream_single(table, dict, dict_len, nullptr, 0, nullptr, 0, 0);
}

int64_t zlz4_stream_compress_fast_continue(uint32_t *table, const uint8_t *src, size_t n, uint8_t *dst, size_t cap,
                                           uint32_t accel) {                  // src/lz4.zig:822-836
    if (!table) return ZLZ4_ERR_INVALID_STATE;
    if (n > ZLZ4_MAX_INPUT_SIZE) return ZLZ4_ERR_INPUT_TOO_LARGE;   // :823 (table untouched)
    if (n == 0) return 0;                                           // :824
    return run_stream_single(table, nullptr, 0, src, n, dst, cap, accel);
}

// DESIGN.md section 4.1c; the entry checks are compressFastContinue's (src/lz4.zig:823-824)
int64_t zlz4_compress_fast_using_dict(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const uint8_t *dict,
                                      size_t dict_len, uint32_t accel) {
    if (!dict && dict_len) return ZLZ4_ERR_INVALID_STATE;
    if (n > ZLZ4_MAX_INPUT_SIZE) return ZLZ4_ERR_INPUT_TOO_LARGE;   // :823
    if (n == 0) return 0;                                           // :824
    return run_dict_compress_single(src, n, dst, cap, dict, dict_len, accel);
}

// DESIGN.md section 4.3c; the entry checks are compressHC's and compressHCExtState's (src/lz4hc.zig:1442-1445, :1461)
int64_t zlz4_compress_hc_using_dict(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const uint8_t *dict,
                                    size_t dict_len, int32_t level) {
    if (!dict && dict_len) return ZLZ4_ERR_INVALID_STATE;
    level = hc_dict_level(level);
    if (level == 0) return ZLZ4_ERR_UNSUPPORTED;                    // as the batch call: before any record is looked at
    if (n > ZLZ4_MAX_INPUT_SIZE) return ZLZ4_ERR_INPUT_TOO_LARGE;   // :1442
    if (n == 0) return 0;                                           // :1443
    if (cap == 0) return ZLZ4_ERR_OUTPUT_TOO_SMALL;                 // :1461
    return run_hc_dict_single(src, n, dst, cap, dict, dict_len, level);
}

size_t zlz4_sizeof_state(void) { return 4096 * sizeof(uint32_t); }  // src/lz4.zig:524-526, :263-265

// src/lz4hc.zig:1492-1494: @sizeOf(Context) -- hashTable 32768 x u32 + chainTable 65536 x u16 (:391-393) + the scalars
size_t zlz4_sizeof_state_hc(void) { return 32768u * 4u + 65536u * 2u + 3u * 8u + 3u * 4u + 2u + 1u + 1u + 8u; }

// src/lz4hc.zig:1457-1489.  Differences from compressHC: no `< 2 -> 9` clamp (level < 1 -> 9, level 1 takes the
// table's row 1 = lz4mid, :72-97), dst.len == 0 is checked here (:1461).
int64_t zlz4_compress_hc_ext_state(void *state, size_t state_len, const uint8_t *src, size_t n, uint8_t *dst, size_t cap,
                                   int32_t level) {
    if (!state || state_len < zlz4_sizeof_state_hc()) return ZLZ4_ERR_INVALID_STATE;
    if (n > ZLZ4_MAX_INPUT_SIZE) return ZLZ4_ERR_INPUT_TOO_LARGE;   // :1459
    if (n == 0) return 0;                                           // :1460
    if (cap == 0) return ZLZ4_ERR_OUTPUT_TOO_SMALL;                 // :1461
    if (level < 1) level = ZLZ4HC_CLEVEL_DEFAULT;                   // :1464-1466
    if (level > ZLZ4HC_CLEVEL_MAX) level = ZLZ4HC_CLEVEL_MAX;
    if (level == 1) level = 2;                                      // clevelTable[1] == clevelTable[2] (:73-75)
    return run_single(Op::Hc, src, n, dst, cap, 0, level);
}

int64_t zlz4_compress_fast_ext_state(void *state, size_t state_len, const uint8_t *src, size_t n, uint8_t *dst,
                                     size_t cap, uint32_t accel) {
    (void)state;
    if (state_len < zlz4_sizeof_state()) return ZLZ4_ERR_INVALID_STATE;   // src/lz4.zig:532
    return zlz4_compress_fast(src, n, dst, cap, accel);                  // :534-545
}

int64_t zlz4_compress_dest_size(const uint8_t *src, uint8_t *dst, size_t cap, size_t *src_size) {
    const size_t max_src = *src_size;
    if (max_src == 0) { *src_size = 0; return 0; }                  // src/lz4.zig:553-556
    if (cap >= zlz4_compress_bound(max_src)) {                      // :559-564
        const int64_t r = zlz4_compress_default(src, max_src, dst, cap);
        if (r < 0) return r;
        *src_size = max_src;
        return r;
    }
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    if (max_src <= ZLZ4_MAX_INPUT_SIZE) return dest_size_batch_of_one(src, dst, cap, src_size);
    // Inputs past the limit: the search runs on the host, one device compression per probe.  Probes larger than the
    // limit fail with InputTooLarge in the reference (:594-607 -> `high = mid - 1`), so the device never needs more
    // than ZLZ4_MAX_INPUT_SIZE source bytes.
    const size_t stage = (size_t)ZLZ4_MAX_INPUT_SIZE;
    const uint32_t cap32 = clamp_cap32(cap);
    DevBuf d_in(stage), d_out(cap32);
    Staged<BlockRec> rec(nullptr);
    if (!d_in.p || !d_out.p || !rec.d) return ZLZ4_ERR_ALLOCATION_FAILED;
    if (hipMemcpy(d_in.p, src, stage, hipMemcpyHostToDevice) != hipSuccess) return ZLZ4_ERR_DEVICE;
    rec.h.out_cap = cap32;
    BlockRec *r = rec.d;
    // one probe = compressDefault(src[0..len], dst) on the device; the input stays resident
    auto probe = [&](size_t len) -> int64_t {
        if (len > ZLZ4_MAX_INPUT_SIZE) return ZLZ4_ERR_INPUT_TOO_LARGE;        // src/lz4.zig:296
        if (len == 0) return 0;                                                // :299
        rec.h.in_len = (uint32_t)len;
        if (hipMemcpy(r, &rec.h, sizeof rec.h, hipMemcpyHostToDevice) != hipSuccess) return ZLZ4_ERR_DEVICE;
        const int rc = zlz4_launch_compress_fast(nullptr, d_in.as<uint8_t>(), &r->in_off, &r->in_len, d_out.as<uint8_t>(),
                                                 &r->out_off, &r->out_cap, &r->result, 1, (uint32_t)len, 1);
        if (rc != 0) return rc;
        int64_t res = 0;
        if (hipMemcpy(&res, &r->result, sizeof res, hipMemcpyDeviceToHost) != hipSuccess) return ZLZ4_ERR_DEVICE;
        return res;
    };
    size_t low = 1, high = max_src, best = 0, best_c = 0, last_ok_len = (size_t)-1;     // :567-570
    auto attempt = [&](size_t len, bool &fits) -> int64_t {
        const int64_t r = probe(len);
        fits = r >= 0 && (size_t)r <= cap;
        last_ok_len = r >= 0 ? len : (size_t)-1;      // a failed probe leaves a partial stream in d_out
        return r;
    };
    if (cap <= max_src) {                                           // :573-586
        const size_t estimate = cap < max_src ? cap : max_src;
        bool fits;
        const int64_t r = attempt(estimate, fits);
        if (r == ZLZ4_ERR_DEVICE) return r;
        if (fits) { best = estimate; best_c = (size_t)r; low = estimate + 1; }
        else high = estimate - 1;
    }
    while (low <= high) {                                           // :589-612
        const size_t mid = low + (high - low) / 2;
        if (mid == 0 || mid > max_src) break;
        bool fits;
        const int64_t r = attempt(mid, fits);
        if (r == ZLZ4_ERR_DEVICE) return r;
        if (fits) {
            best = mid; best_c = (size_t)r;
            if (mid == max_src) break;
            low = mid + 1;
        } else {
            high = mid - 1;
        }
        if (low > max_src) break;
    }
    if (best > 0) {
        if (last_ok_len != best) { bool f; if (attempt(best, f) < 0) return ZLZ4_ERR_DEVICE; }   // put the best one into d_out
        if (hipMemcpy(dst, d_out.p, best_c, hipMemcpyDeviceToHost) != hipSuccess) return ZLZ4_ERR_DEVICE;
    }
    *src_size = best;                                               // :614-615
    return (int64_t)best_c;
}

// ---------------------------------------------------------------- batch, device pointers
int32_t zlz4_batch_compress_fast(void *stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                 uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                 int64_t *d_result, uint32_t nblocks, uint32_t max_in_len, uint32_t acceleration) {
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_compress_fast((hipStream_t)stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap,
                                     d_result, nblocks, max_in_len, acceleration);
}

int32_t zlz4_batch_decompress_safe(void *stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                   const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                   const uint32_t *d_out_cap, int64_t *d_result, uint32_t nblocks) {
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_decompress_safe((hipStream_t)stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap,
                                       d_result, nblocks);
}

int32_t zlz4_batch_decompress_safe_using_dict(void *stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                              const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                              const uint32_t *d_out_cap, const uint8_t *d_dict, const uint64_t *d_dict_off,
                                              const uint32_t *d_dict_len, int64_t *d_result, uint32_t nblocks) {
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_decompress_safe_using_dict((hipStream_t)stream, d_in, d_in_off, d_in_len, d_out, d_out_off,
                                                  d_out_cap, d_result, nblocks, d_dict, d_dict_off, d_dict_len);
}

// prefix decoding per block: d_out_cap[i] = bytes wanted = slot size (k_decompress_safe, kPartial)
int32_t zlz4_batch_decompress_safe_prefix(void *stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                          const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                          const uint32_t *d_out_cap, int64_t *d_result, uint32_t nblocks) {
    if (nblocks == 0) return 0;
    if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_result) return ZLZ4_ERR_INVALID_STATE;
    if (((uintptr_t)d_in_off | (uintptr_t)d_out_off | (uintptr_t)d_result) & 7u ||
        ((uintptr_t)d_in_len | (uintptr_t)d_out_cap) & 3u)
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_decompress_safe_prefix((hipStream_t)stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap,
                                              d_result, nblocks);
}

int32_t zlz4_batch_decompress_safe_prefix_using_dict(void *stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                                     const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                                     const uint32_t *d_out_cap, const uint8_t *d_dict,
                                                     const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                                                     int64_t *d_result, uint32_t nblocks) {
    if (nblocks == 0) return 0;
    // (d_dict may be null: every dictionary empty)
    if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_dict_off || !d_dict_len || !d_result)
        return ZLZ4_ERR_INVALID_STATE;
    if (((uintptr_t)d_in_off | (uintptr_t)d_out_off | (uintptr_t)d_dict_off | (uintptr_t)d_result) & 7u ||
        ((uintptr_t)d_in_len | (uintptr_t)d_out_cap | (uintptr_t)d_dict_len) & 3u)
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_decompress_safe_prefix_using_dict((hipStream_t)stream, d_in, d_in_off, d_in_len, d_out, d_out_off,
                                                         d_out_cap, d_result, nblocks, d_dict, d_dict_off, d_dict_len);
}

int32_t zlz4_batch_load_dict(void *stream, const uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                             uint32_t *d_tables, int64_t *d_result, uint32_t ndicts) {
    if (ndicts == 0) return 0;
    if (!d_dict_off || !d_dict_len || !d_tables || !d_result) return ZLZ4_ERR_INVALID_STATE;
    if ((uintptr_t)d_tables & 15u) return ZLZ4_ERR_INVALID_STATE;   // the header's 16-byte table alignment
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_load_dict((hipStream_t)stream, d_dict, d_dict_off, d_dict_len, d_tables, d_result, ndicts);
}

int32_t zlz4_batch_compress_fast_continue(void *stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                          const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                          const uint32_t *d_out_cap, const uint32_t *d_table_in,
                                          const uint32_t *d_table_idx, uint32_t *d_table_out, int64_t *d_result,
                                          uint32_t nblocks, uint32_t max_in_len, uint32_t acceleration) {
    if (nblocks == 0) return 0;
    if (!d_table_in) return ZLZ4_ERR_INVALID_STATE;
    if (d_table_idx && d_table_out == d_table_in) return ZLZ4_ERR_INVALID_STATE;   // in place needs identity indexing
    // the kernel moves tables in 16-byte vectors (k_compress_fast, kSeed)
    if (((uintptr_t)d_table_in | (uintptr_t)d_table_out) & 15u) return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_compress_fast_continue((hipStream_t)stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap,
                                              d_table_in, d_table_idx, d_table_out, d_result, nblocks, max_in_len,
                                              acceleration);
}

int32_t zlz4_batch_compress_fast_using_dict(void *stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                            const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                            const uint32_t *d_out_cap, const uint8_t *d_dict, const uint64_t *d_dict_off,
                                            const uint32_t *d_dict_len, const uint32_t *d_table,
                                            const uint32_t *d_table_idx, int64_t *d_result, uint32_t nblocks,
                                            uint32_t max_in_len, uint32_t max_dict_len, uint32_t acceleration) {
    if (nblocks == 0) return 0;
    if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_dict_off || !d_dict_len || !d_table ||
        !d_result || (!d_dict && max_dict_len))
        return ZLZ4_ERR_INVALID_STATE;
    if ((uintptr_t)d_table & 15u) return ZLZ4_ERR_INVALID_STATE;    // the kernel loads tables in 16-byte vectors
    if (((uintptr_t)d_in_off | (uintptr_t)d_out_off | (uintptr_t)d_dict_off | (uintptr_t)d_result) & 7u ||
        ((uintptr_t)d_in_len | (uintptr_t)d_out_cap | (uintptr_t)d_dict_len | (uintptr_t)d_table_idx) & 3u)
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_compress_fast_using_dict((hipStream_t)stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap,
                                                d_dict, d_dict_off, d_dict_len, d_table, d_table_idx, d_result, nblocks,
                                                max_in_len, max_dict_len, acceleration);
}

size_t zlz4_batch_compress_hc_using_dict_workspace(uint32_t nblocks, uint32_t max_in_len, uint32_t max_dict_len) {
    return zlz4_hc_dict_workspace_bytes(nblocks, max_in_len, max_dict_len);
}

int32_t zlz4_batch_compress_hc_using_dict(void *stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                          const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                          const uint32_t *d_out_cap, const uint8_t *d_dict, const uint64_t *d_dict_off,
                                          const uint32_t *d_dict_len, int64_t *d_result, uint32_t nblocks,
                                          uint32_t max_in_len, uint32_t max_dict_len, int32_t compression_level,
                                          void *d_workspace, size_t workspace_bytes) {
    if (nblocks == 0) return 0;
    if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_dict_off || !d_dict_len || !d_result ||
        (!d_dict && max_dict_len))
        return ZLZ4_ERR_INVALID_STATE;
    if (((uintptr_t)d_in_off | (uintptr_t)d_out_off | (uintptr_t)d_dict_off | (uintptr_t)d_result) & 7u ||
        ((uintptr_t)d_in_len | (uintptr_t)d_out_cap | (uintptr_t)d_dict_len) & 3u)
        return ZLZ4_ERR_INVALID_STATE;
    const int32_t level = hc_dict_level(compression_level);
    if (level == 0) return ZLZ4_ERR_UNSUPPORTED;
    // the staged blocks, the links and the results are moved in 16-byte vectors
    if (!d_workspace || ((uintptr_t)d_workspace & 15u) ||
        workspace_bytes < zlz4_hc_dict_workspace_bytes(nblocks, max_in_len, max_dict_len))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_compress_hc_dict((hipStream_t)stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_dict,
                                        d_dict_off, d_dict_len, d_result, nblocks, max_in_len, max_dict_len, level,
                                        d_workspace, workspace_bytes);
}

int32_t zlz4_batch_decompressed_size(void *stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                     const uint32_t *d_dict_len, int64_t *d_size, uint32_t nblocks) {
    if (nblocks == 0) return 0;
    if (!d_in || !d_in_off || !d_in_len || !d_size) return ZLZ4_ERR_INVALID_STATE;
    if (((uintptr_t)d_in_off | (uintptr_t)d_size) & 7u || ((uintptr_t)d_in_len | (uintptr_t)d_dict_len) & 3u)
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_decompressed_size((hipStream_t)stream, d_in, d_in_off, d_in_len, d_dict_len, d_size, nblocks);
}

int32_t zlz4_batch_plan_outputs(void *stream, const int64_t *d_size, uint32_t n, uint32_t align, uint64_t *d_out_off,
                                uint32_t *d_out_cap, uint64_t *d_total) {
    if (align > 4096u || (align & (align - 1u))) return ZLZ4_ERR_INVALID_STATE;      // 0, 1 or a power of two up to 4096
    if (!d_total || (n && (!d_size || !d_out_off || !d_out_cap))) return ZLZ4_ERR_INVALID_STATE;
    if (((uintptr_t)d_size | (uintptr_t)d_out_off | (uintptr_t)d_total) & 7u || (uintptr_t)d_out_cap & 3u)
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_plan_outputs((hipStream_t)stream, d_size, n, align ? align : 1u, d_out_off, d_out_cap, d_total);
}

size_t zlz4_batch_decompress_safe_continue_workspace(uint32_t nblocks, uint32_t nstreams) {
    return zlz4_sd_workspace_bytes(nblocks, nstreams);
}

int32_t zlz4_batch_decompress_safe_continue(void *stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                            const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                            const uint32_t *d_out_cap, const uint32_t *d_run_start,
                                            zlz4_stream_decode_t *d_state, int64_t *d_result, uint32_t nblocks,
                                            uint32_t nstreams, void *d_workspace, size_t workspace_bytes) {
    if (nstreams == 0 && nblocks == 0) return 0;
    if (!d_run_start || !d_state || (nblocks && !d_result) || !d_workspace || ((uintptr_t)d_workspace & 15u) ||
        workspace_bytes < zlz4_sd_workspace_bytes(nblocks, nstreams))
        return ZLZ4_ERR_INVALID_STATE;
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    return zlz4_launch_stream_decode((hipStream_t)stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap,
                                     d_run_start, reinterpret_cast<uint64_t *>(d_state), d_result, nblocks, nstreams,
                                     d_workspace);
}

size_t zlz4_batch_compress_hc_workspace(uint32_t nblocks, uint32_t max_in_len) {
    return zlz4_hc_workspace_bytes(nblocks, max_in_len);
}

int32_t zlz4_batch_compress_hc(void *stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                               uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                               int64_t *d_result, uint32_t nblocks, uint32_t max_in_len, int32_t level,
                               void *d_workspace, size_t workspace_bytes) {
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    level = normalise_hc_level(level);
    if (workspace_bytes < zlz4_hc_workspace_bytes(nblocks, max_in_len) || (!d_workspace && nblocks))
        return ZLZ4_ERR_INVALID_STATE;
    return zlz4_launch_compress_hc((hipStream_t)stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap,
                                   d_result, nblocks, max_in_len, level, d_workspace, workspace_bytes);
}

size_t zlz4_batch_compress_dest_size_workspace(uint32_t nblocks, uint32_t max_in_len) {
    return zlz4_dest_size_workspace_bytes(nblocks, max_in_len);
}

int32_t zlz4_batch_compress_dest_size(void *stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                      uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                      int64_t *d_result, uint32_t *d_consumed, uint32_t nblocks, uint32_t max_in_len,
                                      void *d_workspace, size_t workspace_bytes) {
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    if (nblocks == 0) return 0;
    if (!d_workspace || workspace_bytes < zlz4_dest_size_workspace_bytes(nblocks, max_in_len) ||
        ((uintptr_t)d_workspace & 7u))
        return ZLZ4_ERR_INVALID_STATE;
    return zlz4_launch_compress_dest_size((hipStream_t)stream, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap,
                                          d_result, d_consumed, nblocks, max_in_len, d_workspace, nullptr, nullptr);
}

// ---------------------------------------------------------------- opt-in round-trip check (levels 10..12)
}  // extern "C"

namespace {
// decode descriptors from the compress results: length 0 for a block that reported an error, capacity = the input length
__global__ void k_verify_prep(const int64_t *__restrict__ comp_result, const uint32_t *__restrict__ in_len,
                              const uint64_t *__restrict__ in_off, uint64_t base_off, uint32_t *__restrict__ clen,
                              uint64_t *__restrict__ dec_off, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t r = comp_result[i];
    clen[i] = r > 0 ? (uint32_t)r : 0u;
    dec_off[i] = in_off[i] - base_off;
    (void)in_len;
}
// one wavefront per block: decoded size and bytes against the input
__global__ __launch_bounds__(256) void k_verify_compare(const uint8_t *__restrict__ d_in, const uint64_t *__restrict__ in_off,
                                                        const uint32_t *__restrict__ in_len, const uint8_t *__restrict__ d_dec,
                                                        const uint64_t *__restrict__ dec_off, const int64_t *__restrict__ dec_result,
                                                        const int64_t *__restrict__ comp_result, int64_t *__restrict__ verify,
                                                        unsigned long long *__restrict__ nbad, uint32_t n) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t cr = comp_result[i];
    int64_t out = cr;
    if (cr >= 0) {
        const uint32_t len = in_len[i];
        bool bad = dec_result[i] != (int64_t)len && !(len == 0 && cr == 0);
        if (!bad) {
            const uint8_t *a = d_in + in_off[i], *b = d_dec + dec_off[i];
            bool diff = false;
            for (uint32_t k = lane; k < len; k += 64u) diff |= a[k] != b[k];
            bad = __ballot(diff) != 0;
        }
        if (bad) out = ZLZ4_ERR_VERIFY;
    }
    if (lane == 0) {
        verify[i] = out;
        if (out == ZLZ4_ERR_VERIFY) atomicAdd(nbad, 1ull);
    }
}
}  // namespace

extern "C" int64_t zlz4_batch_verify(void *stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                     const uint8_t *d_comp, const uint64_t *d_comp_off, const int64_t *d_comp_result,
                                     int64_t *d_verify, uint32_t nblocks) {
    if (!device_ok()) return ZLZ4_ERR_DEVICE;
    if (nblocks == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    // the extent of the input arena (descriptors come back to the host: this call synchronises anyway)
    std::vector<uint64_t> off(nblocks);
    std::vector<uint32_t> len(nblocks);
    if (hipMemcpyAsync(off.data(), d_in_off, nblocks * sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(len.data(), d_in_len, nblocks * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) return ZLZ4_ERR_DEVICE;
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t i = 0; i < nblocks; i++) {
        if (off[i] < lo) lo = off[i];
        if (off[i] + len[i] > hi) hi = off[i] + len[i];
    }
    DeviceCall call(st);
    DevBuf d_dec((size_t)(hi - lo) + 64, &call), d_clen((size_t)nblocks * 4, &call), d_doff((size_t)nblocks * 8, &call),
        d_dres((size_t)nblocks * 8, &call), d_nbad(8, &call);
    if (!d_dec.p || !d_clen.p || !d_doff.p || !d_dres.p || !d_nbad.p) return ZLZ4_ERR_ALLOCATION_FAILED;
    call.launched();
    if (hipMemsetAsync(d_nbad.p, 0, 8, st) != hipSuccess) return ZLZ4_ERR_DEVICE;
    hipLaunchKernelGGL(k_verify_prep, dim3((nblocks + 255) / 256), dim3(256), 0, st, d_comp_result, d_in_len, d_in_off, lo,
                       d_clen.as<uint32_t>(), d_doff.as<uint64_t>(), nblocks);
    const int rc = zlz4_launch_decompress_safe(st, d_comp, d_comp_off, d_clen.as<uint32_t>(), d_dec.as<uint8_t>(),
                                               d_doff.as<uint64_t>(), d_in_len, d_dres.as<int64_t>(), nblocks);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(k_verify_compare, dim3((nblocks + 3) / 4), dim3(256), 0, st, d_in, d_in_off, d_in_len, d_dec.as<uint8_t>(),
                       d_doff.as<uint64_t>(), d_dres.as<int64_t>(), d_comp_result, d_verify,
                       d_nbad.as<unsigned long long>(), nblocks);
    unsigned long long nbad = 0;
    if (hipMemcpyAsync(&nbad, d_nbad.p, 8, hipMemcpyDeviceToHost, st) != hipSuccess || !call.sync() ||
        hipGetLastError() != hipSuccess) return ZLZ4_ERR_DEVICE;
    return (int64_t)nbad;
}
