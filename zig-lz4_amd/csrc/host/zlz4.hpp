// zlz4.hpp -- C++ host-side mirror of the reference's public facade (src/root.zig:1-57) over the C ABI.
//
// The reference is compiled Zig and no zig toolchain exists in the build image, so the compiled-language
// host layer above the C ABI is this header (the Zig binding itself is zig/root.zig, delivered as source).
// Same names and argument meaning as the reference; Zig error unions become zlz4::Result { value, error }.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../../include/zlz4_amd.h"

namespace zlz4 {

struct Result {
    std::size_t value = 0;   // bytes written when ok()
    std::int64_t error = 0;  // 0 or a ZLZ4_ERR_* / ZLZ4F_ERR_* code
    bool ok() const { return error == 0; }
    std::string error_name() const { return zlz4_error_name(error); }
};
inline Result wrap(std::int64_t r) { return r >= 0 ? Result{(std::size_t)r, 0} : Result{0, r}; }

constexpr int MINMATCH = ZLZ4_MINMATCH;
constexpr std::uint32_t LZ4_MAX_INPUT_SIZE = ZLZ4_MAX_INPUT_SIZE;
constexpr std::uint32_t LZ4_DISTANCE_MAX = ZLZ4_DISTANCE_MAX;
constexpr int LZ4HC_CLEVEL_MIN = ZLZ4HC_CLEVEL_MIN, LZ4HC_CLEVEL_DEFAULT = ZLZ4HC_CLEVEL_DEFAULT,
              LZ4HC_CLEVEL_MAX = ZLZ4HC_CLEVEL_MAX;

// lz4.compressBound, src/lz4.zig:80-83
inline std::size_t compressBound(std::size_t n) { return zlz4_compress_bound(n); }
// lz4.compressDefault, src/lz4.zig:283-285
inline Result compressDefault(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap) {
    return wrap(zlz4_compress_default(src, n, dst, cap));
}
// lz4.compressFast, src/lz4.zig:292-447
inline Result compressFast(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap, std::uint32_t accel) {
    return wrap(zlz4_compress_fast(src, n, dst, cap, accel));
}
// lz4.decompressSafe, src/lz4.zig:257-259
inline Result decompressSafe(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap) {
    return wrap(zlz4_decompress_safe(src, n, dst, cap));
}
// lz4.decompressSafePartial, src/lz4.zig:619-621
inline Result decompressSafePartial(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap, std::size_t target) {
    return wrap(zlz4_decompress_safe_partial(src, n, dst, cap, target));
}
// lz4.decompressSafeUsingDict / decompressSafePartialUsingDict, src/lz4.zig:960-969 (dict must not overlap dst)
inline Result decompressSafeUsingDict(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap,
                                      const std::uint8_t *dict, std::size_t dict_len) {
    return wrap(zlz4_decompress_safe_using_dict(src, n, dst, cap, dict, dict_len));
}
inline Result decompressSafePartialUsingDict(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap,
                                             std::size_t target, const std::uint8_t *dict, std::size_t dict_len) {
    return wrap(zlz4_decompress_safe_partial_using_dict(src, n, dst, cap, target, dict, dict_len));
}
// no counterpart in the reference: the first `cap` bytes of the block (all of it where it decodes to fewer), never
// OutputTooSmall; the result is min(decoded size, cap) (include/zlz4_amd.h)
inline Result decompressSafePrefix(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap) {
    return wrap(zlz4_decompress_safe_prefix(src, n, dst, cap));
}
inline Result decompressSafePrefixUsingDict(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap,
                                            const std::uint8_t *dict, std::size_t dict_len) {
    return wrap(zlz4_decompress_safe_prefix_using_dict(src, n, dst, cap, dict, dict_len));
}
// no counterpart in the reference (its Stream never refers to a loaded dictionary): compressFast's loop on the last 64 KiB
// of `dict` followed by `src`, from the table Stream.loadDict(dict) leaves; decodes with decompressSafeUsingDict
inline Result compressFastUsingDict(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap,
                                    const std::uint8_t *dict, std::size_t dict_len, std::uint32_t accel = 1) {
    return wrap(zlz4_compress_fast_using_dict(src, n, dst, cap, dict, dict_len, accel));
}
// lz4.Stream, src/lz4.zig:751-866: the table lives on the host and is computed on the device by loadDict /
// compressFastContinue; the rest is bookkeeping.  A loaded dictionary only changes which in-block matches are found (the
// reference reads table entries as positions in the current block): no block refers to it, and saveDict copies the
// loaded dictionary, not the compressed history.
struct Stream {
    std::uint32_t hashTable[ZLZ4_STREAM_TABLE_ENTRIES] = {};
    const std::uint8_t *dictionary = nullptr;   // borrowed, as in the reference
    std::size_t dictionaryLen = 0;
    std::uint32_t currentOffset = 0;
    std::uint32_t dictSize = 0;

    void resetFast() {                                              // :789-795
        for (auto &e : hashTable) e = 0;
        dictionary = nullptr; dictionaryLen = 0; currentOffset = 0; dictSize = 0;
    }
    // :798-820; a negative value = the device call failed (the reference returns usize)
    std::int64_t loadDict(const std::uint8_t *dict, std::size_t len) {
        resetFast();
        const std::int64_t r = zlz4_stream_load_dict(hashTable, dict, len);
        if (r > 0) { dictionary = dict + (len - (std::size_t)r); dictionaryLen = (std::size_t)r; dictSize = (std::uint32_t)r; }
        return r;
    }
    // :822-836
    Result compressFastContinue(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap, std::uint32_t accel = 1) {
        const Result r = wrap(zlz4_stream_compress_fast_continue(hashTable, src, n, dst, cap, accel));
        if (r.ok() && n >= 13) currentOffset = currentOffset + n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (std::uint32_t)(currentOffset + n);
        return r;
    }
    // :839-855
    std::size_t saveDict(std::uint8_t *safeBuffer, std::size_t safeLen, std::size_t maxDictSize) const {
        if (maxDictSize == 0 || !dictionary) return 0;
        std::size_t size = dictionaryLen < maxDictSize ? dictionaryLen : maxDictSize;
        if (size > 65536) size = 65536;
        if (size > safeLen) size = safeLen;
        for (std::size_t i = 0; i < size; i++) safeBuffer[i] = dictionary[dictionaryLen - size + i];
        return size;
    }
};

// lz4.StreamDecode, src/lz4.zig:870-957: the reference's fields as addresses (zlz4_stream_decode_t).  A call never reads
// the previous output; see the WARNING in include/zlz4_amd.h for output placed below the previous output.
struct StreamDecode {
    zlz4_stream_decode_t st{0, 0, 0, 0};
    StreamDecode() { zlz4_stream_decode_init(&st); }
    void setStreamDecode(const std::uint8_t *dict, std::size_t dict_len) { zlz4_set_stream_decode(&st, dict, dict_len); }
    Result decompressSafeContinue(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap) {
        return wrap(zlz4_decompress_safe_continue(&st, src, n, dst, cap));
    }
};
inline std::size_t decoderRingBufferSize(std::size_t max_block_size) { return zlz4_decoder_ring_buffer_size(max_block_size); }

// no counterpart in the reference: what decompressSafe (dict_len 0) / decompressSafeUsingDict with a dictionary of dict_len
// bytes returns for `src` into a destination of 0xFFFFFFFF bytes; nothing is decoded
inline Result decompressedSize(const std::uint8_t *src, std::size_t n, std::size_t dict_len = 0) {
    return wrap(zlz4_decompressed_size(src, n, dict_len));
}

// lz4.sizeofState / compressFastExtState / compressDestSize, src/lz4.zig:524-616
inline std::size_t sizeofState() { return zlz4_sizeof_state(); }
inline Result compressFastExtState(void *state, std::size_t state_len, const std::uint8_t *src, std::size_t n,
                                   std::uint8_t *dst, std::size_t cap, std::uint32_t accel) {
    return wrap(zlz4_compress_fast_ext_state(state, state_len, src, n, dst, cap, accel));
}
inline Result compressDestSize(const std::uint8_t *src, std::uint8_t *dst, std::size_t cap, std::size_t *src_size) {
    return wrap(zlz4_compress_dest_size(src, dst, cap, src_size));
}
// lz4hc.compressHC, src/lz4hc.zig:1440-1453
inline Result compressHC(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap, std::int32_t level) {
    return wrap(zlz4_compress_hc(src, n, dst, cap, level));
}

// levels 3..9 against a dictionary (no counterpart in the reference): compressHashChain on dict-tail ++ src, the parse
// starting at the record; levels 2 and 10..12 are Unsupported
inline Result compressHCUsingDict(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap,
                                  const std::uint8_t *dict, std::size_t dict_len, std::int32_t level) {
    return wrap(zlz4_compress_hc_using_dict(src, n, dst, cap, dict, dict_len, level));
}

// Dictionary training (no counterpart in the reference): one dictionary of at most dict_cap (<= 65536) bytes from samples
// that lie back to back, sample i having sample_sizes[i] bytes (include/zlz4_amd.h, zlz4_train_dict)
using TrainParams = zlz4_train_params;
inline Result trainDict(const std::uint8_t *samples, const std::size_t *sample_sizes, std::uint32_t nsamples, std::uint8_t *dict,
                        std::size_t dict_cap, const TrainParams &params = TrainParams{8, 256, 20, 0}) {
    return wrap(zlz4_train_dict(samples, sample_sizes, nsamples, dict, dict_cap, &params));
}

// lz4hc.sizeofStateHC / compressHCExtState, src/lz4hc.zig:1457-1494 (fresh context, passed as the bytes it occupies)
inline std::size_t sizeofStateHC() { return zlz4_sizeof_state_hc(); }
inline Result compressHCExtState(void *ctx, std::size_t ctx_len, const std::uint8_t *src, std::size_t n, std::uint8_t *dst,
                                 std::size_t cap, std::int32_t level) {
    return wrap(zlz4_compress_hc_ext_state(ctx, ctx_len, src, n, dst, cap, level));
}

// The hot path itself: many independent blocks per call, DEVICE pointers, asynchronous on `stream` (hipStream_t as
// void*).  A host-side slice-of-slices becomes the four descriptor arrays (they live in device memory too).
namespace device {
struct Blocks {
    const std::uint8_t *in; const std::uint64_t *in_off; const std::uint32_t *in_len;
    std::uint8_t *out; const std::uint64_t *out_off; const std::uint32_t *out_cap;
    std::int64_t *result; std::uint32_t nblocks;
};
inline Result compressFastBatch(void *stream, const Blocks &b, std::uint32_t max_in_len, std::uint32_t accel = 1) {
    return wrap(zlz4_batch_compress_fast(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.result, b.nblocks, max_in_len, accel));
}
inline Result decompressSafeBatch(void *stream, const Blocks &b) {
    return wrap(zlz4_batch_decompress_safe(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.result, b.nblocks));
}
// per-block dictionaries: block i reads dict + dict_off[i] (dict_len[i] bytes); shared = the same offset everywhere
struct DictBlocks {
    const std::uint8_t *dict; const std::uint64_t *dict_off; const std::uint32_t *dict_len;
};
inline Result decompressSafeUsingDictBatch(void *stream, const Blocks &b, const DictBlocks &d) {
    return wrap(zlz4_batch_decompress_safe_using_dict(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, d.dict,
                                                      d.dict_off, d.dict_len, b.result, b.nblocks));
}
// prefix decoding: b.out_cap[i] is the number of bytes wanted of block i and the size of its slot
inline Result decompressSafePrefixBatch(void *stream, const Blocks &b) {
    return wrap(zlz4_batch_decompress_safe_prefix(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.result, b.nblocks));
}
inline Result decompressSafePrefixUsingDictBatch(void *stream, const Blocks &b, const DictBlocks &d) {
    return wrap(zlz4_batch_decompress_safe_prefix_using_dict(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap,
                                                             d.dict, d.dict_off, d.dict_len, b.result, b.nblocks));
}
// decompressed sizes: size[i] = what decompressSafeBatch returns for block i into 0xFFFFFFFF bytes, or
// decompressSafeUsingDictBatch with a dictionary of dict_len[i] bytes (nullptr = no dictionary); only b.in* and b.nblocks
// are read
inline Result decompressedSizeBatch(void *stream, const Blocks &b, const std::uint32_t *d_dict_len, std::int64_t *d_size) {
    return wrap(zlz4_batch_decompressed_size(stream, b.in, b.in_off, b.in_len, d_dict_len, d_size, b.nblocks));
}
// packed output slots from sizes: out_off / out_cap as Blocks takes them, *total = bytes of all slots (align 0, 1 or a
// power of two up to 4096)
inline Result planOutputs(void *stream, const std::int64_t *d_size, std::uint32_t n, std::uint32_t align,
                          std::uint64_t *d_out_off, std::uint32_t *d_out_cap, std::uint64_t *d_total) {
    return wrap(zlz4_batch_plan_outputs(stream, d_size, n, align, d_out_off, d_out_cap, d_total));
}
// StreamDecode.decompressSafeContinue over whole streams: stream s makes the calls [run_start[s], run_start[s + 1]) of b
// from d_state[s] (device addresses, updated in place)
inline std::size_t decompressSafeContinueWorkspace(std::uint32_t nblocks, std::uint32_t nstreams) {
    return zlz4_batch_decompress_safe_continue_workspace(nblocks, nstreams);
}
inline Result decompressSafeContinueBatch(void *stream, const Blocks &b, const std::uint32_t *d_run_start,
                                          zlz4_stream_decode_t *d_state, std::uint32_t nstreams, void *d_workspace,
                                          std::size_t workspace_bytes) {
    return wrap(zlz4_batch_decompress_safe_continue(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap,
                                                    d_run_start, d_state, b.result, b.nblocks, nstreams, d_workspace,
                                                    workspace_bytes));
}
// Stream.loadDict per dictionary (table i of d_tables, ZLZ4_STREAM_TABLE_ENTRIES u32 each; result[i] = dictSize)
inline Result loadDictBatch(void *stream, const DictBlocks &d, std::uint32_t *d_tables, std::int64_t *d_result, std::uint32_t ndicts) {
    return wrap(zlz4_batch_load_dict(stream, d.dict, d.dict_off, d.dict_len, d_tables, d_result, ndicts));
}
// Stream.compressFastContinue per block: block i starts from table table_idx[i] of table_in (nullptr = table i), its
// final table goes to table i of table_out (nullptr = not written; in place only without table_idx)
struct StreamTables {
    const std::uint32_t *table_in; const std::uint32_t *table_idx; std::uint32_t *table_out;
};
inline Result compressFastContinueBatch(void *stream, const Blocks &b, const StreamTables &t, std::uint32_t max_in_len,
                                        std::uint32_t accel = 1) {
    return wrap(zlz4_batch_compress_fast_continue(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, t.table_in,
                                                  t.table_idx, t.table_out, b.result, b.nblocks, max_in_len, accel));
}
// compressFastUsingDict per block: block i against dictionary d from table table_idx[i] of d_table (nullptr = table i),
// the tables being loadDictBatch's of the dictionaries
inline Result compressFastUsingDictBatch(void *stream, const Blocks &b, const DictBlocks &d, const std::uint32_t *d_table,
                                         const std::uint32_t *d_table_idx, std::uint32_t max_in_len,
                                         std::uint32_t max_dict_len, std::uint32_t accel = 1) {
    return wrap(zlz4_batch_compress_fast_using_dict(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, d.dict,
                                                    d.dict_off, d.dict_len, d_table, d_table_idx, b.result, b.nblocks,
                                                    max_in_len, max_dict_len, accel));
}
inline std::size_t compressHCWorkspace(std::uint32_t nblocks, std::uint32_t max_in_len) {
    return zlz4_batch_compress_hc_workspace(nblocks, max_in_len);
}
inline Result compressHCBatch(void *stream, const Blocks &b, std::uint32_t max_in_len, std::int32_t level, void *ws, std::size_t ws_bytes) {
    return wrap(zlz4_batch_compress_hc(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.result, b.nblocks, max_in_len, level, ws, ws_bytes));
}
inline std::size_t compressHCUsingDictWorkspace(std::uint32_t nblocks, std::uint32_t max_in_len, std::uint32_t max_dict_len) {
    return zlz4_batch_compress_hc_using_dict_workspace(nblocks, max_in_len, max_dict_len);
}
// compressHCUsingDict per block: block i against dictionary d; ws = device memory of compressHCUsingDictWorkspace() bytes
inline Result compressHCUsingDictBatch(void *stream, const Blocks &b, const DictBlocks &d, std::uint32_t max_in_len,
                                       std::uint32_t max_dict_len, std::int32_t level, void *ws, std::size_t ws_bytes) {
    return wrap(zlz4_batch_compress_hc_using_dict(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, d.dict,
                                                  d.dict_off, d.dict_len, b.result, b.nblocks, max_in_len, max_dict_len, level,
                                                  ws, ws_bytes));
}
// one dictionary per group of samples: the arrays of zlz4_batch_train_dict
struct TrainGroups {
    const std::uint8_t *src;           // sample arena
    const std::uint64_t *src_off;      // per sample: offset into `src`
    const std::uint32_t *src_len;      // per sample: bytes
    std::uint32_t nsamples;
    const std::uint32_t *group_first;  // ngroups + 1: group g is samples group_first[g] .. group_first[g + 1] - 1
    std::uint32_t ngroups;
    std::uint8_t *dict;                // dictionary arena
    const std::uint64_t *dict_off;     // per group: offset of its slot
    const std::uint32_t *dict_cap;     // per group: capacity (<= 65536)
    std::int64_t *result;              // per group: the dictionary's length or an error code
};
inline std::size_t trainDictWorkspace(std::uint32_t ngroups, std::uint64_t total_sample_bytes, std::uint32_t max_dict_cap,
                                      const TrainParams &params) {
    return zlz4_batch_train_dict_workspace(ngroups, total_sample_bytes, max_dict_cap, &params);
}
// trainDict per group; ws = device memory of trainDictWorkspace() bytes
inline Result trainDictBatch(void *stream, const TrainGroups &g, std::uint32_t max_dict_cap, const TrainParams &params, void *ws,
                             std::size_t ws_bytes) {
    return wrap(zlz4_batch_train_dict(stream, g.src, g.src_off, g.src_len, g.nsamples, g.group_first, g.ngroups, g.dict,
                                      g.dict_off, g.dict_cap, g.result, max_dict_cap, &params, ws, ws_bytes));
}
inline std::size_t compressDestSizeWorkspace(std::uint32_t nblocks, std::uint32_t max_in_len) {
    return zlz4_batch_compress_dest_size_workspace(nblocks, max_in_len);
}
// compressDestSize per block: in_len[i] = bytes available, out_cap[i] = dst.len; consumed[i] = source bytes consumed
inline Result compressDestSizeBatch(void *stream, const Blocks &b, std::uint32_t *consumed, std::uint32_t max_in_len, void *ws,
                                    std::size_t ws_bytes) {
    return wrap(zlz4_batch_compress_dest_size(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.result, consumed,
                                              b.nblocks, max_in_len, ws, ws_bytes));
}
}  // namespace device

namespace lz4f {   // src/lz4f.zig
using Preferences = zlz4f_prefs;
constexpr std::uint32_t MAGICNUMBER = ZLZ4F_MAGICNUMBER;
inline std::size_t compressFrameBound(std::size_t n, const Preferences *p = nullptr) { return zlz4f_compress_frame_bound(n, p); }
inline Result compressFrame(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap, const Preferences *p = nullptr) {
    return wrap(zlz4f_compress_frame(src, n, dst, cap, p));
}
inline Result decompressFrame(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap) {
    return wrap(zlz4f_decompress_frame(src, n, dst, cap));
}
inline Result headerSize(const std::uint8_t *src, std::size_t n) { return wrap(zlz4f_header_size(src, n)); }
// device-resident frames and per-rank frame segments (BASELINE configs[4])
inline Result compressFrameDevice(void *stream, const std::uint8_t *d_src, std::size_t n, std::uint8_t *d_dst, std::size_t cap, const Preferences *p = nullptr) {
    return wrap(zlz4f_compress_frame_device(stream, d_src, n, d_dst, cap, p));
}
inline Result decompressFrameDevice(void *stream, const std::uint8_t *d_src, std::size_t n, std::uint8_t *d_dst, std::size_t cap) {
    return wrap(zlz4f_decompress_frame_device(stream, d_src, n, d_dst, cap));
}
inline Result compressFrameSegmentDevice(void *stream, const std::uint8_t *d_src, std::size_t n, std::uint8_t *d_dst, std::size_t cap, const Preferences *p, std::uint32_t seg) {
    return wrap(zlz4f_compress_frame_segment_device(stream, d_src, n, d_dst, cap, p, seg));
}
inline Result decompressFrameSegmentDevice(void *stream, const std::uint8_t *d_src, std::size_t n, std::uint8_t *d_dst, std::size_t cap, const Preferences *p, std::uint32_t seg) {
    return wrap(zlz4f_decompress_frame_segment_device(stream, d_src, n, d_dst, cap, p, seg));
}
// batch frames (device pointers, asynchronous): frame f reads src + src_off[f] (src_len[f] bytes), writes dst + dst_off[f]
// (capacity dst_cap[f]); result[f] = frame size / decompressed size or the frame's error code
struct Frames {
    const std::uint8_t *src; const std::uint64_t *src_off; const std::uint64_t *src_len;
    std::uint8_t *dst; const std::uint64_t *dst_off; const std::uint64_t *dst_cap;
    std::int64_t *result; std::uint32_t nframes;
};
constexpr std::uint32_t BATCH_CONTENT_SIZE = ZLZ4F_BATCH_CONTENT_SIZE;
inline std::size_t compressFrameBatchWorkspace(std::uint32_t nframes, std::uint32_t max_blocks, const Preferences *p = nullptr) {
    return zlz4f_batch_compress_frame_workspace(nframes, max_blocks, p);
}
inline Result compressFrameBatch(void *stream, const Frames &f, std::uint32_t max_blocks, const Preferences *p, std::uint32_t batch_flags,
                                 void *ws, std::size_t ws_bytes) {
    return wrap(zlz4f_batch_compress_frame(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes,
                                           max_blocks, p, batch_flags, ws, ws_bytes));
}
inline std::size_t decompressFrameBatchWorkspace(std::uint32_t nframes, std::uint32_t max_blocks) {
    return zlz4f_batch_decompress_frame_workspace(nframes, max_blocks);
}
inline Result decompressFrameBatch(void *stream, const Frames &f, std::uint32_t max_blocks, void *ws, std::size_t ws_bytes) {
    return wrap(zlz4f_batch_decompress_frame(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes,
                                             max_blocks, ws, ws_bytes));
}
// decompressed size of frames: what decompressFrame(Batch) returns into a destination that is large enough (the content
// checksum is not verified); nothing is decoded.  Only f.src*, f.nframes are read; d_size receives the sizes.
inline Result frameDecompressedSize(const std::uint8_t *src, std::size_t n) { return wrap(zlz4f_frame_decompressed_size(src, n)); }
inline std::size_t frameDecompressedSizeBatchWorkspace(std::uint32_t nframes, std::uint32_t max_blocks) {
    return zlz4f_batch_frame_decompressed_size_workspace(nframes, max_blocks);
}
inline Result frameDecompressedSizeBatch(void *stream, const Frames &f, std::int64_t *d_size, std::uint32_t max_blocks, void *ws,
                                         std::size_t ws_bytes) {
    return wrap(zlz4f_batch_frame_decompressed_size(stream, f.src, f.src_off, f.src_len, d_size, f.nframes, max_blocks, ws, ws_bytes));
}
// linked-block frames (include/zlz4_amd.h; no counterpart in the reference).  DECODE_LINKED: a frame whose FLG declares
// linked blocks is decoded in block order, block k against the 64 KiB of output in front of it (liblz4's default frames);
// BATCH_LINK_BLOCKS: compressFrameBatch writes such frames at the fast level, compressFrameBatchEx also at the HC levels
// 3..9 (block k = compressHCUsingDict against the 64 KiB of input in front of it); workspace from
// compressFrameBatchWorkspaceEx.
constexpr std::uint32_t DECODE_LINKED = ZLZ4F_DECODE_LINKED;
constexpr std::uint32_t BATCH_LINK_BLOCKS = ZLZ4F_BATCH_LINK_BLOCKS;
inline std::size_t compressFrameBatchWorkspaceEx(std::uint32_t nframes, std::uint32_t max_blocks, const Preferences *p, std::uint32_t batch_flags) {
    return zlz4f_batch_compress_frame_workspace_ex(nframes, max_blocks, p, batch_flags);
}
inline Result compressFrameBatchEx(void *stream, const Frames &f, std::uint32_t max_blocks, const Preferences *p, std::uint32_t batch_flags,
                                   void *ws, std::size_t ws_bytes) {
    return wrap(zlz4f_batch_compress_frame_ex(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes,
                                              max_blocks, p, batch_flags, ws, ws_bytes));
}
// one frame through compressFrameBatchEx (batch_flags 0: the answer of compressFrame / compressFrameDevice)
inline Result compressFrameEx(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap, const Preferences *p,
                              std::uint32_t batch_flags) {
    return wrap(zlz4f_compress_frame_ex(src, n, dst, cap, p, batch_flags));
}
inline Result compressFrameDeviceEx(void *stream, const std::uint8_t *d_src, std::size_t n, std::uint8_t *d_dst, std::size_t cap,
                                    const Preferences *p, std::uint32_t batch_flags) {
    return wrap(zlz4f_compress_frame_device_ex(stream, d_src, n, d_dst, cap, p, batch_flags));
}
inline std::size_t decompressFrameBatchWorkspaceEx(std::uint32_t nframes, std::uint32_t max_blocks, std::uint32_t decode_flags) {
    return zlz4f_batch_decompress_frame_workspace_ex(nframes, max_blocks, decode_flags);
}
inline Result decompressFrameBatchEx(void *stream, const Frames &f, std::uint32_t max_blocks, std::uint32_t decode_flags, void *ws,
                                     std::size_t ws_bytes) {
    return wrap(zlz4f_batch_decompress_frame_ex(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes,
                                                max_blocks, decode_flags, ws, ws_bytes));
}
inline std::size_t frameDecompressedSizeBatchWorkspaceEx(std::uint32_t nframes, std::uint32_t max_blocks, std::uint32_t decode_flags) {
    return zlz4f_batch_frame_decompressed_size_workspace_ex(nframes, max_blocks, decode_flags);
}
inline Result frameDecompressedSizeBatchEx(void *stream, const Frames &f, std::int64_t *d_size, std::uint32_t max_blocks,
                                           std::uint32_t decode_flags, void *ws, std::size_t ws_bytes) {
    return wrap(zlz4f_batch_frame_decompressed_size_ex(stream, f.src, f.src_off, f.src_len, d_size, f.nframes, max_blocks, decode_flags,
                                                       ws, ws_bytes));
}
// one frame through the batch calls (the segment calls have no such form: a rank's first block would need the previous
// rank's output)
inline Result decompressFrameEx(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap, std::uint32_t decode_flags) {
    return wrap(zlz4f_decompress_frame_ex(src, n, dst, cap, decode_flags));
}
inline Result decompressFrameDeviceEx(void *stream, const std::uint8_t *d_src, std::size_t n, std::uint8_t *d_dst, std::size_t cap,
                                      std::uint32_t decode_flags) {
    return wrap(zlz4f_decompress_frame_device_ex(stream, d_src, n, d_dst, cap, decode_flags));
}
inline Result frameDecompressedSizeEx(const std::uint8_t *src, std::size_t n, std::uint32_t decode_flags) {
    return wrap(zlz4f_frame_decompressed_size_ex(src, n, decode_flags));
}
// frame prefix decoding (include/zlz4_amd.h; no counterpart in the reference): the first `cap` bytes of the frame's content
// (all of it where the frame holds fewer), history-aware; the result is min(content size, cap), a defect behind the cut is
// not reported.  Batch: f.dst_cap[i] is the number of bytes wanted of frame i and the size of its slot; one launch, no
// workspace, no max_blocks.  FrameDicts: dictionary d is dict + off[d], len[d] bytes; frame i uses dictionary idx[i]
// (nullptr: dictionary 0); ndicts == 0 is the plain call.
struct FrameDicts {
    const std::uint8_t *dict; const std::uint64_t *off; const std::uint32_t *len; std::uint32_t ndicts; const std::uint32_t *idx;
};
inline Result decompressFramePrefix(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap) {
    return wrap(zlz4f_decompress_frame_prefix(src, n, dst, cap));
}
inline Result decompressFramePrefixUsingDict(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap,
                                             const std::uint8_t *dict, std::size_t dict_len) {
    return wrap(zlz4f_decompress_frame_prefix_using_dict(src, n, dst, cap, dict, dict_len));
}
inline Result decompressFramePrefixBatch(void *stream, const Frames &f) {
    return wrap(zlz4f_batch_decompress_frame_prefix(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result,
                                                    f.nframes));
}
inline Result decompressFramePrefixBatchUsingDict(void *stream, const Frames &f, const FrameDicts &d) {
    return wrap(zlz4f_batch_decompress_frame_prefix_using_dict(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap,
                                                               f.result, f.nframes, d.dict, d.off, d.len, d.ndicts, d.idx));
}
// frame index and range decoding (include/zlz4_amd.h; no counterpart in the reference): frameIndexBatch keeps the per-block
// decoded sizes of the size query as (position, decoded offset) entries, planFrameRanges sizes the slots and the item table
// from the index alone, decompressFrameRangeBatch decodes only the blocks that overlap [a, b): range r's bytes stand at
// dst + dst_off[r] + skip[r].  The index is the caller's data and is checked against the frame.  decompressFrameRange: one
// frame from host memory, exactly [a, b) at dst; it builds the index on every call.
using IndexEntry = zlz4f_index_entry;
using Range = zlz4f_range;
struct FrameIndex { const IndexEntry *index; const std::uint64_t *idx_off; const std::int64_t *idx_n; };
inline std::size_t frameIndexBatchWorkspace(std::uint32_t nframes, std::uint32_t max_blocks) {
    return zlz4f_batch_frame_index_workspace(nframes, max_blocks);
}
inline Result frameIndexBatch(void *stream, const Frames &f, IndexEntry *d_index, const std::uint64_t *d_idx_off,
                              const std::uint64_t *d_idx_cap, std::int64_t *d_idx_n, std::uint32_t max_blocks, void *ws,
                              std::size_t ws_bytes) {
    return wrap(zlz4f_batch_frame_index(stream, f.src, f.src_off, f.src_len, d_index, d_idx_off, d_idx_cap, d_idx_n, f.nframes,
                                        max_blocks, ws, ws_bytes));
}
inline Result planFrameRanges(void *stream, const FrameIndex &x, std::uint32_t nframes, const Range *d_range, std::uint32_t nranges,
                              std::uint32_t align, std::uint64_t *d_dst_off, std::uint64_t *d_dst_cap, std::uint64_t *d_totals) {
    return wrap(zlz4f_batch_plan_frame_ranges(stream, x.index, x.idx_off, x.idx_n, nframes, d_range, nranges, align, d_dst_off,
                                              d_dst_cap, d_totals));
}
inline std::size_t decompressFrameRangeBatchWorkspace(std::uint32_t nranges, std::uint32_t max_items) {
    return zlz4f_batch_decompress_frame_range_workspace(nranges, max_items);
}
// f.dst, f.dst_off, f.dst_cap, f.result are per RANGE here (nranges of them), f.src* and f.nframes per frame
inline Result decompressFrameRangeBatch(void *stream, const Frames &f, const FrameIndex &x, const Range *d_range,
                                        std::uint64_t *d_skip, std::uint32_t nranges, std::uint32_t max_items, void *ws,
                                        std::size_t ws_bytes) {
    return wrap(zlz4f_batch_decompress_frame_range(stream, f.src, f.src_off, f.src_len, x.index, x.idx_off, x.idx_n, f.nframes,
                                                   d_range, f.dst, f.dst_off, f.dst_cap, d_skip, f.result, nranges, max_items, ws,
                                                   ws_bytes));
}
inline Result decompressFrameRange(const std::uint8_t *src, std::size_t n, std::uint64_t a, std::uint64_t b, std::uint8_t *dst,
                                   std::size_t cap) {
    return wrap(zlz4f_decompress_frame_range(src, n, a, b, dst, cap));
}
// multiframe buffers (include/zlz4_amd.h; no counterpart in the reference): frames and skippable frames back to back, as in
// a .lz4 file.  multiframeSplitBatch delimits the members of every buffer (t.member == nullptr: count mode) and writes them
// as the items of the frame batch calls; multiframePlanBatch packs a buffer's items into one run of bytes;
// multiframeFinishBatch folds the item results: the first member that is not OK decides, else the decoded size.  Whatever
// the split cannot delimit is the last member and reaches to the end of its buffer.
using Member = zlz4f_member;
struct Multiframes { const std::uint8_t *src; const std::uint64_t *src_off, *src_len; std::uint32_t nbuf; };
struct MemberTable {
    Member *member; const std::uint64_t *mem_off, *mem_cap;
    std::uint64_t *item_first, *item_off, *item_len; std::int64_t *result;
};
inline Result multiframeSplitBatch(void *stream, const Multiframes &m, std::uint64_t *d_count, std::uint64_t *d_totals,
                                   const MemberTable &t) {
    return wrap(zlz4f_batch_multiframe_split(stream, m.src, m.src_off, m.src_len, m.nbuf, d_count, d_totals, t.member, t.mem_off,
                                             t.mem_cap, t.item_first, t.item_off, t.item_len, t.result));
}
inline Result multiframePlanBatch(void *stream, const std::int64_t *d_size, const std::uint64_t *d_item_first, std::uint32_t nbuf,
                                  std::uint32_t align, std::uint64_t *d_dst_off, std::uint64_t *d_dst_cap,
                                  std::uint64_t *d_out_off, std::uint64_t *d_out_size, std::uint64_t *d_totals) {
    return wrap(zlz4f_batch_multiframe_plan(stream, d_size, d_item_first, nbuf, align, d_dst_off, d_dst_cap, d_out_off, d_out_size,
                                            d_totals));
}
inline Result multiframeFinishBatch(void *stream, const MemberTable &t, const std::int64_t *d_size,
                                    const std::int64_t *d_item_result, std::uint32_t nbuf, std::int64_t *d_result) {
    return wrap(zlz4f_batch_multiframe_finish(stream, t.member, t.mem_off, t.result, t.item_first, d_size, d_item_result, nbuf,
                                              d_result));
}
inline Result multiframeDecompressedSize(const std::uint8_t *src, std::size_t n, std::uint32_t decode_flags = 0) {
    return wrap(zlz4f_multiframe_decompressed_size(src, n, decode_flags));
}
inline Result decompressMultiframe(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap,
                                   std::uint32_t decode_flags = 0) {
    return wrap(zlz4f_decompress_multiframe(src, n, dst, cap, decode_flags));
}
// file index and file range decoding (include/zlz4_amd.h; no counterpart in the reference): bytes [a, b) of whole .lz4 files.
// fileIndexBatch is the frame index across the members of a record-mode split (split_totals: a HOST pointer to the split's
// four totals): one run of (position in the buffer, offset in the file's content) per block in member order; it writes
// idx_off itself.  The plan is planFrameRanges with nframes = the buffers.  decompressFileRangeBatch is
// decompressFrameRangeBatch whose items each find their own member: a range may cross frame, skippable and legacy members.
// decompressFileRange: one file from host memory, exactly [a, b) at dst; it builds the index on every call.
struct FileSplit {
    const Member *member; const std::uint64_t *mem_off; const std::int64_t *split_result;
    const std::uint64_t *item_first, *item_off, *item_len, *leg_len; const std::uint64_t *split_totals;
};
inline std::size_t fileIndexBatchWorkspace(std::uint32_t nbuf, const std::uint64_t *split_totals) {
    return zlz4f_batch_file_index_workspace(nbuf, split_totals);
}
inline Result fileIndexBatch(void *stream, const Multiframes &m, const FileSplit &s, IndexEntry *d_index, std::uint64_t *d_idx_off,
                             std::uint64_t idx_cap, std::int64_t *d_idx_n, void *ws, std::size_t ws_bytes) {
    return wrap(zlz4f_batch_file_index(stream, m.src, m.src_off, m.src_len, m.nbuf, s.member, s.mem_off, s.split_result,
                                       s.item_first, s.item_off, s.item_len, s.leg_len, s.split_totals, d_index, d_idx_off,
                                       idx_cap, d_idx_n, ws, ws_bytes));
}
inline std::size_t decompressFileRangeBatchWorkspace(std::uint32_t nranges, std::uint32_t max_items) {
    return zlz4f_batch_decompress_file_range_workspace(nranges, max_items);
}
// f.dst, f.dst_off, f.dst_cap, f.result are per RANGE here (nranges of them), f.src* and f.nframes per buffer
inline Result decompressFileRangeBatch(void *stream, const Frames &f, const FrameIndex &x, const FileSplit &s,
                                       const Range *d_range, std::uint64_t *d_skip, std::uint32_t nranges,
                                       std::uint32_t max_items, void *ws, std::size_t ws_bytes) {
    return wrap(zlz4f_batch_decompress_file_range(stream, f.src, f.src_off, f.src_len, x.index, x.idx_off, x.idx_n, f.nframes,
                                                  s.member, s.mem_off, s.split_result, d_range, f.dst, f.dst_off, f.dst_cap,
                                                  d_skip, f.result, nranges, max_items, ws, ws_bytes));
}
inline Result decompressFileRange(const std::uint8_t *src, std::size_t n, std::uint64_t a, std::uint64_t b, std::uint8_t *dst,
                                  std::size_t cap, std::uint32_t split_flags = ZLZ4F_SPLIT_LEGACY) {
    return wrap(zlz4f_decompress_file_range(src, n, a, b, dst, cap, split_flags));
}
// seekable files (include/zlz4_amd.h; no counterpart in the reference): a SEEK TABLE is the last, skippable member of a file
// and stores the file's member rows and index entries.  appendSeekTableBatch writes it behind every buffer from the split
// and the file index; loadSeekTableBatch reads both tables back from the file's tail (count mode: d_member null), checking
// their shape only -- the range call stays the judge; concatBatch lays items back to back, file by file.  seekTable writes
// the table member of one file in host memory to dst; decompressFileRangeEx takes the tables from the file's seek table
// where range_flags asks for it and the file ends in a well-formed one.
constexpr std::uint32_t SEEK_TABLE_MAGICNUMBER = ZLZ4F_SEEK_TABLE_MAGICNUMBER, RANGE_SEEK_TABLE = ZLZ4F_RANGE_SEEK_TABLE;
inline std::size_t seekTableBound(std::uint64_t nmembers, std::uint64_t nblocks) {
    return zlz4f_seek_table_bound(nmembers, nblocks);
}
inline Result appendSeekTableBatch(void *stream, std::uint8_t *d_buf, const std::uint64_t *d_buf_off,
                                   const std::uint64_t *d_buf_len, const std::uint64_t *d_buf_cap, std::uint32_t nbuf,
                                   const FileSplit &s, const FrameIndex &x, std::int64_t *d_result) {
    return wrap(zlz4f_batch_append_seek_table(stream, d_buf, d_buf_off, d_buf_len, d_buf_cap, nbuf, s.member, s.mem_off,
                                              s.split_result, x.index, x.idx_off, x.idx_n, d_result));
}
inline Result loadSeekTableBatch(void *stream, const Multiframes &m, std::uint64_t *d_count, std::uint64_t *d_totals,
                                 Member *d_member, const std::uint64_t *d_mem_off, const std::uint64_t *d_mem_cap,
                                 std::int64_t *d_split_result, IndexEntry *d_index, std::uint64_t *d_idx_off,
                                 std::uint64_t idx_cap, std::int64_t *d_idx_n) {
    return wrap(zlz4f_batch_load_seek_table(stream, m.src, m.src_off, m.src_len, m.nbuf, d_count, d_totals, d_member, d_mem_off,
                                            d_mem_cap, d_split_result, d_index, d_idx_off, idx_cap, d_idx_n));
}
inline std::size_t concatBatchWorkspace(std::uint32_t nitems) { return zlz4f_batch_concat_workspace(nitems); }
inline Result concatBatch(void *stream, const std::uint8_t *d_src, const std::uint64_t *d_item_off, const std::int64_t *d_item_len,
                          const std::uint64_t *d_item_first, std::uint32_t nbuf, std::uint32_t nitems, std::uint8_t *d_dst,
                          const std::uint64_t *d_dst_off, const std::uint64_t *d_dst_cap, std::int64_t *d_result, void *ws,
                          std::size_t ws_bytes) {
    return wrap(zlz4f_batch_concat(stream, d_src, d_item_off, d_item_len, d_item_first, nbuf, nitems, d_dst, d_dst_off, d_dst_cap,
                                   d_result, ws, ws_bytes));
}
inline Result seekTable(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap,
                        std::uint32_t split_flags = ZLZ4F_SPLIT_LEGACY) {
    return wrap(zlz4f_seek_table(src, n, dst, cap, split_flags));
}
inline Result decompressFileRangeEx(const std::uint8_t *src, std::size_t n, std::uint64_t a, std::uint64_t b, std::uint8_t *dst,
                                    std::size_t cap, std::uint32_t split_flags = ZLZ4F_SPLIT_LEGACY,
                                    std::uint32_t range_flags = ZLZ4F_RANGE_SEEK_TABLE) {
    return wrap(zlz4f_decompress_file_range_ex(src, n, a, b, dst, cap, split_flags, range_flags));
}
// dictionary files (include/zlz4_amd.h; no counterpart in the reference): the file calls with ONE DICTIONARY PER FILE.
// FrameDicts here has one idx entry per buffer (nullptr: dictionary 0).  Every block of a member that declares independent
// blocks sees the dictionary's last 64 KiB, block 0 of one that declares linked blocks, no block of a legacy member.  The
// index call needs the lengths alone.  multiframeItemDictsBatch spreads the per-buffer index over the items of a split, for
// the dictionary frame calls; decompressFileRangeUsingDict is decompressFileRangeEx with a dictionary.
inline std::size_t fileIndexUsingDictBatchWorkspace(std::uint32_t nbuf, const std::uint64_t *split_totals) {
    return zlz4f_batch_file_index_using_dict_workspace(nbuf, split_totals);
}
inline Result fileIndexUsingDictBatch(void *stream, const Multiframes &m, const FileSplit &s, IndexEntry *d_index,
                                      std::uint64_t *d_idx_off, std::uint64_t idx_cap, std::int64_t *d_idx_n,
                                      const FrameDicts &d, void *ws, std::size_t ws_bytes) {
    return wrap(zlz4f_batch_file_index_using_dict(stream, m.src, m.src_off, m.src_len, m.nbuf, s.member, s.mem_off,
                                                  s.split_result, s.item_first, s.item_off, s.item_len, s.leg_len, s.split_totals,
                                                  d_index, d_idx_off, idx_cap, d_idx_n, d.len, d.ndicts, d.idx, ws, ws_bytes));
}
inline std::size_t decompressFileRangeUsingDictBatchWorkspace(std::uint32_t nranges, std::uint32_t max_items) {
    return zlz4f_batch_decompress_file_range_using_dict_workspace(nranges, max_items);
}
inline Result decompressFileRangeUsingDictBatch(void *stream, const Frames &f, const FrameIndex &x, const FileSplit &s,
                                                const Range *d_range, std::uint64_t *d_skip, std::uint32_t nranges,
                                                std::uint32_t max_items, const FrameDicts &d, void *ws, std::size_t ws_bytes) {
    return wrap(zlz4f_batch_decompress_file_range_using_dict(stream, f.src, f.src_off, f.src_len, x.index, x.idx_off, x.idx_n,
                                                             f.nframes, s.member, s.mem_off, s.split_result, d_range, f.dst,
                                                             f.dst_off, f.dst_cap, d_skip, f.result, nranges, max_items, d.dict,
                                                             d.off, d.len, d.ndicts, d.idx, ws, ws_bytes));
}
inline Result multiframeItemDictsBatch(void *stream, const std::uint64_t *d_item_first, std::uint32_t nbuf, std::uint32_t nitems,
                                       const std::uint32_t *d_dict_idx, std::uint32_t *d_item_dict_idx) {
    return wrap(zlz4f_batch_multiframe_item_dicts(stream, d_item_first, nbuf, nitems, d_dict_idx, d_item_dict_idx));
}
inline Result decompressFileRangeUsingDict(const std::uint8_t *src, std::size_t n, std::uint64_t a, std::uint64_t b,
                                           std::uint8_t *dst, std::size_t cap, const std::uint8_t *dict, std::size_t dict_len,
                                           std::uint32_t split_flags = ZLZ4F_SPLIT_LEGACY, std::uint32_t range_flags = 0) {
    return wrap(zlz4f_decompress_file_range_using_dict(src, n, a, b, dst, cap, split_flags, range_flags, dict, dict_len));
}
// legacy frames (include/zlz4_amd.h; no counterpart in the reference): what `lz4 -l` writes -- the magic 0x184C2102, then
// { u32 size, block } repeated.  One frame in host memory per call; `consumed` (may be null) receives where the frame ends,
// which is where the next member of a concatenated file starts.  The batch calls are those of the C header.
namespace legacy {
using Prefs = zlz4f_legacy_prefs;                 // block_size 0 = 8 MiB; compression_level <= 0 = fast
constexpr std::uint32_t MAGICNUMBER = ZLZ4F_LEGACY_MAGICNUMBER, BLOCK_SIZE = ZLZ4F_LEGACY_BLOCK_SIZE,
                        BLOCK_BOUND = ZLZ4F_LEGACY_BLOCK_BOUND;
inline std::size_t compressFrameBound(std::size_t src_size, const Prefs *prefs = nullptr) {
    return zlz4f_legacy_compress_frame_bound(src_size, prefs);
}
inline Result compressFrame(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap,
                            const Prefs *prefs = nullptr) {
    return wrap(zlz4f_compress_legacy_frame(src, n, dst, cap, prefs));
}
inline Result frameDecompressedSize(const std::uint8_t *src, std::size_t n, std::size_t *consumed = nullptr) {
    return wrap(zlz4f_legacy_frame_decompressed_size(src, n, consumed));
}
inline Result decompressFrame(const std::uint8_t *src, std::size_t n, std::uint8_t *dst, std::size_t cap,
                              std::size_t *consumed = nullptr) {
    return wrap(zlz4f_decompress_legacy_frame(src, n, dst, cap, consumed));
}
}  // namespace legacy
}  // namespace lz4f

}  // namespace zlz4
