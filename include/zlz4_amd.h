/*
 * zlz4_amd.h -- C ABI of the MI355X-native LZ4 block codec (drop-in for the
 * hot path of jedisct1/zig-lz4).  Every entry point below replaces one name
 * that the reference re-exports from src/root.zig; the reference-side binding
 * (Zig `extern "c"` declarations) is shown in INTEGRATION.md.
 *
 * All citations are relative to the reference tree (/root/reference/).
 * Plain pointers and sizes only: no torch / HIP types in the signatures
 * (a HIP stream is passed as `void*`, NULL = the default stream).
 *
 * Result convention (reference: Zig error unions, src/lz4.zig:48-55):
 *   >= 0  number of bytes written
 *   <  0  error, mirroring lz4.Error / lz4f.Error in declaration order.
 * The library is HIP-only: there is NO CPU fallback.  If no gfx950 device is
 * usable every compute entry point returns ZLZ4_ERR_DEVICE.
 */
#ifndef ZLZ4_AMD_H
#define ZLZ4_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lz4.Error (src/lz4.zig:48-55) ---- */
#define ZLZ4_ERR_OUTPUT_TOO_SMALL      (-1)
#define ZLZ4_ERR_INPUT_TOO_LARGE       (-2)
#define ZLZ4_ERR_CORRUPTED_DATA        (-3)
#define ZLZ4_ERR_DECOMPRESSION_FAILED  (-4)
#define ZLZ4_ERR_INVALID_STATE         (-5)
#define ZLZ4_ERR_ALLOCATION_FAILED     (-6)
/* ---- new in this library ---- */
#define ZLZ4_ERR_DEVICE                (-7)   /* HIP runtime / no gfx950 device / launch failure */
#define ZLZ4_ERR_UNSUPPORTED           (-8)   /* a request the device path cannot serve (content checksum of a split frame) */
#define ZLZ4_ERR_VERIFY                (-9)   /* zlz4_batch_verify: the compressed block does not decode back to its input */

/* ---- lz4f.Error (src/lz4f.zig:31-55): -(100 + 1-based declaration index) ---- */
#define ZLZ4F_ERR_GENERIC                   (-101)
#define ZLZ4F_ERR_MAX_BLOCK_SIZE_INVALID    (-102)
#define ZLZ4F_ERR_BLOCK_MODE_INVALID        (-103)
#define ZLZ4F_ERR_PARAMETER_INVALID         (-104)
#define ZLZ4F_ERR_COMPRESSION_LEVEL_INVALID (-105)
#define ZLZ4F_ERR_HEADER_VERSION_WRONG      (-106)
#define ZLZ4F_ERR_BLOCK_CHECKSUM_INVALID    (-107)
#define ZLZ4F_ERR_RESERVED_FLAG_SET         (-108)
#define ZLZ4F_ERR_ALLOCATION_FAILED         (-109)
#define ZLZ4F_ERR_SRC_SIZE_TOO_LARGE        (-110)
#define ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL    (-111)
#define ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE   (-112)
#define ZLZ4F_ERR_FRAME_TYPE_UNKNOWN        (-113)
#define ZLZ4F_ERR_FRAME_SIZE_WRONG          (-114)
#define ZLZ4F_ERR_SRC_PTR_WRONG             (-115)
#define ZLZ4F_ERR_DECOMPRESSION_FAILED      (-116)
#define ZLZ4F_ERR_HEADER_CHECKSUM_INVALID   (-117)
#define ZLZ4F_ERR_CONTENT_CHECKSUM_INVALID  (-118)

/* ---- constants re-exported by src/root.zig:46-49 / src/lz4.zig:12-25 / src/lz4hc.zig:28-31 ---- */
#define ZLZ4_MINMATCH            4
#define ZLZ4_MAX_INPUT_SIZE      0x7E000000u
#define ZLZ4_DISTANCE_MAX        65535u
#define ZLZ4HC_CLEVEL_MIN        2
#define ZLZ4HC_CLEVEL_DEFAULT    9
#define ZLZ4HC_CLEVEL_MAX        12
#define ZLZ4F_MAGICNUMBER        0x184D2204u     /* src/lz4f.zig:12 */
#define ZLZ4_STREAM_TABLE_ENTRIES 4096u          /* Stream.hashTable, src/lz4.zig:752 (LZ4_HASH_SIZE_U32, :33) */

/* ======================================================================
 * 1. Single-buffer entry points, HOST pointers -- the names root.zig binds.
 *    Each stages the buffer to the current HIP device, runs the batch kernel
 *    on one block and copies the result back (PCIe-inclusive).  Re-entrant
 *    like the reference (no global state besides the lazily created device
 *    context).
 *
 *    CORRECT, NOT FAST -- USE THE BATCH CALLS (section 2) OR THE FRAME CALLS
 *    (section 3) FOR THROUGHPUT.  One block is one wavefront's serial chain:
 *    a 64 KiB zlz4_compress_default call takes ~1.9 ms (912 windows of ~2 us,
 *    measured on MI355X; the one-thread host port of the reference needs
 *    0.2 ms), zlz4_decompress_safe ~1.0 ms, whatever the staging costs -- the
 *    greedy parse of ONE block cannot be spread over the chip without changing
 *    its output.  A program that loops over blocks through these calls gets
 *    slower, not faster; hand the whole batch to zlz4_batch_* instead (65 536
 *    blocks per call run at ~94 GiB/s compress / ~410 GiB/s decompress).
 * ====================================================================== */

/* replaces lz4.compressBound, src/lz4.zig:80-83 (pure arithmetic, no device) */
size_t  zlz4_compress_bound(size_t input_size);

/* replaces lz4.compressDefault, src/lz4.zig:283-285 */
int64_t zlz4_compress_default(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap);

/* replaces lz4.compressFast, src/lz4.zig:292-447 (acceleration clamped to [1,65537] as :321) */
int64_t zlz4_compress_fast(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                           uint32_t acceleration);

/* replaces lz4hc.compressHC, src/lz4hc.zig:1440-1453.  Levels <2 -> 9, >12 -> 12 (:1445).
 * All strategies of the level table (:72-86) run on the device: 2 lz4mid, 3..9 lz4hc, 10..12 lz4opt.
 *
 * HAZARD, levels 10..12: the output is the reference's output byte for byte, and the reference's lz4opt has a defect
 * (its "good enough -> encode now" branch, src/lz4hc.zig:1207-1256, reads arrival records as forward steps): the
 * stream it emits does NOT always decode back to the input.  Level 10 loses ordinary text blocks (every 64 KiB block
 * of the benchmark's text), levels 11 and 12 lose some inputs; a few inputs return OutputTooSmall where the reference
 * itself underflows.  Bit-parity with the reference is the contract here, so nothing is "fixed" silently: callers that
 * need their data back should use levels 2..9, or verify by decoding (zlz4_decompress_safe) before they drop the
 * source.  The same applies to zlz4f_compress_frame(_device) with compression_level >= 10 -- add a content checksum
 * there and the decoder will at least report the damage. */
int64_t zlz4_compress_hc(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                         int32_t compression_level);

/* replaces lz4hc.sizeofStateHC, src/lz4hc.zig:1492-1494 (= @sizeOf(Context), tables + scalars) */
size_t  zlz4_sizeof_state_hc(void);

/* replaces lz4hc.compressHCExtState, src/lz4hc.zig:1457-1489, for a context in its initial state (Context.init(),
 * :405-419 -- what compressHC itself passes, :1450): level < 1 -> 9, level 1 -> lz4mid, > 12 -> 12; dst_cap == 0 ->
 * OutputTooSmall.  The device keeps its tables in LDS / its own workspace: `state` is only validated (non-null,
 * >= zlz4_sizeof_state_hc() bytes, else InvalidState) and never read or written, so a context that still holds the
 * tables of an earlier call (the reference would search them, :1001-1006 resets only the index base) is treated as
 * fresh -- carrying history from call to call is the streaming API, which is out of scope. */
int64_t zlz4_compress_hc_ext_state(void *state, size_t state_len, const uint8_t *src, size_t src_len,
                                   uint8_t *dst, size_t dst_cap, int32_t compression_level);

/* replaces lz4.decompressSafe, src/lz4.zig:257-259 (decompressGeneric :89-251, no dict) */
int64_t zlz4_decompress_safe(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap);

/* replaces lz4.decompressSafePartial, src/lz4.zig:619-621: decompressGeneric with targetOutputSize as the
 * output limit (:99, :109) -- i.e. OutputTooSmall as soon as a sequence would pass `target_output_size`.  The call that
 * returns the first bytes of a block instead is zlz4_decompress_safe_prefix. */
int64_t zlz4_decompress_safe_partial(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                     size_t target_output_size);

/* replaces lz4.decompressSafeUsingDict, src/lz4.zig:960-962: decompressGeneric (:89-251) with the external dictionary
 * `dict` in front of dst.  A match whose offset reaches in front of dst reads dict ++ dst (:181-225); CorruptedData iff
 * offset > op + dict_len (:189-192), checked after the match's OutputTooSmall (:174).  An empty dictionary (dict_len == 0,
 * dict may be NULL) gives exactly zlz4_decompress_safe.  Only the last min(dict_len, 65536) bytes are staged (offsets
 * are <= 65535).  dict must not overlap dst.  dict == NULL with dict_len > 0 -> InvalidState. */
int64_t zlz4_decompress_safe_using_dict(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                        const uint8_t *dict, size_t dict_len);

/* replaces lz4.decompressSafePartialUsingDict, src/lz4.zig:967-969: the same with target_output_size as the output
 * limit (:99, :109), as zlz4_decompress_safe_partial.  The call that returns the first bytes of a block instead is
 * zlz4_decompress_safe_prefix_using_dict. */
int64_t zlz4_decompress_safe_partial_using_dict(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                                size_t target_output_size, const uint8_t *dict, size_t dict_len);

/* Prefix decoding: the first dst_cap bytes of a block (no counterpart in the reference; what liblz4's
 * LZ4_decompress_safe_partial(src, dst, src_len, dst_cap, dst_cap) gives for a valid block).  dst_cap is both the number
 * of bytes wanted and the size of dst.  The walk is decompressGeneric's (src/lz4.zig:89-251) with oend = dst_cap and these
 * changes:
 *   - it stops and returns dst_cap as soon as dst_cap bytes are out: tested at the top of the loop (beside :113), right
 *     after the literal copy and right after the match copy.  Nothing behind that point is read: after literals that end
 *     exactly at dst_cap, the offset and match length of that sequence are not validated;
 *   - literals: the length bytes and :136 are unchanged (a run that passes the end of src is CorruptedData even when the
 *     cut falls inside it); instead of :137, min(lit, dst_cap - op) bytes are copied;
 *   - match: :146, :149, :154 (offset 0) and the extension bytes (:160-168) are unchanged, :174 is dropped, CorruptedData
 *     iff offset > op + dict_len (:181-192 / :231) on the full offset, then the first min(ml, dst_cap - op) bytes of the
 *     match are copied with the reference's byte-by-byte meaning (it may start in the dictionary, cross its end and run
 *     over itself).
 * The result is never OutputTooSmall: it is dst_cap (cut), the decoded size S < dst_cap (the block ended first), or
 * CorruptedData for a defect met before dst_cap bytes were out.  src_len == 0 or dst_cap == 0 gives 0 (:97-98).
 * Consequences: where zlz4_decompressed_size gives S >= 0 the result is min(S, dst_cap) and the bytes are the first
 * min(S, dst_cap) bytes of the full decode; for dst_cap >= S the result and the first S bytes are those of
 * zlz4_decompress_safe(_using_dict).  One limit, the size query's: a single literal or match length saturates at
 * 0xFFFF0000 as in the decoders, so this holds for blocks in which no single run or match is longer than that.
 * The _using_dict call stages only the last min(dict_len, 65536) bytes; dict == NULL with dict_len > 0 -> InvalidState. */
int64_t zlz4_decompress_safe_prefix(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap);
int64_t zlz4_decompress_safe_prefix_using_dict(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                               const uint8_t *dict, size_t dict_len);

/* Streaming compression, lz4.Stream (src/lz4.zig:751-866).  `table` is Stream.hashTable: ZLZ4_STREAM_TABLE_ENTRIES
 * u32 in HOST memory, staged with the data (correct, not fast -- the batch calls of section 2 are the fast path).  The
 * rest of the Stream struct (dictionary slice, dictSize, currentOffset, saveDict) is host bookkeeping in the bindings.
 *
 * zlz4_stream_load_dict replaces Stream.loadDict (:798-820): the table is reset, then
 * table[hash4(rd32(tail + i))] = i for i in [0, dictSize - 5] of tail = the last dictSize = min(dict_len, 65536)
 * bytes (last writer wins; 4 bytes or fewer hash nothing).  Returns dictSize (0 for an empty dictionary).
 *
 * zlz4_stream_compress_fast_continue replaces Stream.compressFastContinue (:822-836): compressFast's loop starting from
 * `table`, which receives the final table on success.  InputTooLarge, 0 bytes, 1..12 bytes (compressAsLiterals) and
 * any error leave the table unchanged.
 * The reference reads every table entry as a position in the CURRENT src (:656-659), so a loaded dictionary only
 * changes which in-block matches the greedy parse finds; no output block refers to the dictionary, every block
 * decodes with plain decompressSafe, and the ratio gains nothing from it.  This is reproduced byte for byte.
 * table == NULL, or dict == NULL with dict_len > 0 -> InvalidState. */
int64_t zlz4_stream_load_dict(uint32_t *table, const uint8_t *dict, size_t dict_len);
int64_t zlz4_stream_compress_fast_continue(uint32_t *table, const uint8_t *src, size_t src_len, uint8_t *dst,
                                           size_t dst_cap, uint32_t acceleration);

/* Compression against an external dictionary (no counterpart in the reference: its Stream.compressFastContinue reads
 * every loaded table entry as a position in the current block, src/lz4.zig:656-659, so its blocks never refer to the
 * dictionary).  With tail = the last D = min(dict_len, 65536) bytes of `dict` and V = tail ++ src: the entry checks of
 * compressFastContinue (:823-827: InputTooLarge above ZLZ4_MAX_INPUT_SIZE, 0 for 0 bytes, compressAsLiterals for 1..12
 * bytes), then compressFastWithHashTable's loop (:624-740) statement for statement on V, with
 *   - the table starting as Stream.loadDict(dict) leaves it (:798-820; what zlz4_batch_load_dict writes),
 *   - anchor = D and ip = max(D, 1) at entry (:626-633): the record's first byte may match into the dictionary,
 *   - mflimitPlusOne = D + src_len - 12, matchLimit = D + src_len - 5, every position a position in V,
 *   - nothing else changed: validity test, unconditional put, skip schedule, no backward extension, forward extension
 *     up to matchLimit (it may run from the dictionary into the record and over itself), one put after a match, every
 *     OutputTooSmall test at the same point, offset = ip - match.  Position 0 of V is never matchable (0 = empty).
 * The block decodes with zlz4_decompress_safe_using_dict(dst, .., dict, dict_len) (and with liblz4's decoder) to src;
 * its size is at most zlz4_compress_bound(src_len).  With an empty dictionary the bytes and the status are
 * zlz4_compress_fast's.  The record and the tail are staged and the table is computed on the device (correct, not
 * fast: zlz4_batch_compress_fast_using_dict is the fast path).  dict == NULL with dict_len > 0 -> InvalidState. */
int64_t zlz4_compress_fast_using_dict(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                      const uint8_t *dict, size_t dict_len, uint32_t acceleration);

/* Levels 3..9 with a dictionary (no counterpart in the reference: its HC stream type is not ported).
 * With tail = the last D = min(dict_len, 65536) bytes of `dict`, V = tail ++ src and N = D + src_len:
 *   - entry checks: dict == NULL with dict_len > 0 -> InvalidState; the level is normalised as compressHC does (< 2 -> 9,
 *     > 12 -> 12, src/lz4hc.zig:1446-1452) and a level of 2, 10, 11 or 12 -> ZLZ4_ERR_UNSUPPORTED, nothing touched (level 2's
 *     tables depend on the parse, so its state is not a function of the bytes; levels 10..12 reproduce a defect of the
 *     reference whose streams do not always decode, see the HAZARD note at zlz4_compress_hc); then compressHC's and
 *     compressHCExtState's checks on the record (:1442-1445, :1461): InputTooLarge above ZLZ4_MAX_INPUT_SIZE, 0 for 0
 *     bytes, OutputTooSmall for dst_cap == 0;
 *   - src_len < 13: encodeLiterals(src) (:995-998, :1394-1425), the dictionary plays no part;
 *   - otherwise compressHashChain (:976-1064) statement for statement on V with a fresh context, nextToUpdate = 0,
 *     prefixStart = V, dictLimit = lowLimit = 0 (the index of a byte is its position in V), ip = anchor = D, iend = N,
 *     mflimit = N - 12, matchlimit = N - 5.  So insertHC puts every position of V below ip into the chain (all of the
 *     tail before the first search), insertAndGetWiderMatch runs with iLowLimit = ip (no backward extension; position 0
 *     of V reads as empty; nbAttempts counts dictionary and record candidates alike), level 9 runs the pattern analysis
 *     (its reverse count may run down into the tail), a match may start in the tail, run into the record and over itself,
 *     and the last literals are refused where the reference would overrun, as in zlz4_compress_hc.
 * The block decodes with zlz4_decompress_safe_using_dict(dst, .., dict, dict_len) (and with liblz4's decoder) to src;
 * its size is at most zlz4_compress_bound(src_len).  With an empty dictionary the bytes and the status are
 * zlz4_compress_hc's.  The record and the tail are staged and the batch pipeline runs on one block (correct, not fast:
 * zlz4_batch_compress_hc_using_dict is the fast path). */
int64_t zlz4_compress_hc_using_dict(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                    const uint8_t *dict, size_t dict_len, int32_t compression_level);

/* Streaming decompression, lz4.StreamDecode (src/lz4.zig:870-957).  The reference's fields as byte addresses (0 = null):
 * dict / dict_len = externalDict / extDictSize, prefix / prefix_len = prefixEnd.ptr / prefixSize.  The state holds no
 * data: a call never reads the previous output, only compares its address with the new dst (see the warning below).
 *
 * zlz4_stream_decode_init = StreamDecode.init (all zero).  zlz4_set_stream_decode = setStreamDecode (:904-909):
 * (dict, dict_len, null, 0); dict == NULL is the null slice (dict_len is then taken as 0).
 *
 * zlz4_decompress_safe_continue = decompressSafeContinue (:912-939) on host buffers:
 *   A  prefix_len == 0 && dict_len == 0: zlz4_decompress_safe; on success (prefix, prefix_len) = (dst, result).
 *   B  otherwise, with a dictionary (dict_len > 0): zlz4_decompress_safe_using_dict (only its last 64 KiB is staged);
 *      without one: decompressGeneric with lowPrefix = prefix (dst if prefix is 0), i.e. a match at output position op
 *      with offset o is CorruptedData unless op - o >= max(0, prefix - dst), tested where decompressSafe tests
 *      o > op.  On success the state becomes (0, 0, dst, result): the dictionary is used once (:936).
 *   Any error leaves the state unchanged.  src_len == 0 or dst_cap == 0 return 0, a success (in B the pending
 *   dictionary is consumed).  A state with dict_len > 0 and prefix != 0 (unreachable through these calls; the reference
 *   would underflow at :213) returns InvalidState; sd == NULL -> InvalidState.  The previous output is never staged.
 *
 * WARNING (a defect of the reference, reproduced): lowPrefix is where the previous output STARTS, and without a
 * dictionary nothing in front of it may be referenced.  When the previous output lies ABOVE dst in memory, every match
 * that reaches further back than prefix - dst bytes before dst + op fails with CorruptedData.  Two layouts hit this: a
 * ring buffer of zlz4_decoder_ring_buffer_size bytes once it wraps to its start, and a double buffer whose second half
 * is lower in memory than the first.  Blocks whose matches stay inside their own output are not affected.
 *
 * zlz4_decoder_ring_buffer_size = decoderRingBufferSize (:954-957): 0 for 0, else 65536 + 14 + max_block_size. */
typedef struct zlz4_stream_decode {
    uint64_t dict, dict_len, prefix, prefix_len;
} zlz4_stream_decode_t;
void    zlz4_stream_decode_init(zlz4_stream_decode_t *sd);
void    zlz4_set_stream_decode(zlz4_stream_decode_t *sd, const uint8_t *dict, size_t dict_len);
int64_t zlz4_decompress_safe_continue(zlz4_stream_decode_t *sd, const uint8_t *src, size_t src_len, uint8_t *dst,
                                      size_t dst_cap);
size_t  zlz4_decoder_ring_buffer_size(size_t max_block_size);

/* Decompressed size of one block, HOST pointer (no counterpart in the reference, whose callers must know it): what
 * zlz4_decompress_safe returns for `src` into a destination of 0xFFFFFFFF bytes, or, with dict_len > 0, what
 * zlz4_decompress_safe_using_dict returns there with a dictionary of dict_len bytes -- the size, CorruptedData, or
 * OutputTooSmall for a block that decodes to more than 0xFFFFFFFF bytes.  Only the dictionary's length matters (:189-192);
 * its bytes are not needed.  src_len == 0 gives 0.  Nothing is decoded: see zlz4_batch_decompressed_size. */
int64_t zlz4_decompressed_size(const uint8_t *src, size_t src_len, size_t dict_len);

/* replaces lz4.sizeofState, src/lz4.zig:524-526 (= @sizeOf(HashTable) = 16384) */
size_t  zlz4_sizeof_state(void);

/* replaces lz4.compressFastExtState, src/lz4.zig:531-546: InvalidState when the caller's state buffer is
 * smaller than sizeofState(), otherwise the output of compressFast (the device keeps its tables in LDS;
 * the state buffer is only validated, never written). */
int64_t zlz4_compress_fast_ext_state(void *state, size_t state_len, const uint8_t *src, size_t src_len,
                                     uint8_t *dst, size_t dst_cap, uint32_t acceleration);

/* replaces lz4.compressDestSize, src/lz4.zig:551-616: largest prefix of src whose compressDefault output fits
 * dst (the reference's binary search, same probes in the same order).  *src_size: in = bytes available,
 * out = bytes consumed.  Returns the compressed size.  dst holds the compression of the consumed prefix (the
 * reference leaves the output of its LAST probe there, which is not always that one). */
int64_t zlz4_compress_dest_size(const uint8_t *src, uint8_t *dst, size_t dst_cap, size_t *src_size);

/* ======================================================================
 * 2. Batch entry points, DEVICE pointers -- the data-parallel hot path.
 *    Block i reads  d_in  + d_in_off[i]  (d_in_len[i] bytes) and writes
 *    d_out + d_out_off[i] (capacity d_out_cap[i]); d_result[i] receives what
 *    the single-buffer call would have returned for that block.  All arrays
 *    live in device memory.  Kernels are enqueued on `stream` (hipStream_t)
 *    and the call returns without synchronising.  Return: 0 or ZLZ4_ERR_*.
 *
 *    PRECONDITION of the compress calls: d_in_len[i] <= max_in_len for every
 *    block.  max_in_len selects the table width (16-bit positions up to
 *    64 KiB blocks) and sizes the HC workspace; a block that is longer gets
 *    d_result[i] = ZLZ4_ERR_INVALID_STATE and is not compressed (nothing is
 *    written outside its own output slot, the other blocks are unaffected).
 * ====================================================================== */
int32_t zlz4_batch_compress_fast(void *stream,
                                 const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                 uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                 int64_t *d_result, uint32_t nblocks, uint32_t max_in_len,
                                 uint32_t acceleration);

int32_t zlz4_batch_decompress_safe(void *stream,
                                   const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                   uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                   int64_t *d_result, uint32_t nblocks);

/* decompressSafeUsingDict (src/lz4.zig:960-962) per block: block i reads the dictionary d_dict + d_dict_off[i]
 * (d_dict_len[i] bytes, any length; only its last 65536 bytes can be reached).  A dictionary shared by every block is
 * one copy with the same offset for all.  Dictionaries are read-only and must not overlap any output slot.  Same
 * contract as zlz4_batch_decompress_safe: device pointers, asynchronous, no allocation (graph-capturable). */
int32_t zlz4_batch_decompress_safe_using_dict(void *stream,
                                              const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                              uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                              const uint8_t *d_dict, const uint64_t *d_dict_off,
                                              const uint32_t *d_dict_len, int64_t *d_result, uint32_t nblocks);

/* Prefix decoding per block (zlz4_decompress_safe_prefix above): the argument lists of the two
 * decode calls above, with d_out_cap[i] both the number of bytes wanted of block i and the size of its slot.
 * d_result[i] = min(decoded size, d_out_cap[i]), or CorruptedData for a defect met before d_out_cap[i] bytes were out;
 * never OutputTooSmall.  The walk of block i ends where its prefix does: a 4 KiB prefix of a 64 KiB block costs about a
 * sixteenth of the full decode's walk.  No byte outside [d_out_off[i], d_out_off[i] + d_out_cap[i]) is written; bytes of
 * the slot behind d_result[i] are left as they were.  Same contract as the decode calls: device pointers, asynchronous,
 * no allocation, no read-back (graph-capturable).  A null array (d_dict may be null: dictionaries of length 0) or a
 * misaligned one (8 bytes for the 64-bit arrays, 4 for the 32-bit ones) returns InvalidState and launches nothing. */
int32_t zlz4_batch_decompress_safe_prefix(void *stream,
                                          const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                          uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                          int64_t *d_result, uint32_t nblocks);
int32_t zlz4_batch_decompress_safe_prefix_using_dict(void *stream,
                                                     const uint8_t *d_in, const uint64_t *d_in_off,
                                                     const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                                     const uint32_t *d_out_cap, const uint8_t *d_dict,
                                                     const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                                                     int64_t *d_result, uint32_t nblocks);

/* Decompressed sizes, for compressed blocks whose decoded size the caller does not know (an LZ4 block does not carry it;
 * no counterpart in the reference).  d_size[i] = what decompressSafe (src/lz4.zig:257-259) returns for block i into a
 * destination of 0xFFFFFFFF bytes, the library's per-block limit; with d_dict_len given, what decompressSafeUsingDict
 * (:960-962) returns there with a dictionary of d_dict_len[i] bytes (d_dict_len == NULL: no dictionary; only the length
 * takes part, :189-192, no dictionary byte is read).  So d_size[i] is the size, CorruptedData, or OutputTooSmall for a
 * block that decodes to more than 0xFFFFFFFF bytes; d_in_len[i] == 0 gives 0.  The walk is decompressGeneric's (:89-251)
 * with the decoder's decision order; no output is touched.
 * Consequence: for s = d_size[i] >= 1, zlz4_batch_decompress_safe(_using_dict) of block i with capacity s returns s, and
 * with a capacity of s - 1 >= 1 it returns OutputTooSmall: s is the smallest capacity that decodes the block.  One
 * limit: the decoders saturate a single literal or match length at 0xFFFF0000 while the query
 * counts exactly, so the consequence holds for blocks in which no single literal run or match is longer than
 * 0xFFFF0000 bytes; a block with a longer one gets its true size here and is not decoded to it.
 * Device pointers, asynchronous, no allocation, no read-back (graph-capturable).  A null d_in / d_in_off / d_in_len /
 * d_size or a misaligned array (8 bytes for the 64-bit arrays, 4 for the 32-bit ones) returns InvalidState and launches
 * nothing.  StreamDecode runs have no size query: whether a match is valid there depends on where the caller puts the
 * outputs; for outputs placed back to back, query every call's block on its own. */
int32_t zlz4_batch_decompressed_size(void *stream,
                                     const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                     const uint32_t *d_dict_len, int64_t *d_size, uint32_t nblocks);

/* Output slots from sizes, on the device: slot i holds max(d_size[i], 0) bytes rounded up to a multiple of `align`,
 * d_out_off[i] is the exclusive scan of the slot sizes (slots are packed in block order), d_out_cap[i] = d_size[i], or 0
 * for a failed block (a decode call then returns 0 for it and writes nothing), *d_total = the bytes all slots take.  The
 * three outputs are what zlz4_batch_decompress_safe takes as d_out_off / d_out_cap, so size -> plan -> decode needs one
 * read-back (the total, to allocate) or none (an arena of known size).  align: 0 or 1 = packed, else a power of two up to
 * 4096; anything else returns InvalidState.  Null or misaligned arrays return InvalidState and launch nothing (n == 0
 * needs only d_total, which receives 0).  Asynchronous, no allocation, graph-capturable. */
int32_t zlz4_batch_plan_outputs(void *stream, const int64_t *d_size, uint32_t n, uint32_t align,
                                uint64_t *d_out_off, uint32_t *d_out_cap, uint64_t *d_total);

/* Stream.loadDict (src/lz4.zig:798-820) per dictionary: table i (d_tables + i * ZLZ4_STREAM_TABLE_ENTRIES u32) receives
 * the table of dictionary i = d_dict + d_dict_off[i] (d_dict_len[i] bytes); d_result[i] = its return value, dictSize.
 * d_tables must be 16-byte aligned (as every table of zlz4_batch_compress_fast_continue), else InvalidState. */
int32_t zlz4_batch_load_dict(void *stream, const uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                             uint32_t *d_tables, int64_t *d_result, uint32_t ndicts);

/* Stream.compressFastContinue (src/lz4.zig:822-836) per block: block i starts from table d_table_idx[i] of d_table_in
 * (d_table_idx == NULL: table i) and its final table goes to table i of d_table_out (NULL: not written).  Tables are
 * ZLZ4_STREAM_TABLE_ENTRIES u32 each; d_table_in and d_table_out must be 16-byte aligned (the kernel moves tables in
 * 16-byte vectors), else the call returns InvalidState and launches nothing.  d_table_out[i] always holds what the reference's Stream.hashTable holds after the
 * call: the input table where the block did not compress (InputTooLarge, InvalidState, 0..12 bytes, OutputTooSmall).
 * A shared dictionary = one loaded table every block points at; a chained stream step = identity indexing with
 * d_table_out == d_table_in (in place; anything else that overlaps, or in place with an index array, is not allowed:
 * the latter returns InvalidState).  Same contract as zlz4_batch_compress_fast otherwise (max_in_len, asynchronous,
 * no allocation).  Blocks compress exactly as in zlz4_stream_compress_fast_continue above: no ratio gain from a
 * dictionary. */
int32_t zlz4_batch_compress_fast_continue(void *stream,
                                          const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                          uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                          const uint32_t *d_table_in, const uint32_t *d_table_idx, uint32_t *d_table_out,
                                          int64_t *d_result, uint32_t nblocks, uint32_t max_in_len,
                                          uint32_t acceleration);

/* zlz4_compress_fast_using_dict per block (no counterpart in the reference): block i is compressed against the
 * dictionary d_dict + d_dict_off[i] (d_dict_len[i] bytes, any length; only the last 65536 take part) starting from
 * table d_table_idx[i] of d_table (d_table_idx == NULL: table i), which must be what zlz4_batch_load_dict wrote for
 * that dictionary: ZLZ4_STREAM_TABLE_ENTRIES u32 per table, d_table 16-byte aligned as for
 * zlz4_batch_compress_fast_continue.  Any other table contents still give a block that decodes to the input
 * (`match < ip` bounds every read, the 4-byte compare vouches for every match); only the dictionary's own table gives the
 * specified bytes.  A shared dictionary = one dictionary, one table, the same offset and index for every block.  The
 * previous record as dictionary = dictionaries inside d_in, their tables from one zlz4_batch_load_dict over the
 * records.  Dictionaries and tables are read-only and must not overlap any output slot; no table is returned.
 * max_in_len and max_dict_len are preconditions that select the table width (16-bit positions while
 * max_in_len + min(max_dict_len, 65536) <= 65547): a block with d_in_len[i] > max_in_len or
 * min(d_dict_len[i], 65536) > max_dict_len gets InvalidState and writes nothing.  d_result[i] = what the single call
 * returns; no byte outside the block's output slot is written.  Null arrays (d_dict may be NULL when max_dict_len == 0),
 * a d_table that is not 16-byte aligned or another misaligned array (8 bytes for the 64-bit arrays, 4 for the 32-bit
 * ones) return InvalidState and launch nothing.  Asynchronous, no allocation, no read-back (graph-capturable). */
int32_t zlz4_batch_compress_fast_using_dict(void *stream,
                                            const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                            uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                            const uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                                            const uint32_t *d_table, const uint32_t *d_table_idx,
                                            int64_t *d_result, uint32_t nblocks, uint32_t max_in_len,
                                            uint32_t max_dict_len, uint32_t acceleration);

/* StreamDecode.decompressSafeContinue (src/lz4.zig:912-939) over whole streams in one call.  Stream s makes the calls
 * [d_run_start[s], d_run_start[s + 1]) in that order (d_run_start: nstreams + 1 ascending entries, the first 0, the
 * last nblocks), call i decoding block i as in zlz4_batch_decompress_safe, from the state d_state[s] (device memory;
 * dict / prefix are DEVICE addresses).  d_result[i] = what the i-th call returns; every successful slot holds its bytes
 * (failed slots are unspecified); d_state[s] ends as the reference's StreamDecode after the run.  One step of N streams
 * is d_run_start[s] = s; one long stream is nstreams = 1.  A state with a dictionary and a prefix gives InvalidState
 * for every call of its run (as the single call); a block outside every run gets InvalidState.  Output slots must not
 * overlap each other, the inputs or the dictionaries.  The WARNING of zlz4_decompress_safe_continue applies: a slot
 * placed below the previous call's slot of its stream sees only the bytes above the previous slot's start.
 * Asynchronous, no allocation, nothing read back: the launch sequence does not depend on the data (graph-capturable).
 * d_workspace: zlz4_batch_decompress_safe_continue_workspace(nblocks, nstreams) bytes, 16-byte aligned, else
 * InvalidState (DESIGN.md section 4.2c describes the passes). */
size_t  zlz4_batch_decompress_safe_continue_workspace(uint32_t nblocks, uint32_t nstreams);
int32_t zlz4_batch_decompress_safe_continue(void *stream,
                                            const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                            uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                            const uint32_t *d_run_start, zlz4_stream_decode_t *d_state,
                                            int64_t *d_result, uint32_t nblocks, uint32_t nstreams,
                                            void *d_workspace, size_t workspace_bytes);

/* workspace for the HC path: bytes needed for `nblocks` blocks of at most `max_in_len` bytes (448 KiB per 64 KiB block
 * up to 8192 blocks = 3.5 GiB, about 6 GiB at most for large blocks; longer batches are processed in rounds) */
size_t  zlz4_batch_compress_hc_workspace(uint32_t nblocks, uint32_t max_in_len);
int32_t zlz4_batch_compress_hc(void *stream,
                               const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                               uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                               int64_t *d_result, uint32_t nblocks, uint32_t max_in_len,
                               int32_t compression_level, void *d_workspace, size_t workspace_bytes);

/* zlz4_compress_hc_using_dict per block: block i against the dictionary d_dict + d_dict_off[i] (d_dict_len[i] bytes, any
 * length; only the last 65536 take part).  No table argument: the HC state is derived from the bytes.  A shared
 * dictionary = one copy, the same offset for every block; dictionaries may lie inside d_in (the previous record); they
 * are read-only and must not overlap any output slot.  Every block is staged as tail ++ record in the workspace
 * (zlz4_batch_compress_hc_using_dict_workspace bytes, 16-byte aligned; longer batches run in rounds).  max_in_len and
 * max_dict_len are preconditions that size the workspace and select the link width: chain links in LDS while
 * min(max_dict_len, 65536) + max_in_len <= 65536, in device memory otherwise -- both give the specified bytes.  A block
 * with d_in_len[i] > max_in_len or min(d_dict_len[i], 65536) > max_dict_len gets InvalidState and writes nothing; other
 * blocks are unaffected.  d_result[i] = what the single call returns; no byte outside the block's output slot is
 * written.  Null arrays (d_dict may be NULL when max_dict_len == 0), a misaligned array (8 bytes for the 64-bit arrays, 4
 * for the 32-bit ones), a workspace that is too small, null or misaligned return InvalidState, a level the single call
 * does not serve returns ZLZ4_ERR_UNSUPPORTED; all of them launch nothing.  Asynchronous, no allocation, no read-back
 * (graph-capturable like zlz4_batch_compress_hc). */
size_t  zlz4_batch_compress_hc_using_dict_workspace(uint32_t nblocks, uint32_t max_in_len, uint32_t max_dict_len);
int32_t zlz4_batch_compress_hc_using_dict(void *stream,
                                          const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                          uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                          const uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                                          int64_t *d_result, uint32_t nblocks, uint32_t max_in_len, uint32_t max_dict_len,
                                          int32_t compression_level, void *d_workspace, size_t workspace_bytes);

/* Dictionary training (no counterpart in the reference, which takes dictionaries and makes none).
 * A fastCover-style selection in integers only, so that the device and the model (tools/pyref/zig_lz4_train_dict.py)
 * agree byte for byte.  One GROUP is a run of samples and yields one dictionary; the result is a raw lz4 dictionary (bytes
 * to put in front of a record, no header), ready for every *_using_dict call.
 *   - Parameters, for the whole call: d in {4, 6, 8} the d-mer length, k in 16..1024 with k >= d the segment length, f in
 *     10..24 the log2 of the frequency table; m = k - d + 1.  `reserved` is not read.
 *   - Per group a capacity C <= 65536 (lz4 never looks further back than 64 KiB).
 *   - Buffer: B = the group's samples back to back in order, S bytes, S <= 2^27; d-mers may span sample boundaries.
 *     nd = S - d + 1.  nd <= 0 or C == 0: the result is 0, nothing is written.
 *   - Hash: v = the d bytes at p as a little-endian integer; h(p) = ((v << (64 - 8d)) * 0xCF1BBCDCB7A56463 mod 2^64)
 *     >> (64 - f).
 *   - Frequencies: freq[x] = the number of p in [0, nd) with h(p) == x.
 *   - Epochs: nseg = ceil(C / k); E = max(1, min(nseg, nd / (8k))) (integer division); size = nd / E; epoch e is
 *     [e * size, (e + 1) * size), the last epoch ends at nd.
 *   - Steps: at most T = 2 * nseg.  tail = C, ep = 0, zero = 0.  A step
 *       1. takes epoch ep as [b, e);
 *       2. for every window start s in [b, e): score(s) = the sum of freq[h(p)] over p in [s, min(s + m, e)), where each
 *          distinct hash value counts once per window (its first occurrence in the window counts, the rest do not);
 *       3. the winner is the largest score, the lowest s on a tie;
 *       4. ep = (ep + 1) % E;
 *       5. score 0: zero += 1, stop when zero == E;
 *       6. otherwise zero = 0; seg = min(k, tail, S - s); tail -= seg; out[tail .. tail + seg) = B[s .. s + seg);
 *          freq[h(p)] = 0 for p in [s, min(s + m, e)); stop when tail == 0.
 *   - Result: L = C - tail; the dictionary is out[tail .. C), moved to the front of the group's slot (bytes [L, C) of the
 *     slot are not written).  The first segment picked stands last, nearest to the record.
 *
 * zlz4_batch_train_dict: sample i is d_src + d_src_off[i], d_src_len[i] bytes; group g is samples d_group_first[g] ..
 * d_group_first[g + 1] - 1 (ngroups + 1 entries, non-decreasing, the last at most nsamples); its dictionary goes to d_dict
 * + d_dict_off[g] (d_dict_cap[g] = C bytes) and d_result[g] = L.  A group with C > min(max_dict_cap, 65536), S > 2^27, a
 * run of samples that is none, or more bytes than the workspace was sized for gets InvalidState and writes nothing; the
 * other groups are unaffected.  max_dict_cap fixes the number of step launches (2 * ceil(min(max_dict_cap, 65536) / k)
 * pairs of score and commit; a group that is done returns at once).  The workspace:
 * zlz4_batch_train_dict_workspace(ngroups, total bytes of all samples, max_dict_cap, params) bytes, 16-byte aligned (per
 * group a state record, an output buffer and a table of 2^f counters; per sample byte the byte, its hash and its reach
 * distance: 7 bytes); the function returns 0 for parameters the call refuses.  ngroups == 0 returns 0 and reads nothing.
 * A bad d, k or f, params == NULL, ngroups > 65535, null arrays (d_src, d_src_off and d_src_len may be NULL when nsamples
 * == 0, d_dict when max_dict_cap == 0), a misaligned array (8 bytes for the 64-bit arrays, 4 for the 32-bit ones), a
 * workspace that is null, misaligned or smaller than the one for no sample bytes return InvalidState and launch nothing.
 * Asynchronous, no allocation, no read-back: samples in device memory in, dictionaries out. */
typedef struct zlz4_train_params { uint32_t d, k, f, reserved; } zlz4_train_params;
size_t  zlz4_batch_train_dict_workspace(uint32_t ngroups, uint64_t total_sample_bytes, uint32_t max_dict_cap,
                                        const zlz4_train_params *params);
int32_t zlz4_batch_train_dict(void *stream,
                              const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_len, uint32_t nsamples,
                              const uint32_t *d_group_first, uint32_t ngroups,
                              uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_cap, int64_t *d_result,
                              uint32_t max_dict_cap, const zlz4_train_params *params,
                              void *d_workspace, size_t workspace_bytes);

/* One dictionary from samples in host memory, as ZDICT_trainFromBuffer takes them: the samples lie back to back in
 * `samples`, sample i has sample_sizes[i] bytes.  Returns L (the dictionary is dict[0 .. L)) or a code.  Decided on the
 * host, in this order: a bad d, k or f, params == NULL, sample_sizes == NULL with nsamples > 0, dict == NULL with dict_cap >
 * 0, dict_cap > 65536, more than 2^27 sample bytes, samples == NULL with sample bytes -> InvalidState; fewer than d sample
 * bytes or dict_cap == 0 -> 0.  Otherwise the samples are staged and zlz4_batch_train_dict runs with one group. */
int64_t zlz4_train_dict(const uint8_t *samples, const size_t *sample_sizes, uint32_t nsamples, uint8_t *dict, size_t dict_cap,
                        const zlz4_train_params *params);

/* lz4.compressDestSize (src/lz4.zig:551-616) per block: d_in_len[i] is *srcSizePtr on entry and d_out_cap[i] is dst.len.
 * d_result[i] and d_consumed[i] receive what zlz4_compress_dest_size returns and leaves in *src_size; bytes [0, result)
 * of the output slot hold compressDefault of the consumed prefix (the best probe, as in the single call), bytes
 * [result, cap) are not written.  A block longer than max_in_len gets InvalidState and consumed 0 (nothing written).
 * Every block is compressed once at full length into the workspace (zlz4_batch_compress_dest_size_workspace bytes,
 * 8-byte aligned, at least nblocks x compressBound(max_in_len)); the reference's search is then replayed on the device
 * from that one stream.  A workspace that is too small, null or misaligned returns InvalidState and launches nothing.
 * Same contract as zlz4_batch_compress_fast otherwise (asynchronous, no allocation, no read-back). */
size_t  zlz4_batch_compress_dest_size_workspace(uint32_t nblocks, uint32_t max_in_len);
int32_t zlz4_batch_compress_dest_size(void *stream,
                                      const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                      uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                      int64_t *d_result, uint32_t *d_consumed, uint32_t nblocks, uint32_t max_in_len,
                                      void *d_workspace, size_t workspace_bytes);

/* Opt-in check for the levels whose output the reference itself does not always get right (10..12, see the HAZARD note
 * at zlz4_compress_hc): decodes every compressed block on the device and compares it with its input.
 *   d_comp_result[i] : what the compress call wrote for block i (size, or a negative code, which is passed through)
 *   d_verify[i]      : receives d_comp_result[i] if the block decodes back to its d_in_len[i] input bytes,
 *                      ZLZ4_ERR_VERIFY if it does not
 * Returns the number of blocks that failed the check (0 = all good), or ZLZ4_ERR_*.  Unlike the calls above this one
 * allocates its scratch memory itself (a decode arena as large as the input) and synchronises `stream` before returning;
 * it is a safety net, not part of the hot path.  No counterpart in the reference. */
int64_t zlz4_batch_verify(void *stream,
                          const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                          const uint8_t *d_comp, const uint64_t *d_comp_off, const int64_t *d_comp_result,
                          int64_t *d_verify, uint32_t nblocks);

/* ======================================================================
 * 3. Frame container (src/lz4f.zig), HOST pointers.
 * ====================================================================== */
/* src/lz4f.zig:106-122 (FrameInfo + Preferences flattened; NULL = defaults) */
typedef struct zlz4f_prefs {
    uint32_t block_size_id;     /* 0 default, 4 = 64 KiB, 5 = 256 KiB, 6 = 1 MiB, 7 = 4 MiB  (:64-79) */
    uint32_t block_mode;        /* 0 linked, 1 independent (header bit only, :159-161)         */
    uint32_t content_checksum;  /* 0 / 1                                                      */
    uint32_t block_checksum;    /* 0 / 1                                                      */
    uint64_t content_size;      /* 0 = unknown                                                */
    uint32_t dict_id;           /* 0 = none                                                   */
    int32_t  compression_level; /* <= 0 fast (accel 1); > 0 -> compressHC(level)  (:393-404)   */
} zlz4f_prefs;

/* replaces lz4f.compressFrameBound, src/lz4f.zig:274-301 (pure arithmetic) */
size_t  zlz4f_compress_frame_bound(size_t src_size, const zlz4f_prefs *prefs);
/* replaces lz4f.compressFrame, src/lz4f.zig:354-446 (the unused allocator argument is dropped) */
int64_t zlz4f_compress_frame(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                             const zlz4f_prefs *prefs);
/* replaces lz4f.decompressFrame, src/lz4f.zig:541-638 */
int64_t zlz4f_decompress_frame(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap);
/* replaces lz4f.headerSize, src/lz4f.zig:451-480 (pure arithmetic) */
int64_t zlz4f_header_size(const uint8_t *src, size_t src_len);

/* Device-resident frame variants (config 5: per-GPU shard already in HBM).
 * src/dst are DEVICE pointers; the frame header/end-mark bytes and the size
 * prefix sum are produced on the device too.  Synchronises `stream` before
 * returning the frame size. */
int64_t zlz4f_compress_frame_device(void *stream, const uint8_t *d_src, size_t src_len,
                                    uint8_t *d_dst, size_t dst_cap, const zlz4f_prefs *prefs);
int64_t zlz4f_decompress_frame_device(void *stream, const uint8_t *d_src, size_t src_len,
                                      uint8_t *d_dst, size_t dst_cap);

/* One frame over several GPUs (BASELINE configs[4]).  compressFrame's block loop (src/lz4f.zig:379-430) carries no
 * state from block to block, so rank r of G compresses its contiguous range of blocks and the frame is the plain
 * concatenation of the ranks' segments in rank order:
 *     segment = [frame header, if ZLZ4F_SEG_FIRST] [block header, data, block checksum]* [end mark, if ZLZ4F_SEG_LAST]
 * d_src is the rank's byte range of the input; every range but the last must be a multiple of the block size.  The
 * only cross-rank step is the prefix sum of the returned segment sizes (where each segment goes).  A content checksum
 * is one serial XXH32 chain over the whole input (:384-386) and is refused here (ZLZ4_ERR_UNSUPPORTED) unless the
 * segment is the whole frame.  With both flags the call is zlz4f_compress_frame_device. */
#define ZLZ4F_SEG_FIRST 1u
#define ZLZ4F_SEG_LAST  2u
int64_t zlz4f_compress_frame_segment_device(void *stream, const uint8_t *d_src, size_t src_len,
                                            uint8_t *d_dst, size_t dst_cap, const zlz4f_prefs *prefs,
                                            uint32_t segment_flags);
/* The inverse for one rank: decodes the blocks of a segment (src/lz4f.zig:563-621).  A segment without
 * ZLZ4F_SEG_FIRST has no frame header, so `prefs` must carry the frame's block_checksum flag and block_size_id
 * (what rank 0 read from the header); without ZLZ4F_SEG_LAST no end mark is expected. */
int64_t zlz4f_decompress_frame_segment_device(void *stream, const uint8_t *d_src, size_t src_len,
                                              uint8_t *d_dst, size_t dst_cap, const zlz4f_prefs *prefs,
                                              uint32_t segment_flags);

/* Batch frames, DEVICE pointers: N independent frames in one launch sequence.  Frame f reads d_src + d_src_off[f]
 * (d_src_len[f] bytes) and writes d_dst + d_dst_off[f] (capacity d_dst_cap[f]); d_result[f] receives what
 * zlz4f_compress_frame_device / zlz4f_decompress_frame_device return for that frame alone (frame size, decompressed
 * size or the frame's error code).  Same contract as the block batch calls of section 2: all pointers are device
 * pointers, kernels are enqueued on `stream` and the call returns without synchronising; nothing is allocated and
 * nothing is read back, so both calls can be captured into a hipGraph.  Return: 0, ZLZ4_ERR_DEVICE, or
 * ZLZ4_ERR_INVALID_STATE when the workspace is smaller than its size function says (then nothing is launched).
 * Output slots must not overlap each other or any source.  Bytes inside a failed frame's slot are unspecified; no byte
 * outside [d_dst_off[f], d_dst_off[f] + d_dst_cap[f]) is ever written.
 *
 * max_blocks is the capacity of the block table that all frames share.  Blocks are numbered in frame order; a frame
 * with blocks whose numbers do not all fall below max_blocks gets ZLZ4_ERR_INVALID_STATE and nothing is written for
 * it (a frame without blocks needs no entries).  Earlier frames are unaffected.  Compress: a frame has
 * ceil(src_len[f] / block size) blocks.  Decompress: what the frame's block chain holds, found on the device.
 *
 * Compress: `prefs` is shared by the batch (block size, checksums, dict_id, level routing of compressFrame: fast with
 * acceleration 1 for level <= 0, compressHC with the level clamped otherwise).  Without ZLZ4F_BATCH_CONTENT_SIZE
 * prefs->content_size goes into every header as given; with it prefs->content_size must be 0 (else
 * ZLZ4F_ERR_PARAMETER_INVALID) and frame f carries src_len[f] as its content size (none for an empty frame).  A frame
 * whose d_dst_cap[f] < zlz4f_compress_frame_bound(src_len[f], prefs) gets ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL
 * (src/lz4f.zig:363-366).  The workspace holds the block table, a compressBound-sized slot per entry and, for
 * compression_level > 0, the HC workspace of max_blocks blocks.
 * Decompress: every parameter comes from the frame's own header, so one batch may mix frames of any block size and
 * checksum flags (compressFrame, the lz4 CLI); error order of src/lz4f.zig:541-638 per frame. */
#define ZLZ4F_BATCH_CONTENT_SIZE 1u   /* batch_flags: frame f's header carries src_len[f] as its content size */
/* batch_flags: write LINKED frames (no counterpart in the reference, whose block_mode is a header bit only).  Block k of
 * frame f is zlz4_compress_fast_using_dict(block, dict = frame input[max(0, k * bs - 65536) .. k * bs]) with that
 * dictionary's own zlz4_batch_load_dict table and acceleration 1 -- the dictionary is the INPUT in front of the block,
 * also when the previous block ends up stored.  Block 0, and so every one-block frame, is compressFast's bytes.
 * Everything else is as without the flag: stored-block rule, checksums, content size, compressFrameBound check, header,
 * end mark.  Every block of every frame is still independent work.  liblz4's LZ4F_decompress and
 * zlz4f_batch_decompress_frame_ex(ZLZ4F_DECODE_LINKED) decode such a frame; the calls without that flag do not.
 * The flag needs prefs->block_mode == 0, so that FLG declares what the blocks are (else ZLZ4F_ERR_PARAMETER_INVALID),
 * compression_level <= 0 in THIS call (else ZLZ4_ERR_UNSUPPORTED: the HC levels are linked by
 * zlz4f_batch_compress_frame_ex below) and a workspace of zlz4f_batch_compress_frame_workspace_ex(.., batch_flags) bytes,
 * which adds one loadDict table (16 KiB) and a dictionary descriptor per table entry (smaller: ZLZ4_ERR_INVALID_STATE); in
 * each case nothing is launched. */
#define ZLZ4F_BATCH_LINK_BLOCKS 4u   /* (2u is unassigned: ZLZ4F_ERR_PARAMETER_INVALID) */
size_t  zlz4f_batch_compress_frame_workspace_ex(uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs *prefs,
                                                uint32_t batch_flags);
size_t  zlz4f_batch_compress_frame_workspace(uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs *prefs);
int32_t zlz4f_batch_compress_frame(void *stream,
                                   const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                   uint8_t *d_dst, const uint64_t *d_dst_off, const uint64_t *d_dst_cap,
                                   int64_t *d_result, uint32_t nframes, uint32_t max_blocks,
                                   const zlz4f_prefs *prefs, uint32_t batch_flags, void *d_workspace,
                                   size_t workspace_bytes);
/* zlz4f_batch_compress_frame with linked frames at the HC levels (what `lz4 -9 -BD` and liblz4's LZ4F_* API with a level
 * write).  Same arguments.  L = prefs->compression_level as the frame calls read it: <= 0 is the fast level, 1 becomes 9,
 * above 12 becomes 12.
 *   - without ZLZ4F_BATCH_LINK_BLOCKS, or with it at the fast level: zlz4f_batch_compress_frame -- the same bytes,
 *     statuses and launch sequence (one implementation).
 *   - with ZLZ4F_BATCH_LINK_BLOCKS and L in 3..9: block k of frame f is zlz4_compress_hc_using_dict(block, dict = frame
 *     input[max(0, k * bs - 65536) .. k * bs], L) -- the dictionary is the INPUT in front of the block, also when the
 *     previous block ends up stored.  Block 0 has an empty dictionary and carries compressHC's bytes; a one-block frame
 *     is the HC frame of the plain call with the FLG block-independence bit clear.  Everything else as above: stored-block
 *     rule (csize >= len), block and content checksums, content size, the compressFrameBound check per frame, header, end
 *     mark, max_blocks / ZLZ4_ERR_INVALID_STATE per frame, the slot guarantee.  tail ++ block is a contiguous stretch of
 *     d_src, so the HC kernels read it where it lies (the staged copy of zlz4_batch_compress_hc_using_dict is not made);
 *     they may read a few bytes past a block's end inside d_src's allocation, as the plain HC levels do.  Nothing is
 *     allocated or read back, the launch sequence is fixed (graph-capturable).
 *   - with the flag and L in {2, 10, 11, 12}: ZLZ4_ERR_UNSUPPORTED, nothing launched (the levels
 *     zlz4_batch_compress_hc_using_dict refuses: lz4mid and the price-based parse have no dictionary form here).
 *   - the other refusals are the plain call's, in its order: unknown flag bits, block_mode != 0 with the flag,
 *     ZLZ4F_BATCH_CONTENT_SIZE with prefs->content_size != 0 (ZLZ4F_ERR_PARAMETER_INVALID); then the device; then a
 *     workspace that is too small, null or not 16-byte aligned (ZLZ4_ERR_INVALID_STATE).
 * zlz4f_batch_compress_frame itself keeps answering ZLZ4_ERR_UNSUPPORTED for the flag with L > 0.
 * Workspace: zlz4f_batch_compress_frame_workspace_ex(nframes, max_blocks, prefs, ZLZ4F_BATCH_LINK_BLOCKS) with L in 3..9 is
 *     the block table and slots of zlz4f_batch_compress_frame_workspace at the fast level
 *   + chunk x (12 x stride + 4 x bm_stride) bytes of links (u32), results (u64) and visited bits, where
 *     stride = 65536 + block size, bm_stride = (stride / 32 + 1) rounded up to 4 words, and
 *     chunk = min(max_blocks, 8192, 6 GiB / per-entry bytes) (at least 1): longer tables run in rounds
 *   + 20 bytes of descriptors per table entry,
 * each area rounded up to 256 bytes.  It holds no loadDict tables, no plain-HC workspace and no staged copy.  For every
 * other combination of arguments the function returns what it returned before.
 * The single-frame calls run one frame through zlz4f_batch_compress_frame_ex (max_blocks = ceil(src_len / bs), workspace
 * from the device cache; their result is the batch call's for that frame) and synchronise.  With batch_flags 0 the answer
 * is that of the call they are named after.  Their refusals are host arithmetic and come before the device check.
 * zlz4f_compress_frame_ex is the way to write one linked frame, at any supported level, from HOST memory. */
int32_t zlz4f_batch_compress_frame_ex(void *stream,
                                      const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                      uint8_t *d_dst, const uint64_t *d_dst_off, const uint64_t *d_dst_cap,
                                      int64_t *d_result, uint32_t nframes, uint32_t max_blocks,
                                      const zlz4f_prefs *prefs, uint32_t batch_flags, void *d_workspace,
                                      size_t workspace_bytes);
int64_t zlz4f_compress_frame_device_ex(void *stream, const uint8_t *d_src, size_t src_len,
                                       uint8_t *d_dst, size_t dst_cap, const zlz4f_prefs *prefs, uint32_t batch_flags);
int64_t zlz4f_compress_frame_ex(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                const zlz4f_prefs *prefs, uint32_t batch_flags);
size_t  zlz4f_batch_decompress_frame_workspace(uint32_t nframes, uint32_t max_blocks);
int32_t zlz4f_batch_decompress_frame(void *stream,
                                     const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                     uint8_t *d_dst, const uint64_t *d_dst_off, const uint64_t *d_dst_cap,
                                     int64_t *d_result, uint32_t nframes, uint32_t max_blocks, void *d_workspace,
                                     size_t workspace_bytes);

/* Decompressed size of frames.  d_size[f] = what zlz4f_batch_decompress_frame stores in d_result[f] when d_dst_cap[f] is
 * large enough: the decoded size, or the frame's error in the order of src/lz4f.zig:541-638 -- the header errors, then per
 * block FrameSizeWrong (a missing block checksum, :591), BlockChecksumInvalid (:596), DecompressionFailed (:611), the
 * first failing block deciding, then FrameSizeWrong of a broken chain (:565, :582) or of a missing content-checksum word
 * (:626).  ONE EXCEPTION: the content checksum is not verified (it is a hash of the decoded bytes): a frame whose only
 * defect is a wrong content checksum reports its size here and ContentChecksumInvalid when it is decoded.  Stored blocks
 * count their data size.  The header's content_size field is not consulted (the reference's decoder ignores it).
 * max_blocks and ZLZ4_ERR_INVALID_STATE per frame as in zlz4f_batch_decompress_frame.  The walk, scan and block-checksum
 * passes are that call's; then the size kernel of zlz4_batch_decompressed_size runs over the block table and one
 * wavefront per frame adds up.  Nothing is written besides d_size and the workspace
 * (zlz4f_batch_frame_decompressed_size_workspace bytes, 16-byte aligned; too small, null or misaligned returns
 * InvalidState and launches nothing).  Asynchronous, no allocation, no read-back (graph-capturable).
 * zlz4f_frame_decompressed_size is the same for one frame in HOST memory. */
int64_t zlz4f_frame_decompressed_size(const uint8_t *src, size_t src_len);
size_t  zlz4f_batch_frame_decompressed_size_workspace(uint32_t nframes, uint32_t max_blocks);
int32_t zlz4f_batch_frame_decompressed_size(void *stream,
                                            const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                            int64_t *d_size, uint32_t nframes, uint32_t max_blocks, void *d_workspace,
                                            size_t workspace_bytes);

/* Linked-block frames (no counterpart in the reference: its decompressFrame gives every block only its own output, so a
 * frame whose blocks refer to earlier output -- the default of liblz4's LZ4F_* API -- fails there, and in the calls
 * above, with DecompressionFailed).  Each _ex call takes decode_flags; with 0 it is the call it is named after (an
 * unknown bit: ZLZ4F_ERR_PARAMETER_INVALID, nothing launched).  With ZLZ4F_DECODE_LINKED, per frame:
 *   - FLG has the block-independence bit (0x20) SET: today's path, bytes and status as without the flag.
 *   - the bit is CLEAR: the blocks are walked in order, pos = the bytes of this frame decoded so far.  A stored block is
 *     copied (and is history for later blocks); a compressed block is zlz4_decompress_safe_using_dict(block, dst[pos ..
 *     cap], dict = dst[max(0, pos - 65536) .. pos]): a match may reach min(pos, 65536) bytes in front of the block, never
 *     in front of the frame's first output byte (src/lz4.zig:189-192).  Error order of src/lz4f.zig:541-638 as above;
 *     DecompressionFailed (:611) is decided by the history-aware decode.  Frames this library writes with default prefs
 *     declare "linked" while their blocks are independent: they take this path and give the same bytes.
 *   max_blocks, ZLZ4_ERR_INVALID_STATE per frame and the slot guarantee are unchanged.  One wavefront decodes one linked
 *   frame (a frame is a serial chain), so the parallelism is across frames; the launch sequence is fixed (no read-back,
 *   no allocation, graph-capturable).  The size query with the flag is the same walk without output: block k is what
 *   zlz4_batch_decompressed_size gives with dict_len = min(pos, 65536); the content checksum is excepted as above.
 * The workspaces grow by 8 bytes per frame (the _workspace_ex functions).  The single-frame calls run one frame through
 * the batch call (their result is the batch call's for that frame) and synchronise; zlz4f_decompress_frame_device,
 * zlz4f_decompress_frame and zlz4f_frame_decompressed_size are not rerouted.  The segment calls have no _ex form: a rank's
 * first block would need the previous rank's output. */
#define ZLZ4F_DECODE_LINKED 1u
size_t  zlz4f_batch_decompress_frame_workspace_ex(uint32_t nframes, uint32_t max_blocks, uint32_t decode_flags);
int32_t zlz4f_batch_decompress_frame_ex(void *stream,
                                        const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                        uint8_t *d_dst, const uint64_t *d_dst_off, const uint64_t *d_dst_cap,
                                        int64_t *d_result, uint32_t nframes, uint32_t max_blocks, uint32_t decode_flags,
                                        void *d_workspace, size_t workspace_bytes);
size_t  zlz4f_batch_frame_decompressed_size_workspace_ex(uint32_t nframes, uint32_t max_blocks, uint32_t decode_flags);
int32_t zlz4f_batch_frame_decompressed_size_ex(void *stream,
                                               const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                               int64_t *d_size, uint32_t nframes, uint32_t max_blocks, uint32_t decode_flags,
                                               void *d_workspace, size_t workspace_bytes);
int64_t zlz4f_decompress_frame_device_ex(void *stream, const uint8_t *d_src, size_t src_len,
                                         uint8_t *d_dst, size_t dst_cap, uint32_t decode_flags);
int64_t zlz4f_decompress_frame_ex(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, uint32_t decode_flags);
int64_t zlz4f_frame_decompressed_size_ex(const uint8_t *src, size_t src_len, uint32_t decode_flags);

/* Dictionary frames (the lz4 frame format's dictID frames: `lz4 -D dict`, liblz4's LZ4F_compressFrame_usingCDict /
 * LZ4F_decompress_usingDict; no counterpart in the reference).  T is the last D = min(dict_len, 65536) bytes of a frame's
 * dictionary, pos the bytes of the frame decoded (or consumed) so far.  Header (prefs->dict_id as given), block headers,
 * the stored-block rule, checksums, content size and the end mark are those of the calls above.
 *
 * Dictionary arguments, the same in every batch call: dictionary d is d_dict + d_dict_off[d], d_dict_len[d] bytes (any
 * length), d < ndicts; frame f uses dictionary d_dict_idx[f] (d_dict_idx == NULL: dictionary 0 for every frame; one shared
 * dictionary is ndicts = 1 with a NULL index).  d_dict_idx[f] >= ndicts gives that frame ZLZ4_ERR_INVALID_STATE (in front
 * of every other status of the frame), nothing is written for it and the other frames are unaffected.  Dictionaries are
 * read-only and must not overlap any destination slot.  The header's dictID stays informational: the caller picks the
 * dictionary, as with liblz4 (zlz4f_batch_frame_dict_id reads the field: d_dict_id[f] = the dictID, 0 when the frame has
 * none, or the header's error code; one lane per frame, so that a d_dict_idx can be built on the device).
 *
 * Decode (always history-aware, no decode_flags).  A compressed block of a frame whose FLG has the block-independence bit
 *   - SET is zlz4_decompress_safe_using_dict(block, dst[pos .. cap], dict = T): every block sees the dictionary.  These
 *     frames stay on the parallel pipeline of zlz4f_batch_decompress_frame with a dictionary descriptor per table entry.
 *   - CLEAR has the last 65536 bytes of T ++ dst[0 .. pos) as its history: a match at block output position op with offset
 *     o copies from index D + pos + op - o of W = T ++ dst[0 .. pos + op), byte by byte -- it may start in T, run across
 *     T's end into the frame's first output bytes and run over itself -- and is CorruptedData iff o > op + pos + D
 *     (tested after the match's OutputTooSmall test, src/lz4.zig:174, :189-192).  Stored blocks are copied and are
 *     history.  One wavefront per frame, as with ZLZ4F_DECODE_LINKED -- except a frame of one block, whose history is T
 *     alone: it is decoded with the independent frames (the same bytes and status; what the default preferences write for
 *     a small record).
 *   With D == 0: bytes and status of zlz4f_batch_decompress_frame_ex(.., ZLZ4F_DECODE_LINKED, ..).  Error order of
 *   src/lz4f.zig:541-638 as there; DecompressionFailed (:611) is decided by the dictionary-aware decode.
 *   Workspace: the layout of zlz4f_batch_decompress_frame_workspace_ex(.., ZLZ4F_DECODE_LINKED) + 12 bytes per frame (where
 *   T ends, D) + 12 bytes per table entry (dictionary descriptors), each area rounded up to 256 bytes.
 * Size query: the same two paths with nothing written; only the dictionary lengths are needed (zlz4_batch_decompressed_size);
 *   the content checksum is excepted as in zlz4f_batch_frame_decompressed_size.  Workspace: that of
 *   zlz4f_batch_frame_decompressed_size_workspace_ex(.., ZLZ4F_DECODE_LINKED) + 4 bytes per frame + 4 bytes per table entry.
 *
 * Compress: the fast level only (compression_level <= 0, acceleration 1); prefs->block_mode decides, so that FLG declares
 * what the blocks are:
 *   - block_mode == 1: block k = zlz4_compress_fast_using_dict(X_k, dict = T) with T's own zlz4_batch_load_dict table, every k.
 *   - block_mode == 0: block 0 is the same call; block k >= 1 is the ZLZ4F_BATCH_LINK_BLOCKS block (dict = the input
 *     [k * bs - 65536, k * bs): block sizes are >= 64 KiB, so T is out of reach from block 1 on).
 *   With an empty dictionary, byte for byte and status for status: zlz4f_batch_compress_frame (block_mode 1) and
 *   zlz4f_batch_compress_frame(.., ZLZ4F_BATCH_LINK_BLOCKS) (block_mode 0).  A using-dict block is at most
 *   zlz4_compress_bound(len), so the compressFrameBound check per frame and zlz4f_compress_frame_bound stay as they are.
 *   batch_flags: ZLZ4F_BATCH_CONTENT_SIZE only (with its rule about prefs->content_size).  Refusals, each launching nothing,
 *   in this order: another flag bit, ZLZ4F_BATCH_LINK_BLOCKS included, or the content-size rule (ZLZ4F_ERR_PARAMETER_INVALID);
 *   compression_level > 0 (ZLZ4_ERR_UNSUPPORTED); the device; null or misaligned arrays (8 bytes for the 64-bit arrays, 4
 *   for the 32-bit ones; d_dict may be NULL when max_dict_len == 0), a workspace that is too small, null or not 16-byte
 *   aligned (ZLZ4_ERR_INVALID_STATE).
 *   max_src_len and max_dict_len are preconditions as in the block calls: a frame with d_src_len[f] > max_src_len
 *   (max_src_len == 0: no bound) or whose dictionary has min(len, 65536) > max_dict_len gets ZLZ4_ERR_INVALID_STATE and
 *   writes nothing.  The dictionary compressor is given min(bs, max_src_len) as its max_in_len, so small records against a
 *   small dictionary keep the 16-bit table; output bytes do not depend on it.  The ndicts dictionaries are hashed once per
 *   call, not once per frame.
 *   Workspace: frames | 3 x u64, 4 x u32, i64 per table entry | a compressBound-sized slot per entry | one loadDict table
 *   (16 KiB) and an i64 per dictionary | 20 bytes of descriptors per entry; when block_mode == 0 and a frame may have a
 *   second block (max_src_len == 0 or > block size) also one loadDict table and 36 bytes per entry; each area rounded up to
 *   256 bytes.  batch_flags and max_dict_len do not change it.
 * max_blocks, ZLZ4_ERR_INVALID_STATE per frame, the slot guarantee and "nothing allocated, nothing read back, fixed launch
 * sequence, graph-capturable" are those of the batch frame calls above.  The single-frame calls take HOST pointers, stage
 * the frame and the dictionary's tail and run a batch of one; dict == NULL with dict_len > 0 gives InvalidState.
 * HC levels with a frame dictionary are served by the _ex calls below; the segment calls have no dictionary form. */
size_t  zlz4f_batch_compress_frame_using_dict_workspace(uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs *prefs,
                                                        uint32_t batch_flags, uint32_t ndicts, uint64_t max_src_len,
                                                        uint32_t max_dict_len);
int32_t zlz4f_batch_compress_frame_using_dict(void *stream,
                                              const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                              uint8_t *d_dst, const uint64_t *d_dst_off, const uint64_t *d_dst_cap,
                                              int64_t *d_result, uint32_t nframes, uint32_t max_blocks,
                                              const zlz4f_prefs *prefs, uint32_t batch_flags,
                                              const uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                                              uint32_t ndicts, const uint32_t *d_dict_idx,
                                              uint64_t max_src_len, uint32_t max_dict_len,
                                              void *d_workspace, size_t workspace_bytes);
size_t  zlz4f_batch_decompress_frame_using_dict_workspace(uint32_t nframes, uint32_t max_blocks);
int32_t zlz4f_batch_decompress_frame_using_dict(void *stream,
                                                const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                                uint8_t *d_dst, const uint64_t *d_dst_off, const uint64_t *d_dst_cap,
                                                int64_t *d_result, uint32_t nframes, uint32_t max_blocks,
                                                const uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                                                uint32_t ndicts, const uint32_t *d_dict_idx,
                                                void *d_workspace, size_t workspace_bytes);
size_t  zlz4f_batch_frame_decompressed_size_using_dict_workspace(uint32_t nframes, uint32_t max_blocks);
int32_t zlz4f_batch_frame_decompressed_size_using_dict(void *stream,
                                                       const uint8_t *d_src, const uint64_t *d_src_off,
                                                       const uint64_t *d_src_len, int64_t *d_size, uint32_t nframes,
                                                       uint32_t max_blocks, const uint32_t *d_dict_len, uint32_t ndicts,
                                                       const uint32_t *d_dict_idx, void *d_workspace, size_t workspace_bytes);
int32_t zlz4f_batch_frame_dict_id(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                  int64_t *d_dict_id, uint32_t nframes);
int64_t zlz4f_compress_frame_using_dict(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                        const zlz4f_prefs *prefs, const uint8_t *dict, size_t dict_len);
int64_t zlz4f_decompress_frame_using_dict(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                          const uint8_t *dict, size_t dict_len);
int64_t zlz4f_frame_decompressed_size_using_dict(const uint8_t *src, size_t src_len, size_t dict_len);

/* ---- frame prefix decoding: the first n bytes of every frame (no counterpart in the reference; what liblz4's
 * LZ4F_decompress(_usingDict) leaves in a destination of n bytes).  FP(frame, n, T), DESIGN.md section 4.4f: n =
 * d_dst_cap[f] is both the number of bytes wanted and the size of the slot, T the last D = min(dict_len, 65536) bytes of
 * the frame's dictionary (D = 0 without one), pos the bytes out so far.
 *   1. The header is parsed as by the decode calls (src/lz4f.zig:547); a header error is the result, also when n == 0.
 *      After a good header n == 0 gives 0.
 *   2. Stop rule: at the top of the block loop, in front of its condition and of the next block header, pos == n returns n.
 *      Nothing behind that point is read or validated: later block headers, checksums, the end mark, the content checksum.
 *   3. The chain is that of the decode calls (:563-600): input ending at a block boundary ends the loop, srcPos + 4 > len
 *      is FrameSizeWrong (:565), a zero word is the end mark, srcPos + sz > len is FrameSizeWrong (:582).
 *   4. With FLG bit 0x10: a missing checksum word is FrameSizeWrong (:591), a mismatch BlockChecksumInvalid (:596).  The
 *      checksum covers the block's whole data, also when only part of it will be decoded, and is checked in front of the
 *      decode.  Only blocks the walk reaches are hashed.
 *   5. A stored block: min(sz, n - pos) bytes are copied, and they are history.  Never DstMaxSizeTooSmall.
 *   6. A compressed block is the prefix decode of zlz4_decompress_safe_prefix_using_dict (section 4.2e) with n - pos bytes
 *      wanted (at most 0xFFFFFFFF); any error from it is DecompressionFailed (:611).  History is always on, as in
 *      zlz4f_batch_decompress_frame_using_dict: FLG bit 0x20 set, every block sees T alone; clear, the last 65536 bytes of
 *      T ++ dst[0 .. pos) -- a match may start in T, cross into the frame's output and run over itself.  CorruptedData iff
 *      offset > op + hist, on the full offset.
 *   7. The chain ended with pos < n (the whole frame is out): the chain's error; then, with FLG bit 0x04, FrameSizeWrong for
 *      a missing checksum word (:626), then ContentChecksumInvalid (:631) over dst[0 .. pos).  The result is pos.
 * The result is n (the frame was cut), S < n (the frame ended first) or a frame error for a defect met before n bytes were
 * out; never DstMaxSizeTooSmall, never OutputTooSmall.  Bytes of the slot behind the result are left as they were; no byte
 * outside [d_dst_off[f], d_dst_off[f] + n) is written.
 * Consequences.  Let R be the result of zlz4f_batch_decompress_frame_using_dict with a capacity that is large enough (D == 0:
 * of zlz4f_batch_decompress_frame_ex(.., ZLZ4F_DECODE_LINKED, ..)).  R = S >= 0: the result is min(S, n) and the bytes are
 * the first min(S, n) bytes of that decode.  For n > S, and for a failing frame once n exceeds the bytes that decode in
 * front of the defect, the result is R itself, error codes included.  At n == S exactly the result is S and a defect
 * behind the last byte (a bad content checksum, a broken chain tail) is not reported.  A single literal or match length
 * saturates at 0xFFFF0000 as in the decoders.
 * Batch calls: device pointers, one fixed launch (one wavefront per frame), no workspace, no max_blocks; asynchronous,
 * nothing allocated, nothing read back: graph-capturable.  Dictionary arguments as in the calls above (d_dict_idx == NULL:
 * dictionary 0; d_dict_idx[f] >= ndicts: ZLZ4_ERR_INVALID_STATE for that frame in front of every other status, nothing
 * written, the other frames unaffected; d_dict may be NULL when every dictionary is empty).  ndicts == 0 is the plain call:
 * no frame has a dictionary and no dictionary argument is read.  nframes == 0 returns 0.  A null array or a misaligned one
 * (8 bytes for the 64-bit arrays, 4 for the 32-bit ones) returns ZLZ4_ERR_INVALID_STATE and launches nothing.
 * The host calls stage the frame and the dictionary's last 64 KiB and run a batch of one; dict == NULL with dict_len > 0
 * gives InvalidState.  The cut is at the end only (a start offset: the frame range calls below); the StreamDecode calls
 * and the segment calls have no prefix form. */
int32_t zlz4f_batch_decompress_frame_prefix(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                            const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                            const uint64_t *d_dst_cap, int64_t *d_result, uint32_t nframes);
int32_t zlz4f_batch_decompress_frame_prefix_using_dict(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                                       const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                                       const uint64_t *d_dst_cap, int64_t *d_result, uint32_t nframes,
                                                       const uint8_t *d_dict, const uint64_t *d_dict_off,
                                                       const uint32_t *d_dict_len, uint32_t ndicts,
                                                       const uint32_t *d_dict_idx);
int64_t zlz4f_decompress_frame_prefix(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap);
int64_t zlz4f_decompress_frame_prefix_using_dict(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                                 const uint8_t *dict, size_t dict_len);

/* ---- frame index and range decoding: bytes [a, b) of single frames whose blocks decode on their own (no counterpart in
 * the reference).  Every item is ONE frame (a multiframe buffer, below, is not served: index and
 * range see its first frame only; the file index and range calls further below see every member).  A frame is a chain of blocks; the INDEX says where block k lies and at which decoded
 * offset it starts, the RANGE DECODE decodes only the blocks that overlap [a, b), one wavefront per block.
 *
 * zlz4f_batch_frame_index: frame f with nb blocks in its chain gets nb + 1 entries at d_index + d_idx_off[f] (offsets and
 *   capacities count entries): entry k < nb = { pos: the byte position of block k's header word inside the frame, dec: the
 *   decoded offset at which block k starts }, entry nb = { pos: where the chain ended (the end mark, or the end of the
 *   input), dec: S, the decoded size }; d_result[f] = nb.  Statuses are exactly those of zlz4f_batch_frame_decompressed_size
 *   (flags 0: every block is sized as an independent block, the content checksum is set aside): wherever that query
 *   answers an error the index answers the same error and writes no entry, wherever it answers S the last entry's dec is
 *   S.  nb + 1 > d_idx_cap[f]: ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL, no entry written.  max_blocks and ZLZ4_ERR_INVALID_STATE
 *   per frame as there.  Workspace: zlz4f_batch_frame_index_workspace (= the query's), 16-byte aligned.  A null array, a
 *   d_index / d_idx_off / d_idx_cap that is not 8-byte aligned or a refused workspace return ZLZ4_ERR_INVALID_STATE and
 *   launch nothing; no device is the last refusal.  nframes == 0 returns 0.
 *
 * zlz4f_batch_plan_frame_ranges reads the index alone (d_idx_n = the index call's d_result).  Range r = { frame, reserved
 *   (0), a, b } of a frame with decoded size S = entry[nb].dec: a' = min(a, S), b' = min(b, S); k0 = the block that holds
 *   byte a', k1 the block that holds byte b' - 1 (k = the last entry of 0..nb with dec <= the byte, found by bisection; a
 *   block that decodes to nothing never holds a byte).  d_dst_cap[r] = b' - dec[k0], the slot the decode call needs; it is
 *   0, with no items, when a' == b', d_idx_n[frame] < 0, a > b or frame >= nframes (the decode call reports those), and
 *   when the entries found are no such blocks (an index that is not sorted).  d_dst_off = the exclusive scan of the slot
 *   sizes rounded up to `align` (0, 1 or a power of two up to 4096, as zlz4_batch_plan_outputs); d_totals[0] = the arena
 *   size, d_totals[1] = the sum of k1 - k0 + 1 = the max_items of the decode call.  One 16-byte read-back sizes everything.
 *   nranges == 0 stores two zeros.  Null or misaligned (8 bytes) arrays: ZLZ4_ERR_INVALID_STATE, nothing launched.
 *
 * zlz4f_batch_decompress_frame_range.  OUTPUT (zero-copy, block-aligned): slot r receives the decode of blocks k0..k1 from
 *   the start of block k0 up to byte b'; the wanted bytes stand at d_dst + d_dst_off[r] + d_skip[r], d_skip[r] = a' -
 *   dec[k0], and d_result[r] = b' - a'.  (The head of block k0 has to exist somewhere, the bytes behind it refer to it;
 *   left in the slot it costs no scratch and no second pass.)  No byte outside [d_dst_off[r], d_dst_off[r] + b' - dec[k0])
 *   is written; on any error d_skip[r] = 0 and nothing of the slot is promised.  The index is the caller's data and is NOT
 *   trusted: every position taken from it is checked against the frame before it is used as an address.  FLG and the block
 *   size come from the frame's own header.  Per range, in this order:
 *   1. ZLZ4_ERR_INVALID_STATE for frame >= nframes, a > b, reserved != 0.  Then d_idx_n[frame] < 0: that code.  Then a
 *      header error of the frame: that code.  Then ZLZ4_ERR_INVALID_STATE when entry 0's pos is not the header size, or
 *      -- a' < b' -- the entries k0..k1+1 are not a chain: k0 / k1 not found or k1 < k0, dec[k0] > a', dec[k1] >= b',
 *      dec[k1+1] < b', or for a k in k0..k1 pos[k+1] <= pos[k], pos[k] + 4 > src_len, pos[k+1] > src_len, dec[k+1] < dec[k],
 *      dec[k+1] - dec[k] above the header's block size.
 *   2. a' == b': 0, d_skip[r] = 0; nothing of the frame behind the header is read.
 *   3. d_dst_cap[r] < b' - dec[k0]: ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL.
 *   4. The range's k1 - k0 + 1 items do not fit max_items (items are laid out in range order; a range that does not fit
 *      still takes its room, as a frame in max_blocks): ZLZ4_ERR_INVALID_STATE.
 *   5. The first failing block in block order decides.  Block k, header word w at pos[k], sz = w & 0x7FFFFFFF:
 *      w == 0 (the end mark) or pos[k] + 4 + sz (+ 4 with FLG 0x10) != pos[k+1]: ZLZ4_ERR_INVALID_STATE (not this frame's index).  A block
 *      checksum mismatch: ZLZ4F_ERR_BLOCK_CHECKSUM_INVALID (over the whole block, also for a cut block).  A stored block:
 *      sz != dec[k+1] - dec[k] is ZLZ4_ERR_INVALID_STATE, else the wanted part is copied.  A compressed block wanted in full
 *      (dec[k+1] <= b'): zlz4_batch_decompress_safe with capacity dec[k+1] - dec[k]; an error or another result is
 *      ZLZ4F_ERR_DECOMPRESSION_FAILED, so a wrong dec of a full block is caught (one exception: a step of 0 is a capacity
 *      of 0, which the decoder answers with 0 without reading, src/lz4.zig:98).  The one block that b' cuts:
 *      zlz4_batch_decompress_safe_prefix with b' - dec[k1] bytes wanted; an error, or fewer bytes than wanted, is
 *      ZLZ4F_ERR_DECOMPRESSION_FAILED; nothing behind the cut is validated.
 *   6. Otherwise b' - a'.
 *   NOTHING outside blocks k0..k1 is read or validated: a defect elsewhere in the frame is not reported, the content
 *   checksum is never checked.  A linked-declared frame (FLG 0x20 clear) is taken as it is: a touched block that refers to
 *   earlier output answers ZLZ4F_ERR_DECOMPRESSION_FAILED, as zlz4f_batch_decompress_frame does (and zlz4f_batch_frame_index
 *   answers that for the frame).  Dictionary frames, a start offset inside one block and the segment calls are not served.
 *   Workspace: zlz4f_batch_decompress_frame_range_workspace(nranges, max_items) bytes, 16-byte aligned.  Null arrays
 *   (d_dst may be null only when max_items == 0), misaligned (8 bytes) arrays or a refused workspace: ZLZ4_ERR_INVALID_STATE,
 *   nothing launched; then the device.  nranges == 0 returns 0.
 * All three: asynchronous on `stream`, a fixed launch sequence, nothing allocated, nothing read back (graph-capturable).
 * The index stays valid for every later read of the same frame bytes.
 *
 * zlz4f_decompress_frame_range: one frame in HOST memory; exactly the b' - a' wanted bytes arrive at dst[0..).  Header errors
 *   are answered on the host, then a > b (ZLZ4_ERR_INVALID_STATE); the frame is staged, a host walk of the chain sizes the
 *   table, then index, plan and range run as a batch of one.  An index error is the result; dst_cap < b' - a' gives
 *   ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL in front of the decode.  It BUILDS THE INDEX ON EVERY CALL (one size query of the whole
 *   frame): a caller with several reads of one frame keeps the index and uses the batch calls. */
typedef struct { uint64_t pos; uint64_t dec; } zlz4f_index_entry;                            /* 16 bytes */
typedef struct { uint32_t frame; uint32_t reserved; uint64_t a; uint64_t b; } zlz4f_range;   /* 24 bytes */
size_t  zlz4f_batch_frame_index_workspace(uint32_t nframes, uint32_t max_blocks);
int32_t zlz4f_batch_frame_index(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                zlz4f_index_entry *d_index, const uint64_t *d_idx_off, const uint64_t *d_idx_cap,
                                int64_t *d_result, uint32_t nframes, uint32_t max_blocks, void *d_workspace,
                                size_t workspace_bytes);
int32_t zlz4f_batch_plan_frame_ranges(void *stream, const zlz4f_index_entry *d_index, const uint64_t *d_idx_off,
                                      const int64_t *d_idx_n, uint32_t nframes, const zlz4f_range *d_range, uint32_t nranges,
                                      uint32_t align, uint64_t *d_dst_off, uint64_t *d_dst_cap, uint64_t *d_totals);
size_t  zlz4f_batch_decompress_frame_range_workspace(uint32_t nranges, uint32_t max_items);
int32_t zlz4f_batch_decompress_frame_range(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                           const uint64_t *d_src_len, const zlz4f_index_entry *d_index,
                                           const uint64_t *d_idx_off, const int64_t *d_idx_n, uint32_t nframes,
                                           const zlz4f_range *d_range, uint8_t *d_dst, const uint64_t *d_dst_off,
                                           const uint64_t *d_dst_cap, uint64_t *d_skip, int64_t *d_result, uint32_t nranges,
                                           uint32_t max_items, void *d_workspace, size_t workspace_bytes);
int64_t zlz4f_decompress_frame_range(const uint8_t *src, size_t src_len, uint64_t a, uint64_t b, uint8_t *dst,
                                     size_t dst_cap);

/* ---- dictionary frames at the HC levels 3..9 (what `lz4 -9 -D dict` and LZ4F_compressFrame_usingCDict with a level
 * produce; no counterpart in the reference).  The _ex calls are the calls they are named after, with the same argument
 * lists; the plain calls keep refusing every level > 0.  L = prefs->compression_level as the frame calls read it (<= 0:
 * fast, 1 -> 9, > 12 -> 12); T, X_k, bs as above.
 *   - L <= 0: the plain call -- the same bytes, statuses, workspace size and launch sequence.
 *   - L in 3..9, block_mode == 1: block k = zlz4_compress_hc_using_dict(X_k, dict = T, L), every k.
 *   - L in 3..9, block_mode == 0: block 0 is the same call; block k >= 1 is the ZLZ4F_BATCH_LINK_BLOCKS block of
 *     zlz4f_batch_compress_frame_ex at level L (dict = the input [k * bs - 65536, k * bs), read where it lies in d_src; bs
 *     >= 65536, so T is out of reach from block 1 on).
 *   - L in { 2, 10, 11, 12 }: ZLZ4_ERR_UNSUPPORTED, nothing launched (the levels zlz4_batch_compress_hc_using_dict refuses).
 *   Header, stored-block rule (csize >= len), checksums, ZLZ4F_BATCH_CONTENT_SIZE, the compressFrameBound check per frame,
 *   the end mark, max_blocks and the three per-frame preconditions (d_dict_idx[f] >= ndicts, d_src_len[f] > max_src_len, D >
 *   max_dict_len: ZLZ4_ERR_INVALID_STATE, nothing written) are the plain call's.  An HC dictionary block is at most
 *   zlz4_compress_bound(len), so zlz4f_compress_frame_bound stands.
 *   With an empty dictionary, byte for byte and status for status: zlz4f_batch_compress_frame at level L (block_mode 1) and
 *   zlz4f_batch_compress_frame_ex(.., ZLZ4F_BATCH_LINK_BLOCKS) at level L (block_mode 0).  Every frame decodes with
 *   zlz4f_batch_decompress_frame_using_dict and the same dictionary, and with liblz4's LZ4F_decompress_usingDict.
 *   Refusals, each launching nothing, in this order: a flag bit other than ZLZ4F_BATCH_CONTENT_SIZE or that flag's
 *   content_size rule (ZLZ4F_ERR_PARAMETER_INVALID); an unsupported level (ZLZ4_ERR_UNSUPPORTED); the device; null or
 *   misaligned arrays, a workspace that is too small, null or not 16-byte aligned (ZLZ4_ERR_INVALID_STATE).
 *   Two compressor launches, one after the other on `stream`: A = the HC dictionary compressor over every block of an
 *   independent frame and block 0 of a linked one, with the dictionaries read from d_dict (no loadDict table is built),
 *   max_in_len = min(bs, max_src_len) and max_dict_len as given -- records and dictionary tail that together fit 65536
 *   bytes (4 KiB records against a dictionary of 60 KiB or less) keep the chain links in LDS; B, only when block_mode == 0
 *   and a frame may have a second block (max_src_len == 0 or > bs) = the linked HC compressor over the blocks k >= 1.  An
 *   entry that takes no part in a launch has record and dictionary length 0 there: nothing is staged for it, its result is
 *   0 and nothing is written.  Output bytes do not depend on max_src_len, max_dict_len or the link width they select.
 *   Workspace for L in 3..9: frames | 3 x u64, 4 x u32, i64 per table entry | a compressBound-sized slot per entry | 20
 *   bytes of launch A's descriptors per entry | ONE HC scratch region of max(zlz4_batch_compress_hc_using_dict_workspace(
 *   max_blocks, min(bs, max_src_len), max_dict_len), the linked HC scratch of zlz4f_batch_compress_frame_workspace_ex) --
 *   launch B is ordered behind all of launch A's work, the side stream of the HC launchers included, so the two share it
 *   -- | with launch B also 32 bytes per entry (len_b, v_off, { v_len, start }, v_len, csize_b); each area rounded up to
 *   256 bytes.  max_dict_len CHANGES this size (it sizes the staged V = T ++ record); batch_flags does not.  For every
 *   other level the function returns what zlz4f_batch_compress_frame_using_dict_workspace returns.  The chunking of the HC
 *   launchers (8192 blocks, about 6 GiB of scratch) applies as it is: longer batches run in rounds.
 *   The host call stages the frame and the dictionary's tail and runs a batch of one; its refusals are host arithmetic and
 *   come before the device check; dict == NULL with dict_len > 0 gives ZLZ4_ERR_INVALID_STATE.
 *   Nothing is allocated, nothing is read back and the launch sequence is fixed.  Under stream capture the call behaves as
 *   its HC launchers do (they fork K3 to a side stream and join it before they return, as zlz4_batch_compress_hc does):
 *   that property is inherited from them, not new. */
size_t  zlz4f_batch_compress_frame_using_dict_workspace_ex(uint32_t nframes, uint32_t max_blocks, const zlz4f_prefs *prefs,
                                                           uint32_t batch_flags, uint32_t ndicts, uint64_t max_src_len,
                                                           uint32_t max_dict_len);
int32_t zlz4f_batch_compress_frame_using_dict_ex(void *stream,
                                                 const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                                 uint8_t *d_dst, const uint64_t *d_dst_off, const uint64_t *d_dst_cap,
                                                 int64_t *d_result, uint32_t nframes, uint32_t max_blocks,
                                                 const zlz4f_prefs *prefs, uint32_t batch_flags,
                                                 const uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                                                 uint32_t ndicts, const uint32_t *d_dict_idx,
                                                 uint64_t max_src_len, uint32_t max_dict_len,
                                                 void *d_workspace, size_t workspace_bytes);
int64_t zlz4f_compress_frame_using_dict_ex(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                           const zlz4f_prefs *prefs, const uint8_t *dict, size_t dict_len);

/* ---- multiframe buffers: concatenated and skippable frames (what a .lz4 file is; no counterpart in the reference;
 * DESIGN.md section 4.4h).  A MULTIFRAME is a buffer that holds zero or more frames back to back, each of them a MEMBER.
 * Every other zlz4f_* decode call takes exactly one frame per item and ignores what follows its end mark.
 *
 * zlz4f_batch_multiframe_split walks buffer s (d_src + d_src_off[s], d_src_len[s] = n bytes) from position 0.  At pos < n:
 *   - 4 bytes remain and (magic & 0xFFFFFFF0) == 0x184D2A50: a skippable frame.  sz = the u32 LE at pos + 4; the member is
 *     { pos, 8 + sz, ZLZ4F_MEMBER_SKIPPABLE | (magic & 15) << 8 }.  Fewer than 8 bytes remain, or pos + 8 + sz > n: the kind
 *     is ZLZ4F_MEMBER_SKIPPABLE_TRUNCATED (| nibble << 8), the member reaches to n and is the last one.
 *   - anything else is a frame member { pos, len, ZLZ4F_MEMBER_FRAME }: the header (up to 19 bytes), then the block chain
 *     (header word w, sz = w & 0x7FFFFFFF, + 4 with FLG 0x10) up to and including the end mark, then the 4-byte content
 *     checksum word with FLG 0x04.
 *   - WHATEVER CANNOT BE DELIMITED IS THE LAST MEMBER AND REACHES TO n: a header error (unknown magic, the legacy magic
 *     0x184C2102, fewer than 7 bytes, ...), a chain that runs off the buffer, a missing end mark, a missing checksum word.
 *     The split never judges a frame: the frame calls give that member its error -- or, for a chain that merely lacks its
 *     end mark at the end of the buffer, its content -- exactly as they do for a frame that stands alone.  So a multiframe
 *     of one frame answers what the frame call answers for it, byte for byte and code for code.
 *   kind & 0xFF is the ZLZ4F_MEMBER_* kind, (kind >> 8) & 15 the low nibble of a skippable magic.
 *   COUNT MODE (d_member == NULL; every argument behind it is ignored): d_count[s] = the members of buffer s, d_totals =
 *     { members of all buffers, blocks of all frame members' chains (the max_blocks of the frame calls) }: one 16-byte
 *     read-back sizes everything that follows.
 *   RECORD MODE: the count again (d_count and d_totals as above), then d_item_first = the exclusive scan of d_count, nbuf + 1
 *     entries; member k of buffer s is item i = d_item_first[s] + k and is written to d_member[d_mem_off[s] + k] (offsets
 *     and capacities count entries), with the item arrays of the frame batch calls: d_item_off[i] = d_src_off[s] + pos,
 *     d_item_len[i] = len for a frame member and 0 for a skippable one.  An item of length 0 is answered by the frame calls
 *     with ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE without a byte read or written; the calls below know from `kind` to ignore
 *     that answer.  d_count[s] > d_mem_cap[s]: d_result[s] = ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL, no entry of that buffer is
 *     written and its items keep their room with length 0; otherwise d_result[s] = d_count[s].
 *   Null or 8-byte-misaligned arrays: ZLZ4_ERR_INVALID_STATE, nothing launched; the device check is the last refusal.
 *   nbuf == 0 returns 0 and stores two zeros.
 *
 * zlz4f_batch_multiframe_plan: d_size[i] = what zlz4f_batch_frame_decompressed_size_ex answered for item i (over d_item_off /
 *   d_item_len, with the caller's decode_flags).  d_dst_cap[i] = d_size[i], or 0 for an item whose query failed -- every
 *   skippable item among them; d_out_size[s] = the sum over the items of buffer s; d_out_off[s] = the exclusive scan of
 *   d_out_size rounded up to `align` (0, 1 or a power of two up to 4096, as zlz4_batch_plan_outputs); d_dst_off[i] =
 *   d_out_off[s] + the capacities of the buffer's earlier items: the decoded members of a buffer form ONE RUN of bytes in
 *   member order.  d_totals = { arena bytes, the sum of d_out_size }.  The member table is not read: the query's answer
 *   says all the plan needs.  Refusals as above; nbuf == 0 stores two zeros.
 *
 * The decode is zlz4f_batch_decompress_frame_ex over the item arrays with d_dst_off / d_dst_cap of the plan, nframes =
 *   d_totals[0] of the split and max_blocks = d_totals[1] of the split.
 *
 * zlz4f_batch_multiframe_finish folds the items into d_result[s]: a split result < 0 is the result; else the first member
 *   in member order that is not OK decides -- a frame member's d_size[i] when negative, else its d_item_result[i] when
 *   negative; ZLZ4F_MEMBER_SKIPPABLE_TRUNCATED: ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE when fewer than 8 bytes remained, else
 *   ZLZ4F_ERR_FRAME_SIZE_WRONG -- otherwise the sum of the frame members' d_item_result, which equals d_out_size[s].  An
 *   empty buffer and a buffer of skippable frames give 0.  On an error nothing of the buffer's slot is promised; no byte
 *   outside [d_out_off[s], d_out_off[s] + d_out_size[s]) is ever written.  The item results stay the caller's to read: the
 *   members in front of a defect are decoded and can be salvaged.  (With d_item_result = d_size the call folds the size
 *   query alone: what the decode answers apart from the content checksums.)
 * All three: asynchronous on `stream`, a fixed launch sequence per mode, nothing allocated, nothing read back.
 *
 * zlz4f_multiframe_decompressed_size / zlz4f_decompress_multiframe: one buffer in HOST memory, staged and run as a batch
 *   of one: count (read-back), record, size query, plan (read-back), decode, finish.  An unknown decode_flags bit:
 *   ZLZ4F_ERR_PARAMETER_INVALID, then a null pointer with a length: ZLZ4_ERR_INVALID_STATE, both before the device check.
 *   The planned total above dst_cap: ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL in front of the decode.
 *
 * NOT SERVED: a dictionary per MEMBER chosen by dictID (a member with a dictID decodes as the plain frame call decodes it;
 *   one dictionary per buffer: zlz4f_batch_multiframe_item_dicts and the dictionary frame calls over the items, below);
 *   writing multiframes (they are the concatenation of what the compress calls return).
 *   Legacy frames (magic 0x184C2102) are a member that cannot be delimited by THESE calls: ZLZ4F_ERR_FRAME_TYPE_UNKNOWN; the
 *   _ex calls below with ZLZ4F_SPLIT_LEGACY serve them.
 *
 * ---- whole .lz4 files: legacy members in multiframe buffers.  What `lz4 -d` accepts is any
 * sequence of modern frames, skippable frames and legacy frames (below).  The _ex calls take a SPLIT_FLAGS word; with
 * split_flags == 0 every output equals that of the call without _ex on the same input.  An unknown split_flags bit:
 * ZLZ4F_ERR_PARAMETER_INVALID, before any other refusal of the batch call; the host calls refuse an unknown decode_flags
 * bit first, then an unknown split_flags bit, then a null pointer with a length, all before the device check.
 *
 * zlz4f_batch_multiframe_split_ex: the arguments of zlz4f_batch_multiframe_split, split_flags, and d_leg_len.  With
 *   ZLZ4F_SPLIT_LEGACY, at a position where at least 4 bytes remain and the word is ZLZ4F_LEGACY_MAGICNUMBER the member is
 *   { pos, consumed, ZLZ4F_MEMBER_LEGACY }, consumed as READING step 2 below says: the member ends at the end of the buffer
 *   or in front of the first size word above ZLZ4F_LEGACY_BLOCK_BOUND.  It is not the last member (the walk ends on pos == n
 *   anyway) unless the walk meets a defect -- a torn size word, a size word of 0, a block that runs off the buffer -- where
 *   consumed = n: the same rule as every member that cannot be delimited.  The split never judges; the legacy call gives
 *   the member its code.  The magic alone (then the end of the buffer or a foreign word) is a member of 0 blocks and 0 bytes
 *   of content.  A foreign word that is no magic starts a frame member that cannot be delimited and gets what the frame
 *   call answers (the CLI's "stream followed by undecodable data").
 *   d_totals has FOUR entries: { members, blocks of the frame members' chains, legacy members, blocks of the legacy
 *   members }: one 32-byte read-back sizes everything.  Legacy blocks are not counted into entry 1.
 *   RECORD MODE: d_item_off as above; d_item_len[i] = len for a FRAME member, else 0; d_leg_len[i] = len for a LEGACY member,
 *   else 0 (d_leg_len: 8-byte aligned, one entry per item, required in record mode, ignored in count mode); both are 0 for
 *   every item of a buffer whose member table overflowed.  nbuf == 0 stores four zeros.
 *
 * zlz4f_batch_multiframe_select: d_out[i] = d_from_legacy[i] for the item of a LEGACY member, else d_from_frame[i]; the
 *   items of a buffer whose split result is negative take d_from_frame.  d_out may be d_from_frame itself.  One wavefront
 *   per buffer; refusals as the finish call; nbuf == 0 returns 0.
 *
 * zlz4f_batch_multiframe_finish reads a ZLZ4F_MEMBER_LEGACY member as it reads a frame member: a negative d_size[i]
 *   decides, else d_item_result[i].
 *
 * THE SEQUENCE: split_ex (count mode), read back 32 bytes, split_ex (record mode);
 *   zlz4f_batch_frame_decompressed_size_ex over (d_item_off, d_item_len) with max_blocks = totals[1];
 *   zlz4f_batch_legacy_frame_decompressed_size over (d_item_off, d_leg_len) with max_blocks = totals[3]; select; plan, read
 *   back; zlz4f_batch_decompress_frame_ex and zlz4f_batch_decompress_legacy_frame into the same arena with the plan's
 *   d_dst_off / d_dst_cap (an item of length 0 is answered ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE by either family and writes
 *   nothing whatever its capacity, so the two decodes never touch each other's slots); select; finish.  nframes =
 *   totals[0] for both families.  WHEN totals[2] == 0 THE LEGACY CALLS AND BOTH SELECTS ARE SKIPPED and the sequence is
 *   that of the calls above; otherwise the legacy calls' workspace, sized by their _workspace functions for (totals[0],
 *   totals[3]), is never empty (it holds a record per item), also where totals[3] == 0.
 *
 * zlz4f_multiframe_decompressed_size_ex / zlz4f_decompress_multiframe_ex: one buffer in HOST memory, staged and run as a
 *   batch of one through that sequence; with split_flags == 0 they make the calls of zlz4f_multiframe_decompressed_size /
 *   zlz4f_decompress_multiframe.  zlz4f_decompress_multiframe_ex(.., ZLZ4F_DECODE_LINKED, ZLZ4F_SPLIT_LEGACY) returns what
 *   `lz4 -dc` prints for the file, or the code of the first member that is not OK.
 *
 * NOT SERVED: a dictionary per MEMBER chosen by dictID (a dictionary per FILE: the dictionary file calls below).  Prefix and
 *   range decoding of a file: the file index and range calls below. */
#define ZLZ4F_MEMBER_FRAME               1u
#define ZLZ4F_MEMBER_SKIPPABLE           2u
#define ZLZ4F_MEMBER_SKIPPABLE_TRUNCATED 3u
typedef struct { uint64_t pos; uint64_t len; uint32_t kind; uint32_t buf; } zlz4f_member;    /* 24 bytes */
int32_t zlz4f_batch_multiframe_split(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                     const uint64_t *d_src_len, uint32_t nbuf, uint64_t *d_count, uint64_t *d_totals,
                                     zlz4f_member *d_member, const uint64_t *d_mem_off, const uint64_t *d_mem_cap,
                                     uint64_t *d_item_first, uint64_t *d_item_off, uint64_t *d_item_len,
                                     int64_t *d_result);
int32_t zlz4f_batch_multiframe_plan(void *stream, const int64_t *d_size, const uint64_t *d_item_first, uint32_t nbuf,
                                    uint32_t align, uint64_t *d_dst_off, uint64_t *d_dst_cap, uint64_t *d_out_off,
                                    uint64_t *d_out_size, uint64_t *d_totals);
int32_t zlz4f_batch_multiframe_finish(void *stream, const zlz4f_member *d_member, const uint64_t *d_mem_off,
                                      const int64_t *d_split_result, const uint64_t *d_item_first, const int64_t *d_size,
                                      const int64_t *d_item_result, uint32_t nbuf, int64_t *d_result);
int64_t zlz4f_multiframe_decompressed_size(const uint8_t *src, size_t src_len, uint32_t decode_flags);
int64_t zlz4f_decompress_multiframe(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                    uint32_t decode_flags);
#define ZLZ4F_SPLIT_LEGACY  1u      /* split_flags: delimit legacy frames as members */
#define ZLZ4F_MEMBER_LEGACY 4u
int32_t zlz4f_batch_multiframe_split_ex(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                        const uint64_t *d_src_len, uint32_t nbuf, uint64_t *d_count, uint64_t *d_totals,
                                        zlz4f_member *d_member, const uint64_t *d_mem_off, const uint64_t *d_mem_cap,
                                        uint64_t *d_item_first, uint64_t *d_item_off, uint64_t *d_item_len,
                                        int64_t *d_result, uint32_t split_flags, uint64_t *d_leg_len);
int32_t zlz4f_batch_multiframe_select(void *stream, const zlz4f_member *d_member, const uint64_t *d_mem_off,
                                      const int64_t *d_split_result, const uint64_t *d_item_first,
                                      const int64_t *d_from_frame, const int64_t *d_from_legacy, uint32_t nbuf,
                                      int64_t *d_out);
int64_t zlz4f_multiframe_decompressed_size_ex(const uint8_t *src, size_t src_len, uint32_t decode_flags,
                                              uint32_t split_flags);
int64_t zlz4f_decompress_multiframe_ex(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                       uint32_t decode_flags, uint32_t split_flags);

/* ---- legacy frames: what `lz4 -l` writes and the Linux kernel's unlz4 reads (vmlinuz.lz4, lz4 initramfs images); no
 * counterpart in the reference; DESIGN.md section 4.4i.  The format, as lz4io.c's LZ4IO_compressFilename_Legacy and
 * LZ4IO_decodeLegacyStream fix it: the 4-byte magic 0x184C2102, then { u32 LE size, block } repeated.  No checksums, no
 * stored blocks, no end mark; every block is an independent LZ4 block that decodes to at most 8 MiB.
 *
 * READING frame f (d_src + d_src_off[f], d_src_len[f] = n bytes):
 *   1. n < 4: ZLZ4F_ERR_FRAME_HEADER_INCOMPLETE.  A first word that is not the legacy magic: ZLZ4F_ERR_FRAME_TYPE_UNKNOWN.
 *      consumed = n in both cases.
 *   2. pos = 4, then repeat:  pos == n: the frame ends, consumed = n.  1..3 bytes remain: ZLZ4F_ERR_FRAME_SIZE_WRONG (a torn
 *      size word).  w = the u32 LE at pos.  w > ZLZ4F_LEGACY_BLOCK_BOUND: the frame ends in front of that word, consumed =
 *      pos (the CLI's "maybe a new stream": every lz4 magic -- frame, skippable, legacy -- is larger than the bound, so the
 *      next member of a concatenated file starts at consumed).  w == 0: ZLZ4F_ERR_DECOMPRESSION_FAILED (liblz4 fails an
 *      empty block; the block calls of this library answer 0 for one).  pos + 4 + w > n: ZLZ4F_ERR_FRAME_SIZE_WRONG.
 *      Otherwise { pos + 4, w } is a block and pos += 4 + w.  consumed = n after every defect of the walk.
 *   3. Block k decodes as decompressSafe into a capacity of 8 MiB: its size is what zlz4_batch_decompressed_size answers;
 *      a negative answer or a size above 8 MiB is ZLZ4F_ERR_DECOMPRESSION_FAILED.  A block of the single token 0x00
 *      decodes to 0 bytes and is valid; blocks shorter than 8 MiB are valid anywhere in the chain.
 *   4. THE FIRST DEFECT IN STREAM ORDER DECIDES (what a sequential reader meets first): a bad block in front of a torn
 *      tail gives the block's code.  Block contents never move consumed: it is the walk's alone.
 *   5. Without a defect the content is the blocks' outputs back to back, and its length is the result.
 *   6. The decode call only: content above d_dst_cap[f] is ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL, decided from the sizes before a
 *      byte of that frame is written.
 *   7. A frame whose blocks do not all number below max_blocks gets ZLZ4_ERR_INVALID_STATE and nothing is written for it;
 *      earlier frames are unaffected (the frame batch contract above; a frame without blocks needs no entries).
 *
 * WRITING frame f from n source bytes: the magic, then for every chunk of bs bytes (the last one shorter) the u32 LE
 *   compressed size and the block; n == 0 writes the magic alone, as the CLI does.  bs = prefs->block_size: 0 means 8 MiB,
 *   1 .. 8 MiB is taken as given (smaller blocks are still legal legacy frames -- `lz4 -d` and unlz4 take any block that
 *   decodes to 8 MiB or less -- and are what lets one frame use more than a handful of wavefronts), anything larger is
 *   ZLZ4F_ERR_MAX_BLOCK_SIZE_INVALID and nothing is launched.  The block is compressFast(chunk, acceleration 1) for
 *   prefs->compression_level <= 0, else compressHC(chunk, level) with the level read as zlz4_batch_compress_hc reads it
 *   (1 becomes 9, above 12 becomes 12; the HAZARD note of section 1 holds for 10..12).  The format has no stored blocks:
 *   an incompressible chunk grows, up to zlz4_compress_bound(chunk).  A block whose compressor returns an error makes its
 *   frame fail with that code.
 *   zlz4f_legacy_compress_frame_bound(n, prefs) = 4 + the sum over the chunks of 4 + zlz4_compress_bound(chunk length): host
 *   arithmetic; 0 for an invalid block_size.  n > ZLZ4_MAX_INPUT_SIZE: ZLZ4F_ERR_SRC_SIZE_TOO_LARGE; else d_dst_cap[f] below
 *   the bound: ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL; nothing is written for either.  A frame has ceil(n / bs) blocks.
 *   The bytes differ from the CLI's (these are the reference's block algorithms); they decode everywhere.
 *
 * The batch calls keep the contract of zlz4f_batch_compress_frame / zlz4f_batch_decompress_frame: device pointers,
 *   asynchronous on `stream`, a fixed launch sequence, nothing allocated, nothing read back; nframes == 0 returns 0.  A null
 *   array, an array that is not 8-byte aligned, or a workspace that is null, not 16-byte aligned or smaller than its size
 *   function says: ZLZ4_ERR_INVALID_STATE, nothing launched (d_consumed may be null: it is not written then).  The device
 *   check is the last refusal.  No byte outside a frame's slot is ever written; bytes inside a failed frame's slot are
 *   unspecified.
 * zlz4f_batch_legacy_frame_count: the walk alone, no workspace.  d_nblocks[f] = the blocks of frame f's chain, d_consumed[f]
 *   as above, d_totals[0] = the blocks of all frames (the max_blocks of the calls below): one 8-byte read-back sizes them.
 * zlz4f_batch_legacy_frame_decompressed_size: d_size[f] = what the decode call stores in d_result[f] when d_dst_cap[f] is
 *   large enough.  The walk (count, scan, record), the size kernel of zlz4_batch_decompressed_size over the block table,
 *   one wavefront per frame for the fold.
 * zlz4f_batch_decompress_legacy_frame: the same, the fold also places every block inside the frame's slot and empties the
 *   table entries of every frame that fails; then the kernel of zlz4_batch_decompress_safe over the table, and a finish.
 * zlz4f_batch_compress_legacy_frame: descriptors, the kernel of zlz4_batch_compress_fast / zlz4_batch_compress_hc over the
 *   table with max_in_len = bs into compressBound-sized workspace slots, a prefix sum per frame, a scatter of size words
 *   and blocks.  The workspace holds the table, the slots and, for compression_level > 0,
 *   zlz4_batch_compress_hc_workspace(max_blocks, bs) bytes.
 * The three host calls stage one frame and run the batch of one ("correct, not fast"); consumed may be null.  Before the
 *   device check they answer: a null pointer with a length (ZLZ4_ERR_INVALID_STATE), an invalid block_size, then a source
 *   above ZLZ4_MAX_INPUT_SIZE and a dst_cap below the bound (compress); step 1 above, and a defect of the walk in front of
 *   the first block (decode and size query, which walk the host bytes to size the block table).
 *
 * NOT SERVED: dictionaries (the format has none); the segment calls.  Legacy members of a concatenated file: the
 *   multiframe _ex calls above with ZLZ4F_SPLIT_LEGACY.  Prefix and range decoding of a legacy frame: the file index and
 *   range calls below, over the frame as a file of one member. */
#define ZLZ4F_LEGACY_MAGICNUMBER 0x184C2102u
#define ZLZ4F_LEGACY_BLOCK_SIZE  (8u << 20)
#define ZLZ4F_LEGACY_BLOCK_BOUND 8421520u        /* zlz4_compress_bound(ZLZ4F_LEGACY_BLOCK_SIZE) = LZ4_compressBound(8 MiB) */
typedef struct { uint32_t block_size; int32_t compression_level; } zlz4f_legacy_prefs;      /* NULL = { 0, 0 } */
size_t  zlz4f_legacy_compress_frame_bound(size_t src_size, const zlz4f_legacy_prefs *prefs);
size_t  zlz4f_batch_compress_legacy_frame_workspace(uint32_t nframes, uint32_t max_blocks, const zlz4f_legacy_prefs *prefs);
int32_t zlz4f_batch_compress_legacy_frame(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                          const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                          const uint64_t *d_dst_cap, int64_t *d_result, uint32_t nframes, uint32_t max_blocks,
                                          const zlz4f_legacy_prefs *prefs, void *d_workspace, size_t workspace_bytes);
int32_t zlz4f_batch_legacy_frame_count(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                       const uint64_t *d_src_len, uint32_t nframes, uint64_t *d_nblocks, uint64_t *d_consumed,
                                       uint64_t *d_totals);
size_t  zlz4f_batch_legacy_frame_decompressed_size_workspace(uint32_t nframes, uint32_t max_blocks);
int32_t zlz4f_batch_legacy_frame_decompressed_size(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                                   const uint64_t *d_src_len, int64_t *d_size, uint64_t *d_consumed,
                                                   uint32_t nframes, uint32_t max_blocks, void *d_workspace,
                                                   size_t workspace_bytes);
size_t  zlz4f_batch_decompress_legacy_frame_workspace(uint32_t nframes, uint32_t max_blocks);
int32_t zlz4f_batch_decompress_legacy_frame(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                            const uint64_t *d_src_len, uint8_t *d_dst, const uint64_t *d_dst_off,
                                            const uint64_t *d_dst_cap, int64_t *d_result, uint64_t *d_consumed,
                                            uint32_t nframes, uint32_t max_blocks, void *d_workspace, size_t workspace_bytes);
int64_t zlz4f_compress_legacy_frame(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                    const zlz4f_legacy_prefs *prefs);
int64_t zlz4f_legacy_frame_decompressed_size(const uint8_t *src, size_t src_len, size_t *consumed);
int64_t zlz4f_decompress_legacy_frame(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, size_t *consumed);

/* ---- file index and file range decoding: bytes [a, b) of whole .lz4 files (no counterpart in the reference; DESIGN.md
 * section 4.4k).  A FILE is a buffer as the record-mode zlz4f_batch_multiframe_split_ex delimits it: frame, skippable and
 * legacy members in any order.  The frame index and range calls above see one frame; these see every member, so a log that
 * was appended to, `cat a.lz4 legacy.lz4 b.lz4` or an initramfs followed by modern frames can be read at any offset, and a
 * file PREFIX is the range [0, n).
 *
 * zlz4f_batch_file_index.  INPUT: the buffers (d_src, d_src_off, d_src_len, nbuf), the outputs of the record-mode split over
 *   them (d_member, d_mem_off, d_split_result = the split's d_result, d_item_first, d_item_off, d_item_len, d_leg_len) and
 *   split_totals, a HOST pointer to the split's four totals as they were read back.  After a split with split_flags == 0
 *   there is no legacy member (a legacy magic stays ZLZ4F_ERR_FRAME_TYPE_UNKNOWN, as everywhere); split_totals[2] == 0
 *   skips the legacy kernels and d_leg_len may be null.
 *   OUTPUT per buffer s with nb blocks: nb + 1 entries of zlz4f_index_entry at d_index + d_idx_off[s].  Entry k < nb is
 *   block k of the file, counted across its frame and legacy members in member order: pos = the position of the block's
 *   header word (frame) or size word (legacy) INSIDE THE BUFFER, dec = the offset at which the block starts INSIDE THE
 *   FILE'S CONTENT.  Entry nb = { where the chain of the last frame or legacy member ended -- the end mark or the end of
 *   the input for a frame, the member's end for a legacy frame; 0 for a file without such a member --, S = the file's
 *   decoded size }.  Skippable members, frames without blocks and a legacy magic alone contribute no entry.
 *   PACKING: the call writes d_idx_off itself, nbuf + 1 entries: the exclusive scan of every buffer's room, its chain blocks
 *   plus one.  The room is the walks' count alone, so a buffer that fails keeps its room.  The caller sizes d_index from the
 *   split's read-back: idx_cap = split_totals[1] + split_totals[3] + nbuf entries always suffice; a buffer whose room ends
 *   behind idx_cap answers ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL and writes no entry.
 *   d_result[s] = nb, or the code that zlz4f_batch_multiframe_finish gives the file when it folds the two size queries at
 *   decode_flags == 0: a split result < 0, else the first member in member order that is not OK -- a frame member's size
 *   query error (every block sized as an independent block, the content checksum set aside, as zlz4f_batch_frame_index: a
 *   member whose blocks refer to earlier output is ZLZ4F_ERR_DECOMPRESSION_FAILED), a legacy member's, a truncated
 *   skippable member's.  The index capacity is the last check.  On an error no entry of that buffer is promised.  A buffer
 *   of one frame has exactly the entries and the result of zlz4f_batch_frame_index.
 *   Workspace: zlz4f_batch_file_index_workspace(nbuf, split_totals) bytes, 16-byte aligned.  A null array, a misaligned (8
 *   bytes) one, a null split_totals or one with a count above 2^32 - 1, or a refused workspace: ZLZ4_ERR_INVALID_STATE,
 *   nothing launched; then the device.  nbuf == 0 returns 0.  Launches: the frame size query's sequence over the items up
 *   to its fold; with legacy members the legacy walk (count, scan, record) and the size kernel over their blocks; the
 *   rooms, their scan, and the fold -- one wavefront per buffer that walks the members, carries the decoded base and the
 *   block count from member to member and writes the rebased entries, 64 blocks a step.
 *
 * THE PLAN is zlz4f_batch_plan_frame_ranges, unchanged: nframes = nbuf, zlz4f_range.frame names the buffer.
 *
 * zlz4f_batch_decompress_file_range: the arguments of zlz4f_batch_decompress_frame_range (nframes = nbuf) and the member
 *   table, d_mem_off and the split results.  OUTPUT as there: slot r holds the decode from the start of block k0 to b', the
 *   wanted bytes stand d_skip[r] bytes in, d_result[r] = b' - a', no byte outside [d_dst_off[r], d_dst_off[r] + b' - dec[k0])
 *   is written.  A RANGE MAY SPAN MEMBERS: every item (one block of one range) finds its member by bisection over the
 *   buffer's member table by pos and takes from it what the frame call takes from the one header -- for a frame member its
 *   OWN FLG 0x10 (block checksum), the stored bit of the block word and the header's block size as the bound; for a legacy
 *   member no checksum, no stored bit, a bound of 8 MiB and a size word that is neither 0 nor above
 *   ZLZ4F_LEGACY_BLOCK_BOUND.  Two neighbouring blocks of one range may differ in all of these.
 *   THE INDEX IS NOT TRUSTED; no position from it becomes an address before it is checked.  Per range, in this order:
 *   1. ZLZ4_ERR_INVALID_STATE for frame >= nbuf, a > b, reserved != 0.  Then d_idx_n[buf] < 0: that code.
 *   2. a' == b': 0, d_skip[r] = 0; nothing behind the tables (index, member table) is read.
 *   3. ZLZ4_ERR_INVALID_STATE ("not this file's index") when the entries k0..k1+1 are no chain: k0 / k1 not found or k1 <
 *      k0, dec[k0] > a', dec[k1] >= b', dec[k1+1] < b', the buffer has no member table (split result <= 0), or for a k in
 *      k0..k1: no member starts at or in front of pos[k]; that member is neither FRAME nor LEGACY, does not lie inside the
 *      buffer, or its header is none (a frame header error, a word that is not the legacy magic); pos[k] lies in front of
 *      the end of that header or fewer than 4 bytes in front of the member's end; pos[k+1] <= pos[k]; dec[k+1] < dec[k];
 *      dec[k+1] - dec[k] above the member's bound.
 *   4. d_dst_cap[r] < b' - dec[k0]: ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL.  5. max_items, as the frame call.
 *   6. The first failing block in block order decides.  Block k with size sz from its word: ZLZ4_ERR_INVALID_STATE when the
 *      word is an end mark (frame) or 0 or above the bound (legacy); when the block (+ 4 with a block checksum) runs past
 *      its member's end; when pos[k+1] lies inside the member (at or in front of its end) and the block does not end exactly
 *      there; when pos[k+1] lies behind the member and the block is not the member's last -- it ends on the frame member's
 *      end mark, or at the member's end for a chain without one and for a legacy member.  Then the block checksum, the
 *      stored block, zlz4_batch_decompress_safe for a block wanted in full and zlz4_batch_decompress_safe_prefix for the one
 *      that b' cuts, with the codes of the frame call.
 *   Nothing outside the touched blocks and their members' headers is read or validated; content checksums are never
 *   checked.  Workspace: zlz4f_batch_decompress_file_range_workspace(nranges, max_items).  Refusals as the frame call,
 *   with the three member arrays among the arrays.  The frame range kernels' scan, checksum, copy and finish are reused;
 *   the frame calls themselves are unchanged.
 * Both calls: asynchronous on `stream`, a fixed launch sequence (it depends on split_totals alone), nothing allocated,
 *   nothing read back: graph-capturable.  The index stays valid for every later read of the same bytes.
 *
 * zlz4f_decompress_file_range: one file in HOST memory; exactly the b' - a' wanted bytes arrive at dst[0..).  Before the
 *   device check: an unknown split_flags bit (ZLZ4F_ERR_PARAMETER_INVALID), then a null pointer with a length and a > b
 *   (ZLZ4_ERR_INVALID_STATE).  Then split (count, record), index, plan and range as a batch of one.  An index error is the
 *   result; dst_cap < b' - a' gives ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL in front of the decode.  IT BUILDS THE INDEX ON EVERY
 *   CALL (a size query of the whole file): a caller with several reads of one file keeps the index and uses the batch calls.
 *
 * NOT SERVED: a dictionary per MEMBER chosen by dictID (a dictionary per FILE: the _using_dict forms below); history-aware
 *   ranges of linked members; a start offset inside one block.  (A serialised index: the seek table, below.) */
size_t  zlz4f_batch_file_index_workspace(uint32_t nbuf, const uint64_t *split_totals);
int32_t zlz4f_batch_file_index(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                               uint32_t nbuf, const zlz4f_member *d_member, const uint64_t *d_mem_off,
                               const int64_t *d_split_result, const uint64_t *d_item_first, const uint64_t *d_item_off,
                               const uint64_t *d_item_len, const uint64_t *d_leg_len, const uint64_t *split_totals,
                               zlz4f_index_entry *d_index, uint64_t *d_idx_off, uint64_t idx_cap, int64_t *d_result,
                               void *d_workspace, size_t workspace_bytes);
size_t  zlz4f_batch_decompress_file_range_workspace(uint32_t nranges, uint32_t max_items);
int32_t zlz4f_batch_decompress_file_range(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                          const uint64_t *d_src_len, const zlz4f_index_entry *d_index,
                                          const uint64_t *d_idx_off, const int64_t *d_idx_n, uint32_t nbuf,
                                          const zlz4f_member *d_member, const uint64_t *d_mem_off,
                                          const int64_t *d_split_result, const zlz4f_range *d_range, uint8_t *d_dst,
                                          const uint64_t *d_dst_off, const uint64_t *d_dst_cap, uint64_t *d_skip,
                                          int64_t *d_result, uint32_t nranges, uint32_t max_items, void *d_workspace,
                                          size_t workspace_bytes);
int64_t zlz4f_decompress_file_range(const uint8_t *src, size_t src_len, uint64_t a, uint64_t b, uint8_t *dst,
                                    size_t dst_cap, uint32_t split_flags);

/* ---- seekable .lz4 files: a stored seek table, and a writer for such files (no counterpart in the reference; DESIGN.md
 * section 4.4l).  The file index above is a size query of the whole file and the split in front of it a serial walk; both
 * were computed by whoever wrote the file.  A SEEK TABLE stores them: it is one skippable frame, always the LAST MEMBER of
 * its file, that holds the file's member rows and index entries.  Every lz4 decoder steps over it, the calls above
 * included: to them it is a skippable member with nibble 0xC, and they answer for a file with a table exactly what they
 * answer for any file.  (This closes "a serialised index" and "writing such files" of the NOT SERVED list above.)
 *
 * THE FORMAT, little-endian throughout.  A table over nm member rows and nb index blocks is T = 40 + 24*nm + 16*(nb + 1)
 * bytes:
 *   0          u32  0x184D2A5C                      ZLZ4F_SEEK_TABLE_MAGICNUMBER (a skippable magic, nibble 0xC)
 *   4          u32  P = T - 8                       the skippable frame's payload size
 *   8          nm     x { u64 pos, u64 len, u32 kind, u32 0 }   the members of the file in order, THIS ONE INCLUDED as the
 *                                                   last row; kind as the record-mode split writes it: ZLZ4F_MEMBER_* |
 *                                                   nibble << 8, so the last row's is ZLZ4F_MEMBER_SKIPPABLE | 0xC << 8
 *   8 + 24*nm  nb + 1 x { u64 pos, u64 dec }        the entries of zlz4f_batch_file_index for the file
 *   T - 32     u64 nm, u64 nb, u64 file_len (the file's length with this member), u32 version = 1, u32 0x4B53345A ("Z4SK")
 *   The footer is the end of the file, so a reader finds the table from the tail.  The rows are zlz4f_member (buf is 0 in
 *   the file) and zlz4f_index_entry as they stand in memory.  The table lists itself and its entries are those of the file
 *   WITH the table: for a file G that ends in its table, the loaded tables equal, row for row, what the record-mode
 *   zlz4f_batch_multiframe_split_ex and zlz4f_batch_file_index compute for G.  No checksum covers the table; it is not
 *   trusted (below).
 * zlz4f_seek_table_bound(nmembers, nblocks) = T for nmembers + 1 member rows (the file's members and the table's own row)
 *   and nblocks + 1 entries; 0 when P does not fit 32 bits.
 *
 * zlz4f_batch_append_seek_table, the writer of the table.  INPUT: the buffers with room behind each one (buffer s is
 *   d_buf_len[s] = n bytes at d_buf + d_buf_off[s], of a region of d_buf_cap[s] bytes from there), the record-mode split
 *   over them (d_member, d_mem_off, d_split_result) and their file index (d_index, d_idx_off, d_idx_n).  OUTPUT: the table
 *   at [n, n + T) of buffer s and d_result[s] = n + T.  Refusals per file, in this order, nothing written on any of them:
 *   1. a split result < 0: that code.  2. d_idx_n[s] < 0: that code.  3. ZLZ4_ERR_INVALID_STATE when the last member is a
 *   frame member whose chain lacks its end mark (entry[nb].pos + 4 > that member's end): appended bytes would be read as its
 *   next block word.  4. ZLZ4_ERR_UNSUPPORTED when P does not fit 32 bits.  5. ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL when n + T >
 *   d_buf_cap[s].  Bytes [0, n) are never touched, read or written, and no byte at or behind n + T is written.  A file that
 *   already ends in a table gets a second one that lists the first as an ordinary member; the loader uses the last.  One
 *   launch: the table is T / 8 64-bit fields that depend on their number alone, spread over lanes and, 256 at a time,
 *   over the workgroups a file has; a table at an odd address is written as aligned words with its head and tail bytes
 *   stored singly.
 *
 * zlz4f_batch_load_seek_table, the reader.  COUNT MODE (d_member == NULL): one lane per file reads the footer and the 8
 *   bytes at n - T; d_count[s] = nm, or 0 for a file without a well-formed footer; d_totals = { the sum of nm, the sum of
 *   the rooms }, a file's room being nb + 1, or 0 without such a footer: one 16-byte read-back sizes d_member and d_index.
 *   RECORD MODE writes the member rows to d_member[d_mem_off[s] ..] with buf = s; d_idx_off itself, nbuf + 1 entries, the
 *   exclusive scan of the rooms; the entries to d_index + d_idx_off[s]; d_split_result[s] = nm, or 0 (no table: n < 80 or
 *   the tail magic is absent), or ZLZ4_ERR_INVALID_STATE (the tail magic is there and the table is MALFORMED), or
 *   ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL (nm > d_mem_cap[s], or the room ends behind idx_cap; no row of that file is written);
 *   d_idx_n[s] = nb when the split result is positive, else the negative split result, else ZLZ4_ERR_INVALID_STATE.  These
 *   outputs are, unchanged, what zlz4f_batch_plan_frame_ranges and zlz4f_batch_decompress_file_range take.
 *   MALFORMED: the footer's version != 1, T overflows or exceeds n, file_len != n, nm == 0, the word at n - T is not the
 *   magic or the next one not P; a member row with pos[0] != 0, len == 0, pos[k] + len[k] != pos[k+1] (checked with
 *   overflow), a last row that is not { n - T, T, ZLZ4F_MEMBER_SKIPPABLE | 0xC << 8 }, another row whose kind & 0xFF is not
 *   FRAME, SKIPPABLE or LEGACY or that has bits outside 0xFFF, a reserved word that is set; an entry with pos > n - T, or
 *   for k < nb pos[k+1] <= pos[k] or dec[k+1] < dec[k].  The rows of a malformed table are not promised.
 *   THE LOADER CHECKS SHAPE ONLY; the range call stays the judge.  zlz4f_batch_decompress_file_range treats index and
 *   member table as the caller's data and checks every position against the file before it becomes an address, so a
 *   well-shaped table of ANOTHER file loads fine and is then refused (ZLZ4_ERR_INVALID_STATE) or answered correctly by
 *   the range call, never with wrong bytes.
 *   Launches: the footers (one lane per file), the scan of the rooms, the verdicts (one lane per file), the rows -- one
 *   row per lane, 256 rows a slice, the slices of a file over the workgroups it has; each row is compared with its
 *   neighbour and a slice that finds one out of shape lowers the file's verdict with one atomic.
 *
 * zlz4f_batch_concat, what a device-side file writer lacked: file s is its items d_item_first[s] .. d_item_first[s+1],
 *   item i is d_item_len[i] bytes (int64: the compress call's d_result) at d_src + d_item_off[i]; the items are laid back
 *   to back at d_dst + d_dst_off[s] and d_result[s] is the total -- or the first negative item length in item order, or
 *   ZLZ4F_ERR_DST_MAX_SIZE_TOO_SMALL against d_dst_cap[s]; nothing of that file is written then.  Source and destination do
 *   not overlap.  Workspace: zlz4f_batch_concat_workspace(nitems) bytes, 8-byte aligned (every item's place).  One
 *   wavefront per file places the items, 64 a step; one workgroup per item copies.
 * All three: asynchronous on `stream`, a fixed launch sequence, nothing allocated, nothing read back.  A null or 8-byte
 *   misaligned array: ZLZ4_ERR_INVALID_STATE, nothing launched; then the device.  nbuf == 0 returns 0.
 *
 * zlz4f_seek_table: one file in HOST memory; only the table member is written, to dst[0..T), and T returned -- the caller
 *   appends it to the file.  Split (count, record), index and append as a batch of one; a refusal of the append is the
 *   result.  zlz4f_decompress_file_range_ex: zlz4f_decompress_file_range with range_flags.  0: exactly that call.
 *   ZLZ4F_RANGE_SEEK_TABLE: the tables are loaded when the file ends in a well-formed seek table, and the index is built as
 *   before when it does not.  Both refuse, before the device check, an unknown flag bit (ZLZ4F_ERR_PARAMETER_INVALID),
 *   then a null pointer with a length, and a > b (ZLZ4_ERR_INVALID_STATE).
 *
 * NOT SERVED: a dictionary per MEMBER chosen by dictID and zlz4f_seek_table with a dictionary (the table does not name a
 *   dictionary; zlz4f_batch_append_seek_table takes the index of zlz4f_batch_file_index_using_dict as it takes any, and
 *   the reader passes the dictionary again); linked members with history; a table anywhere but at the file's end; any foreign
 *   seekable format; a checksum over the table; partial staging in the host call -- zlz4f_decompress_file_range_ex still
 *   copies the WHOLE file to the device, where the tail and the touched blocks would do. */
#define ZLZ4F_SEEK_TABLE_MAGICNUMBER  0x184D2A5Cu
#define ZLZ4F_SEEK_TABLE_FOOTER_MAGIC 0x4B53345Au
#define ZLZ4F_SEEK_TABLE_VERSION      1u
#define ZLZ4F_RANGE_SEEK_TABLE        1u     /* range_flags: take the tables from the file's seek table */
size_t  zlz4f_seek_table_bound(uint64_t nmembers, uint64_t nblocks);
int32_t zlz4f_batch_append_seek_table(void *stream, uint8_t *d_buf, const uint64_t *d_buf_off, const uint64_t *d_buf_len,
                                      const uint64_t *d_buf_cap, uint32_t nbuf, const zlz4f_member *d_member,
                                      const uint64_t *d_mem_off, const int64_t *d_split_result,
                                      const zlz4f_index_entry *d_index, const uint64_t *d_idx_off, const int64_t *d_idx_n,
                                      int64_t *d_result);
int32_t zlz4f_batch_load_seek_table(void *stream, const uint8_t *d_src, const uint64_t *d_src_off, const uint64_t *d_src_len,
                                    uint32_t nbuf, uint64_t *d_count, uint64_t *d_totals, zlz4f_member *d_member,
                                    const uint64_t *d_mem_off, const uint64_t *d_mem_cap, int64_t *d_split_result,
                                    zlz4f_index_entry *d_index, uint64_t *d_idx_off, uint64_t idx_cap, int64_t *d_idx_n);
size_t  zlz4f_batch_concat_workspace(uint32_t nitems);
int32_t zlz4f_batch_concat(void *stream, const uint8_t *d_src, const uint64_t *d_item_off, const int64_t *d_item_len,
                           const uint64_t *d_item_first, uint32_t nbuf, uint32_t nitems, uint8_t *d_dst,
                           const uint64_t *d_dst_off, const uint64_t *d_dst_cap, int64_t *d_result, void *d_workspace,
                           size_t workspace_bytes);
int64_t zlz4f_seek_table(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, uint32_t split_flags);
int64_t zlz4f_decompress_file_range_ex(const uint8_t *src, size_t src_len, uint64_t a, uint64_t b, uint8_t *dst,
                                       size_t dst_cap, uint32_t split_flags, uint32_t range_flags);

/* ---- dictionary .lz4 files: the file calls with ONE DICTIONARY PER FILE (no counterpart in the reference; DESIGN.md
 * section 4.4m): what `lz4 -D dict` writes, and what zlz4f_batch_compress_frame_using_dict writes into a file.
 * THE RULE.  File s uses dictionary d = d_dict_idx[s]; a NULL d_dict_idx means dictionary 0 for every file (the caller picks
 *   the dictionary, as `lz4 -d -D dict file` does; the header's dictID stays informational).  T is the last D =
 *   min(d_dict_len[d], 65536) bytes of the dictionary.  A legacy member's blocks never see T.  Every block of a frame member
 *   whose FLG declares independent blocks (0x20) sees T.  Of a member that declares linked blocks, block 0 alone sees T --
 *   the block whose word stands at the end of the member's header; its history is T alone -- and its blocks k >= 1 are
 *   sized and decoded as independent blocks without a dictionary, exactly as the plain file calls do: one that refers to
 *   earlier output or to T is ZLZ4F_ERR_DECOMPRESSION_FAILED in the index.  With D == 0 for every file each call answers
 *   what its plain counterpart answers: bytes, statuses, index entries, d_skip.
 * Dictionary arguments as in the dictionary frame calls, except that d_dict_idx has nbuf entries.  Dictionaries are
 *   read-only and overlap no slot.  Workspace, alignment, null and refusal rules are the plain counterparts', with the
 *   dictionary arrays among the arrays (d_dict_off 8-aligned, d_dict_len and d_dict_idx 4-aligned; with ndicts != 0
 *   d_dict_len and, for the range call, d_dict_off not null); d_dict may be NULL only when every length is 0.
 *   Asynchronous, a fixed launch sequence, nothing allocated, nothing read back.
 * zlz4f_batch_file_index_using_dict: zlz4f_batch_file_index whose size pass gets a dictionary length per table entry, D
 *   where the block sees T, else 0; no dictionary byte is read; the legacy family is unchanged.  d_dict_idx[s] >= ndicts
 *   gives file s ZLZ4_ERR_INVALID_STATE in front of every other status of the file, the split's included; its room is
 *   kept and the other files are unaffected.  Launches: the plain call's and two small kernels.
 * zlz4f_batch_decompress_file_range_using_dict: zlz4f_batch_decompress_file_range where step 1 also refuses a range whose
 *   file has d_dict_idx >= ndicts (ZLZ4_ERR_INVALID_STATE) and every item gets a dictionary descriptor, { d_dict_off[d] +
 *   d_dict_len[d] - D, D } where its block sees T, else length 0.  A block wanted in full goes through the decoder of
 *   zlz4_batch_decompress_safe_using_dict, the one that b' cuts through the prefix decoder with a dictionary; everything
 *   else is unchanged.  INDEX, MEMBER TABLE AND DICTIONARY ARE THE CALLER'S DATA: a dictionary of another LENGTH than the
 *   index was built with is answered per block by the decoder, right bytes or ZLZ4F_ERR_DECOMPRESSION_FAILED; other
 *   CONTENT of the same length gives other bytes, as with liblz4.
 * zlz4f_batch_multiframe_item_dicts: d_item_dict_idx[i] = d_dict_idx[s] for item i of buffer s (0 for a NULL index),
 *   unchanged, so an out-of-range value gets the frame call's own refusal: what zlz4f_batch_decompress_frame_using_dict
 *   and the _size_using_dict call take over the items of a split.  d_item_first: the split's, nbuf + 1 entries.  One
 *   launch, one lane per item.  nbuf == 0 or nitems == 0 returns 0; a null or misaligned array: ZLZ4_ERR_INVALID_STATE.
 * zlz4f_decompress_file_range_using_dict: zlz4f_decompress_file_range_ex with a dictionary, one file in HOST memory; the
 *   dictionary's last 64 KiB alone are staged.  dict == NULL with dict_len > 0 is ZLZ4_ERR_INVALID_STATE among the other
 *   null checks; dict_len == 0 is exactly the _ex call.
 * NOT SERVED: a dictionary per MEMBER chosen by dictID; linked members with history; the frame range calls with a
 *   dictionary; zlz4f_seek_table with a dictionary (the table does not name one); partial staging in the host call. */
size_t  zlz4f_batch_file_index_using_dict_workspace(uint32_t nbuf, const uint64_t *split_totals);
int32_t zlz4f_batch_file_index_using_dict(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                          const uint64_t *d_src_len, uint32_t nbuf, const zlz4f_member *d_member,
                                          const uint64_t *d_mem_off, const int64_t *d_split_result,
                                          const uint64_t *d_item_first, const uint64_t *d_item_off, const uint64_t *d_item_len,
                                          const uint64_t *d_leg_len, const uint64_t *split_totals, zlz4f_index_entry *d_index,
                                          uint64_t *d_idx_off, uint64_t idx_cap, int64_t *d_result, const uint32_t *d_dict_len,
                                          uint32_t ndicts, const uint32_t *d_dict_idx, void *d_workspace,
                                          size_t workspace_bytes);
size_t  zlz4f_batch_decompress_file_range_using_dict_workspace(uint32_t nranges, uint32_t max_items);
int32_t zlz4f_batch_decompress_file_range_using_dict(void *stream, const uint8_t *d_src, const uint64_t *d_src_off,
                                                     const uint64_t *d_src_len, const zlz4f_index_entry *d_index,
                                                     const uint64_t *d_idx_off, const int64_t *d_idx_n, uint32_t nbuf,
                                                     const zlz4f_member *d_member, const uint64_t *d_mem_off,
                                                     const int64_t *d_split_result, const zlz4f_range *d_range, uint8_t *d_dst,
                                                     const uint64_t *d_dst_off, const uint64_t *d_dst_cap, uint64_t *d_skip,
                                                     int64_t *d_result, uint32_t nranges, uint32_t max_items,
                                                     const uint8_t *d_dict, const uint64_t *d_dict_off,
                                                     const uint32_t *d_dict_len, uint32_t ndicts, const uint32_t *d_dict_idx,
                                                     void *d_workspace, size_t workspace_bytes);
int32_t zlz4f_batch_multiframe_item_dicts(void *stream, const uint64_t *d_item_first, uint32_t nbuf, uint32_t nitems,
                                          const uint32_t *d_dict_idx, uint32_t *d_item_dict_idx);
int64_t zlz4f_decompress_file_range_using_dict(const uint8_t *src, size_t src_len, uint64_t a, uint64_t b, uint8_t *dst,
                                               size_t dst_cap, uint32_t split_flags, uint32_t range_flags,
                                               const uint8_t *dict, size_t dict_len);

/* ======================================================================
 * 4. Introspection
 * ====================================================================== */
/* 0 if a gfx950 device is usable by this process, else ZLZ4_ERR_DEVICE */
int32_t     zlz4_device_check(void);
const char *zlz4_version_string(void);
/* human-readable name of a ZLZ4_ERR_* / ZLZ4F_ERR_* code (mirrors the Zig error names) */
const char *zlz4_error_name(int64_t code);
/* The frame calls park their device scratch buffers (block slots, descriptors) in a small per-process cache instead of
 * hipFree-ing them; this gives that memory back.  (No counterpart in the reference, which allocates nothing.) */
void        zlz4_release_device_cache(void);

#ifdef __cplusplus
}
#endif
#endif /* ZLZ4_AMD_H */
