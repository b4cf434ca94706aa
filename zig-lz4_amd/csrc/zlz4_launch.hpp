// zlz4_launch.hpp -- the internal launchers: every extern "C" function that one .hip file defines, another calls and
// include/zlz4_amd.h does not declare.  The only place they are declared: each defining file includes this header, so
// the compiler holds the definition against the declaration, and so does each calling file.  All pointers are device
// pointers; the per-block arrays are those of the batch calls of include/zlz4_amd.h.  A launcher returns 0 or a
// ZLZ4_ERR_* code and enqueues on `stream` without synchronising.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/zlz4_amd.h"

// how a launcher ends: 0, or ZLZ4_ERR_DEVICE when the launch (or an earlier asynchronous call) failed
inline int zlz4_launch_status() { return hipGetLastError() == hipSuccess ? 0 : ZLZ4_ERR_DEVICE; }

// workgroups of `threads` items that cover `items` (at least one, at most `cap`)
inline uint32_t grid_of(uint64_t items, uint32_t threads, uint32_t cap = 0xFFFFFFFFu) {
    const uint64_t g = (items + threads - 1) / threads;
    return g == 0 ? 1u : (g > cap ? cap : (uint32_t)g);
}

extern "C" {

// zlz4_compress_fast.hip
int zlz4_launch_compress_fast(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                              uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap, int64_t *d_result,
                              uint32_t nblocks, uint32_t max_in_len, uint32_t acceleration);
int zlz4_launch_compress_fast_continue(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                       const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                       const uint32_t *d_out_cap, const uint32_t *d_table_in, const uint32_t *d_table_idx,
                                       uint32_t *d_table_out, int64_t *d_result, uint32_t nblocks, uint32_t max_in_len,
                                       uint32_t acceleration);
int zlz4_launch_load_dict(hipStream_t stream, const uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_len,
                          uint32_t *d_tables, int64_t *d_result, uint32_t ndicts);

// zlz4_compress_dict.hip
int zlz4_launch_compress_fast_using_dict(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                         const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                         const uint32_t *d_out_cap, const uint8_t *d_dict, const uint64_t *d_dict_off,
                                         const uint32_t *d_dict_len, const uint32_t *d_table, const uint32_t *d_table_idx,
                                         int64_t *d_result, uint32_t nblocks, uint32_t max_in_len, uint32_t max_dict_len,
                                         uint32_t acceleration);

// zlz4_compress_hc.hip
size_t zlz4_hc_workspace_bytes(uint32_t nblocks, uint32_t max_in_len);
int zlz4_launch_compress_hc(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                            uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap, int64_t *d_result,
                            uint32_t nblocks, uint32_t max_in_len, int32_t level, void *ws, size_t ws_bytes);
size_t zlz4_hc_dict_workspace_bytes(uint32_t nblocks, uint32_t max_in_len, uint32_t max_dict_len);
int zlz4_launch_compress_hc_dict(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                 uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap, const uint8_t *d_dict,
                                 const uint64_t *d_dict_off, const uint32_t *d_dict_len, int64_t *d_result, uint32_t nblocks,
                                 uint32_t max_in_len, uint32_t max_dict_len, int32_t level, void *ws, size_t ws_bytes);
size_t zlz4_hc_linked_workspace_bytes(uint32_t nblocks, uint32_t max_block_len);
int zlz4_launch_compress_hc_linked(hipStream_t stream, const uint8_t *d_in, const uint64_t *v_off, const uint32_t *v_len,
                                   const uint32_t *v_pair, uint8_t *d_out, const uint64_t *d_out_off,
                                   const uint32_t *d_out_cap, int64_t *d_result, uint32_t nblocks, uint32_t max_block_len,
                                   int32_t level, void *ws, size_t ws_bytes);

// zlz4_compress_hc_dict.hip (called by zlz4_launch_compress_hc_dict)
int zlz4_launch_hc_dict_stage(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                              const uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_len, uint8_t *d_v,
                              uint64_t v_stride, uint64_t *v_off, uint32_t *v_len, uint32_t *v_pair, uint32_t blk0,
                              uint32_t nblocks, uint32_t slot0, uint32_t max_in_len, uint32_t dmax);

// zlz4_compress_hc_serial.hip (levels 2 and 10..12; called by zlz4_launch_compress_hc)
size_t zlz4_hc_mid_workspace_bytes(uint32_t chunk_blocks);
size_t zlz4_hc_opt_workspace_bytes(uint32_t chunk_blocks);
int zlz4_launch_hc_mid(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                       uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap, int64_t *d_result,
                       uint32_t nblocks, void *ws, uint32_t chunk, uint32_t max_in_len);
int zlz4_launch_hc_opt_parse(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                             uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap, int64_t *d_result,
                             const void *d_res, uint64_t res_stride, int wide, void *d_opt, uint32_t b0, uint32_t nb,
                             uint32_t sufficient_len, uint32_t max_in_len);

// zlz4_dest_size.hip
size_t zlz4_dest_size_workspace_bytes(uint32_t nblocks, uint32_t max_in_len);
uint32_t zlz4_dest_size_slot_cap(uint32_t max_in_len);
int zlz4_launch_compress_dest_size(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                   const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                   const uint32_t *d_out_cap, int64_t *d_result, uint32_t *d_consumed, uint32_t nblocks,
                                   uint32_t max_in_len, void *d_workspace, const uint64_t *d_slot_off,
                                   const uint32_t *d_slot_cap);

// zlz4_decompress.hip
int zlz4_launch_decompress_safe(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap, int64_t *d_result,
                                uint32_t nblocks);
int zlz4_launch_decompress_safe_using_dict(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                           const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                           const uint32_t *d_out_cap, int64_t *d_result, uint32_t nblocks,
                                           const uint8_t *d_dict, const uint64_t *d_dict_off, const uint32_t *d_dict_len);
int zlz4_launch_decompress_safe_bound(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                      const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                      const uint32_t *d_out_cap, int64_t *d_result, uint32_t nblocks, const uint8_t *d_dict,
                                      const uint64_t *d_dict_off, const uint32_t *d_dict_len, int with_dict);
// prefix decoding (k_decompress_safe, kPartial): d_out_cap[i] = bytes wanted of block i = size of its slot
int zlz4_launch_decompress_safe_prefix(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                       const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                       const uint32_t *d_out_cap, int64_t *d_result, uint32_t nblocks);
int zlz4_launch_decompress_safe_prefix_using_dict(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                                  const uint32_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                                  const uint32_t *d_out_cap, int64_t *d_result, uint32_t nblocks,
                                                  const uint8_t *d_dict, const uint64_t *d_dict_off,
                                                  const uint32_t *d_dict_len);
int zlz4_launch_decompress_sizes(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                 const uint64_t *d_out_off, const uint32_t *d_out_cap, int64_t *d_result, uint32_t nblocks);

// the size pass with a dictionary per block: only d_dict_len decides (a match may reach min(d_dict_len[i], 65536) bytes in
// front of the block); no dictionary byte is read.  d_dict_off must be a readable array of nblocks entries.
int zlz4_launch_decompress_sizes_using_dict(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                            const uint32_t *d_in_len, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                            int64_t *d_result, uint32_t nblocks, const uint64_t *d_dict_off,
                                            const uint32_t *d_dict_len);

// zlz4_stream_decode.hip
size_t zlz4_sd_workspace_bytes(uint32_t nblocks, uint32_t nstreams);
int zlz4_launch_stream_decode(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                              uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                              const uint32_t *d_run_start, uint64_t *d_state, int64_t *d_result, uint32_t nblocks,
                              uint32_t nstreams, void *d_workspace);

// zlz4_sizes.hip
int zlz4_launch_decompressed_size(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                  const uint32_t *d_dict_len, int64_t *d_size, uint32_t nblocks);
int zlz4_launch_plan_outputs(hipStream_t stream, const int64_t *d_size, uint32_t n, uint32_t align, uint64_t *d_out_off,
                             uint32_t *d_out_cap, uint64_t *d_total);

// zlz4_frame_linked.hip; `frames` is the BFrame array of zlz4_frame_batch.hpp
int zlz4_launch_bfl_save(hipStream_t st, const void *frames, uint32_t nframes, int64_t *walk_err);
int zlz4_launch_bfl_mask(hipStream_t st, const void *frames, const uint32_t *fidx, uint32_t max_blocks, uint32_t *cap,
                         uint32_t *len);
int zlz4_launch_bfl_decode(hipStream_t st, int write, void *frames, uint32_t nframes, uint32_t max_blocks, const uint8_t *src,
                           const uint64_t *data_off, const uint32_t *data_len, const uint32_t *flags, const uint32_t *cks_ok,
                           const int64_t *walk_err, uint8_t *dst, const uint64_t *dst_off, const uint64_t *dst_cap,
                           const uint64_t *src_len, int64_t *d_size);
int zlz4_launch_bfl_decode_dict(hipStream_t st, int write, void *frames, uint32_t nframes, uint32_t max_blocks,
                                const uint8_t *src, const uint64_t *data_off, const uint32_t *data_len, const uint32_t *flags,
                                const uint32_t *cks_ok, const int64_t *walk_err, uint8_t *dst, const uint64_t *dst_off,
                                const uint64_t *dst_cap, const uint64_t *src_len, int64_t *d_size, const uint8_t *dict,
                                const uint64_t *fd_end, const uint32_t *fd_len);
// frame prefix decoding (k_bfp_decode): one launch, no workspace; dst_cap[f] = bytes wanted of frame
// f = size of its slot.  The plain call is the dictionary call with ndicts == 0 (no dictionary argument is read then).
int zlz4_launch_bfp_decode(hipStream_t st, const uint8_t *src, const uint64_t *src_off, const uint64_t *src_len, uint8_t *dst,
                           const uint64_t *dst_off, const uint64_t *dst_cap, int64_t *result, uint32_t nframes);
int zlz4_launch_bfp_decode_dict(hipStream_t st, const uint8_t *src, const uint64_t *src_off, const uint64_t *src_len,
                                uint8_t *dst, const uint64_t *dst_off, const uint64_t *dst_cap, int64_t *result,
                                uint32_t nframes, const uint8_t *dict, const uint64_t *dict_off, const uint32_t *dict_len,
                                uint32_t ndicts, const uint32_t *dict_idx);
// dictionary frames: per-frame and per-entry dictionary descriptors of the decode, the
// preconditions, descriptors and result merge of the compress call
int zlz4_launch_bfdd_frame(hipStream_t st, void *frames, uint32_t nframes, const uint64_t *dict_off, const uint32_t *dict_len,
                           uint32_t ndicts, const uint32_t *dict_idx, uint64_t *fd_end, uint32_t *fd_len);
int zlz4_launch_bfdd_entry(hipStream_t st, const void *frames, const uint32_t *fidx, uint32_t max_blocks,
                           const uint64_t *fd_end, const uint32_t *fd_len, uint64_t *e_off, uint32_t *e_len);
int zlz4_launch_bfdd_mask(hipStream_t st, const void *frames, const uint32_t *fidx, uint32_t max_blocks, uint32_t *cap,
                          uint32_t *len);
int zlz4_launch_bfcd_pre(hipStream_t st, void *frames, uint32_t nframes, const uint64_t *src_len, const uint32_t *dict_len,
                         uint32_t ndicts, const uint32_t *dict_idx, uint64_t max_src_len, uint32_t max_dict_len);
int zlz4_launch_bfcd_desc(hipStream_t st, const void *frames, uint32_t nframes, uint32_t max_blocks, int with_b,
                          const uint64_t *dict_off, const uint32_t *dict_len, const uint32_t *dict_idx, const uint32_t *in_len,
                          uint32_t *len_a, uint32_t *len_b, uint64_t *a_off, uint32_t *a_len, uint32_t *a_tix);
int zlz4_launch_bfcd_merge(hipStream_t st, const uint32_t *len_b, const int64_t *csize_b, int64_t *csize,
                           uint32_t max_blocks);
int zlz4_launch_bfl_dict_desc(hipStream_t st, const void *frames, uint32_t nframes, uint32_t max_blocks,
                              const uint64_t *src_off, const uint64_t *in_off, const uint32_t *in_len, uint64_t *dict_off,
                              uint32_t *dict_len);
int zlz4_launch_bfl_hc_desc(hipStream_t st, const void *frames, uint32_t nframes, uint32_t max_blocks, const uint64_t *src_off,
                            const uint64_t *in_off, const uint32_t *in_len, uint64_t *v_off, uint32_t *v_len,
                            uint32_t *v_pair);

// zlz4_frame.hip, for zlz4_frame_seek.hip: zlz4f_decompress_file_range with the D > 0 last bytes of a dictionary (host memory)
int64_t zlz4_host_file_range_dict(const uint8_t *src, size_t n, uint64_t a, uint64_t b, uint8_t *dst, size_t cap,
                                  uint32_t split_flags, const uint8_t *tail, uint32_t D);

}  // extern "C"
