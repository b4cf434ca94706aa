//! Drop-in replacement for jedisct1/zig-lz4's `src/root.zig` (reference src/root.zig:1-57):
//! same `pub` names, same slices-in / error-union-out signatures, but every hot-path call is
//! forwarded to the MI355X library `libzlz4_amd.so` through its C ABI (include/zlz4_amd.h).
//! Host code stays pure Zig; link with `-lzlz4_amd` (see INTEGRATION.md).
//!
//! NOTE: this file could not be compiled in the build container (no zig toolchain); it is the
//! binding a maintainer adds, kept deliberately mechanical.

const std = @import("std");

// ---- C ABI (include/zlz4_amd.h) ----
extern "c" fn zlz4_compress_bound(input_size: usize) usize;
extern "c" fn zlz4_compress_default(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize) i64;
extern "c" fn zlz4_compress_fast(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, acceleration: u32) i64;
extern "c" fn zlz4_compress_hc(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, level: i32) i64;
extern "c" fn zlz4_decompress_safe(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize) i64;
extern "c" fn zlz4_decompress_safe_partial(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, target: usize) i64;
extern "c" fn zlz4_decompress_safe_using_dict(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, dict: ?[*]const u8, dict_len: usize) i64;
extern "c" fn zlz4_decompress_safe_partial_using_dict(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, target: usize, dict: ?[*]const u8, dict_len: usize) i64;
extern "c" fn zlz4_stream_load_dict(table: *[LZ4_HASH_SIZE_U32]u32, dict: ?[*]const u8, dict_len: usize) i64;
extern "c" fn zlz4_stream_compress_fast_continue(table: *[LZ4_HASH_SIZE_U32]u32, src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, acceleration: u32) i64;
extern "c" fn zlz4_compress_fast_using_dict(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, dict: ?[*]const u8, dict_len: usize, acceleration: u32) i64;
extern "c" fn zlz4_sizeof_state() usize;
extern "c" fn zlz4_compress_fast_ext_state(state: [*]u8, state_len: usize, src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, acceleration: u32) i64;
extern "c" fn zlz4_compress_dest_size(src: [*]const u8, dst: [*]u8, dst_cap: usize, src_size: *usize) i64;
extern "c" fn zlz4_sizeof_state_hc() usize;
extern "c" fn zlz4_compress_hc_ext_state(state: [*]u8, state_len: usize, src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, level: i32) i64;

// the data-parallel hot path: device pointers, one wavefront (HC: one workgroup) per block, results per block
extern "c" fn zlz4_batch_compress_fast(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_out: [*]u8, d_out_off: [*]const u64, d_out_cap: [*]const u32, d_result: [*]i64, nblocks: u32, max_in_len: u32, acceleration: u32) i32;
extern "c" fn zlz4_decompress_safe_prefix(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize) i64;
extern "c" fn zlz4_decompress_safe_prefix_using_dict(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, dict: ?[*]const u8, dict_len: usize) i64;
extern "c" fn zlz4_batch_decompress_safe_prefix(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_out: [*]u8, d_out_off: [*]const u64, d_out_cap: [*]const u32, d_result: [*]i64, nblocks: u32) i32;
extern "c" fn zlz4_batch_decompress_safe_prefix_using_dict(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_out: [*]u8, d_out_off: [*]const u64, d_out_cap: [*]const u32, d_dict: ?[*]const u8, d_dict_off: [*]const u64, d_dict_len: [*]const u32, d_result: [*]i64, nblocks: u32) i32;
extern "c" fn zlz4_batch_decompress_safe(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_out: [*]u8, d_out_off: [*]const u64, d_out_cap: [*]const u32, d_result: [*]i64, nblocks: u32) i32;
extern "c" fn zlz4_batch_decompress_safe_using_dict(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_out: [*]u8, d_out_off: [*]const u64, d_out_cap: [*]const u32, d_dict: [*]const u8, d_dict_off: [*]const u64, d_dict_len: [*]const u32, d_result: [*]i64, nblocks: u32) i32;
extern "c" fn zlz4_decompress_safe_continue(sd: *CStreamDecode, src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize) i64;
extern "c" fn zlz4_decoder_ring_buffer_size(max_block_size: usize) usize;
extern "c" fn zlz4_batch_decompress_safe_continue_workspace(nblocks: u32, nstreams: u32) usize;
extern "c" fn zlz4_batch_decompress_safe_continue(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_out: [*]u8, d_out_off: [*]const u64, d_out_cap: [*]const u32, d_run_start: [*]const u32, d_state: [*]CStreamDecode, d_result: [*]i64, nblocks: u32, nstreams: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4_batch_load_dict(stream: ?*anyopaque, d_dict: [*]const u8, d_dict_off: [*]const u64, d_dict_len: [*]const u32, d_tables: [*]u32, d_result: [*]i64, ndicts: u32) i32;
extern "c" fn zlz4_batch_compress_fast_continue(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_out: [*]u8, d_out_off: [*]const u64, d_out_cap: [*]const u32, d_table_in: [*]const u32, d_table_idx: ?[*]const u32, d_table_out: ?[*]u32, d_result: [*]i64, nblocks: u32, max_in_len: u32, acceleration: u32) i32;
extern "c" fn zlz4_batch_compress_fast_using_dict(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_out: [*]u8, d_out_off: [*]const u64, d_out_cap: [*]const u32, d_dict: ?[*]const u8, d_dict_off: [*]const u64, d_dict_len: [*]const u32, d_table: [*]const u32, d_table_idx: ?[*]const u32, d_result: [*]i64, nblocks: u32, max_in_len: u32, max_dict_len: u32, acceleration: u32) i32;
extern "c" fn zlz4_batch_compress_hc_workspace(nblocks: u32, max_in_len: u32) usize;
extern "c" fn zlz4_compress_hc_using_dict(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, dict: ?[*]const u8, dict_len: usize, level: i32) i64;
extern "c" fn zlz4_batch_compress_hc_using_dict_workspace(nblocks: u32, max_in_len: u32, max_dict_len: u32) usize;
extern "c" fn zlz4_batch_compress_hc_using_dict(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_out: [*]u8, d_out_off: [*]const u64, d_out_cap: [*]const u32, d_dict: ?[*]const u8, d_dict_off: [*]const u64, d_dict_len: [*]const u32, d_result: [*]i64, nblocks: u32, max_in_len: u32, max_dict_len: u32, level: i32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
pub const TrainParams = extern struct { d: u32 = 8, k: u32 = 256, f: u32 = 20, reserved: u32 = 0 };
extern "c" fn zlz4_train_dict(samples: ?[*]const u8, sample_sizes: ?[*]const usize, nsamples: u32, dict: ?[*]u8, dict_cap: usize, params: ?*const TrainParams) i64;
extern "c" fn zlz4_batch_train_dict_workspace(ngroups: u32, total_sample_bytes: u64, max_dict_cap: u32, params: ?*const TrainParams) usize;
extern "c" fn zlz4_batch_train_dict(stream: ?*anyopaque, d_src: ?[*]const u8, d_src_off: ?[*]const u64, d_src_len: ?[*]const u32, nsamples: u32, d_group_first: [*]const u32, ngroups: u32, d_dict: ?[*]u8, d_dict_off: [*]const u64, d_dict_cap: [*]const u32, d_result: [*]i64, max_dict_cap: u32, params: ?*const TrainParams, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4_batch_compress_hc(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_out: [*]u8, d_out_off: [*]const u64, d_out_cap: [*]const u32, d_result: [*]i64, nblocks: u32, max_in_len: u32, level: i32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4_batch_compress_dest_size_workspace(nblocks: u32, max_in_len: u32) usize;
extern "c" fn zlz4_batch_compress_dest_size(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_out: [*]u8, d_out_off: [*]const u64, d_out_cap: [*]const u32, d_result: [*]i64, d_consumed: [*]u32, nblocks: u32, max_in_len: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4_decompressed_size(src: [*]const u8, src_len: usize, dict_len: usize) i64;
extern "c" fn zlz4_batch_decompressed_size(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_dict_len: ?[*]const u32, d_size: [*]i64, nblocks: u32) i32;
extern "c" fn zlz4_batch_plan_outputs(stream: ?*anyopaque, d_size: [*]const i64, n: u32, alignment: u32, d_out_off: [*]u64, d_out_cap: [*]u32, d_total: *u64) i32;
extern "c" fn zlz4_batch_verify(stream: ?*anyopaque, d_in: [*]const u8, d_in_off: [*]const u64, d_in_len: [*]const u32, d_comp: [*]const u8, d_comp_off: [*]const u64, d_comp_result: [*]const i64, d_verify: [*]i64, nblocks: u32) i64;

pub const CPrefs = extern struct {
    block_size_id: u32 = 0,
    block_mode: u32 = 0,
    content_checksum: u32 = 0,
    block_checksum: u32 = 0,
    content_size: u64 = 0,
    dict_id: u32 = 0,
    compression_level: i32 = 0,
};
extern "c" fn zlz4f_compress_frame_bound(src_size: usize, prefs: ?*const CPrefs) usize;
extern "c" fn zlz4f_compress_frame(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, prefs: ?*const CPrefs) i64;
extern "c" fn zlz4f_decompress_frame(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize) i64;
extern "c" fn zlz4f_header_size(src: [*]const u8, src_len: usize) i64;
extern "c" fn zlz4f_compress_frame_device(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize, prefs: ?*const CPrefs) i64;
extern "c" fn zlz4f_decompress_frame_device(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize) i64;
extern "c" fn zlz4f_compress_frame_segment_device(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize, prefs: ?*const CPrefs, segment_flags: u32) i64;
extern "c" fn zlz4f_decompress_frame_segment_device(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize, prefs: ?*const CPrefs, segment_flags: u32) i64;
extern "c" fn zlz4f_batch_compress_frame_workspace(nframes: u32, max_blocks: u32, prefs: ?*const CPrefs) usize;
extern "c" fn zlz4f_batch_compress_frame(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_dst: [*]u8, d_dst_off: [*]const u64, d_dst_cap: [*]const u64, d_result: [*]i64, nframes: u32, max_blocks: u32, prefs: ?*const CPrefs, batch_flags: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_batch_decompress_frame_workspace(nframes: u32, max_blocks: u32) usize;
extern "c" fn zlz4f_frame_decompressed_size(src: [*]const u8, src_len: usize) i64;
extern "c" fn zlz4f_batch_frame_decompressed_size_workspace(nframes: u32, max_blocks: u32) usize;
extern "c" fn zlz4f_batch_frame_decompressed_size(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_size: [*]i64, nframes: u32, max_blocks: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_batch_compress_frame_workspace_ex(nframes: u32, max_blocks: u32, prefs: ?*const CPrefs, batch_flags: u32) usize;
extern "c" fn zlz4f_batch_compress_frame_ex(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_dst: [*]u8, d_dst_off: [*]const u64, d_dst_cap: [*]const u64, d_result: [*]i64, nframes: u32, max_blocks: u32, prefs: ?*const CPrefs, batch_flags: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_compress_frame_device_ex(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize, prefs: ?*const CPrefs, batch_flags: u32) i64;
extern "c" fn zlz4f_compress_frame_ex(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, prefs: ?*const CPrefs, batch_flags: u32) i64;
extern "c" fn zlz4f_batch_decompress_frame_workspace_ex(nframes: u32, max_blocks: u32, decode_flags: u32) usize;
extern "c" fn zlz4f_batch_decompress_frame_ex(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_dst: [*]u8, d_dst_off: [*]const u64, d_dst_cap: [*]const u64, d_result: [*]i64, nframes: u32, max_blocks: u32, decode_flags: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_batch_frame_decompressed_size_workspace_ex(nframes: u32, max_blocks: u32, decode_flags: u32) usize;
extern "c" fn zlz4f_batch_frame_decompressed_size_ex(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_size: [*]i64, nframes: u32, max_blocks: u32, decode_flags: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_decompress_frame_device_ex(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize, decode_flags: u32) i64;
extern "c" fn zlz4f_decompress_frame_ex(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, decode_flags: u32) i64;
extern "c" fn zlz4f_frame_decompressed_size_ex(src: [*]const u8, src_len: usize, decode_flags: u32) i64;
extern "c" fn zlz4f_batch_compress_frame_using_dict_workspace(nframes: u32, max_blocks: u32, prefs: ?*const CPrefs, batch_flags: u32, ndicts: u32, max_src_len: u64, max_dict_len: u32) usize;
extern "c" fn zlz4f_batch_compress_frame_using_dict_workspace_ex(nframes: u32, max_blocks: u32, prefs: ?*const CPrefs, batch_flags: u32, ndicts: u32, max_src_len: u64, max_dict_len: u32) usize;
extern "c" fn zlz4f_batch_compress_frame_using_dict(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_dst: [*]u8, d_dst_off: [*]const u64, d_dst_cap: [*]const u64, d_result: [*]i64, nframes: u32, max_blocks: u32, prefs: ?*const CPrefs, batch_flags: u32, d_dict: ?[*]const u8, d_dict_off: [*]const u64, d_dict_len: [*]const u32, ndicts: u32, d_dict_idx: ?[*]const u32, max_src_len: u64, max_dict_len: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_batch_compress_frame_using_dict_ex(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_dst: [*]u8, d_dst_off: [*]const u64, d_dst_cap: [*]const u64, d_result: [*]i64, nframes: u32, max_blocks: u32, prefs: ?*const CPrefs, batch_flags: u32, d_dict: ?[*]const u8, d_dict_off: [*]const u64, d_dict_len: [*]const u32, ndicts: u32, d_dict_idx: ?[*]const u32, max_src_len: u64, max_dict_len: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_batch_decompress_frame_using_dict_workspace(nframes: u32, max_blocks: u32) usize;
extern "c" fn zlz4f_batch_decompress_frame_using_dict(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_dst: [*]u8, d_dst_off: [*]const u64, d_dst_cap: [*]const u64, d_result: [*]i64, nframes: u32, max_blocks: u32, d_dict: ?[*]const u8, d_dict_off: [*]const u64, d_dict_len: [*]const u32, ndicts: u32, d_dict_idx: ?[*]const u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_batch_frame_decompressed_size_using_dict_workspace(nframes: u32, max_blocks: u32) usize;
extern "c" fn zlz4f_batch_frame_decompressed_size_using_dict(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_size: [*]i64, nframes: u32, max_blocks: u32, d_dict_len: [*]const u32, ndicts: u32, d_dict_idx: ?[*]const u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_batch_frame_dict_id(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_dict_id: [*]i64, nframes: u32) i32;
extern "c" fn zlz4f_compress_frame_using_dict(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, prefs: ?*const CPrefs, dict: ?[*]const u8, dict_len: usize) i64;
extern "c" fn zlz4f_compress_frame_using_dict_ex(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, prefs: ?*const CPrefs, dict: ?[*]const u8, dict_len: usize) i64;
extern "c" fn zlz4f_decompress_frame_using_dict(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, dict: ?[*]const u8, dict_len: usize) i64;
extern "c" fn zlz4f_frame_decompressed_size_using_dict(src: [*]const u8, src_len: usize, dict_len: usize) i64;
extern "c" fn zlz4f_batch_decompress_frame_prefix(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_dst: [*]u8, d_dst_off: [*]const u64, d_dst_cap: [*]const u64, d_result: [*]i64, nframes: u32) i32;
extern "c" fn zlz4f_batch_decompress_frame_prefix_using_dict(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_dst: [*]u8, d_dst_off: [*]const u64, d_dst_cap: [*]const u64, d_result: [*]i64, nframes: u32, d_dict: ?[*]const u8, d_dict_off: ?[*]const u64, d_dict_len: ?[*]const u32, ndicts: u32, d_dict_idx: ?[*]const u32) i32;
extern "c" fn zlz4f_decompress_frame_prefix(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize) i64;
extern "c" fn zlz4f_decompress_frame_prefix_using_dict(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, dict: ?[*]const u8, dict_len: usize) i64;
extern "c" fn zlz4f_batch_frame_index_workspace(nframes: u32, max_blocks: u32) usize;
extern "c" fn zlz4f_batch_frame_index(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_index: [*]IndexEntry, d_idx_off: [*]const u64, d_idx_cap: [*]const u64, d_result: [*]i64, nframes: u32, max_blocks: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_batch_plan_frame_ranges(stream: ?*anyopaque, d_index: [*]const IndexEntry, d_idx_off: [*]const u64, d_idx_n: [*]const i64, nframes: u32, d_range: [*]const Range, nranges: u32, alignment: u32, d_dst_off: [*]u64, d_dst_cap: [*]u64, d_totals: [*]u64) i32;
extern "c" fn zlz4f_batch_decompress_frame_range_workspace(nranges: u32, max_items: u32) usize;
extern "c" fn zlz4f_batch_decompress_frame_range(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_index: [*]const IndexEntry, d_idx_off: [*]const u64, d_idx_n: [*]const i64, nframes: u32, d_range: [*]const Range, d_dst: [*]u8, d_dst_off: [*]const u64, d_dst_cap: [*]const u64, d_skip: [*]u64, d_result: [*]i64, nranges: u32, max_items: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_decompress_frame_range(src: [*]const u8, src_len: usize, a: u64, b: u64, dst: [*]u8, dst_cap: usize) i64;
extern "c" fn zlz4f_batch_multiframe_split(stream: ?*anyopaque, d_src: ?[*]const u8, d_src_off: ?[*]const u64, d_src_len: ?[*]const u64, nbuf: u32, d_count: ?[*]u64, d_totals: [*]u64, d_member: ?[*]Member, d_mem_off: ?[*]const u64, d_mem_cap: ?[*]const u64, d_item_first: ?[*]u64, d_item_off: ?[*]u64, d_item_len: ?[*]u64, d_result: ?[*]i64) i32;
extern "c" fn zlz4f_batch_multiframe_plan(stream: ?*anyopaque, d_size: ?[*]const i64, d_item_first: ?[*]const u64, nbuf: u32, alignment: u32, d_dst_off: ?[*]u64, d_dst_cap: ?[*]u64, d_out_off: ?[*]u64, d_out_size: ?[*]u64, d_totals: [*]u64) i32;
extern "c" fn zlz4f_batch_multiframe_finish(stream: ?*anyopaque, d_member: ?[*]const Member, d_mem_off: ?[*]const u64, d_split_result: ?[*]const i64, d_item_first: ?[*]const u64, d_size: ?[*]const i64, d_item_result: ?[*]const i64, nbuf: u32, d_result: ?[*]i64) i32;
extern "c" fn zlz4f_multiframe_decompressed_size(src: [*]const u8, src_len: usize, decode_flags: u32) i64;
extern "c" fn zlz4f_decompress_multiframe(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, decode_flags: u32) i64;
extern "c" fn zlz4f_batch_multiframe_split_ex(stream: ?*anyopaque, d_src: ?[*]const u8, d_src_off: ?[*]const u64, d_src_len: ?[*]const u64, nbuf: u32, d_count: ?[*]u64, d_totals: [*]u64, d_member: ?[*]Member, d_mem_off: ?[*]const u64, d_mem_cap: ?[*]const u64, d_item_first: ?[*]u64, d_item_off: ?[*]u64, d_item_len: ?[*]u64, d_result: ?[*]i64, split_flags: u32, d_leg_len: ?[*]u64) i32;
extern "c" fn zlz4f_batch_multiframe_select(stream: ?*anyopaque, d_member: ?[*]const Member, d_mem_off: ?[*]const u64, d_split_result: ?[*]const i64, d_item_first: ?[*]const u64, d_from_frame: ?[*]const i64, d_from_legacy: ?[*]const i64, nbuf: u32, d_out: ?[*]i64) i32;
extern "c" fn zlz4f_multiframe_decompressed_size_ex(src: [*]const u8, src_len: usize, decode_flags: u32, split_flags: u32) i64;
extern "c" fn zlz4f_decompress_multiframe_ex(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, decode_flags: u32, split_flags: u32) i64;
extern "c" fn zlz4f_batch_file_index_workspace(nbuf: u32, split_totals: ?[*]const u64) usize;
extern "c" fn zlz4f_batch_file_index(stream: ?*anyopaque, d_src: ?[*]const u8, d_src_off: ?[*]const u64, d_src_len: ?[*]const u64, nbuf: u32, d_member: ?[*]const Member, d_mem_off: ?[*]const u64, d_split_result: ?[*]const i64, d_item_first: ?[*]const u64, d_item_off: ?[*]const u64, d_item_len: ?[*]const u64, d_leg_len: ?[*]const u64, split_totals: ?[*]const u64, d_index: ?[*]IndexEntry, d_idx_off: ?[*]u64, idx_cap: u64, d_result: ?[*]i64, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_batch_decompress_file_range_workspace(nranges: u32, max_items: u32) usize;
extern "c" fn zlz4f_batch_decompress_file_range(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_index: [*]const IndexEntry, d_idx_off: [*]const u64, d_idx_n: [*]const i64, nbuf: u32, d_member: [*]const Member, d_mem_off: [*]const u64, d_split_result: [*]const i64, d_range: [*]const Range, d_dst: [*]u8, d_dst_off: [*]const u64, d_dst_cap: [*]const u64, d_skip: [*]u64, d_result: [*]i64, nranges: u32, max_items: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_decompress_file_range(src: [*]const u8, src_len: usize, a: u64, b: u64, dst: [*]u8, dst_cap: usize, split_flags: u32) i64;
extern "c" fn zlz4f_seek_table_bound(nmembers: u64, nblocks: u64) usize;
extern "c" fn zlz4f_batch_append_seek_table(stream: ?*anyopaque, d_buf: ?[*]u8, d_buf_off: ?[*]const u64, d_buf_len: ?[*]const u64, d_buf_cap: ?[*]const u64, nbuf: u32, d_member: ?[*]const Member, d_mem_off: ?[*]const u64, d_split_result: ?[*]const i64, d_index: ?[*]const IndexEntry, d_idx_off: ?[*]const u64, d_idx_n: ?[*]const i64, d_result: ?[*]i64) i32;
extern "c" fn zlz4f_batch_load_seek_table(stream: ?*anyopaque, d_src: ?[*]const u8, d_src_off: ?[*]const u64, d_src_len: ?[*]const u64, nbuf: u32, d_count: ?[*]u64, d_totals: [*]u64, d_member: ?[*]Member, d_mem_off: ?[*]const u64, d_mem_cap: ?[*]const u64, d_split_result: ?[*]i64, d_index: ?[*]IndexEntry, d_idx_off: ?[*]u64, idx_cap: u64, d_idx_n: ?[*]i64) i32;
extern "c" fn zlz4f_batch_concat_workspace(nitems: u32) usize;
extern "c" fn zlz4f_batch_concat(stream: ?*anyopaque, d_src: ?[*]const u8, d_item_off: ?[*]const u64, d_item_len: ?[*]const i64, d_item_first: ?[*]const u64, nbuf: u32, nitems: u32, d_dst: ?[*]u8, d_dst_off: ?[*]const u64, d_dst_cap: ?[*]const u64, d_result: ?[*]i64, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_seek_table(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, split_flags: u32) i64;
extern "c" fn zlz4f_decompress_file_range_ex(src: [*]const u8, src_len: usize, a: u64, b: u64, dst: [*]u8, dst_cap: usize, split_flags: u32, range_flags: u32) i64;
extern "c" fn zlz4f_batch_file_index_using_dict_workspace(nbuf: u32, split_totals: ?[*]const u64) usize;
extern "c" fn zlz4f_batch_file_index_using_dict(stream: ?*anyopaque, d_src: ?[*]const u8, d_src_off: ?[*]const u64, d_src_len: ?[*]const u64, nbuf: u32, d_member: ?[*]const Member, d_mem_off: ?[*]const u64, d_split_result: ?[*]const i64, d_item_first: ?[*]const u64, d_item_off: ?[*]const u64, d_item_len: ?[*]const u64, d_leg_len: ?[*]const u64, split_totals: ?[*]const u64, d_index: ?[*]IndexEntry, d_idx_off: ?[*]u64, idx_cap: u64, d_result: ?[*]i64, d_dict_len: ?[*]const u32, ndicts: u32, d_dict_idx: ?[*]const u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_batch_decompress_file_range_using_dict_workspace(nranges: u32, max_items: u32) usize;
extern "c" fn zlz4f_batch_decompress_file_range_using_dict(stream: ?*anyopaque, d_src: ?[*]const u8, d_src_off: ?[*]const u64, d_src_len: ?[*]const u64, d_index: ?[*]const IndexEntry, d_idx_off: ?[*]const u64, d_idx_n: ?[*]const i64, nbuf: u32, d_member: ?[*]const Member, d_mem_off: ?[*]const u64, d_split_result: ?[*]const i64, d_range: ?[*]const Range, d_dst: ?[*]u8, d_dst_off: ?[*]const u64, d_dst_cap: ?[*]const u64, d_skip: ?[*]u64, d_result: ?[*]i64, nranges: u32, max_items: u32, d_dict: ?[*]const u8, d_dict_off: ?[*]const u64, d_dict_len: ?[*]const u32, ndicts: u32, d_dict_idx: ?[*]const u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;
extern "c" fn zlz4f_batch_multiframe_item_dicts(stream: ?*anyopaque, d_item_first: ?[*]const u64, nbuf: u32, nitems: u32, d_dict_idx: ?[*]const u32, d_item_dict_idx: ?[*]u32) i32;
extern "c" fn zlz4f_decompress_file_range_using_dict(src: [*]const u8, src_len: usize, a: u64, b: u64, dst: [*]u8, dst_cap: usize, split_flags: u32, range_flags: u32, dict: [*]const u8, dict_len: usize) i64;
/// zlz4f_legacy_prefs of include/zlz4_amd.h: block_size 0 = 8 MiB, 1 .. 8 MiB as given; compression_level <= 0 = fast
pub const LegacyPrefs = extern struct { block_size: u32 = 0, compression_level: i32 = 0 };
extern "c" fn zlz4f_legacy_compress_frame_bound(src_size: usize, prefs: ?*const LegacyPrefs) usize;
extern "c" fn zlz4f_compress_legacy_frame(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, prefs: ?*const LegacyPrefs) i64;
extern "c" fn zlz4f_legacy_frame_decompressed_size(src: [*]const u8, src_len: usize, consumed: ?*usize) i64;
extern "c" fn zlz4f_decompress_legacy_frame(src: [*]const u8, src_len: usize, dst: [*]u8, dst_cap: usize, consumed: ?*usize) i64;
/// zlz4f_member of include/zlz4_amd.h: kind & 0xFF is a MEMBER_* kind, (kind >> 8) & 15 the nibble of a skippable magic
pub const Member = extern struct { pos: u64, len: u64, kind: u32, buf: u32 };
/// zlz4f_index_entry / zlz4f_range of include/zlz4_amd.h
pub const IndexEntry = extern struct { pos: u64, dec: u64 };
pub const Range = extern struct { frame: u32, reserved: u32 = 0, a: u64, b: u64 };
extern "c" fn zlz4f_batch_decompress_frame(stream: ?*anyopaque, d_src: [*]const u8, d_src_off: [*]const u64, d_src_len: [*]const u64, d_dst: [*]u8, d_dst_off: [*]const u64, d_dst_cap: [*]const u64, d_result: [*]i64, nframes: u32, max_blocks: u32, d_workspace: ?*anyopaque, workspace_bytes: usize) i32;

// ---- constants (reference src/lz4.zig:12-25, src/lz4hc.zig:28-31) ----
pub const MINMATCH = 4;
pub const LZ4_MAX_INPUT_SIZE = 0x7E000000;
pub const LZ4_DISTANCE_MAX = 65535;
pub const LZ4HC_CLEVEL_MIN = 2;
pub const LZ4HC_CLEVEL_DEFAULT = 9;
pub const LZ4HC_CLEVEL_MAX = 12;
/// Stream.hashTable entries (reference src/lz4.zig:33, :752)
pub const LZ4_HASH_SIZE_U32 = 4096;

/// reference src/lz4.zig:48-55 plus the two device-side additions
pub const Error = error{
    OutputTooSmall,
    InputTooLarge,
    CorruptedData,
    DecompressionFailed,
    InvalidState,
    AllocationFailed,
    DeviceError,
    Unsupported,
};

fn mapBlock(code: i64) Error!usize {
    if (code >= 0) return @intCast(code);
    return switch (code) {
        -1 => error.OutputTooSmall,
        -2 => error.InputTooLarge,
        -3 => error.CorruptedData,
        -4 => error.DecompressionFailed,
        -5 => error.InvalidState,
        -6 => error.AllocationFailed,
        -8 => error.Unsupported,
        else => error.DeviceError,
    };
}

pub fn compressBound(inputSize: usize) usize {
    return zlz4_compress_bound(inputSize);
}
pub fn compressDefault(src: []const u8, dst: []u8) Error!usize {
    return mapBlock(zlz4_compress_default(src.ptr, src.len, dst.ptr, dst.len));
}
pub fn compressFast(src: []const u8, dst: []u8, acceleration: u32) Error!usize {
    return mapBlock(zlz4_compress_fast(src.ptr, src.len, dst.ptr, dst.len, acceleration));
}
pub fn decompressSafe(src: []const u8, dst: []u8) Error!usize {
    return mapBlock(zlz4_decompress_safe(src.ptr, src.len, dst.ptr, dst.len));
}
/// reference src/lz4.zig:619-621
pub fn decompressSafePartial(src: []const u8, dst: []u8, targetOutputSize: usize) Error!usize {
    return mapBlock(zlz4_decompress_safe_partial(src.ptr, src.len, dst.ptr, dst.len, targetOutputSize));
}
/// reference src/lz4.zig:960-962: `dict` is the data in front of dst (only its last 64 KiB can be referenced);
/// it must not overlap dst
pub fn decompressSafeUsingDict(src: []const u8, dst: []u8, dict: []const u8) Error!usize {
    return mapBlock(zlz4_decompress_safe_using_dict(src.ptr, src.len, dst.ptr, dst.len, dict.ptr, dict.len));
}
/// reference src/lz4.zig:967-969
pub fn decompressSafePartialUsingDict(src: []const u8, dst: []u8, targetOutputSize: usize, dict: []const u8) Error!usize {
    return mapBlock(zlz4_decompress_safe_partial_using_dict(src.ptr, src.len, dst.ptr, dst.len, targetOutputSize, dict.ptr, dict.len));
}
/// No counterpart in the reference: the first dst.len bytes of the block (all of it where it decodes to fewer), never
/// OutputTooSmall -- decompressGeneric with oend = dst.len, a walk that stops once dst is full and copies of the last
/// sequence cut there (include/zlz4_amd.h).  Returns min(decoded size, dst.len).
pub fn decompressSafePrefix(src: []const u8, dst: []u8) Error!usize {
    return mapBlock(zlz4_decompress_safe_prefix(src.ptr, src.len, dst.ptr, dst.len));
}
/// decompressSafePrefix with `dict` in front of dst, as decompressSafeUsingDict
pub fn decompressSafePrefixUsingDict(src: []const u8, dst: []u8, dict: []const u8) Error!usize {
    return mapBlock(zlz4_decompress_safe_prefix_using_dict(src.ptr, src.len, dst.ptr, dst.len, dict.ptr, dict.len));
}
/// No counterpart in the reference (its Stream never refers to a loaded dictionary): compressFastWithHashTable's loop
/// (src/lz4.zig:624-740) on the last 64 KiB of `dict` followed by `src`, from the table Stream.loadDict(dict) leaves
/// (:798-820), so that matches may reach into the dictionary.  decompressSafeUsingDict(dst[0..r], out, dict) gives src back.
pub fn compressFastUsingDict(src: []const u8, dst: []u8, dict: []const u8, acceleration: u32) Error!usize {
    return mapBlock(zlz4_compress_fast_using_dict(src.ptr, src.len, dst.ptr, dst.len, dict.ptr, dict.len, acceleration));
}
/// No counterpart in the reference: what decompressSafe (dict_len 0) or decompressSafeUsingDict with a dictionary of
/// dict_len bytes returns for `src` into a destination of 0xFFFFFFFF bytes.  Nothing is decoded.
pub fn decompressedSize(src: []const u8, dict_len: usize) Error!usize {
    return mapBlock(zlz4_decompressed_size(src.ptr, src.len, dict_len));
}
/// reference src/lz4.zig:524-526
pub fn sizeofState() usize {
    return zlz4_sizeof_state();
}
/// reference src/lz4.zig:531-546
pub fn compressFastExtState(state: []u8, src: []const u8, dst: []u8, acceleration: u32) Error!usize {
    return mapBlock(zlz4_compress_fast_ext_state(state.ptr, state.len, src.ptr, src.len, dst.ptr, dst.len, acceleration));
}
/// reference src/lz4.zig:551-616 (srcSizePtr: in = available, out = consumed)
pub fn compressDestSize(src: []const u8, dst: []u8, srcSizePtr: *usize) Error!usize {
    return mapBlock(zlz4_compress_dest_size(src.ptr, dst.ptr, dst.len, srcSizePtr));
}
/// No counterpart in the reference: compressHashChain (src/lz4hc.zig:976-1064) on dict-tail ++ src with the parse starting
/// at the record, levels 3..9 (below 2 becomes 9 as in compressHC; 2 and 10..12 are error.Unsupported).  Decodes with
/// decompressSafeUsingDict(dst[0..n], out, dict).
pub fn compressHCUsingDict(src: []const u8, dst: []u8, dict: []const u8, compressionLevel: i32) Error!usize {
    return mapBlock(zlz4_compress_hc_using_dict(src.ptr, src.len, dst.ptr, dst.len, dict.ptr, dict.len, compressionLevel));
}
/// Dictionary training (no counterpart in the reference): one dictionary of at most dict.len (<= 65536) bytes from samples
/// that lie back to back in `samples`, sample i having sampleSizes[i] bytes; the fastCover-style selection specified in
/// include/zlz4_amd.h.  Returns the dictionary's length; dict[0..len] goes into every ...UsingDict call.
pub fn trainDict(samples: []const u8, sampleSizes: []const usize, dict: []u8, params: TrainParams) Error!usize {
    return mapBlock(zlz4_train_dict(samples.ptr, sampleSizes.ptr, @intCast(sampleSizes.len), dict.ptr, dict.len, &params));
}
pub fn compressHC(src: []const u8, dst: []u8, compressionLevel: i32) Error!usize {
    return mapBlock(zlz4_compress_hc(src.ptr, src.len, dst.ptr, dst.len, compressionLevel));
}
/// reference src/lz4hc.zig:1492-1494
pub fn sizeofStateHC() usize {
    return zlz4_sizeof_state_hc();
}
/// reference src/lz4hc.zig:1457-1489.  The reference takes `*Context`; its tables live on the device here, so the
/// context is passed as the bytes it occupies (a fresh `Context.init()`, as compressHC itself uses, :1450).
pub fn compressHCExtState(ctx: []u8, src: []const u8, dst: []u8, compressionLevel: i32) Error!usize {
    return mapBlock(zlz4_compress_hc_ext_state(ctx.ptr, ctx.len, src.ptr, src.len, dst.ptr, dst.len, compressionLevel));
}

/// reference src/lz4.zig:744-748 (carried, never read, as in the reference)
const TableType = enum(u32) {
    byU32 = 1,
    byU16 = 2,
    byPtr = 3,
};

/// The streaming compressor, reference src/lz4.zig:751-856: same fields and methods.  loadDict and compressFastContinue
/// compute the table on the device (zlz4_stream_load_dict / zlz4_stream_compress_fast_continue); the rest is host
/// bookkeeping.  The reference reads every table entry as a position in the CURRENT block (:656-659), so a loaded
/// dictionary only changes which in-block matches are found: no block refers to it, every block decodes with plain
/// decompressSafe, and saveDict copies the loaded dictionary, not the compressed history.  Reproduced as is.
pub const Stream = struct {
    hashTable: [LZ4_HASH_SIZE_U32]u32,
    dictionary: ?[]const u8,
    dictCtx: ?*const Stream,
    currentOffset: u32,
    tableType: TableType,
    dictSize: u32,
    allocator: ?std.mem.Allocator,

    /// reference :761-766
    pub fn create(allocator: std.mem.Allocator) Error!*Stream {
        const stream = allocator.create(Stream) catch return error.AllocationFailed;
        stream.* = init();
        stream.allocator = allocator;
        return stream;
    }
    /// reference :769-773
    pub fn destroy(self: *Stream) void {
        if (self.allocator) |alloc| {
            alloc.destroy(self);
        }
    }
    /// reference :776-786
    pub fn init() Stream {
        return .{
            .hashTable = [_]u32{0} ** LZ4_HASH_SIZE_U32,
            .dictionary = null,
            .dictCtx = null,
            .currentOffset = 0,
            .tableType = .byU32,
            .dictSize = 0,
            .allocator = null,
        };
    }
    /// reference :789-795
    pub fn resetFast(self: *Stream) void {
        @memset(&self.hashTable, 0);
        self.dictionary = null;
        self.dictCtx = null;
        self.currentOffset = 0;
        self.dictSize = 0;
    }
    /// reference :798-820.  The signature has no error union; a missing device is a loud failure, never a silently
    /// empty table.
    pub fn loadDict(self: *Stream, dict: []const u8) usize {
        self.resetFast();
        const r = zlz4_stream_load_dict(&self.hashTable, dict.ptr, dict.len);
        if (r < 0) @panic("Stream.loadDict: libzlz4_amd has no usable gfx950 device");
        const dictSize: usize = @intCast(r);
        if (dictSize > 0) {
            self.dictionary = dict[dict.len - dictSize ..];
            self.dictSize = @intCast(dictSize);
        }
        return dictSize;
    }
    /// reference :822-836: the table changes only when a block of 13 or more bytes compresses
    pub fn compressFastContinue(self: *Stream, src: []const u8, dst: []u8, acceleration: u32) Error!usize {
        const result = try mapBlock(zlz4_stream_compress_fast_continue(&self.hashTable, src.ptr, src.len, dst.ptr, dst.len, acceleration));
        if (src.len >= 13) self.currentOffset +|= @intCast(src.len);
        return result;
    }
    /// reference :839-855
    pub fn saveDict(self: *Stream, safeBuffer: []u8, maxDictSize: usize) usize {
        if (maxDictSize == 0) return 0;
        if (self.dictionary == null) return 0;
        const dict = self.dictionary.?;
        const dictSize = @min(@min(dict.len, maxDictSize), 64 * 1024);
        if (dictSize > safeBuffer.len) {
            const copySize = @min(dictSize, safeBuffer.len);
            @memcpy(safeBuffer[0..copySize], dict[dict.len - copySize ..]);
            return copySize;
        }
        @memcpy(safeBuffer[0..dictSize], dict[dict.len - dictSize ..]);
        return dictSize;
    }
};
/// reference src/lz4.zig:858-860
pub fn createStream(allocator: std.mem.Allocator) Error!*Stream {
    return Stream.create(allocator);
}
/// reference src/lz4.zig:863-865
pub fn freeStream(stream: *Stream) void {
    stream.destroy();
}

/// zlz4_stream_decode_t: StreamDecode's fields as byte addresses (0 = null); also the device state of
/// `device.decompressSafeContinueBatch`
pub const CStreamDecode = extern struct {
    dict: u64,
    dict_len: u64,
    prefix: u64,
    prefix_len: u64,
};

/// The streaming decompressor, reference src/lz4.zig:870-951: same fields and methods.  A call never reads the previous
/// output, only compares its address with dst (include/zlz4_amd.h): each call is one zlz4_decompress_safe_continue.
/// WARNING (a defect of the reference, reproduced): when the previous output lies above dst in memory -- a ring buffer
/// of decoderRingBufferSize bytes once it wraps, a double buffer whose second half is lower -- every match reaching
/// further back than prefix - dst bytes before the match position fails with CorruptedData.
pub const StreamDecode = struct {
    externalDict: ?[]const u8,
    prefixEnd: ?[]const u8,
    extDictSize: usize,
    prefixSize: usize,
    allocator: ?std.mem.Allocator,

    pub fn create(allocator: std.mem.Allocator) Error!*StreamDecode {
        const stream = allocator.create(StreamDecode) catch return error.AllocationFailed;
        stream.* = init();
        stream.allocator = allocator;
        return stream;
    }
    pub fn destroy(self: *StreamDecode) void {
        if (self.allocator) |alloc| alloc.destroy(self);
    }
    pub fn init() StreamDecode {
        return .{ .externalDict = null, .prefixEnd = null, .extDictSize = 0, .prefixSize = 0, .allocator = null };
    }
    /// reference src/lz4.zig:904-909
    pub fn setStreamDecode(self: *StreamDecode, dict: ?[]const u8) void {
        self.externalDict = dict;
        self.prefixEnd = null;
        self.extDictSize = if (dict) |d| d.len else 0;
        self.prefixSize = 0;
    }
    /// reference src/lz4.zig:912-939; errors leave the state unchanged
    pub fn decompressSafeContinue(self: *StreamDecode, src: []const u8, dst: []u8) Error!usize {
        var c = CStreamDecode{
            .dict = if (self.externalDict) |d| @intFromPtr(d.ptr) else 0,
            .dict_len = self.extDictSize,
            .prefix = if (self.prefixEnd) |p| @intFromPtr(p.ptr) else 0,
            .prefix_len = self.prefixSize,
        };
        const result = try mapBlock(zlz4_decompress_safe_continue(&c, src.ptr, src.len, dst.ptr, dst.len));
        self.prefixEnd = dst[0..result];
        self.prefixSize = result;
        if (c.dict == 0) self.externalDict = null; // :936 (mode A keeps it)
        self.extDictSize = @intCast(c.dict_len);
        return result;
    }
};
/// reference src/lz4.zig:943-945
pub fn createStreamDecode(allocator: std.mem.Allocator) Error!*StreamDecode {
    return StreamDecode.create(allocator);
}
/// reference src/lz4.zig:948-950
pub fn freeStreamDecode(stream: *StreamDecode) void {
    stream.destroy();
}
/// reference src/lz4.zig:954-957
pub fn decoderRingBufferSize(maxBlockSize: usize) usize {
    return zlz4_decoder_ring_buffer_size(maxBlockSize);
}

/// `@import("lz4").lz4.compressDefault(...)` and `.lz4hc.compressHC(...)` keep working (reference src/root.zig:3-5)
const root = @This();
pub const lz4 = struct {
    pub const Error = root.Error;
    pub const MINMATCH = 4;
    pub const LZ4_MAX_INPUT_SIZE = 0x7E000000;
    pub const LZ4_DISTANCE_MAX = 65535;
    pub const compressBound = root.compressBound;
    pub const compressDefault = root.compressDefault;
    pub const compressFast = root.compressFast;
    pub const compressDestSize = root.compressDestSize;
    pub const decompressSafe = root.decompressSafe;
    pub const decompressSafePartial = root.decompressSafePartial;
    pub const decompressSafeUsingDict = root.decompressSafeUsingDict;
    pub const decompressSafePartialUsingDict = root.decompressSafePartialUsingDict;
    pub const compressFastUsingDict = root.compressFastUsingDict;
    pub const decompressedSize = root.decompressedSize;
    pub const sizeofState = root.sizeofState;
    pub const compressFastExtState = root.compressFastExtState;
    pub const LZ4_HASH_SIZE_U32 = root.LZ4_HASH_SIZE_U32;
    pub const Stream = root.Stream;
    pub const createStream = root.createStream;
    pub const freeStream = root.freeStream;
    pub const StreamDecode = root.StreamDecode;
    pub const createStreamDecode = root.createStreamDecode;
    pub const freeStreamDecode = root.freeStreamDecode;
    pub const decoderRingBufferSize = root.decoderRingBufferSize;
};
pub const lz4hc = struct {
    pub const LZ4HC_CLEVEL_MIN = 2;
    pub const LZ4HC_CLEVEL_DEFAULT = 9;
    pub const LZ4HC_CLEVEL_MAX = 12;
    pub const compressHC = root.compressHC;
    pub const compressHCExtState = root.compressHCExtState;
    pub const compressHCUsingDict = root.compressHCUsingDict;
    pub const trainDict = root.trainDict;
    pub const TrainParams = root.TrainParams;
    pub const sizeofStateHC = root.sizeofStateHC;
};

/// The hot path itself (no counterpart in the reference, whose calls take one block): many independent blocks per
/// call, all pointers DEVICE pointers (`[*]` = raw device address), asynchronous on `stream` (a hipStream_t, null =
/// default stream).  `descs` is the slice-of-slices view a Zig caller has, flattened into the four descriptor arrays
/// the C ABI takes; they live in device memory like the payload.
pub const device = struct {
    pub const Blocks = struct {
        in: [*]const u8, // input arena
        in_off: [*]const u64, // per block: offset into `in`
        in_len: [*]const u32, // per block: bytes
        out: [*]u8, // output arena
        out_off: [*]const u64, // per block: offset into `out`
        out_cap: [*]const u32, // per block: capacity
        result: [*]i64, // per block: bytes written or -(lz4.Error index)
        nblocks: u32,
    };
    pub const DictBlocks = root.DictBlocks;
    pub const decompressSafeUsingDictBatch = root.decompressSafeUsingDictBatch;
    fn mapLaunch(rc: i32) Error!void {
        if (rc == 0) return;
        _ = try mapBlock(rc);
    }
    /// batch form of compressFast (src/lz4.zig:292-447); every in_len[i] <= max_in_len
    pub fn compressFastBatch(stream: ?*anyopaque, b: Blocks, max_in_len: u32, acceleration: u32) Error!void {
        return mapLaunch(zlz4_batch_compress_fast(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.result, b.nblocks, max_in_len, acceleration));
    }
    /// batch form of decompressSafe (src/lz4.zig:257-259)
    pub fn decompressSafeBatch(stream: ?*anyopaque, b: Blocks) Error!void {
        return mapLaunch(zlz4_batch_decompress_safe(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.result, b.nblocks));
    }
    /// batch form of decompressSafePrefix: b.out_cap[i] is the number of bytes wanted of block i and the size of its slot
    pub fn decompressSafePrefixBatch(stream: ?*anyopaque, b: Blocks) Error!void {
        return mapLaunch(zlz4_batch_decompress_safe_prefix(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.result, b.nblocks));
    }
    /// decompressed sizes (zlz4_batch_decompressed_size): size[i] = what decompressSafeBatch returns for block i into
    /// 0xFFFFFFFF bytes, or decompressSafeUsingDictBatch with a dictionary of dict_len[i] bytes (null = no dictionary)
    pub fn decompressedSizeBatch(stream: ?*anyopaque, in: [*]const u8, in_off: [*]const u64, in_len: [*]const u32, dict_len: ?[*]const u32, size: [*]i64, nblocks: u32) Error!void {
        return mapLaunch(zlz4_batch_decompressed_size(stream, in, in_off, in_len, dict_len, size, nblocks));
    }
    /// packed output slots from sizes (zlz4_batch_plan_outputs): out_off / out_cap as `Blocks` takes them, total = bytes
    /// of all slots; alignment 0, 1 or a power of two up to 4096
    pub fn planOutputs(stream: ?*anyopaque, size: [*]const i64, n: u32, alignment: u32, out_off: [*]u64, out_cap: [*]u32, total: *u64) Error!void {
        return mapLaunch(zlz4_batch_plan_outputs(stream, size, n, alignment, out_off, out_cap, total));
    }
    pub fn decompressSafeContinueWorkspace(nblocks: u32, nstreams: u32) usize {
        return zlz4_batch_decompress_safe_continue_workspace(nblocks, nstreams);
    }
    /// StreamDecode.decompressSafeContinue (src/lz4.zig:912-939) over whole streams: stream s makes the calls
    /// [run_start[s], run_start[s + 1]) of `b` in order (nstreams + 1 entries) from state[s] (device addresses, updated in
    /// place); b.result[i] = what call i returns.  Output slots must not overlap (zlz4_batch_decompress_safe_continue).
    pub fn decompressSafeContinueBatch(stream: ?*anyopaque, b: Blocks, run_start: [*]const u32, state: [*]CStreamDecode, nstreams: u32, workspace: ?*anyopaque, workspace_bytes: usize) Error!void {
        return mapLaunch(zlz4_batch_decompress_safe_continue(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, run_start, state, b.result, b.nblocks, nstreams, workspace, workspace_bytes));
    }
    /// batch form of Stream.loadDict (src/lz4.zig:798-820): table i of `tables` (LZ4_HASH_SIZE_U32 u32 each) receives
    /// the table of dict[dict_off[i] ..][0..dict_len[i]]; result[i] = dictSize
    pub fn loadDictBatch(stream: ?*anyopaque, dict: [*]const u8, dict_off: [*]const u64, dict_len: [*]const u32, tables: [*]u32, result: [*]i64, ndicts: u32) Error!void {
        return mapLaunch(zlz4_batch_load_dict(stream, dict, dict_off, dict_len, tables, result, ndicts));
    }
    /// Stream tables of `compressFastContinueBatch`: block i starts from table table_idx[i] of table_in (null = table i)
    /// and its final table goes to table i of table_out (null = not written; may equal table_in when table_idx is null)
    pub const StreamTables = struct {
        table_in: [*]const u32,
        table_idx: ?[*]const u32 = null,
        table_out: ?[*]u32 = null,
    };
    /// batch form of Stream.compressFastContinue (src/lz4.zig:822-836); every in_len[i] <= max_in_len
    pub fn compressFastContinueBatch(stream: ?*anyopaque, b: Blocks, t: StreamTables, max_in_len: u32, acceleration: u32) Error!void {
        return mapLaunch(zlz4_batch_compress_fast_continue(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, t.table_in, t.table_idx, t.table_out, b.result, b.nblocks, max_in_len, acceleration));
    }
    /// batch form of compressFastUsingDict (no counterpart in the reference): block i against dictionary d (DictBlocks) from
    /// table table_idx[i] of `table` (null = table i), the tables being loadDictBatch's of the dictionaries; every
    /// in_len[i] <= max_in_len and min(dict_len[i], 65536) <= max_dict_len
    pub fn compressFastUsingDictBatch(stream: ?*anyopaque, b: Blocks, d: DictBlocks, table: [*]const u32, table_idx: ?[*]const u32, max_in_len: u32, max_dict_len: u32, acceleration: u32) Error!void {
        return mapLaunch(zlz4_batch_compress_fast_using_dict(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, d.dict, d.dict_off, d.dict_len, table, table_idx, b.result, b.nblocks, max_in_len, max_dict_len, acceleration));
    }
    pub fn compressHCWorkspace(nblocks: u32, max_in_len: u32) usize {
        return zlz4_batch_compress_hc_workspace(nblocks, max_in_len);
    }
    /// batch form of compressHC (src/lz4hc.zig:1440-1453); `workspace` = device memory of compressHCWorkspace() bytes
    pub fn compressHCBatch(stream: ?*anyopaque, b: Blocks, max_in_len: u32, level: i32, workspace: ?*anyopaque, workspace_bytes: usize) Error!void {
        return mapLaunch(zlz4_batch_compress_hc(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.result, b.nblocks, max_in_len, level, workspace, workspace_bytes));
    }
    pub fn compressHCUsingDictWorkspace(nblocks: u32, max_in_len: u32, max_dict_len: u32) usize {
        return zlz4_batch_compress_hc_using_dict_workspace(nblocks, max_in_len, max_dict_len);
    }
    /// batch form of compressHCUsingDict: block i against dictionary d (DictBlocks); `workspace` = device memory of
    /// compressHCUsingDictWorkspace() bytes, 16-byte aligned
    pub fn compressHCUsingDictBatch(stream: ?*anyopaque, b: Blocks, d: DictBlocks, max_in_len: u32, max_dict_len: u32, level: i32, workspace: ?*anyopaque, workspace_bytes: usize) Error!void {
        return mapLaunch(zlz4_batch_compress_hc_using_dict(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, d.dict, d.dict_off, d.dict_len, b.result, b.nblocks, max_in_len, max_dict_len, level, workspace, workspace_bytes));
    }
    /// one dictionary per group of samples (include/zlz4_amd.h, zlz4_batch_train_dict)
    pub const TrainGroups = struct {
        src: ?[*]const u8, // sample arena
        src_off: ?[*]const u64, // per sample: offset into `src`
        src_len: ?[*]const u32, // per sample: bytes
        nsamples: u32,
        group_first: [*]const u32, // ngroups + 1: group g is samples group_first[g] .. group_first[g + 1] - 1
        ngroups: u32,
        dict: ?[*]u8, // dictionary arena
        dict_off: [*]const u64, // per group: offset of its slot
        dict_cap: [*]const u32, // per group: capacity (<= 65536)
        result: [*]i64, // per group: the dictionary's length or an error code
    };
    pub fn trainDictWorkspace(ngroups: u32, total_sample_bytes: u64, max_dict_cap: u32, params: TrainParams) usize {
        return zlz4_batch_train_dict_workspace(ngroups, total_sample_bytes, max_dict_cap, &params);
    }
    /// batch form of trainDict: every group in the same launches; `workspace` = device memory of trainDictWorkspace()
    /// bytes, 16-byte aligned
    pub fn trainDictBatch(stream: ?*anyopaque, g: TrainGroups, max_dict_cap: u32, params: TrainParams, workspace: ?*anyopaque, workspace_bytes: usize) Error!void {
        return mapLaunch(zlz4_batch_train_dict(stream, g.src, g.src_off, g.src_len, g.nsamples, g.group_first, g.ngroups, g.dict, g.dict_off, g.dict_cap, g.result, max_dict_cap, &params, workspace, workspace_bytes));
    }
    pub fn compressDestSizeWorkspace(nblocks: u32, max_in_len: u32) usize {
        return zlz4_batch_compress_dest_size_workspace(nblocks, max_in_len);
    }
    /// batch form of compressDestSize (src/lz4.zig:551-616): in_len[i] = bytes available, out_cap[i] = dst.len;
    /// result[i] = compressed size, consumed[i] = source bytes consumed; `workspace` = device memory of
    /// compressDestSizeWorkspace() bytes; every in_len[i] <= max_in_len
    pub fn compressDestSizeBatch(stream: ?*anyopaque, b: Blocks, consumed: [*]u32, max_in_len: u32, workspace: ?*anyopaque, workspace_bytes: usize) Error!void {
        return mapLaunch(zlz4_batch_compress_dest_size(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.result, consumed, b.nblocks, max_in_len, workspace, workspace_bytes));
    }
    /// opt-in check for levels 10..12 (include/zlz4_amd.h): decodes the batch a compress call produced (`b` as passed to
    /// it) and compares with the input; verify[i] = b.result[i] or -9; returns the number of blocks that do not round-trip
    pub fn verifyBatch(stream: ?*anyopaque, b: Blocks, verify: [*]i64) Error!usize {
        return mapBlock(zlz4_batch_verify(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.result, verify, b.nblocks));
    }
};

/// Per-block dictionaries of `device.decompressSafeUsingDictBatch` (device memory, like `device.Blocks`): block i reads
/// dict[dict_off[i] ..][0..dict_len[i]].  A shared dictionary is one copy with the same offset for every block.
pub const DictBlocks = struct {
    dict: [*]const u8, // dictionary arena
    dict_off: [*]const u64, // per block: offset into `dict`
    dict_len: [*]const u32, // per block: bytes (any length; only the last 64 KiB can be referenced)
};
/// batch form of decompressSafeUsingDict (src/lz4.zig:960-962); dictionaries are read-only and must not overlap `b.out`
pub fn decompressSafeUsingDictBatch(stream: ?*anyopaque, b: device.Blocks, d: DictBlocks) Error!void {
    return device.mapLaunch(zlz4_batch_decompress_safe_using_dict(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, d.dict, d.dict_off, d.dict_len, b.result, b.nblocks));
}
/// batch form of decompressSafePrefixUsingDict; b.out_cap as in device.decompressSafePrefixBatch
pub fn decompressSafePrefixUsingDictBatch(stream: ?*anyopaque, b: device.Blocks, d: DictBlocks) Error!void {
    return device.mapLaunch(zlz4_batch_decompress_safe_prefix_using_dict(stream, b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, d.dict, d.dict_off, d.dict_len, b.result, b.nblocks));
}

/// Mirror of the `lz4f` namespace (reference src/lz4f.zig); enum/struct shapes as in :64-122.
pub const lz4f = struct {
    pub const MAGICNUMBER: u32 = 0x184D2204;
    /// reference src/lz4f.zig:57-59
    pub fn isError(code: usize) bool {
        return code > @as(usize, @bitCast(@as(isize, -65536)));
    }
    pub const BlockSizeID = enum(u3) {
        default = 0,
        max64KB = 4,
        max256KB = 5,
        max1MB = 6,
        max4MB = 7,

        /// reference src/lz4f.zig:71-78
        pub fn toBlockSize(self: BlockSizeID) Error!usize {
            return switch (self) {
                .default, .max64KB => 64 * 1024,
                .max256KB => 256 * 1024,
                .max1MB => 1024 * 1024,
                .max4MB => 4 * 1024 * 1024,
            };
        }
    };
    pub const BlockMode = enum(u1) { linked = 0, independent = 1 };
    pub const ContentChecksum = enum(u1) { disabled = 0, enabled = 1 };
    pub const BlockChecksum = enum(u1) { disabled = 0, enabled = 1 };
    pub const FrameType = enum(u1) { frame = 0, skippableFrame = 1 };
    pub const FrameInfo = struct {
        blockSizeID: BlockSizeID = .default,
        blockMode: BlockMode = .linked,
        contentChecksumFlag: ContentChecksum = .disabled,
        frameType: FrameType = .frame,   // reference :100-111; compressFrame always writes .frame (:304-351)
        contentSize: u64 = 0,
        dictID: u32 = 0,
        blockChecksumFlag: BlockChecksum = .disabled,
    };
    pub const Preferences = struct {
        frameInfo: FrameInfo = .{},
        compressionLevel: i32 = 0,
        autoFlush: bool = false,
        favorDecSpeed: bool = false,
    };
    /// reference src/lz4f.zig:31-55: every member, under the reference's name (`lz4f.Error`), so that callers that
    /// switch on it or name `lz4f.Error!usize` compile unchanged; + the two device additions
    pub const Error = error{
        Generic, MaxBlockSizeInvalid, BlockModeInvalid, ParameterInvalid, CompressionLevelInvalid, HeaderVersionWrong,
        BlockChecksumInvalid, ReservedFlagSet, AllocationFailed, SrcSizeTooLarge, DstMaxSizeTooSmall,
        FrameHeaderIncomplete, FrameTypeUnknown, FrameSizeWrong, SrcPtrWrong, DecompressionFailed,
        HeaderChecksumInvalid, ContentChecksumInvalid, FrameDecodingAlreadyStarted, CompressionStateUninitialized,
        ParameterNull, MaxCode, OutOfMemory,
        DeviceError, Unsupported,
    };
    pub const FrameError = Error;   // the name earlier revisions of this facade used
    fn mapFrame(code: i64) Error!usize {
        if (code >= 0) return @intCast(code);
        return switch (code) {
            -101 => error.Generic, -102 => error.MaxBlockSizeInvalid, -106 => error.HeaderVersionWrong,
            -107 => error.BlockChecksumInvalid, -108 => error.ReservedFlagSet, -109 => error.AllocationFailed,
            -110 => error.SrcSizeTooLarge, -111 => error.DstMaxSizeTooSmall, -112 => error.FrameHeaderIncomplete,
            -113 => error.FrameTypeUnknown, -114 => error.FrameSizeWrong, -116 => error.DecompressionFailed,
            -117 => error.HeaderChecksumInvalid, -118 => error.ContentChecksumInvalid, -8 => error.Unsupported, -104 => error.ParameterInvalid,
            else => error.DeviceError,
        };
    }
    fn toC(p: Preferences) CPrefs {
        return .{
            .block_size_id = @intFromEnum(p.frameInfo.blockSizeID),
            .block_mode = @intFromEnum(p.frameInfo.blockMode),
            .content_checksum = @intFromEnum(p.frameInfo.contentChecksumFlag),
            .block_checksum = @intFromEnum(p.frameInfo.blockChecksumFlag),
            .content_size = p.frameInfo.contentSize,
            .dict_id = p.frameInfo.dictID,
            .compression_level = p.compressionLevel,
        };
    }
    pub fn compressFrameBound(srcSize: usize, prefs: ?Preferences) usize {
        if (prefs) |p| { const c = toC(p); return zlz4f_compress_frame_bound(srcSize, &c); }
        return zlz4f_compress_frame_bound(srcSize, null);
    }
    /// the allocator argument of the reference (unused there, src/lz4f.zig:443) is kept for source compatibility
    pub fn compressFrame(allocator: std.mem.Allocator, src: []const u8, dst: []u8, prefs: ?Preferences) Error!usize {
        _ = allocator;
        if (prefs) |p| { const c = toC(p); return mapFrame(zlz4f_compress_frame(src.ptr, src.len, dst.ptr, dst.len, &c)); }
        return mapFrame(zlz4f_compress_frame(src.ptr, src.len, dst.ptr, dst.len, null));
    }
    pub fn decompressFrame(allocator: std.mem.Allocator, src: []const u8, dst: []u8) Error!usize {
        _ = allocator;
        return mapFrame(zlz4f_decompress_frame(src.ptr, src.len, dst.ptr, dst.len));
    }
    pub fn headerSize(src: []const u8) Error!usize {
        return mapFrame(zlz4f_header_size(src.ptr, src.len));
    }
    /// No counterpart in the reference: what decompressFrame returns for `src` into a destination that is large enough
    /// (the content checksum is not verified).  Nothing is decoded.
    pub fn frameDecompressedSize(src: []const u8) Error!usize {
        return mapFrame(zlz4f_frame_decompressed_size(src.ptr, src.len));
    }

    /// Device-resident frames (BASELINE configs[4]): `d_src` / `d_dst` are device pointers.
    pub const SEG_FIRST: u32 = 1;
    pub const SEG_LAST: u32 = 2;
    pub fn compressFrameDevice(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize, prefs: ?Preferences) Error!usize {
        if (prefs) |p| { const c = toC(p); return mapFrame(zlz4f_compress_frame_device(stream, d_src, src_len, d_dst, dst_cap, &c)); }
        return mapFrame(zlz4f_compress_frame_device(stream, d_src, src_len, d_dst, dst_cap, null));
    }
    pub fn decompressFrameDevice(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize) Error!usize {
        return mapFrame(zlz4f_decompress_frame_device(stream, d_src, src_len, d_dst, dst_cap));
    }
    /// one rank's block segment of a frame spread over several GPUs (include/zlz4_amd.h)
    pub fn compressFrameSegmentDevice(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize, prefs: Preferences, segment_flags: u32) Error!usize {
        const c = toC(prefs);
        return mapFrame(zlz4f_compress_frame_segment_device(stream, d_src, src_len, d_dst, dst_cap, &c, segment_flags));
    }
    pub fn decompressFrameSegmentDevice(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize, prefs: Preferences, segment_flags: u32) Error!usize {
        const c = toC(prefs);
        return mapFrame(zlz4f_decompress_frame_segment_device(stream, d_src, src_len, d_dst, dst_cap, &c, segment_flags));
    }

    /// Batch frames (include/zlz4_amd.h section 3): frame f reads src[src_off[f]..][0..src_len[f]] and writes
    /// dst[dst_off[f]..][0..dst_cap[f]]; result[f] = what compressFrameDevice / decompressFrameDevice return for it
    /// (size, or a negative code).  Device pointers; asynchronous on `stream`; `workspace` = device memory of the size the
    /// workspace function gives.
    pub const BATCH_CONTENT_SIZE: u32 = 1;
    /// compressFrameBatch: block k against the 64 KiB of input in front of it (fast level, block_mode linked; the
    /// workspace comes from compressFrameBatchWorkspaceEx).  compressFrameBatchEx also links at the HC levels 3..9
    /// (block k = compressHCUsingDict against that input).  No counterpart in the reference.
    pub const BATCH_LINK_BLOCKS: u32 = 4;
    /// decode flag of the ...Ex calls: a frame whose FLG declares linked blocks is decoded in block order, block k
    /// against the 64 KiB of output in front of it (liblz4's default frames).  The segment calls have no such form: a
    /// rank's first block would need the previous rank's output.
    pub const DECODE_LINKED: u32 = 1;
    pub const Frames = struct {
        src: [*]const u8,
        src_off: [*]const u64,
        src_len: [*]const u64,
        dst: [*]u8,
        dst_off: [*]const u64,
        dst_cap: [*]const u64,
        result: [*]i64,
        nframes: u32,
    };
    fn mapBatch(rc: i32) (Error || root.Error)!void {
        if (rc == 0) return;
        if (rc == -104) return error.ParameterInvalid;
        _ = try mapBlock(rc);
    }
    pub fn compressFrameBatchWorkspace(nframes: u32, max_blocks: u32, prefs: ?Preferences) usize {
        if (prefs) |p| { const c = toC(p); return zlz4f_batch_compress_frame_workspace(nframes, max_blocks, &c); }
        return zlz4f_batch_compress_frame_workspace(nframes, max_blocks, null);
    }
    pub fn compressFrameBatch(stream: ?*anyopaque, f: Frames, max_blocks: u32, prefs: ?Preferences, batch_flags: u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        if (prefs) |p| {
            const c = toC(p);
            return mapBatch(zlz4f_batch_compress_frame(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, max_blocks, &c, batch_flags, workspace, workspace_bytes));
        }
        return mapBatch(zlz4f_batch_compress_frame(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, max_blocks, null, batch_flags, workspace, workspace_bytes));
    }
    pub fn decompressFrameBatchWorkspace(nframes: u32, max_blocks: u32) usize {
        return zlz4f_batch_decompress_frame_workspace(nframes, max_blocks);
    }
    pub fn decompressFrameBatch(stream: ?*anyopaque, f: Frames, max_blocks: u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_decompress_frame(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, max_blocks, workspace, workspace_bytes));
    }
    pub fn compressFrameBatchWorkspaceEx(nframes: u32, max_blocks: u32, prefs: ?Preferences, batch_flags: u32) usize {
        if (prefs) |p| { const c = toC(p); return zlz4f_batch_compress_frame_workspace_ex(nframes, max_blocks, &c, batch_flags); }
        return zlz4f_batch_compress_frame_workspace_ex(nframes, max_blocks, null, batch_flags);
    }
    /// compressFrameBatch, and BATCH_LINK_BLOCKS at the HC levels 3..9 (levels 2 and 10..12 with the flag: Unsupported)
    pub fn compressFrameBatchEx(stream: ?*anyopaque, f: Frames, max_blocks: u32, prefs: ?Preferences, batch_flags: u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        if (prefs) |p| {
            const c = toC(p);
            return mapBatch(zlz4f_batch_compress_frame_ex(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, max_blocks, &c, batch_flags, workspace, workspace_bytes));
        }
        return mapBatch(zlz4f_batch_compress_frame_ex(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, max_blocks, null, batch_flags, workspace, workspace_bytes));
    }
    /// one frame through compressFrameBatchEx; batch_flags 0: the answer of compressFrame / compressFrameDevice
    pub fn compressFrameEx(src: []const u8, dst: []u8, prefs: ?Preferences, batch_flags: u32) Error!usize {
        if (prefs) |p| { const c = toC(p); return mapFrame(zlz4f_compress_frame_ex(src.ptr, src.len, dst.ptr, dst.len, &c, batch_flags)); }
        return mapFrame(zlz4f_compress_frame_ex(src.ptr, src.len, dst.ptr, dst.len, null, batch_flags));
    }
    pub fn compressFrameDeviceEx(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize, prefs: ?Preferences, batch_flags: u32) Error!usize {
        if (prefs) |p| { const c = toC(p); return mapFrame(zlz4f_compress_frame_device_ex(stream, d_src, src_len, d_dst, dst_cap, &c, batch_flags)); }
        return mapFrame(zlz4f_compress_frame_device_ex(stream, d_src, src_len, d_dst, dst_cap, null, batch_flags));
    }
    pub fn decompressFrameBatchWorkspaceEx(nframes: u32, max_blocks: u32, decode_flags: u32) usize {
        return zlz4f_batch_decompress_frame_workspace_ex(nframes, max_blocks, decode_flags);
    }
    pub fn decompressFrameBatchEx(stream: ?*anyopaque, f: Frames, max_blocks: u32, decode_flags: u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_decompress_frame_ex(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, max_blocks, decode_flags, workspace, workspace_bytes));
    }
    pub fn frameDecompressedSizeBatchWorkspaceEx(nframes: u32, max_blocks: u32, decode_flags: u32) usize {
        return zlz4f_batch_frame_decompressed_size_workspace_ex(nframes, max_blocks, decode_flags);
    }
    pub fn frameDecompressedSizeBatchEx(stream: ?*anyopaque, src: [*]const u8, src_off: [*]const u64, src_len: [*]const u64, size: [*]i64, nframes: u32, max_blocks: u32, decode_flags: u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_frame_decompressed_size_ex(stream, src, src_off, src_len, size, nframes, max_blocks, decode_flags, workspace, workspace_bytes));
    }
    pub fn decompressFrameEx(src: []const u8, dst: []u8, decode_flags: u32) Error!usize {
        return mapFrame(zlz4f_decompress_frame_ex(src.ptr, src.len, dst.ptr, dst.len, decode_flags));
    }
    pub fn decompressFrameDeviceEx(stream: ?*anyopaque, d_src: [*]const u8, src_len: usize, d_dst: [*]u8, dst_cap: usize, decode_flags: u32) Error!usize {
        return mapFrame(zlz4f_decompress_frame_device_ex(stream, d_src, src_len, d_dst, dst_cap, decode_flags));
    }
    pub fn frameDecompressedSizeEx(src: []const u8, decode_flags: u32) Error!usize {
        return mapFrame(zlz4f_frame_decompressed_size_ex(src.ptr, src.len, decode_flags));
    }
    // dictionary frames (include/zlz4_amd.h): dictionary d = dict[off[d] .. off[d] + len[d]), frame f uses dictionary
    // idx[f] (idx null: dictionary 0 for every frame).  Fast level only; prefs.block_mode says linked or independent.
    pub const Dicts = struct {
        dict: ?[*]const u8,
        off: [*]const u64,
        len: [*]const u32,
        ndicts: u32,
        idx: ?[*]const u32,
    };
    pub fn compressFrameBatchUsingDictWorkspace(nframes: u32, max_blocks: u32, prefs: ?Preferences, batch_flags: u32, ndicts: u32, max_src_len: u64, max_dict_len: u32) usize {
        if (prefs) |p| { const c = toC(p); return zlz4f_batch_compress_frame_using_dict_workspace(nframes, max_blocks, &c, batch_flags, ndicts, max_src_len, max_dict_len); }
        return zlz4f_batch_compress_frame_using_dict_workspace(nframes, max_blocks, null, batch_flags, ndicts, max_src_len, max_dict_len);
    }
    pub fn compressFrameBatchUsingDict(stream: ?*anyopaque, f: Frames, max_blocks: u32, prefs: ?Preferences, batch_flags: u32, d: Dicts, max_src_len: u64, max_dict_len: u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        if (prefs) |p| {
            const c = toC(p);
            return mapBatch(zlz4f_batch_compress_frame_using_dict(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, max_blocks, &c, batch_flags, d.dict, d.off, d.len, d.ndicts, d.idx, max_src_len, max_dict_len, workspace, workspace_bytes));
        }
        return mapBatch(zlz4f_batch_compress_frame_using_dict(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, max_blocks, null, batch_flags, d.dict, d.off, d.len, d.ndicts, d.idx, max_src_len, max_dict_len, workspace, workspace_bytes));
    }
    // the same calls, and prefs.compression_level 3..9 (HC blocks against the dictionary; include/zlz4_amd.h); at those levels
    // max_dict_len changes the workspace size
    pub fn compressFrameBatchUsingDictWorkspaceEx(nframes: u32, max_blocks: u32, prefs: ?Preferences, batch_flags: u32, ndicts: u32, max_src_len: u64, max_dict_len: u32) usize {
        if (prefs) |p| { const c = toC(p); return zlz4f_batch_compress_frame_using_dict_workspace_ex(nframes, max_blocks, &c, batch_flags, ndicts, max_src_len, max_dict_len); }
        return zlz4f_batch_compress_frame_using_dict_workspace_ex(nframes, max_blocks, null, batch_flags, ndicts, max_src_len, max_dict_len);
    }
    pub fn compressFrameBatchUsingDictEx(stream: ?*anyopaque, f: Frames, max_blocks: u32, prefs: ?Preferences, batch_flags: u32, d: Dicts, max_src_len: u64, max_dict_len: u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        if (prefs) |p| {
            const c = toC(p);
            return mapBatch(zlz4f_batch_compress_frame_using_dict_ex(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, max_blocks, &c, batch_flags, d.dict, d.off, d.len, d.ndicts, d.idx, max_src_len, max_dict_len, workspace, workspace_bytes));
        }
        return mapBatch(zlz4f_batch_compress_frame_using_dict_ex(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, max_blocks, null, batch_flags, d.dict, d.off, d.len, d.ndicts, d.idx, max_src_len, max_dict_len, workspace, workspace_bytes));
    }
    pub fn decompressFrameBatchUsingDictWorkspace(nframes: u32, max_blocks: u32) usize {
        return zlz4f_batch_decompress_frame_using_dict_workspace(nframes, max_blocks);
    }
    pub fn decompressFrameBatchUsingDict(stream: ?*anyopaque, f: Frames, max_blocks: u32, d: Dicts, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_decompress_frame_using_dict(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, max_blocks, d.dict, d.off, d.len, d.ndicts, d.idx, workspace, workspace_bytes));
    }
    pub fn frameDecompressedSizeBatchUsingDictWorkspace(nframes: u32, max_blocks: u32) usize {
        return zlz4f_batch_frame_decompressed_size_using_dict_workspace(nframes, max_blocks);
    }
    pub fn frameDecompressedSizeBatchUsingDict(stream: ?*anyopaque, src: [*]const u8, src_off: [*]const u64, src_len: [*]const u64, size: [*]i64, nframes: u32, max_blocks: u32, dict_len: [*]const u32, ndicts: u32, dict_idx: ?[*]const u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_frame_decompressed_size_using_dict(stream, src, src_off, src_len, size, nframes, max_blocks, dict_len, ndicts, dict_idx, workspace, workspace_bytes));
    }
    /// dict_id[f] = the header's dictID, 0 when the frame has none, or the header's error code
    pub fn frameDictIDBatch(stream: ?*anyopaque, src: [*]const u8, src_off: [*]const u64, src_len: [*]const u64, dict_id: [*]i64, nframes: u32) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_frame_dict_id(stream, src, src_off, src_len, dict_id, nframes));
    }
    pub fn compressFrameUsingDict(src: []const u8, dst: []u8, prefs: ?Preferences, dict: []const u8) Error!usize {
        if (prefs) |p| { const c = toC(p); return mapFrame(zlz4f_compress_frame_using_dict(src.ptr, src.len, dst.ptr, dst.len, &c, dict.ptr, dict.len)); }
        return mapFrame(zlz4f_compress_frame_using_dict(src.ptr, src.len, dst.ptr, dst.len, null, dict.ptr, dict.len));
    }
    pub fn compressFrameUsingDictEx(src: []const u8, dst: []u8, prefs: ?Preferences, dict: []const u8) Error!usize {
        if (prefs) |p| { const c = toC(p); return mapFrame(zlz4f_compress_frame_using_dict_ex(src.ptr, src.len, dst.ptr, dst.len, &c, dict.ptr, dict.len)); }
        return mapFrame(zlz4f_compress_frame_using_dict_ex(src.ptr, src.len, dst.ptr, dst.len, null, dict.ptr, dict.len));
    }
    pub fn decompressFrameUsingDict(src: []const u8, dst: []u8, dict: []const u8) Error!usize {
        return mapFrame(zlz4f_decompress_frame_using_dict(src.ptr, src.len, dst.ptr, dst.len, dict.ptr, dict.len));
    }
    /// No counterpart in the reference: the first dst.len bytes of the frame's content (all of it where the frame holds
    /// fewer), history-aware; a defect behind the cut is not reported (include/zlz4_amd.h, frame prefix decoding).
    /// Returns min(content size, dst.len).
    pub fn decompressFramePrefix(src: []const u8, dst: []u8) Error!usize {
        return mapFrame(zlz4f_decompress_frame_prefix(src.ptr, src.len, dst.ptr, dst.len));
    }
    /// decompressFramePrefix with the frame's dictionary, as decompressFrameUsingDict
    pub fn decompressFramePrefixUsingDict(src: []const u8, dst: []u8, dict: []const u8) Error!usize {
        return mapFrame(zlz4f_decompress_frame_prefix_using_dict(src.ptr, src.len, dst.ptr, dst.len, dict.ptr, dict.len));
    }
    /// batch forms: f.dst_cap[i] is the number of bytes wanted of frame i and the size of its slot; one launch, no
    /// workspace, no max_blocks
    pub fn decompressFramePrefixBatch(stream: ?*anyopaque, f: Frames) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_decompress_frame_prefix(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes));
    }
    pub fn decompressFramePrefixBatchUsingDict(stream: ?*anyopaque, f: Frames, d: Dicts) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_decompress_frame_prefix_using_dict(stream, f.src, f.src_off, f.src_len, f.dst, f.dst_off, f.dst_cap, f.result, f.nframes, d.dict, d.off, d.len, d.ndicts, d.idx));
    }
    /// No counterpart in the reference: the frame index and range decoding (include/zlz4_amd.h).  frameIndexBatch keeps the
    /// size query's per-block sizes as (pos, dec) entries; planFrameRanges sizes slots and items from the index alone;
    /// decompressFrameRangeBatch decodes only the blocks that overlap [a, b): range r's bytes stand at dst + dst_off[r] +
    /// skip[r].  The index is the caller's data and is checked against the frame.
    pub fn frameIndexBatchWorkspace(nframes: u32, max_blocks: u32) usize {
        return zlz4f_batch_frame_index_workspace(nframes, max_blocks);
    }
    pub fn frameIndexBatch(stream: ?*anyopaque, src: [*]const u8, src_off: [*]const u64, src_len: [*]const u64, index: [*]IndexEntry, idx_off: [*]const u64, idx_cap: [*]const u64, idx_n: [*]i64, nframes: u32, max_blocks: u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_frame_index(stream, src, src_off, src_len, index, idx_off, idx_cap, idx_n, nframes, max_blocks, workspace, workspace_bytes));
    }
    pub fn planFrameRanges(stream: ?*anyopaque, index: [*]const IndexEntry, idx_off: [*]const u64, idx_n: [*]const i64, nframes: u32, ranges: [*]const Range, nranges: u32, alignment: u32, dst_off: [*]u64, dst_cap: [*]u64, totals: [*]u64) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_plan_frame_ranges(stream, index, idx_off, idx_n, nframes, ranges, nranges, alignment, dst_off, dst_cap, totals));
    }
    pub fn decompressFrameRangeBatchWorkspace(nranges: u32, max_items: u32) usize {
        return zlz4f_batch_decompress_frame_range_workspace(nranges, max_items);
    }
    pub fn decompressFrameRangeBatch(stream: ?*anyopaque, src: [*]const u8, src_off: [*]const u64, src_len: [*]const u64, index: [*]const IndexEntry, idx_off: [*]const u64, idx_n: [*]const i64, nframes: u32, ranges: [*]const Range, dst: [*]u8, dst_off: [*]const u64, dst_cap: [*]const u64, skip: [*]u64, result: [*]i64, nranges: u32, max_items: u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_decompress_frame_range(stream, src, src_off, src_len, index, idx_off, idx_n, nframes, ranges, dst, dst_off, dst_cap, skip, result, nranges, max_items, workspace, workspace_bytes));
    }
    /// bytes [a, b) of one frame in host memory (both clamped to the frame's size) at dst[0..]; builds the index on every call
    pub fn decompressFrameRange(src: []const u8, a: u64, b: u64, dst: []u8) Error!usize {
        return mapFrame(zlz4f_decompress_frame_range(src.ptr, src.len, a, b, dst.ptr, dst.len));
    }
    /// No counterpart in the reference: multiframe buffers, frames and skippable frames back to back as in a .lz4 file
    /// (include/zlz4_amd.h).  multiframeSplitBatch delimits the members of every buffer (member == null: count mode) and
    /// writes them as the items of frameDecompressedSizeBatchEx / decompressFrameBatchEx; multiframePlanBatch packs a
    /// buffer's items into one run of bytes; multiframeFinishBatch folds the item results: the first member that is not OK
    /// decides, else the decoded size.  Whatever the split cannot delimit is the last member and reaches to the end.
    pub const MEMBER_FRAME: u32 = 1;
    pub const MEMBER_SKIPPABLE: u32 = 2;
    pub const MEMBER_SKIPPABLE_TRUNCATED: u32 = 3;
    pub fn multiframeSplitBatch(stream: ?*anyopaque, src: ?[*]const u8, src_off: ?[*]const u64, src_len: ?[*]const u64, nbuf: u32, count: ?[*]u64, totals: [*]u64, member: ?[*]Member, mem_off: ?[*]const u64, mem_cap: ?[*]const u64, item_first: ?[*]u64, item_off: ?[*]u64, item_len: ?[*]u64, result: ?[*]i64) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_multiframe_split(stream, src, src_off, src_len, nbuf, count, totals, member, mem_off, mem_cap, item_first, item_off, item_len, result));
    }
    pub fn multiframePlanBatch(stream: ?*anyopaque, size: ?[*]const i64, item_first: ?[*]const u64, nbuf: u32, alignment: u32, dst_off: ?[*]u64, dst_cap: ?[*]u64, out_off: ?[*]u64, out_size: ?[*]u64, totals: [*]u64) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_multiframe_plan(stream, size, item_first, nbuf, alignment, dst_off, dst_cap, out_off, out_size, totals));
    }
    pub fn multiframeFinishBatch(stream: ?*anyopaque, member: ?[*]const Member, mem_off: ?[*]const u64, split_result: ?[*]const i64, item_first: ?[*]const u64, size: ?[*]const i64, item_result: ?[*]const i64, nbuf: u32, result: ?[*]i64) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_multiframe_finish(stream, member, mem_off, split_result, item_first, size, item_result, nbuf, result));
    }
    /// one buffer in host memory: the sum of its members' decoded sizes (content checksums set aside) / its content at dst
    pub fn multiframeDecompressedSize(src: []const u8, decode_flags: u32) Error!usize {
        return mapFrame(zlz4f_multiframe_decompressed_size(src.ptr, src.len, decode_flags));
    }
    pub fn decompressMultiframe(src: []const u8, dst: []u8, decode_flags: u32) Error!usize {
        return mapFrame(zlz4f_decompress_multiframe(src.ptr, src.len, dst.ptr, dst.len, decode_flags));
    }
    /// Whole .lz4 files: with SPLIT_LEGACY in split_flags a legacy frame is a member too (kind MEMBER_LEGACY).  The split
    /// writes its length to leg_len (0 in item_len), totals has four entries (members, frame chain blocks, legacy members,
    /// legacy blocks), the batch legacy frame calls run over (item_off, leg_len) beside the frame calls, and
    /// multiframeSelectBatch takes the legacy call's answer for every legacy member's item.  split_flags 0: the calls above.
    pub const SPLIT_LEGACY: u32 = 1;
    pub const MEMBER_LEGACY: u32 = 4;
    pub fn multiframeSplitBatchEx(stream: ?*anyopaque, src: ?[*]const u8, src_off: ?[*]const u64, src_len: ?[*]const u64, nbuf: u32, count: ?[*]u64, totals: [*]u64, member: ?[*]Member, mem_off: ?[*]const u64, mem_cap: ?[*]const u64, item_first: ?[*]u64, item_off: ?[*]u64, item_len: ?[*]u64, result: ?[*]i64, split_flags: u32, leg_len: ?[*]u64) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_multiframe_split_ex(stream, src, src_off, src_len, nbuf, count, totals, member, mem_off, mem_cap, item_first, item_off, item_len, result, split_flags, leg_len));
    }
    pub fn multiframeSelectBatch(stream: ?*anyopaque, member: ?[*]const Member, mem_off: ?[*]const u64, split_result: ?[*]const i64, item_first: ?[*]const u64, from_frame: ?[*]const i64, from_legacy: ?[*]const i64, nbuf: u32, out: ?[*]i64) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_multiframe_select(stream, member, mem_off, split_result, item_first, from_frame, from_legacy, nbuf, out));
    }
    pub fn multiframeDecompressedSizeEx(src: []const u8, decode_flags: u32, split_flags: u32) Error!usize {
        return mapFrame(zlz4f_multiframe_decompressed_size_ex(src.ptr, src.len, decode_flags, split_flags));
    }
    pub fn decompressMultiframeEx(src: []const u8, dst: []u8, decode_flags: u32, split_flags: u32) Error!usize {
        return mapFrame(zlz4f_decompress_multiframe_ex(src.ptr, src.len, dst.ptr, dst.len, decode_flags, split_flags));
    }
    /// what `lz4 -dc` prints for the .lz4 file `src`: linked-block frames, skippable frames and legacy frames included
    pub fn decompressFile(src: []const u8, dst: []u8) Error!usize {
        return decompressMultiframeEx(src, dst, DECODE_LINKED, SPLIT_LEGACY);
    }
    /// No counterpart in the reference: the file index and file range decoding, bytes [a, b) of whole .lz4 files
    /// (include/zlz4_amd.h).  fileIndexBatch is the frame index across the members of a record-mode split (split_totals: a
    /// host pointer to the split's four totals) and writes idx_off itself; the plan is planFrameRanges with nframes = the
    /// buffers; decompressFileRangeBatch is decompressFrameRangeBatch whose items each find their own member, so a range may
    /// cross frame, skippable and legacy members.  The index is the caller's data and is checked against the file.
    pub fn fileIndexBatchWorkspace(nbuf: u32, split_totals: [*]const u64) usize {
        return zlz4f_batch_file_index_workspace(nbuf, split_totals);
    }
    pub fn fileIndexBatch(stream: ?*anyopaque, src: ?[*]const u8, src_off: ?[*]const u64, src_len: ?[*]const u64, nbuf: u32, member: ?[*]const Member, mem_off: ?[*]const u64, split_result: ?[*]const i64, item_first: ?[*]const u64, item_off: ?[*]const u64, item_len: ?[*]const u64, leg_len: ?[*]const u64, split_totals: [*]const u64, index: ?[*]IndexEntry, idx_off: ?[*]u64, idx_cap: u64, idx_n: ?[*]i64, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_file_index(stream, src, src_off, src_len, nbuf, member, mem_off, split_result, item_first, item_off, item_len, leg_len, split_totals, index, idx_off, idx_cap, idx_n, workspace, workspace_bytes));
    }
    pub fn decompressFileRangeBatchWorkspace(nranges: u32, max_items: u32) usize {
        return zlz4f_batch_decompress_file_range_workspace(nranges, max_items);
    }
    pub fn decompressFileRangeBatch(stream: ?*anyopaque, src: [*]const u8, src_off: [*]const u64, src_len: [*]const u64, index: [*]const IndexEntry, idx_off: [*]const u64, idx_n: [*]const i64, nbuf: u32, member: [*]const Member, mem_off: [*]const u64, split_result: [*]const i64, ranges: [*]const Range, dst: [*]u8, dst_off: [*]const u64, dst_cap: [*]const u64, skip: [*]u64, result: [*]i64, nranges: u32, max_items: u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_decompress_file_range(stream, src, src_off, src_len, index, idx_off, idx_n, nbuf, member, mem_off, split_result, ranges, dst, dst_off, dst_cap, skip, result, nranges, max_items, workspace, workspace_bytes));
    }
    /// bytes [a, b) of one .lz4 file in host memory (both clamped to the file's size) at dst[0..]; builds the index on every call
    pub fn decompressFileRange(src: []const u8, a: u64, b: u64, dst: []u8) Error!usize {
        return mapFrame(zlz4f_decompress_file_range(src.ptr, src.len, a, b, dst.ptr, dst.len, SPLIT_LEGACY));
    }
    /// No counterpart in the reference: seekable files (include/zlz4_amd.h).  A SEEK TABLE is the last, skippable member of
    /// a file (magic 0x184D2A5C) and stores the file's member rows and index entries.  appendSeekTableBatch writes it
    /// behind every buffer from the split and the file index; loadSeekTableBatch reads both tables back from the file's
    /// tail (count mode: member null) and checks their shape only -- the range call stays the judge; concatBatch lays items
    /// back to back, file by file.
    pub const SEEK_TABLE_MAGICNUMBER: u32 = 0x184D2A5C;
    pub const RANGE_SEEK_TABLE: u32 = 1;
    pub fn seekTableBound(nmembers: u64, nblocks: u64) usize {
        return zlz4f_seek_table_bound(nmembers, nblocks);
    }
    pub fn appendSeekTableBatch(stream: ?*anyopaque, buf: ?[*]u8, buf_off: ?[*]const u64, buf_len: ?[*]const u64, buf_cap: ?[*]const u64, nbuf: u32, member: ?[*]const Member, mem_off: ?[*]const u64, split_result: ?[*]const i64, index: ?[*]const IndexEntry, idx_off: ?[*]const u64, idx_n: ?[*]const i64, result: ?[*]i64) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_append_seek_table(stream, buf, buf_off, buf_len, buf_cap, nbuf, member, mem_off, split_result, index, idx_off, idx_n, result));
    }
    pub fn loadSeekTableBatch(stream: ?*anyopaque, src: ?[*]const u8, src_off: ?[*]const u64, src_len: ?[*]const u64, nbuf: u32, count: ?[*]u64, totals: [*]u64, member: ?[*]Member, mem_off: ?[*]const u64, mem_cap: ?[*]const u64, split_result: ?[*]i64, index: ?[*]IndexEntry, idx_off: ?[*]u64, idx_cap: u64, idx_n: ?[*]i64) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_load_seek_table(stream, src, src_off, src_len, nbuf, count, totals, member, mem_off, mem_cap, split_result, index, idx_off, idx_cap, idx_n));
    }
    pub fn concatBatchWorkspace(nitems: u32) usize {
        return zlz4f_batch_concat_workspace(nitems);
    }
    pub fn concatBatch(stream: ?*anyopaque, src: ?[*]const u8, item_off: ?[*]const u64, item_len: ?[*]const i64, item_first: ?[*]const u64, nbuf: u32, nitems: u32, dst: ?[*]u8, dst_off: ?[*]const u64, dst_cap: ?[*]const u64, result: ?[*]i64, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_concat(stream, src, item_off, item_len, item_first, nbuf, nitems, dst, dst_off, dst_cap, result, workspace, workspace_bytes));
    }
    /// the seek table member of one .lz4 file in host memory at dst[0..]; the caller appends it to the file
    pub fn seekTable(src: []const u8, dst: []u8) Error!usize {
        return mapFrame(zlz4f_seek_table(src.ptr, src.len, dst.ptr, dst.len, SPLIT_LEGACY));
    }
    /// decompressFileRange that takes the tables from the file's seek table where it ends in a well-formed one
    pub fn decompressFileRangeEx(src: []const u8, a: u64, b: u64, dst: []u8, range_flags: u32) Error!usize {
        return mapFrame(zlz4f_decompress_file_range_ex(src.ptr, src.len, a, b, dst.ptr, dst.len, SPLIT_LEGACY, range_flags));
    }
    /// No counterpart in the reference: dictionary files (include/zlz4_amd.h) -- the file calls with ONE DICTIONARY PER
    /// FILE: dict_idx has one entry per buffer (null: dictionary 0).  Every block of a member that declares independent
    /// blocks sees the dictionary's last 64 KiB, block 0 of one that declares linked blocks, no block of a legacy member.
    /// The index call needs the lengths alone; multiframeItemDictsBatch spreads the per-buffer index over the items of a
    /// split, for the dictionary frame calls.
    pub fn fileIndexUsingDictBatchWorkspace(nbuf: u32, split_totals: [*]const u64) usize {
        return zlz4f_batch_file_index_using_dict_workspace(nbuf, split_totals);
    }
    pub fn fileIndexUsingDictBatch(stream: ?*anyopaque, src: ?[*]const u8, src_off: ?[*]const u64, src_len: ?[*]const u64, nbuf: u32, member: ?[*]const Member, mem_off: ?[*]const u64, split_result: ?[*]const i64, item_first: ?[*]const u64, item_off: ?[*]const u64, item_len: ?[*]const u64, leg_len: ?[*]const u64, split_totals: [*]const u64, index: ?[*]IndexEntry, idx_off: ?[*]u64, idx_cap: u64, idx_n: ?[*]i64, dict_len: ?[*]const u32, ndicts: u32, dict_idx: ?[*]const u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_file_index_using_dict(stream, src, src_off, src_len, nbuf, member, mem_off, split_result, item_first, item_off, item_len, leg_len, split_totals, index, idx_off, idx_cap, idx_n, dict_len, ndicts, dict_idx, workspace, workspace_bytes));
    }
    pub fn decompressFileRangeUsingDictBatchWorkspace(nranges: u32, max_items: u32) usize {
        return zlz4f_batch_decompress_file_range_using_dict_workspace(nranges, max_items);
    }
    pub fn decompressFileRangeUsingDictBatch(stream: ?*anyopaque, src: [*]const u8, src_off: [*]const u64, src_len: [*]const u64, index: [*]const IndexEntry, idx_off: [*]const u64, idx_n: [*]const i64, nbuf: u32, member: [*]const Member, mem_off: [*]const u64, split_result: [*]const i64, ranges: [*]const Range, dst: [*]u8, dst_off: [*]const u64, dst_cap: [*]const u64, skip: [*]u64, result: [*]i64, nranges: u32, max_items: u32, dict: ?[*]const u8, dict_off: ?[*]const u64, dict_len: ?[*]const u32, ndicts: u32, dict_idx: ?[*]const u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_decompress_file_range_using_dict(stream, src, src_off, src_len, index, idx_off, idx_n, nbuf, member, mem_off, split_result, ranges, dst, dst_off, dst_cap, skip, result, nranges, max_items, dict, dict_off, dict_len, ndicts, dict_idx, workspace, workspace_bytes));
    }
    pub fn multiframeItemDictsBatch(stream: ?*anyopaque, item_first: ?[*]const u64, nbuf: u32, nitems: u32, dict_idx: ?[*]const u32, item_dict_idx: ?[*]u32) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_multiframe_item_dicts(stream, item_first, nbuf, nitems, dict_idx, item_dict_idx));
    }
    /// decompressFileRangeEx for a file that was written against `dict` (only its last 64 KiB are staged)
    pub fn decompressFileRangeUsingDict(src: []const u8, a: u64, b: u64, dst: []u8, range_flags: u32, dict: []const u8) Error!usize {
        return mapFrame(zlz4f_decompress_file_range_using_dict(src.ptr, src.len, a, b, dst.ptr, dst.len, SPLIT_LEGACY, range_flags, dict.ptr, dict.len));
    }
    /// No counterpart in the reference: legacy frames, what `lz4 -l` writes and the Linux kernel's unlz4 reads -- the magic
    /// 0x184C2102, then { u32 size, block } repeated (include/zlz4_amd.h).  One frame in host memory per call; `consumed`
    /// receives where the frame ends, which is where the next member of a concatenated file starts.
    pub const legacy = struct {
        pub const MAGICNUMBER: u32 = 0x184C2102;
        pub const BLOCK_SIZE: u32 = 8 << 20;
        pub const BLOCK_BOUND: u32 = 8421520;
        pub const Prefs = LegacyPrefs;
        /// 0 for a block_size above 8 MiB
        pub fn compressFrameBound(src_size: usize, prefs: ?Prefs) usize {
            if (prefs) |p| return zlz4f_legacy_compress_frame_bound(src_size, &p);
            return zlz4f_legacy_compress_frame_bound(src_size, null);
        }
        pub fn compressFrame(src: []const u8, dst: []u8, prefs: ?Prefs) Error!usize {
            if (prefs) |p| return mapFrame(zlz4f_compress_legacy_frame(src.ptr, src.len, dst.ptr, dst.len, &p));
            return mapFrame(zlz4f_compress_legacy_frame(src.ptr, src.len, dst.ptr, dst.len, null));
        }
        pub fn frameDecompressedSize(src: []const u8, consumed: ?*usize) Error!usize {
            return mapFrame(zlz4f_legacy_frame_decompressed_size(src.ptr, src.len, consumed));
        }
        pub fn decompressFrame(src: []const u8, dst: []u8, consumed: ?*usize) Error!usize {
            return mapFrame(zlz4f_decompress_legacy_frame(src.ptr, src.len, dst.ptr, dst.len, consumed));
        }
    };
    pub fn frameDecompressedSizeUsingDict(src: []const u8, dict_len: usize) Error!usize {
        return mapFrame(zlz4f_frame_decompressed_size_using_dict(src.ptr, src.len, dict_len));
    }
    pub fn frameDecompressedSizeBatchWorkspace(nframes: u32, max_blocks: u32) usize {
        return zlz4f_batch_frame_decompressed_size_workspace(nframes, max_blocks);
    }
    /// size[f] = what decompressFrameBatch stores in result[f] when dst_cap[f] is large enough (content checksum aside)
    pub fn frameDecompressedSizeBatch(stream: ?*anyopaque, src: [*]const u8, src_off: [*]const u64, src_len: [*]const u64, size: [*]i64, nframes: u32, max_blocks: u32, workspace: ?*anyopaque, workspace_bytes: usize) (Error || root.Error)!void {
        return mapBatch(zlz4f_batch_frame_decompressed_size(stream, src, src_off, src_len, size, nframes, max_blocks, workspace, workspace_bytes));
    }
};
