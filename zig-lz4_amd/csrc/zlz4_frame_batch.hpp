// zlz4_frame_batch.hpp -- the per-frame record and the block flags of the batch frame calls,
// shared by zlz4_frame.hip (the pipeline) and zlz4_frame_linked.hip (the linked-block kernels of section 4.4c).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t kNoFrame = 0xFFFFFFFFu;
constexpr uint32_t kBlkStored = 1u, kBlkNoCks = 2u, kBlkCks = 4u;   // block flags (decompress table)

struct BFrame {
    uint64_t nb;        // block count: ceil(len / bs) (compress), what the block chain holds (decompress)
    uint64_t base;      // first table entry (exclusive scan of nb)
    int64_t status;     // compress: 0, DstMaxSizeTooSmall or SrcSizeTooLarge; decompress: header size or header error
    uint64_t end;       // compress: frame bytes in front of the end mark; decompress: srcPos after the walk
    int64_t err;        // compress: first failing block's code; decompress: the walk's error, then the plan's
    uint64_t total;     // decompress: decoded bytes
    uint64_t bs;        // decompress: block size from BD
    uint32_t flg;       // decompress: FLG
    uint32_t proven;    // decompress: 1 = the speculative layout is proven
};

__device__ __forceinline__ bool bf_fits(const BFrame &F, uint32_t max_blocks) { return F.nb == 0 || F.base + F.nb <= max_blocks; }

// Dictionary frames: which frames the one-wavefront decoder takes.  A linked-declared frame of one
// block has T alone as its history -- what the block of an independent frame sees -- so it stays on the parallel decodes
// (the default preferences write such frames for small records).
__device__ __forceinline__ bool bfd_dict_serial(const BFrame &F) { return !(F.flg & 0x20u) && F.nb > 1; }

}  // namespace
