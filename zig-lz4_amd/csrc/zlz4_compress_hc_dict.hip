// zlz4_compress_hc_dict.hip -- the staging pass of zlz4_batch_compress_hc_using_dict (include/zlz4_amd.h; DESIGN.md
// section 4.3c).  The HC pipeline (zlz4_compress_hc.hip) addresses the bytes of a block as src + position, and the
// dictionary call is that pipeline on V = last min(dict_len, 65536) bytes of the dictionary ++ record: this kernel makes
// V contiguous in the workspace, so that the three kernels need nothing but where the record starts in it.
#include "zlz4_device.hpp"
#include "zlz4_launch.hpp"

namespace zlz4 {

constexpr uint32_t kHcDictRefused = 0xFFFFFFFFu, kHcDictTooLarge = 0xFFFFFFFEu;   // as in zlz4_compress_hc.hip

// One workgroup per block.  slot = slot0 + b: V of block blk0 + b goes to d_v + slot * v_stride (16-byte aligned).
// Writes v_off[blk], v_len[blk] = D + n (K1 reads these) and the pair { D + n, D } (K2s, K3).  A block that the call
// refuses -- its record over ZLZ4_MAX_INPUT_SIZE, over max_in_len, its tail over dmax -- gets an empty V and its reason
// in place of D; nothing of it is read.
__global__ __launch_bounds__(256) void k_hc_dict_stage(const uint8_t *__restrict__ d_in, const uint64_t *__restrict__ d_in_off,
                                                        const uint32_t *__restrict__ d_in_len, const uint8_t *d_dict,
                                                        const uint64_t *__restrict__ d_dict_off,
                                                        const uint32_t *__restrict__ d_dict_len, uint8_t *__restrict__ d_v,
                                                        uint64_t v_stride, uint64_t *__restrict__ v_off,
                                                        uint32_t *__restrict__ v_len, uint32_t *__restrict__ v_pair,
                                                        uint32_t blk0, uint32_t nblocks, uint32_t slot0, uint32_t max_in_len,
                                                        uint32_t dmax) {
    const uint32_t b = blockIdx.x;
    if (b >= nblocks) return;
    const uint32_t blk = blk0 + b;
    const uint32_t n = d_in_len[blk];
    const uint32_t dl = d_dict_len[blk];
    const uint32_t D = dl < 65536u ? dl : 65536u;
    const uint64_t off = (uint64_t)(slot0 + b) * v_stride;
    const bool too_large = n > kMaxInput;                                 // src/lz4hc.zig:1442
    const bool refused = too_large || n > max_in_len || D > dmax;
    if (threadIdx.x == 0) {
        v_off[blk] = off;
        v_len[blk] = refused ? 0u : D + n;
        v_pair[2u * blk] = refused ? 0u : D + n;
        v_pair[2u * blk + 1u] = too_large ? kHcDictTooLarge : refused ? kHcDictRefused : D;
    }
    if (refused) return;
    uint8_t *v = d_v + off;
    const uint8_t *rec = d_in + d_in_off[blk];
    const uint8_t *tail = D ? d_dict + d_dict_off[blk] + (dl - D) : rec;  // (no dictionary: d_dict may be null)
    const uint32_t N = D + n;
    // 16 bytes of V per lane and step: a chunk that lies in the tail or in the record is one load and one aligned store
    for (uint32_t k = threadIdx.x * 16u; k < N; k += 256u * 16u) {
        if (k + 16u <= D) st128(v + k, ld128(tail + k));
        else if (k >= D && k + 16u <= N) st128(v + k, ld128(rec + (k - D)));
        else {
            const uint32_t e = k + 16u < N ? k + 16u : N;
            for (uint32_t q = k; q < e; q++) v[q] = q < D ? tail[q] : rec[q - D];
        }
    }
}

}  // namespace zlz4

extern "C" int zlz4_launch_hc_dict_stage(hipStream_t stream, const uint8_t *d_in, const uint64_t *d_in_off,
                                         const uint32_t *d_in_len, const uint8_t *d_dict, const uint64_t *d_dict_off,
                                         const uint32_t *d_dict_len, uint8_t *d_v, uint64_t v_stride, uint64_t *v_off,
                                         uint32_t *v_len, uint32_t *v_pair, uint32_t blk0, uint32_t nblocks, uint32_t slot0,
                                         uint32_t max_in_len, uint32_t dmax) {
    hipLaunchKernelGGL(zlz4::k_hc_dict_stage, dim3(nblocks), dim3(256), 0, stream, d_in, d_in_off, d_in_len, d_dict, d_dict_off,
                       d_dict_len, d_v, v_stride, v_off, v_len, v_pair, blk0, nblocks, slot0, max_in_len, dmax);
    return zlz4_launch_status();
}
