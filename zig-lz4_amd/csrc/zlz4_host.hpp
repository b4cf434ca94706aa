// zlz4_host.hpp -- host-side infrastructure shared by the C-ABI entry points (zlz4_capi.hip, zlz4_frame.hip): the device
// probe, scratch memory, and the staging of a call on one block or one frame.  Implemented in zlz4_host.hip.
//
// hipMalloc / hipFree of a multi-GiB slot arena cost milliseconds and hipFree synchronises the device, so freed
// buffers are parked in a small per-process cache and handed out again.  A buffer may only be parked once the work
// that uses it has finished: every DevBuf belongs to a DeviceCall, and the first DevBuf that dies while the call's
// stream may still be busy (an early error return after kernels were enqueued) synchronises the stream first.  The
// cache is bounded by count AND by bytes; zlz4_release_device_cache() gives the memory back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace zlz4host {

bool device_ok();                                  // a gfx950 device is present (probed once per process)

void *cache_take(size_t &n, int dev);              // a parked buffer of >= n bytes on `dev` (n := its size), or nullptr
bool cache_give(void *p, size_t n, int dev);       // park it; false = cache full (caller frees)

struct DeviceCall {
    hipStream_t st;
    bool idle = true;                 // false between the first launch and the stream synchronisation that follows it
    explicit DeviceCall(hipStream_t s) : st(s) {}
    void launched() { idle = false; }
    bool sync() { idle = true; return hipStreamSynchronize(st) == hipSuccess; }
};

struct DevBuf {
    void *p = nullptr;
    size_t n = 0;
    int dev = 0;
    DeviceCall *call = nullptr;
    explicit DevBuf(size_t want, DeviceCall *dc = nullptr) : call(dc) {
        n = want ? want : 1;
        if (hipGetDevice(&dev) != hipSuccess) return;
        p = cache_take(n, dev);
        if (!p && hipMalloc(&p, n) != hipSuccess) p = nullptr;
    }
    ~DevBuf() {
        if (!p) return;
        if (call && !call->idle) (void)call->sync();         // error exit with work in flight: wait before anyone reuses p
        if (!cache_give(p, n, dev)) (void)hipFree(p);
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

// ---- a batch of one: the launchers and the batch frame calls take per-block / per-frame arrays on the device; a call on
// one block or frame stages one descriptor record and points every array at a field of it (&rec.d->field: an address
// on the device, never dereferenced on the host).

// the arrays of the block launchers (zlz4_launch.hpp); a call leaves the fields it has no use for at 0
struct BlockRec {
    uint64_t in_off, out_off, dict_off;
    int64_t result, dict_size;        // dict_size: what loadDict reports
    uint32_t in_len, out_cap, dict_len;
    uint32_t bound;                   // dict_len[1] of zlz4_launch_decompress_safe_bound: follows dict_len
};
static_assert(offsetof(BlockRec, bound) == offsetof(BlockRec, dict_len) + 4, "bound follows dict_len");

// the arrays of the zlz4f_batch_* frame calls
struct FrameRec { uint64_t src_off, src_len, dst_off, dst_cap; int64_t result; };

template <typename Rec> struct Staged {
    Rec h{};                          // host copy: filled in, then upload()
    DevBuf buf;
    Rec *d;                           // device copy
    explicit Staged(DeviceCall *dc, size_t bytes = 64) : buf(bytes, dc), d(buf.as<Rec>()) {
        static_assert(sizeof(Rec) <= 256, "record");
    }
    // (bytes: the leading fields alone, for a call that has no use for the rest)
    bool upload(hipStream_t st, size_t bytes = sizeof(Rec)) {
        return hipMemcpyAsync(d, &h, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
    }
};

// n host bytes into `d`, in stream order; nothing to copy is no call
static inline bool upload(const DevBuf &d, const void *src, size_t n, hipStream_t st) {
    return n == 0 || hipMemcpyAsync(d.p, src, n, hipMemcpyHostToDevice, st) == hipSuccess;
}

// what the call left in *d_result, after the stream has drained
static inline bool read_result(DeviceCall &dc, const int64_t *d_result, int64_t &result) {
    return hipMemcpyAsync(&result, d_result, sizeof result, hipMemcpyDeviceToHost, dc.st) == hipSuccess && dc.sync();
}

// the first `result` bytes of d_out into the caller's dst[0..dst_cap); result <= 0 leaves dst unwritten
static inline bool copy_back(uint8_t *dst, size_t dst_cap, const DevBuf &d_out, int64_t result) {
    if (result <= 0) return true;
    if ((uint64_t)result > dst_cap) return false;            // cannot happen; never overrun the caller
    return hipMemcpy(dst, d_out.p, (size_t)result, hipMemcpyDeviceToHost) == hipSuccess;
}

// the kernels index with 32 bits; a destination larger than 4 GiB-1 is clamped (never reached: compressBound(0x7E000000)
// and the largest decodable block both fit)
static inline uint32_t clamp_cap32(size_t dst_cap) { return dst_cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dst_cap; }

// the last min(dict_len, 65536) bytes of a dictionary: offsets are at most 65535, nothing in front of that tail can be
// reached (src/lz4.zig:189-192)
static inline size_t dict_tail(size_t dict_len) { return dict_len < 65536u ? dict_len : 65536u; }

}  // namespace zlz4host
