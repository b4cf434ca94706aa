// The C++ host mirror's linked-frame compress calls (zig-lz4_amd/csrc/host/zlz4.hpp: compressFrameEx,
// compressFrameDeviceEx, compressFrameBatchEx) at level 9 with BATCH_LINK_BLOCKS, built with plain g++ against
// libzlz4_amd.so (the HIP runtime calls it needs are declared by hand, as in host_mirror_check.cpp).
//   host_mirror_linked_hc INPUT OUT_HOST OUT_DEVICE OUT_BATCH
// writes the three frames; tests/test_gpu_linked_frame_hc.py compares them with the model.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../zig-lz4_amd/csrc/host/zlz4.hpp"

extern "C" {   // libamdhip64: hipError_t is an int, 0 = success; hipMemcpyKind 1 = H2D, 2 = D2H
int hipMalloc(void **p, size_t n);
int hipFree(void *p);
int hipMemcpy(void *dst, const void *src, size_t n, int kind);
int hipDeviceSynchronize(void);
}

static bool write_file(const char *path, const unsigned char *p, size_t n) {
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, n, f) == n;
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
    if (argc != 5) return 1;
    std::vector<unsigned char> in;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        unsigned char buf[65536];
        size_t k;
        while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k);
        std::fclose(f);
    }
    namespace zf = zlz4::lz4f;
    zf::Preferences p{};
    p.compression_level = 9;
    const uint32_t link = zf::BATCH_LINK_BLOCKS;
    // refusals are host arithmetic
    if (zf::compressFrameEx(nullptr, 0, nullptr, 0, &p, 8).error_name() != "ParameterInvalid") return 3;
    p.compression_level = 10;
    if (zf::compressFrameEx(nullptr, 0, nullptr, 0, &p, link).error_name() != "Unsupported") return 4;
    p.compression_level = 9;
    const size_t cap = zf::compressFrameBound(in.size(), &p);
    std::vector<unsigned char> out(cap);
    // 1. host pointers
    auto r = zf::compressFrameEx(in.data(), in.size(), out.data(), cap, &p, link);
    if (!r.ok() || !write_file(argv[2], out.data(), r.value)) return 5;
    const size_t want = r.value;
    // 2. device pointers, one frame
    void *d_in, *d_out, *d_meta, *d_ws;
    if (hipMalloc(&d_in, in.size() + 16) || hipMalloc(&d_out, cap) || hipMalloc(&d_meta, 64)) return 6;
    hipMemcpy(d_in, in.data(), in.size(), 1);
    r = zf::compressFrameDeviceEx(nullptr, (const uint8_t *)d_in, in.size(), (uint8_t *)d_out, cap, &p, link);
    if (!r.ok() || r.value != want) return 7;
    hipMemcpy(out.data(), d_out, r.value, 2);
    if (!write_file(argv[3], out.data(), r.value)) return 8;
    // 3. the batch call on a batch of one
    const uint32_t max_blocks = (uint32_t)((in.size() + 65535) / 65536);
    const size_t wsb = zf::compressFrameBatchWorkspaceEx(1, max_blocks, &p, link);
    if (hipMalloc(&d_ws, wsb)) return 9;
    const uint64_t meta[5] = {0, in.size(), 0, cap, 0};          // src_off, src_len, dst_off, dst_cap, result
    hipMemcpy(d_meta, meta, sizeof meta, 1);
    const uint64_t *m = (const uint64_t *)d_meta;
    zf::Frames f{(const uint8_t *)d_in, m, m + 1, (uint8_t *)d_out, m + 2, m + 3, (int64_t *)(m + 4), 1};
    if (!zf::compressFrameBatchEx(nullptr, f, max_blocks, &p, link, d_ws, wsb).ok()) return 10;
    if (zf::compressFrameBatch(nullptr, f, max_blocks, &p, link, d_ws, wsb).error_name() != "Unsupported") return 11;
    hipDeviceSynchronize();
    int64_t res = 0;
    hipMemcpy(&res, (const void *)(m + 4), 8, 2);
    if (res != (int64_t)want) return 12;
    hipMemcpy(out.data(), d_out, (size_t)res, 2);
    if (!write_file(argv[4], out.data(), (size_t)res)) return 13;
    for (void *q : {d_in, d_out, d_meta, d_ws}) hipFree(q);
    std::printf("linked hc mirror ok: %zu -> %zu\n", in.size(), want);
    return 0;
}
