// legacy_walk_check.cpp -- the host build of the shared legacy frame walk (zig-lz4_amd/csrc/zlz4_frame_batch.hpp) over a file of
// cases, for tests/test_legacy_cpu.py.  File: u32 count, then per case u32 length and the bytes.  Per case one line:
//   <verdict> <blocks> <consumed> <offset>:<size> ...            (the walk without a bound)
// and "bounded_walk_differs" behind it where the walk bounded by that block count -- the record pass of the kernels -- does
// not find the same blocks.  Every case lives in a heap buffer of exactly its length.
#include <cstdio>
#include <vector>

#include "../zig-lz4_amd/csrc/zlz4_frame_batch.hpp"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t k = 0; k < count; k++) {
        uint32_t len = 0;
        if (fread(&len, 4, 1, f) != 1) return 2;
        uint8_t *s = new uint8_t[len];
        if (len && fread(s, 1, len, f) != len) return 2;
        std::vector<uint64_t> blocks, again;
        uint64_t nb = 0, consumed = 0, nb2 = 0, consumed2 = 0;
        const int64_t verdict = legacy_walk(s, len, ~0ull, nb, consumed, [&](uint64_t i, uint64_t off, uint32_t size) {
            if (i != blocks.size() / 2) printf("bad index ");
            blocks.push_back(off);
            blocks.push_back(size);
        });
        (void)legacy_walk(s, len, nb, nb2, consumed2, [&](uint64_t, uint64_t off, uint32_t size) {
            again.push_back(off);
            again.push_back(size);
        });
        printf("%lld %llu %llu", (long long)verdict, (unsigned long long)nb, (unsigned long long)consumed);
        for (size_t i = 0; i < blocks.size(); i += 2)
            printf(" %llu:%llu", (unsigned long long)blocks[i], (unsigned long long)blocks[i + 1]);
        if (nb2 != nb || again != blocks) printf(" bounded_walk_differs");
        printf("\n");
        delete[] s;
    }
    fclose(f);
    return 0;
}
