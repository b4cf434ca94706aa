// member_walk_check.cpp -- the host build of the shared multiframe member delimiter (mf_member of
// zig-lz4_amd/csrc/zlz4_frame_batch.hpp) over a file of cases, for tests/test_lz4file_cpu.py.  File: u32 count, then per case
// u32 length and the bytes.  Per case two lines, split_flags 0 and then ZLZ4F_SPLIT_LEGACY, each the members the split's
// loop finds:
//   <pos> <len> <kind> <nb> <last> | <pos> <len> <kind> <nb> <last> | ...          ("-" for a buffer without members)
// Every case lives in a heap buffer of exactly its length.
#include <cstdio>

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
        for (uint32_t flags = 0; flags <= ZLZ4F_SPLIT_LEGACY; flags++) {
            uint64_t pos = 0;
            if (len == 0) printf("-");
            while (pos < len) {
                const MfMember m = mf_member(s + pos, len - pos, flags);
                printf("%s%llu %llu %u %llu %d", pos ? " | " : "", (unsigned long long)pos, (unsigned long long)m.len, m.kind,
                       (unsigned long long)m.nb, m.last ? 1 : 0);
                if (m.len == 0 || m.len > len - pos) { printf(" bad_length"); break; }
                pos += m.len;
                if (m.last) break;
            }
            printf("\n");
        }
        delete[] s;
    }
    fclose(f);
    return 0;
}
