// seek_table_check.cpp -- the host build of the shared seek table functions (seek_footer, seek_member_row, seek_entry_row,
// seek_append_refusal of zig-lz4_amd/csrc/zlz4_frame_batch.hpp) over a file of cases, for tests/test_seek_table_cpu.py.
// File: u32 count, then per case u32 length, the bytes, and the append's arguments for the file: i64 nm, u64 pos, u64 len
// and u32 kind of the split's last member, i64 nb, u64 end_pos, u64 cap.  Per case two lines:
//   L <split result> <idx_n> : <pos> <len> <kind>, ... ; <pos> <dec>, ...     the load as the kernels fold it; rows only
//                                                                              when the split result is positive
//   A <refusal> <T>                                                            the append's verdict for the arguments
// Every case lives in a heap buffer of exactly its length.
#include <cstdio>
#include <vector>

#include "../zig-lz4_amd/csrc/zlz4_frame_batch.hpp"

template <typename T> static bool rd(FILE *f, T &v) { return fread(&v, sizeof v, 1, f) == 1; }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0;
    if (!rd(f, count)) return 2;
    for (uint32_t k = 0; k < count; k++) {
        uint32_t len = 0;
        if (!rd(f, len)) return 2;
        uint8_t *s = new uint8_t[len];
        if (len && fread(s, 1, len, f) != len) return 2;
        int64_t nm = 0, nb = 0;
        uint64_t end_pos = 0, cap = 0;
        zlz4f_member last = {};
        if (!rd(f, nm) || !rd(f, last.pos) || !rd(f, last.len) || !rd(f, last.kind) || !rd(f, nb) || !rd(f, end_pos) || !rd(f, cap))
            return 2;
        SeekFooter F;
        const SeekVerdict v = seek_footer(s, len, F);
        std::vector<zlz4f_member> rows;
        std::vector<zlz4f_index_entry> ents;
        bool bad = v == kSeekMalformed;
        if (v == kSeekOk) {
            for (uint64_t r = 0; r < F.nm; r++) {
                zlz4f_member m;
                if (!seek_member_row(s, len, F, r, m)) bad = true;
                rows.push_back(m);
            }
            for (uint64_t r = 0; r <= F.nb; r++) {
                zlz4f_index_entry e;
                if (!seek_entry_row(s, len, F, r, e)) bad = true;
                ents.push_back(e);
            }
        }
        if (v == kSeekNone) printf("L 0 %d :\n", ZLZ4_ERR_INVALID_STATE);
        else if (bad) printf("L %d %d :\n", ZLZ4_ERR_INVALID_STATE, ZLZ4_ERR_INVALID_STATE);
        else {
            printf("L %llu %llu :", (unsigned long long)F.nm, (unsigned long long)F.nb);
            for (size_t r = 0; r < rows.size(); r++)
                printf("%s %llu %llu %u", r ? "," : "", (unsigned long long)rows[r].pos, (unsigned long long)rows[r].len, rows[r].kind);
            printf(" ;");
            for (size_t r = 0; r < ents.size(); r++)
                printf("%s %llu %llu", r ? "," : "", (unsigned long long)ents[r].pos, (unsigned long long)ents[r].dec);
            printf("\n");
        }
        uint64_t T = 0;
        const int64_t why = seek_append_refusal(nm, last, nb, end_pos, len, cap, T);
        printf("A %lld %llu\n", (long long)why, (unsigned long long)T);
        delete[] s;
    }
    fclose(f);
    return 0;
}
