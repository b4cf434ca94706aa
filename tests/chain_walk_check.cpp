// chain_walk_check.cpp -- the host build of the shared block chain step (zig-lz4_amd/csrc/zlz4_frame_batch.hpp) over a file of
// cases, for tests/test_frame_chain_cpu.py.  File: u32 count, then per case u32 length and the bytes.  Per case one line:
//   <header size or error> <blocks> <cursor after the walk> <ending> <chain_blocks' count>
// Built with -fsanitize=address,undefined: every case lives in a heap buffer of exactly its length.
#include <cstdio>

#include "../zig-lz4_amd/csrc/zlz4_frame_batch.hpp"

static const char *ending(ChainEnd e) {
    switch (e) {
        case kChainBlock: return "block";
        case kChainCksCut: return "cks_cut";
        case kChainBoundary: return "boundary";
        case kChainWordCut: return "word_cut";
        case kChainEndMark: return "end_mark";
        case kChainDataCut: return "data_cut";
    }
    return "?";
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t k = 0; k < count; k++) {
        uint32_t len = 0;
        if (fread(&len, 4, 1, f) != 1) return 2;
        uint8_t *s = new uint8_t[len];                 // exactly len bytes: a read behind the case is a sanitizer report
        if (len && fread(s, 1, len, f) != len) return 2;
        const ParsedHeader ph = parse_header(s, len);
        if (ph.size < 0) {
            printf("%lld 0 0 no_header 0\n", (long long)ph.size);
        } else {
            uint64_t pos = (uint64_t)ph.size, nb = 0;
            bool cks_cut = false;                      // (the flag and the ending must say the same)
            const ChainEnd e = chain_walk(s, len, (ph.flg & 0x10u) != 0, pos, ~0ull, nb, [&](uint64_t i, const ChainBlock &c) {
                cks_cut = (c.flags & kBlkNoCks) != 0;
                if (i != nb - 1 || c.off + c.size > len || (c.cks_off && c.cks_off + 4 > len)) printf("bad block\n");
            });
            printf("%lld %llu %llu %s %llu\n", (long long)ph.size, (unsigned long long)nb, (unsigned long long)pos,
                   cks_cut == (e == kChainCksCut) ? ending(e) : "flag_mismatch", (unsigned long long)chain_blocks(s, len, ph));
        }
        delete[] s;
    }
    fclose(f);
    return 0;
}
