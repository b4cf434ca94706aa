/* hc_dict_ref_driver.c -- a program around tests/hc_dict_ref.c for a sanitizer build (tests/test_hc_dict_cpu.py compiles
 * the two with -fsanitize=address,undefined and runs the result; nothing sanitized is loaded into Python).
 *
 * argv[1]: a file of cases, each  u32 level | u32 cap | u32 dict_len | u32 n | dictionary | record  (little endian).
 * Every buffer is a heap block of exactly its size, so a read or write past a dictionary, a record or a destination is
 * an error.  Prints one line per case: result and an FNV-1a hash of the output. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int64_t hd_compress(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const uint8_t *dict, size_t dict_len, int level);

static int rd_u32(FILE *f, uint32_t *v) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) return 0;
    *v = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t level, cap, dl, n;
    int cases = 0;
    while (rd_u32(f, &level)) {
        if (!rd_u32(f, &cap) || !rd_u32(f, &dl) || !rd_u32(f, &n)) return 3;
        uint8_t *d = (uint8_t *)malloc(dl ? dl : 1), *s = (uint8_t *)malloc(n ? n : 1), *o = (uint8_t *)malloc(cap ? cap : 1);
        if (!d || !s || !o) return 4;
        if (fread(d, 1, dl, f) != dl || fread(s, 1, n, f) != n) return 3;
        const int64_t r = hd_compress(s, n, o, cap, d, dl, (int)level);
        uint32_t h = 2166136261u;
        for (int64_t k = 0; k < r; k++) h = (h ^ o[k]) * 16777619u;
        printf("%lld %08x\n", (long long)r, h);
        free(d);
        free(s);
        free(o);
        cases++;
    }
    fclose(f);
    return cases ? 0 : 5;
}
