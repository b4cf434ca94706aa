/* hc_dict_ref.c -- test-side C restatement of zlz4_compress_hc_using_dict (include/zlz4_amd.h):
 * compressHashChain (src/lz4hc.zig:976-1064) on V = tail ++ src with a fresh context, every index a position in V, and
 * ip = anchor = D at entry.
 *
 * Written from the specification and the Zig, independently of tools/pyref/zig_lz4_hc_dict.py; the two are checked
 * against each other on the CPU, and this one is the checker of the GPU tests.  Built at test time by
 * tests/hcdictcgen.py.  The tables are the reference's own: hashTable u32 x 32768, chainTable u16 x 65536 indexed by
 * the low 16 bits of the position (:391-393, :504), filled one position at a time by insertHC. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define HD_MINMATCH 4
#define HD_MFLIMIT 12u
#define HD_LASTLITERALS 5u
#define HD_MAX_INPUT 0x7E000000u
#define HD_DIST_MAX 65535u
#define HD_ERR_OUTPUT_TOO_SMALL (-1)
#define HD_ERR_INPUT_TOO_LARGE (-2)
#define HD_ERR_ALLOCATION_FAILED (-6)
#define HD_ERR_INVALID_STATE (-5)
#define HD_ERR_UNSUPPORTED (-8)

typedef struct {
    uint32_t hash[32768];
    uint16_t chain[65536];
    uint32_t next_to_update;
} hd_ctx;

static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static uint32_t hash_hc(uint32_t seq) { return (uint32_t)(seq * 2654435761u) >> 17; }                /* :129-131 */

/* the level compressHC runs (:1446-1452), 0 where the dictionary call has none */
static int hd_level(int level) {
    if (level < 2) level = 9;
    if (level > 12) level = 12;
    return level >= 3 && level <= 9 ? level : 0;
}

static void insert_hc(hd_ctx *c, const uint8_t *v, uint32_t target) {                                 /* :491-510 */
    uint32_t idx = c->next_to_update;
    while (idx < target) {
        const uint32_t h = hash_hc(rd32(v + idx));
        const uint32_t prev = c->hash[h];
        uint32_t delta = prev > idx ? HD_DIST_MAX + 1u : idx - prev;
        if (delta > HD_DIST_MAX) delta = HD_DIST_MAX;
        c->chain[idx & 0xFFFFu] = (uint16_t)delta;
        c->hash[h] = idx;
        idx++;
    }
    c->next_to_update = target;
}

static size_t count(const uint8_t *v, size_t a, size_t b, size_t limit) {                             /* :234-264 */
    size_t n = 0;
    while (a < limit && v[a] == v[b]) { a++; b++; n++; }
    return n;
}
/* :170-199, for a pattern that passed isRepetitivePattern (all four bytes equal): bytes equal to it */
static size_t count_pattern(const uint8_t *v, size_t a, size_t end, uint32_t pattern) {
    size_t n = 0;
    while (a < end && v[a] == (uint8_t)pattern) { a++; n++; }
    return n;
}
static size_t reverse_count_pattern(const uint8_t *v, size_t a, size_t low, uint32_t pattern) {       /* :202-222 */
    size_t n = 0;
    while (a > low && v[a - 1] == (uint8_t)pattern) { a--; n++; }
    return n;
}

typedef struct { int32_t len; uint32_t off; } hd_match;

/* insertAndFindBestMatch (:514-535) = insertHC + insertAndGetWiderMatch (:538-681) with iLowLimit = ip, longest = 3 */
static hd_match best_match(hd_ctx *c, const uint8_t *v, uint32_t ip, uint32_t ihigh, int32_t max_attempts, int pattern_analysis) {
    insert_hc(c, v, ip);
    const uint32_t lowest = (HD_DIST_MAX + 1u > ip) ? 0u : ip - HD_DIST_MAX;                          /* :553-554, lowLimit = 0 */
    int32_t nb = max_attempts;
    const uint32_t pattern = rd32(v + ip);
    hd_match r = {HD_MINMATCH - 1, 0};
    uint32_t m = c->hash[hash_hc(pattern)];                                                           /* :563 */
    if (m == 0) return r;                                                                             /* :566 */
    while (m > 0 && nb > 0) {                                                                         /* :571 */
        if (m > ip || ip - m > HD_DIST_MAX) break;                                                    /* :573 */
        nb--;
        if (m >= lowest && rd32(v + m) == pattern) {                                                  /* :579, :586 */
            const int32_t mlt = HD_MINMATCH + (int32_t)count(v, (size_t)ip + 4, (size_t)m + 4, ihigh);
            if (mlt > r.len) {                                                                        /* :607 (back = 0) */
                r.len = mlt;
                r.off = ip - m;
                if (mlt > max_attempts) break;                                                        /* :613 */
            }
        }
        const uint32_t delta = c->chain[m & 0xFFFFu];                                                 /* :619 */
        if (delta == 0 || delta > m) break;
        m -= delta;
    }
    if (pattern_analysis && r.len > 0) {                                                              /* :626 */
        /* (m == 0: the chain ended at "no predecessor"; the reference would go on to index m - 1 if the table's slot 0,
         *  which a block over 64 KiB reuses for position 65536, happened to hold 1 -- no position is below 0) */
        if (m != 0 && c->chain[m & 0xFFFFu] == 1 &&                                                   /* :627-629 */
            (pattern & 0xFFFFu) == (pattern >> 16) && (pattern & 0xFFu) == (pattern >> 24)) {         /* :631 */
            const size_t src_len = count_pattern(v, (size_t)ip + 4, ihigh, pattern) + 4;              /* :633 */
            const uint32_t cand = m - 1;                                                              /* :636 (m >= 1: delta <= m) */
            if (cand >= lowest && rd32(v + cand) == pattern) {                                        /* :637 (dictIdx = 0), :644 */
                const size_t fwd = count_pattern(v, (size_t)cand + 4, ihigh, pattern) + 4;            /* :646 */
                const size_t back = reverse_count_pattern(v, cand, 0, pattern);                       /* :650 */
                uint32_t lo = cand - (uint32_t)back;                                                  /* :653 */
                if (lo < lowest) lo = lowest;
                const uint32_t lim_back = cand - lo;
                const size_t seg = lim_back + fwd;                                                    /* :654 */
                const int32_t max_ml = (int32_t)(seg < src_len ? seg : src_len);                      /* :658 */
                uint32_t nm;
                if (seg >= src_len && fwd <= src_len) nm = cand + (uint32_t)fwd - (uint32_t)src_len;  /* :660-662 */
                else nm = cand - lim_back;                                                            /* :665 */
                if (max_ml > r.len && ip - nm <= HD_DIST_MAX) { r.len = max_ml; r.off = ip - nm; }    /* :669 */
            }
        }
    }
    return r;
}

/* compressHashChain on v[0 .. N) from position D; 13 <= N - D */
static int64_t hash_chain(hd_ctx *c, const uint8_t *v, uint32_t D, uint32_t N, uint8_t *dst, size_t cap, int32_t max_attempts) {
    const int pattern_analysis = max_attempts > 128;                                                  /* :983 */
    const uint32_t mflimit = N - HD_MFLIMIT, matchlimit = N - HD_LASTLITERALS;
    uint32_t ip = D, anchor = D;
    size_t op = 0;
    while (ip <= mflimit) {                                                                           /* :1009 */
        const hd_match mt = best_match(c, v, ip, matchlimit, max_attempts, pattern_analysis);
        if (mt.len < HD_MINMATCH || mt.off == 0) { ip++; continue; }                                  /* :1013 */
        /* encodeSequence (:308-386), limitedOutput */
        const size_t lit = ip - anchor;
        if (op + lit / 255 + lit + (2 + 1 + HD_LASTLITERALS) > cap) return HD_ERR_OUTPUT_TOO_SMALL;   /* :320-325 */
        const size_t tok = op++;
        if (lit >= 15) {
            size_t len = lit - 15;
            dst[tok] = 15 << 4;
            while (len >= 255) { dst[op++] = 255; len -= 255; }
            dst[op++] = (uint8_t)len;
        } else dst[tok] = (uint8_t)(lit << 4);
        memcpy(dst + op, v + anchor, lit);
        op += lit;
        dst[op] = (uint8_t)mt.off;
        dst[op + 1] = (uint8_t)(mt.off >> 8);
        op += 2;
        const size_t ml = (size_t)mt.len - HD_MINMATCH;
        if (op + ml / 255 + (1 + HD_LASTLITERALS) > cap) return HD_ERR_OUTPUT_TOO_SMALL;              /* :355-359 */
        if (ml >= 15) {
            size_t rem = ml - 15;
            dst[tok] += 15;
            while (rem >= 255) { dst[op++] = 255; rem -= 255; }                                       /* :364-374 */
            dst[op++] = (uint8_t)rem;
        } else dst[tok] += (uint8_t)ml;
        ip += (uint32_t)mt.len;
        anchor = ip;
    }
    const size_t fl = N - anchor;                                                                     /* :1035 */
    if (fl > 0) {
        const size_t ext = fl >= 15 ? 1 + (fl - 15) / 255 : 0;
        /* :1037 tests op + fl + 1 only and then writes the extension bytes unchecked; the product refuses instead */
        if (op + fl + 1 > cap || op + 1 + ext + fl > cap) return HD_ERR_OUTPUT_TOO_SMALL;
        if (fl >= 15) {
            size_t len = fl - 15;
            dst[op++] = 15 << 4;
            while (len >= 255) { dst[op++] = 255; len -= 255; }
            dst[op++] = (uint8_t)len;
        } else dst[op++] = (uint8_t)(fl << 4);
        memcpy(dst + op, v + anchor, fl);
        op += fl;
    }
    return (int64_t)op;
}

int64_t hd_compress(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const uint8_t *dict, size_t dict_len, int level) {
    if (!dict && dict_len) return HD_ERR_INVALID_STATE;
    level = hd_level(level);
    if (level == 0) return HD_ERR_UNSUPPORTED;
    if (n > HD_MAX_INPUT) return HD_ERR_INPUT_TOO_LARGE;                                              /* :1442 */
    if (n == 0) return 0;                                                                             /* :1443 */
    if (cap == 0) return HD_ERR_OUTPUT_TOO_SMALL;                                                     /* :1461 */
    if (n < HD_MFLIMIT + 1) {                                                                         /* :995-998, :1394-1425 */
        if (cap < n + 1 + n / 255) return HD_ERR_OUTPUT_TOO_SMALL;
        dst[0] = (uint8_t)(n << 4);
        memcpy(dst + 1, src, n);
        return (int64_t)n + 1;
    }
    const size_t D = dict_len < 65536u ? dict_len : 65536u;
    uint8_t *v = (uint8_t *)malloc(D + n);
    hd_ctx *c = (hd_ctx *)calloc(1, sizeof(hd_ctx));                                                  /* Context.init :405-419 */
    int64_t r = HD_ERR_ALLOCATION_FAILED;
    if (v && c) {
        if (D) memcpy(v, dict + (dict_len - D), D);
        memcpy(v + D, src, n);
        r = hash_chain(c, v, (uint32_t)D, (uint32_t)(D + n), dst, cap, 1 << (level - 1));
    }
    free(v);
    free(c);
    return r;
}

/* a batch as zlz4_batch_compress_hc_using_dict defines it: an unsupported level refuses the call (nothing written); a
 * block over max_in_len or a dictionary tail over max_dict_len gives InvalidState (after InputTooLarge) */
int32_t hd_compress_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint8_t *out,
                          const uint64_t *out_off, const uint32_t *out_cap, const uint8_t *dict, const uint64_t *dict_off,
                          const uint32_t *dict_len, int64_t *results, uint32_t nblocks, uint32_t max_in_len,
                          uint32_t max_dict_len, int level) {
    if (nblocks == 0) return 0;
    if (hd_level(level) == 0) return HD_ERR_UNSUPPORTED;
    for (uint32_t i = 0; i < nblocks; i++) {
        const uint32_t D = dict_len[i] < 65536u ? dict_len[i] : 65536u;
        if (in_len[i] > HD_MAX_INPUT) { results[i] = HD_ERR_INPUT_TOO_LARGE; continue; }
        if (in_len[i] > max_in_len || D > max_dict_len) { results[i] = HD_ERR_INVALID_STATE; continue; }
        results[i] = hd_compress(in + in_off[i], in_len[i], out + out_off[i], out_cap[i],
                                 dict_len[i] ? dict + dict_off[i] : (const uint8_t *)"", dict_len[i], level);
    }
    return 0;
}
