/* dict_compress_ref.c -- test-side C restatement of zlz4_compress_fast_using_dict (include/zlz4_amd.h, DESIGN.md
 * section 4.1c): compressFastWithHashTable (src/lz4.zig:624-740) on V = tail ++ src, the table starting as
 * Stream.loadDict (:798-820) leaves it, anchor = D, ip = max(D, 1), every position a position in V.
 *
 * Written from the specification, independently of tools/pyref/zig_lz4_dict_compress.py; the two are checked against each
 * other on the CPU, and this one is the checker of the GPU tests.  Built at test time by tests/dictcgen.py.  V is never
 * materialised: a position below D reads the tail, any other the record. */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define DC_MINMATCH 4u
#define DC_MFLIMIT 12u
#define DC_LASTLITERALS 5u
#define DC_MAX_INPUT 0x7E000000u
#define DC_DIST_MAX 65535u
#define DC_ERR_OUTPUT_TOO_SMALL (-1)
#define DC_ERR_INPUT_TOO_LARGE (-2)
#define DC_ERR_INVALID_STATE (-5)

typedef struct { const uint8_t *tail; const uint8_t *src; size_t D; } vbuf;

static uint8_t vb(const vbuf *v, size_t p) { return p < v->D ? v->tail[p] : v->src[p - v->D]; }
static uint32_t vrd32(const vbuf *v, size_t p) {
    return (uint32_t)vb(v, p) | (uint32_t)vb(v, p + 1) << 8 | (uint32_t)vb(v, p + 2) << 16 | (uint32_t)vb(v, p + 3) << 24;
}
static uint32_t hash4(uint32_t x) { return (uint32_t)(x * 2654435761u) >> 20; }                      /* :75-77 */

/* Stream.loadDict (:798-820): entry i for the 4-gram at tail[i], i in [0, D - 5], last writer wins, 0 elsewhere */
int64_t dc_load_dict(uint32_t *table, const uint8_t *dict, size_t len) {
    memset(table, 0, 4096 * sizeof(uint32_t));
    const size_t D = len < 65536u ? len : 65536u;
    const uint8_t *tail = dict + (len - D);
    if (D >= DC_MINMATCH)
        for (size_t i = 0; i < D - DC_MINMATCH; i++) {
            const uint32_t x = (uint32_t)tail[i] | (uint32_t)tail[i + 1] << 8 | (uint32_t)tail[i + 2] << 16 | (uint32_t)tail[i + 3] << 24;
            table[hash4(x)] = (uint32_t)i;
        }
    return (int64_t)D;
}

static int put_len(uint8_t *dst, size_t cap, size_t *op, size_t v) {     /* :675-684, :716-725 */
    while (v >= 255) {
        if (*op >= cap) return -1;
        dst[(*op)++] = 255;
        v -= 255;
    }
    if (*op >= cap) return -1;
    dst[(*op)++] = (uint8_t)v;
    return 0;
}

/* compressAsLiterals (:449-482) and finishCompression (:484-519): literals always come from the record */
static int64_t last_literals(const uint8_t *lit, size_t n, uint8_t *dst, size_t cap, size_t op) {
    if (n == 0) return (int64_t)op;
    if (op >= cap) return DC_ERR_OUTPUT_TOO_SMALL;
    const size_t tok = op++;
    if (n >= 15) {
        dst[tok] = 15 << 4;
        if (put_len(dst, cap, &op, n - 15)) return DC_ERR_OUTPUT_TOO_SMALL;
    } else {
        dst[tok] = (uint8_t)(n << 4);
    }
    if (op + n > cap) return DC_ERR_OUTPUT_TOO_SMALL;
    memcpy(dst + op, lit, n);
    return (int64_t)(op + n);
}

/* `table` (4096 u32) is read, never written.  stats (NULL or 2 u64): match bytes whose source lies in the dictionary,
 * all match bytes. */
int64_t dc_compress_with_table(const uint32_t *table, const uint8_t *src, size_t n, uint8_t *dst, size_t cap,
                               const uint8_t *dict, size_t dict_len, uint32_t acceleration, uint64_t *stats) {
    if (n > DC_MAX_INPUT) return DC_ERR_INPUT_TOO_LARGE;                /* :823 */
    if (n == 0) return 0;                                               /* :824 */
    if (n < DC_MFLIMIT + 1) return last_literals(src, n, dst, cap, 0);  /* :825-827 */
    uint32_t t[4096];
    memcpy(t, table, sizeof t);
    vbuf v;
    v.D = dict_len < 65536u ? dict_len : 65536u;
    v.tail = dict + (dict_len - v.D);
    v.src = src;
    const size_t D = v.D, end = D + n;
    const size_t L = end - DC_MFLIMIT, match_limit = end - DC_LASTLITERALS;     /* :630-631 on V */
    const size_t accel = acceleration < 1 ? 1 : (acceleration > 65537u ? 65537u : acceleration);   /* :636 */
    size_t ip = D > 1 ? D : 1, op = 0, anchor = D;                      /* :626-633 */
    while (ip < L) {                                                    /* :635 */
        size_t step = accel, nb = accel, fwd = ip, match;
        for (;;) {                                                      /* :643 */
            ip = fwd;
            fwd += step;
            step = nb >> 6;
            nb++;
            if (fwd > L) return last_literals(src + (anchor - D), end - anchor, dst, cap, op);     /* :649-651 */
            const uint32_t seq = vrd32(&v, ip);
            const uint32_t h = hash4(seq);                              /* :653 */
            match = t[h];                                               /* :654 */
            const int ok = match > 0 && match < ip && match + DC_DIST_MAX >= ip && vrd32(&v, match) == seq;   /* :656-659 */
            t[h] = (uint32_t)ip;                                        /* :661 */
            if (ok) break;
        }
        const size_t lit = ip - anchor;                                 /* :668 */
        const size_t tok = op++;
        if (op >= cap) return DC_ERR_OUTPUT_TOO_SMALL;                  /* :671 */
        if (lit >= 15) {
            dst[tok] = 15 << 4;
            if (put_len(dst, cap, &op, lit - 15)) return DC_ERR_OUTPUT_TOO_SMALL;
        } else {
            dst[tok] = (uint8_t)(lit << 4);
        }
        if (op + lit > cap) return DC_ERR_OUTPUT_TOO_SMALL;             /* :689 */
        memcpy(dst + op, src + (anchor - D), lit);                      /* anchor >= D */
        op += lit;
        if (op + 2 > cap) return DC_ERR_OUTPUT_TOO_SMALL;               /* :696 */
        dst[op] = (uint8_t)(ip - match);                                /* :695-697 */
        dst[op + 1] = (uint8_t)((ip - match) >> 8);
        op += 2;
        ip += DC_MINMATCH;
        match += DC_MINMATCH;
        size_t ml = 0;
        const size_t m0 = match - DC_MINMATCH;
        while (ip < match_limit && vb(&v, ip) == vb(&v, match)) { ip++; match++; ml++; }    /* :704-712 */
        if (stats) {
            const size_t total = ml + DC_MINMATCH;
            stats[1] += total;
            if (m0 < D) stats[0] += (m0 + total <= D) ? total : D - m0;
        }
        if (ml >= 15) {                                                 /* :714-728 */
            dst[tok] |= 15;
            if (put_len(dst, cap, &op, ml - 15)) return DC_ERR_OUTPUT_TOO_SMALL;
        } else {
            dst[tok] |= (uint8_t)ml;
        }
        anchor = ip;                                                    /* :730 */
        if (ip < L) {                                                   /* :732-736 */
            t[hash4(vrd32(&v, ip))] = (uint32_t)ip;
            ip++;
        }
    }
    return last_literals(src + (anchor - D), end - anchor, dst, cap, op);       /* :739 */
}

/* a batch as zlz4_batch_compress_fast_using_dict defines it: block i uses table tables + idx[i] * 4096 (idx NULL: table
 * i); a block over max_in_len or a dictionary tail over max_dict_len gives InvalidState (after InputTooLarge) */
void dc_compress_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint8_t *out,
                       const uint64_t *out_off, const uint32_t *out_cap, const uint8_t *dict, const uint64_t *dict_off,
                       const uint32_t *dict_len, const uint32_t *tables, const uint32_t *idx, int64_t *results,
                       uint32_t nblocks, uint32_t max_in_len, uint32_t max_dict_len, uint32_t accel) {
    for (uint32_t i = 0; i < nblocks; i++) {
        const uint32_t D = dict_len[i] < 65536u ? dict_len[i] : 65536u;
        if (in_len[i] > DC_MAX_INPUT) { results[i] = DC_ERR_INPUT_TOO_LARGE; continue; }
        if (in_len[i] > max_in_len || D > max_dict_len) { results[i] = DC_ERR_INVALID_STATE; continue; }
        results[i] = dc_compress_with_table(tables + (size_t)(idx ? idx[i] : i) * 4096, in + in_off[i], in_len[i],
                                            out + out_off[i], out_cap[i], dict + dict_off[i], dict_len[i], accel, NULL);
    }
}
