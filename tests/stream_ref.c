/* stream_ref.c -- test-side C restatement of the reference's streaming compressor (src/lz4.zig:751-866):
 * Stream.loadDict (:798-820) and compressFastContinue (:822-836) with compressFastWithHashTable (:624-748).
 *
 * Written from the reference's text, independently of tools/pyref/zig_lz4_stream.py; the two are checked against each
 * other on the CPU, and this one is the fast checker for large GPU batches.  Built at test time by tests/streamgen.py.
 * The table is the reference's Stream.hashTable: 4096 u32 (LZ4_HASH_SIZE_U32, :33). */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define SR_MINMATCH 4u
#define SR_MFLIMIT 12u
#define SR_LASTLITERALS 5u
#define SR_MAX_INPUT 0x7E000000u
#define SR_DIST_MAX 65535u
#define SR_ERR_OUTPUT_TOO_SMALL (-1)
#define SR_ERR_INPUT_TOO_LARGE (-2)

static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static uint32_t hash4(uint32_t v) { return (uint32_t)(v * 2654435761u) >> 20; }                      /* :75-77 */

/* Stream.loadDict: resetFast (:800), hash positions [0, dictSize - 5] of the last min(len, 64 KiB) bytes (:806-816) */
int64_t sr_load_dict(uint32_t *table, const uint8_t *dict, size_t len) {
    memset(table, 0, 4096 * sizeof(uint32_t));
    if (len == 0) return 0;
    const size_t size = len < 65536u ? len : 65536u;
    const uint8_t *tail = dict + (len - size);
    if (size >= SR_MINMATCH)
        for (size_t i = 0; i < size - SR_MINMATCH; i++) table[hash4(rd32(tail + i))] = (uint32_t)i;
    return (int64_t)size;
}

/* length code of a saturated nibble: (v - 15) as 255-runs plus the remainder (:368-382, :416-429) */
static int put_len(uint8_t *dst, size_t cap, size_t *op, size_t v) {
    while (v >= 255) {
        if (*op >= cap) return -1;
        dst[(*op)++] = 255;
        v -= 255;
    }
    if (*op >= cap) return -1;
    dst[(*op)++] = (uint8_t)v;
    return 0;
}

/* compressAsLiterals (:449-482) and finishCompression (:484-519): one literal-only sequence */
static int64_t last_literals(const uint8_t *lit, size_t n, uint8_t *dst, size_t cap, size_t op) {
    if (n == 0) return (int64_t)op;
    if (op >= cap) return SR_ERR_OUTPUT_TOO_SMALL;
    const size_t tok = op++;
    if (n >= 15) {
        dst[tok] = 15 << 4;
        if (put_len(dst, cap, &op, n - 15)) return SR_ERR_OUTPUT_TOO_SMALL;
    } else {
        dst[tok] = (uint8_t)(n << 4);
    }
    if (op + n > cap) return SR_ERR_OUTPUT_TOO_SMALL;
    memcpy(dst + op, lit, n);
    return (int64_t)(op + n);
}

/* compressFastWithHashTable on `t` (a working copy) */
static int64_t with_table(uint32_t *t, const uint8_t *src, size_t n, uint8_t *dst, size_t cap, uint32_t acceleration) {
    const size_t L = n - SR_MFLIMIT, match_limit = n - SR_LASTLITERALS;
    const size_t accel = acceleration < 1 ? 1 : (acceleration > 65537u ? 65537u : acceleration);
    size_t ip = 1, op = 0, anchor = 0;
    while (ip < L) {
        size_t step = accel, nb = accel, fwd = ip, match;
        for (;;) {
            ip = fwd;
            fwd += step;
            step = nb >> 6;
            nb++;
            if (fwd > L) return last_literals(src + anchor, n - anchor, dst, cap, op);
            const uint32_t seq = rd32(src + ip);
            const uint32_t h = hash4(seq);
            match = t[h];
            const int ok = match > 0 && match < ip && match + SR_DIST_MAX >= ip && rd32(src + match) == seq;
            t[h] = (uint32_t)ip;
            if (ok) break;
        }
        const size_t lit = ip - anchor;
        const size_t tok = op++;
        if (op >= cap) return SR_ERR_OUTPUT_TOO_SMALL;
        if (lit >= 15) {
            dst[tok] = 15 << 4;
            if (put_len(dst, cap, &op, lit - 15)) return SR_ERR_OUTPUT_TOO_SMALL;
        } else {
            dst[tok] = (uint8_t)(lit << 4);
        }
        if (op + lit > cap) return SR_ERR_OUTPUT_TOO_SMALL;
        memcpy(dst + op, src + anchor, lit);
        op += lit;
        if (op + 2 > cap) return SR_ERR_OUTPUT_TOO_SMALL;
        dst[op] = (uint8_t)(ip - match);
        dst[op + 1] = (uint8_t)((ip - match) >> 8);
        op += 2;
        ip += SR_MINMATCH;
        match += SR_MINMATCH;
        size_t ml = 0;
        while (ip < match_limit && src[ip] == src[match]) { ip++; match++; ml++; }
        if (ml >= 15) {
            dst[tok] |= 15;
            if (put_len(dst, cap, &op, ml - 15)) return SR_ERR_OUTPUT_TOO_SMALL;
        } else {
            dst[tok] |= (uint8_t)ml;
        }
        anchor = ip;
        if (ip < L) {
            t[hash4(rd32(src + ip))] = (uint32_t)ip;
            ip++;
        }
    }
    return last_literals(src + anchor, n - anchor, dst, cap, op);
}

/* Stream.compressFastContinue: `table` is replaced by the final table only on success of a >= 13-byte block */
int64_t sr_compress_continue(uint32_t *table, const uint8_t *src, size_t n, uint8_t *dst, size_t cap, uint32_t accel) {
    if (n > SR_MAX_INPUT) return SR_ERR_INPUT_TOO_LARGE;
    if (n == 0) return 0;
    if (n < SR_MFLIMIT + 1) return last_literals(src, n, dst, cap, 0);
    uint32_t work[4096];
    memcpy(work, table, sizeof work);
    const int64_t r = with_table(work, src, n, dst, cap, accel);
    if (r >= 0) memcpy(table, work, sizeof work);
    return r;
}

/* a batch for the GPU tests: block i uses table tables_in + idx[i] * 4096 (the table is copied to tables_out + i * 4096
 * first, then continued there); results[i] as above */
void sr_compress_continue_batch(const uint32_t *tables_in, const uint32_t *idx, uint32_t *tables_out, const uint8_t *in,
                                const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                                const uint32_t *out_cap, int64_t *results, uint32_t nblocks, uint32_t accel) {
    for (uint32_t i = 0; i < nblocks; i++) {
        uint32_t *t = tables_out + (size_t)i * 4096;
        memcpy(t, tables_in + (size_t)(idx ? idx[i] : i) * 4096, 4096 * sizeof(uint32_t));
        results[i] = sr_compress_continue(t, in + in_off[i], in_len[i], out + out_off[i], out_cap[i], accel);
    }
}
