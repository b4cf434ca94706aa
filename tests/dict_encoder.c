/* dict_encoder.c -- test-side data generator: valid LZ4 blocks whose matches may reach into an external dictionary.
 *
 * Greedy 4-byte hash over the virtual buffer dict ++ block (the dictionary's last 64 KiB), one candidate per hash.
 * It emits matches wholly inside the dictionary, matches that span the dictionary end (periodic ones included) and
 * in-block matches, with offsets up to 65535, and keeps the block format's end rules (last 5 bytes literals, no match
 * starting in the last 12).  It is not a restatement of the reference (whose Stream.loadDict output never references
 * the dictionary) and is not a product path: the tests compile it with cc and load it with ctypes.
 *
 * stats[0..3] (optional): match bytes read from the dictionary, match bytes read from the block, matches wholly in the
 * dictionary, matches that span the dictionary end. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define HBITS_MAX 16

static uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
static uint32_t hash4(uint32_t v, int hb) { return (v * 2654435761u) >> (32 - hb); }

static int put_len(uint8_t *dst, size_t cap, size_t *o, size_t v) {   /* the 255-run after a saturated nibble */
    while (v >= 255) { if (*o >= cap) return -1; dst[(*o)++] = 255; v -= 255; }
    if (*o >= cap) return -1;
    dst[(*o)++] = (uint8_t)v;
    return 0;
}

static int emit(uint8_t *dst, size_t cap, size_t *o, const uint8_t *lit, size_t nlit, uint32_t off, size_t ml) {
    const size_t mc = ml ? ml - 4 : 0;
    if (*o >= cap) return -1;
    dst[(*o)++] = (uint8_t)(((nlit >= 15 ? 15 : nlit) << 4) | (ml ? (mc >= 15 ? 15 : mc) : 0));
    if (nlit >= 15 && put_len(dst, cap, o, nlit - 15)) return -1;
    if (*o + nlit > cap) return -1;
    memcpy(dst + *o, lit, nlit);
    *o += nlit;
    if (!ml) return 0;
    if (*o + 2 > cap) return -1;
    dst[(*o)++] = (uint8_t)off;
    dst[(*o)++] = (uint8_t)(off >> 8);
    if (mc >= 15 && put_len(dst, cap, o, mc - 15)) return -1;
    return 0;
}

/* -> compressed size, or -1 (dst too small / out of memory).  ht0 (optional): the table of the dictionary alone, as
 * left by an earlier call with the same dictionary (dict_encode_batch); hb: hash bits (12 for small inputs) */
static int64_t encode1(const uint8_t *dict, size_t dict_len, const uint8_t *src, size_t n, uint8_t *dst, size_t cap,
                       uint64_t *stats, uint8_t *v, int32_t *ht, const int32_t *ht0, int hb) {
    const size_t dl = dict_len < 65536 ? dict_len : 65536;
    memcpy(v, dict + (dict_len - dl), dl);
    memcpy(v + dl, src, n);
    memset(v + dl + n, 0, 8);
    if (ht0) {
        memcpy(ht, ht0, sizeof(int32_t) << hb);
    } else {
        for (size_t i = 0; i < ((size_t)1 << hb); i++) ht[i] = -1;
        for (size_t p = 0; p + 4 <= dl; p++) ht[hash4(rd32(v + p), hb)] = (int32_t)p;
    }
    uint64_t st[4] = {0, 0, 0, 0};
    size_t o = 0, anchor = 0, i = 0;   /* block coordinates */
    const size_t mflimit = n >= 12 ? n - 12 : 0, mlimit = n >= 5 ? n - 5 : 0;
    while (n >= 13 && i <= mflimit) {
        const size_t p = dl + i;
        const uint32_t h = hash4(rd32(v + p), hb);
        const int32_t c = ht[h];
        ht[h] = (int32_t)p;
        if (c >= 0 && p - (size_t)c <= 65535 && rd32(v + c) == rd32(v + p)) {
            size_t ml = 4;
            while (i + ml < mlimit && v[c + ml] == v[p + ml]) ml++;
            const uint32_t off = (uint32_t)(p - (size_t)c);
            if (emit(dst, cap, &o, src + anchor, i - anchor, off, ml)) return -1;
            if ((size_t)c + ml <= dl) { st[0] += ml; st[2]++; }
            else if ((size_t)c < dl) { st[0] += dl - (size_t)c; st[1] += (size_t)c + ml - dl; st[3]++; }
            else st[1] += ml;
            for (size_t k = 1; k < ml && i + k + 4 <= n; k += 2) ht[hash4(rd32(v + p + k), hb)] = (int32_t)(p + k);
            i += ml;
            anchor = i;
        } else {
            i++;
        }
    }
    if (emit(dst, cap, &o, src + anchor, n - anchor, 0, 0)) return -1;
    if (stats) for (int k = 0; k < 4; k++) stats[k] += st[k];
    return (int64_t)o;
}

int64_t dict_encode(const uint8_t *dict, size_t dict_len, const uint8_t *src, size_t n, uint8_t *dst, size_t cap,
                    uint64_t *stats) {
    const size_t dl = dict_len < 65536 ? dict_len : 65536;
    const int hb = dl + n <= 16384 ? 12 : HBITS_MAX;
    uint8_t *v = (uint8_t *)malloc(dl + n + 8);
    int32_t *ht = (int32_t *)malloc(sizeof(int32_t) << hb);
    int64_t r = -1;
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    if (v && ht) r = encode1(dict, dict_len, src, n, dst, cap, stats, v, ht, NULL, hb);
    free(v);
    free(ht);
    return r;
}

/* nrec records of rec_len bytes (src + i * rec_len) into slots of `slot` bytes (dst + i * slot), sizes to out_len[i].
 * shared != 0: every record with the dictionary `dict`; shared == 0: record i with the previous record (record 0 with
 * `dict`).  -> 0, or -1 */
int64_t dict_encode_batch(const uint8_t *dict, size_t dict_len, const uint8_t *src, size_t rec_len, size_t nrec,
                          int shared, uint8_t *dst, size_t slot, int64_t *out_len, uint64_t *stats) {
    const int hb = (shared ? (dict_len < 65536 ? dict_len : 65536) : rec_len) + rec_len <= 16384 ? 12 : HBITS_MAX;
    uint8_t *v = (uint8_t *)malloc(65536 + rec_len + 8);
    int32_t *ht = (int32_t *)malloc(sizeof(int32_t) << hb), *ht0 = (int32_t *)malloc(sizeof(int32_t) << hb);
    int64_t ret = -1;
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    if (!v || !ht || !ht0) goto out;
    if (shared) {   /* the dictionary's table once */
        const size_t dl = dict_len < 65536 ? dict_len : 65536;
        memcpy(v, dict + (dict_len - dl), dl);
        for (size_t i = 0; i < ((size_t)1 << hb); i++) ht0[i] = -1;
        for (size_t p = 0; p + 4 <= dl; p++) ht0[hash4(rd32(v + p), hb)] = (int32_t)p;
    }
    for (size_t i = 0; i < nrec; i++) {
        const uint8_t *d = shared || i == 0 ? dict : src + (i - 1) * rec_len;
        const size_t dl = shared || i == 0 ? dict_len : rec_len;
        out_len[i] = encode1(d, dl, src + i * rec_len, rec_len, dst + i * slot, slot, stats, v, ht, shared ? ht0 : NULL, hb);
        if (out_len[i] < 0) goto out;
    }
    ret = 0;
out:
    free(v);
    free(ht);
    free(ht0);
    return ret;
}
