/* A C99 consumer of the word-count entry points of include/jiebahip.h: jb_wc_count (the host form of the rule)
 * on spans worked out by hand, the size helpers and jb_wc_fp, then a table on the device filled by
 * jb_wc_batch in the three modes and read back, and the error returns.
 * usage: c_abi_wc <mini_dict.txt> <prob_emit.json>; exits non-zero on a mismatch. */
#include <stdio.h>
#include <string.h>

#include "jiebahip.h"

#define YI "\xE4\xB8\x80"
#define CHA "\xE5\x88\xB9"
#define NA "\xE9\x82\xA3"
#define ZHE "\xE8\xBF\x99"
/* document 0: abc \xFF 这一刹那 abc -> abc | U+FFFD | 这 | 一刹那 | abc (search adds 一刹 and 刹那 in front of 一刹那,
 * full has them around it); document 1 is empty; document 2: abc */
static const char TEXT[] = "abc \xFF" ZHE YI CHA NA " abc" "abc";
static const uint64_t DOC_OFF[] = {0, 21, 21, 24};
/* the plain cut's spans, then a reversed one and one past the end */
static const uint32_t START[] = {0, 4, 5, 8, 18, 21, 9, 20}, END[] = {3, 5, 8, 17, 21, 24, 3, 25};

static int same(const jb_wc_result *r, const char *const *keys, const uint64_t *counts, uint64_t n) {
    uint64_t i;
    if (r->nkeys != n || r->key_off[0] != 0) return 0;
    for (i = 0; i < n; i++) {
        const uint64_t len = r->key_off[i + 1] - r->key_off[i];
        if (len != strlen(keys[i]) || memcmp(r->keys + r->key_off[i], keys[i], len) != 0 || r->counts[i] != counts[i]) return 0;
    }
    return 1;
}

int main(int argc, char **argv) {
    static const char *const K_CUT[] = {"abc", YI CHA NA, ZHE, "\xEF\xBF\xBD"};
    static const uint64_t C_CUT[] = {3, 1, 1, 1};
    static const char *const K_ALL[] = {"abc", YI CHA, YI CHA NA, CHA NA, ZHE, "\xEF\xBF\xBD"};
    static const uint64_t C_ALL[] = {3, 1, 1, 1, 1, 1};
    jb_config cfg;
    jb_ctx *ctx = NULL;
    jb_wc_result r;
    void *table = NULL;
    size_t ntable;
    int ok = 1, mode, rep;
    if (argc < 3) {
        fprintf(stderr, "usage: %s mini_dict.txt prob_emit.json\n", argv[0]);
        return 2;
    }
    if (jb_wc_table_bytes(0, 0) == 0 || jb_wc_work_bytes(0) == 0 || jb_wc_table_bytes(8, 0) > jb_wc_table_bytes(9, 0) ||
        jb_wc_table_bytes(1024, 0) > jb_wc_table_bytes(1024, 1) || jb_wc_work_bytes(1) > jb_wc_work_bytes(100000) ||
        jb_wc_table_bytes(~0ull, ~0ull) < jb_wc_table_bytes(1ull << 30, 1ull << 31) || jb_wc_work_bytes(~0ull) == 0) {
        fprintf(stderr, "a size helper is wrong\n");
        ok = 0;
    }
    if (jb_wc_fp((const uint8_t *)"abc", 3, 64) == 0 || jb_wc_fp((const uint8_t *)"abc", 3, 4) >= 16 ||
        jb_wc_fp((const uint8_t *)"abc", 3, 4) == 0 || jb_wc_fp(NULL, 3, 64) != 0 || jb_wc_fp((const uint8_t *)"abc", 0, 64) != 0 ||
        jb_wc_fp((const uint8_t *)"abc", 3, 65) != 0 || jb_wc_fp((const uint8_t *)"abc", 3, 64) == jb_wc_fp((const uint8_t *)"abd", 3, 64)) {
        fprintf(stderr, "jb_wc_fp is wrong\n");
        ok = 0;
    }
    /* the host form needs no ctx */
    if (jb_wc_count((const uint8_t *)TEXT, 24, START, END, 8, 8, 1, 0, &r) != JB_OK) {
        fprintf(stderr, "jb_wc_count: %s\n", jb_last_error());
        return 1;
    }
    if (!same(&r, K_CUT, C_CUT, 4) || r.nbad != 2 || r.nlong != 0 || r.ndropped != 0 || r.ncollided != 0 || r.ntokens != 8) {
        fprintf(stderr, "jb_wc_count: %llu keys, %llu bad\n", (unsigned long long)r.nkeys, (unsigned long long)r.nbad);
        ok = 0;
    }
    jb_wc_result_free(&r);
    if (r.keys != NULL || r.key_off != NULL || r.counts != NULL) ok = 0;
    /* the filters, and the clamp to cap */
    if (jb_wc_count((const uint8_t *)TEXT, 24, START, END, 100, 6, 2, 0, &r) != JB_OK || !same(&r, K_CUT, C_CUT, 1) ||
        r.ntokens != 6 || r.nbad != 0) {
        fprintf(stderr, "jb_wc_count with min_count 2 is wrong\n");
        ok = 0;
    }
    jb_wc_result_free(&r);
    if (jb_wc_count((const uint8_t *)TEXT, 24, START, END, 8, 8, 0, 2, &r) != JB_OK || !same(&r, K_CUT, C_CUT, 2)) {
        fprintf(stderr, "jb_wc_count with max_keys 2 is wrong\n");
        ok = 0;
    }
    jb_wc_result_free(&r);
    if (jb_wc_count(NULL, 0, NULL, NULL, 5, 0, 1, 0, &r) != JB_OK || r.nkeys != 0 || r.ntokens != 0 || r.key_off == NULL ||
        r.key_off[0] != 0) {
        fprintf(stderr, "jb_wc_count of nothing is wrong\n");
        ok = 0;
    }
    jb_wc_result_free(&r);
    jb_wc_result_free(NULL);
    if (jb_wc_count((const uint8_t *)TEXT, 24, START, END, 8, 8, 1, 0, NULL) != JB_EINVAL ||
        jb_wc_count(NULL, 24, START, END, 8, 8, 1, 0, &r) != JB_EINVAL ||
        jb_wc_count((const uint8_t *)TEXT, 24, NULL, END, 8, 8, 1, 0, &r) != JB_EINVAL ||
        jb_wc_count((const uint8_t *)TEXT, 1ull << 31, START, END, 8, 8, 1, 0, &r) != JB_ELIMIT) {
        fprintf(stderr, "an error return of jb_wc_count is wrong\n");
        ok = 0;
    }
    memset(&cfg, 0, sizeof cfg);
    cfg.dict_path = argv[1];
    cfg.dict_kind = JB_DICT_TXT;
    cfg.emit_path = argv[2];
    cfg.ndevices = 1;
    if (jb_open(&cfg, &ctx) != JB_OK) {
        fprintf(stderr, "jb_open: %s\n", jb_last_error());
        return 2;
    }
    ntable = jb_wc_table_bytes(1024, 4096);
    if (jb_device_alloc(ctx, ntable, &table) != JB_OK || table == NULL) {
        fprintf(stderr, "jb_device_alloc: %s\n", jb_last_error());
        return 2;
    }
    if (jb_wc_init_device(NULL, table, ntable, 1024, 4096, NULL) != JB_EINVAL ||
        jb_wc_init_device(ctx, NULL, ntable, 1024, 4096, NULL) != JB_EINVAL ||
        jb_wc_init_device(ctx, table, ntable, 1000, 4096, NULL) != JB_EINVAL ||
        jb_wc_init_device(ctx, table, ntable, 1ull << 31, 0, NULL) != JB_ELIMIT ||
        jb_wc_init_device(ctx, table, ntable - 1, 1024, 4096, NULL) != JB_EINVAL ||
        jb_wc_init_device(ctx, (char *)table + 4, ntable, 8, 0, NULL) != JB_EINVAL ||
        jb_wc_add_device(ctx, table, ntable, NULL, 1, NULL, NULL, NULL, 0, NULL, NULL, 0) != JB_EINVAL ||
        jb_wc_add_device(ctx, table, 100, NULL, 0, NULL, NULL, (const uint64_t *)table, 0, NULL, NULL, 0) != JB_EINVAL ||
        jb_wc_add_device(ctx, table, ntable, (const uint8_t *)table, 1ull << 31, NULL, NULL, (const uint64_t *)table, 0, NULL, NULL,
                         0) != JB_ELIMIT ||
        jb_wc_read(ctx, table, ntable, NULL, 1, 0, NULL) != JB_EINVAL || jb_wc_read(ctx, NULL, ntable, NULL, 1, 0, &r) != JB_EINVAL ||
        jb_wc_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, 3, table, ntable) != JB_EINVAL ||
        jb_wc_batch(ctx, (const uint8_t *)TEXT, NULL, 3, 0, JB_MODE_CUT, table, ntable) != JB_EINVAL ||
        jb_wc_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, NULL, ntable) != JB_EINVAL) {
        fprintf(stderr, "an error return is wrong\n");
        ok = 0;
    }
    for (mode = JB_MODE_CUT; mode <= JB_MODE_FULL && ok; mode++) {
        if (jb_wc_init_device(ctx, table, ntable, 1024, 4096, NULL) != JB_OK) {
            fprintf(stderr, "jb_wc_init_device: %s\n", jb_last_error());
            ok = 0;
            break;
        }
        for (rep = 1; rep <= 2 && ok; rep++) { /* twice into one table: every count doubles */
            uint64_t want[6], i;
            const int plain = mode == JB_MODE_CUT;
            for (i = 0; i < 6; i++) want[i] = (uint64_t)rep * (plain ? C_CUT[i < 4 ? i : 3] : C_ALL[i]);
            if (jb_wc_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, mode, table, ntable) != JB_OK ||
                jb_wc_read(ctx, table, ntable, NULL, 1, 0, &r) != JB_OK) {
                fprintf(stderr, "mode %d: %s\n", mode, jb_last_error());
                ok = 0;
                break;
            }
            if (!same(&r, plain ? K_CUT : K_ALL, want, plain ? 4 : 6) || r.ntokens != (uint64_t)rep * (plain ? 6 : 8) ||
                r.nbad || r.nlong || r.ndropped || r.ncollided) {
                fprintf(stderr, "mode %d, pass %d: %llu keys of %llu tokens\n", mode, rep, (unsigned long long)r.nkeys,
                        (unsigned long long)r.ntokens);
                ok = 0;
            }
            printf("mode %d: %llu keys of %llu tokens\n", mode, (unsigned long long)r.nkeys, (unsigned long long)r.ntokens);
            jb_wc_result_free(&r);
        }
    }
    /* no document: nothing is added */
    if (ok && (jb_wc_init_device(ctx, table, ntable, 8, 0, NULL) != JB_OK ||
               jb_wc_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 0, 1, JB_MODE_CUT, table, ntable) != JB_OK ||
               jb_wc_read(ctx, table, ntable, NULL, 1, 0, &r) != JB_OK || r.nkeys != 0 || r.ntokens != 0)) {
        fprintf(stderr, "an empty batch: %s\n", jb_last_error());
        ok = 0;
    }
    jb_wc_result_free(&r);
    jb_device_free(ctx, table);
    jb_device_free(ctx, NULL);
    jb_close(ctx);
    if (ok) printf("wc ok\n");
    return ok ? 0 : 1;
}
