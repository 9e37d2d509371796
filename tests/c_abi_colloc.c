/* A C99 consumer of the collocation entry points of include/jiebahip.h: jb_colloc_count and jb_colloc_score (the
 * host form of the rule) on ids worked out by hand, the size helpers, then a table on the device filled by
 * jb_colloc_batch and read back under the three scorers, and the error returns.
 * usage: c_abi_colloc <mini_dict.txt> <prob_emit.json>; exits non-zero on a mismatch. */
#include <stdio.h>
#include <string.h>

#include "jiebahip.h"

#define YI "\xE4\xB8\x80"
#define CHA "\xE5\x88\xB9"
#define NA "\xE9\x82\xA3"
#define ZHE "\xE8\xBF\x99"
/* the vocabulary: abc = 0, 一刹那 = 1, 这 = 2.  Document 0: 这一刹那 abc abc -> 2 1 0 0; document 1 is empty;
 * document 2: abc这 -> 0 2 */
static const char KEYS[] = "abc" YI CHA NA ZHE;
static const uint64_t KEY_OFF[] = {0, 3, 12, 15};
static const char TEXT[] = ZHE YI CHA NA " abc abc" "abc" ZHE;
static const uint64_t DOC_OFF[] = {0, 20, 20, 26};
static const uint32_t IDS[] = {2, 1, 0, 0, 0, 2};
static const uint64_t DOC_TOK[] = {0, 4, 4, 6};
static const uint32_t START[] = {0, 3, 13, 17, 20, 23}, END[] = {3, 12, 16, 20, 23, 26};

static int same(const jb_colloc_result *r, const uint32_t *a, const uint32_t *b, const uint64_t *c, uint64_t n) {
    uint64_t i;
    if (r->n != n) return 0;
    for (i = 0; i < n; i++)
        if (r->a[i] != a[i] || r->b[i] != b[i] || r->count[i] != c[i]) return 0;
    return 1;
}

int main(int argc, char **argv) {
    /* sorted by key: (0,0) (0,2) (1,0) (2,1); with JB_COLLOC_CONTIG only 这|一刹那 and abc|这 touch */
    static const uint32_t A_ALL[] = {0, 0, 1, 2}, B_ALL[] = {0, 2, 0, 1}, A_CON[] = {0, 2}, B_CON[] = {2, 1};
    static const uint64_t C_ONE[] = {1, 1, 1, 1}, C_TWO[] = {2, 2, 2, 2};
    static const uint8_t KEEP[] = {1, 0, 1};
    uint64_t uni[3] = {0, 0, 0};
    jb_config cfg;
    jb_ctx *ctx = NULL;
    jb_colloc_result r;
    void *table = NULL, *d_uni = NULL;
    size_t ntable;
    int ok = 1, rep;
    if (argc < 3) {
        fprintf(stderr, "usage: %s mini_dict.txt prob_emit.json\n", argv[0]);
        return 2;
    }
    if (jb_colloc_table_bytes(0) == 0 || jb_colloc_work_bytes(0, 0) == 0 || jb_colloc_table_bytes(8) > jb_colloc_table_bytes(9) ||
        jb_colloc_work_bytes(1, 0) > jb_colloc_work_bytes(100000, 0) || jb_colloc_work_bytes(5, 1) > jb_colloc_work_bytes(5, 2) ||
        jb_colloc_table_bytes(~0ull) < jb_colloc_table_bytes(1ull << 30) || jb_colloc_work_bytes(~0ull, ~0u) == 0) {
        fprintf(stderr, "a size helper is wrong\n");
        ok = 0;
    }
    /* the host form needs no ctx */
    if (jb_colloc_count(IDS, 6, DOC_TOK, 6, 3, NULL, 0, 0, NULL, NULL, 0, uni, 3, &r) != JB_OK) {
        fprintf(stderr, "jb_colloc_count: %s\n", jb_last_error());
        return 1;
    }
    if (!same(&r, A_ALL, B_ALL, C_ONE, 4) || r.tokens != 6 || r.known != 6 || r.pairs != 4 || r.dropped != 0 || r.distinct != 4 ||
        uni[0] != 3 || uni[1] != 1 || uni[2] != 2) {
        fprintf(stderr, "jb_colloc_count: %llu pairs\n", (unsigned long long)r.n);
        ok = 0;
    }
    jb_colloc_result_free(&r);
    if (r.a != NULL || r.b != NULL || r.count != NULL || r.score != NULL) ok = 0;
    if (jb_colloc_count(IDS, 6, DOC_TOK, 6, 3, NULL, 0, JB_COLLOC_CONTIG, START, END, 0, uni, 3, &r) != JB_OK ||
        !same(&r, A_CON, B_CON, C_ONE, 2) || uni[0] != 6) {
        fprintf(stderr, "jb_colloc_count with JB_COLLOC_CONTIG is wrong\n");
        ok = 0;
    }
    jb_colloc_result_free(&r);
    /* keep drops 一刹那: only abc|abc and abc|这 are left; the unigrams do not care */
    if (jb_colloc_count(IDS, 6, DOC_TOK, 6, 3, KEEP, 3, 0, NULL, NULL, 8, uni, 3, &r) != JB_OK || !same(&r, A_ALL, B_ALL, C_ONE, 2) ||
        uni[1] != 3) {
        fprintf(stderr, "jb_colloc_count with a keep mask is wrong\n");
        ok = 0;
    }
    jb_colloc_result_free(&r);
    /* scores: COUNT orders by count, then by key; a threshold above every score leaves nothing */
    if (jb_colloc_score(A_ALL, B_ALL, C_TWO, 4, uni, 3, 18, JB_COLLOC_COUNT, 1, 0.0f, 3, &r) != JB_OK ||
        !same(&r, A_ALL, B_ALL, C_TWO, 3) || r.score[0] != 2.0f) {
        fprintf(stderr, "jb_colloc_score is wrong\n");
        ok = 0;
    }
    jb_colloc_result_free(&r);
    if (jb_colloc_score(A_ALL, B_ALL, C_TWO, 4, uni, 3, 18, JB_COLLOC_NPMI, 1, 1.5f, 0, &r) != JB_OK || r.n != 0) ok = 0;
    jb_colloc_result_free(&r);
    jb_colloc_result_free(NULL);
    if (jb_colloc_count(IDS, 6, DOC_TOK, 6, 3, NULL, 0, 0, NULL, NULL, 0, uni, 3, NULL) != JB_EINVAL ||
        jb_colloc_count(NULL, 6, DOC_TOK, 6, 3, NULL, 0, 0, NULL, NULL, 0, uni, 3, &r) != JB_EINVAL ||
        jb_colloc_count(IDS, 6, DOC_TOK, 6, 3, NULL, 0, JB_COLLOC_CONTIG, NULL, NULL, 0, uni, 3, &r) != JB_EINVAL ||
        jb_colloc_count(IDS, 6, DOC_TOK, 6, 3, NULL, 0, 0, NULL, NULL, 12, uni, 3, &r) != JB_EINVAL ||
        jb_colloc_score(A_ALL, B_ALL, C_TWO, 4, uni, 3, 18, JB_COLLOC_COUNT, 0, 0.0f, 0, &r) != JB_EINVAL ||
        jb_colloc_score(A_ALL, B_ALL, C_TWO, 4, uni, 3, 18, 7, 1, 0.0f, 0, &r) != JB_EINVAL) {
        fprintf(stderr, "an error return of the host rule is wrong\n");
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
    ntable = jb_colloc_table_bytes(1024);
    if (jb_device_alloc(ctx, ntable, &table) != JB_OK || jb_device_alloc(ctx, 3 * 8, &d_uni) != JB_OK) {
        fprintf(stderr, "jb_device_alloc: %s\n", jb_last_error());
        return 2;
    }
    if (jb_colloc_init_device(NULL, table, ntable, 1024, (uint64_t *)d_uni, 3, NULL) != JB_EINVAL ||
        jb_colloc_init_device(ctx, NULL, ntable, 1024, (uint64_t *)d_uni, 3, NULL) != JB_EINVAL ||
        jb_colloc_init_device(ctx, table, ntable, 1000, (uint64_t *)d_uni, 3, NULL) != JB_EINVAL ||
        jb_colloc_init_device(ctx, table, ntable, 1ull << 31, (uint64_t *)d_uni, 3, NULL) != JB_ELIMIT ||
        jb_colloc_init_device(ctx, table, ntable - 1, 1024, (uint64_t *)d_uni, 3, NULL) != JB_EINVAL ||
        jb_colloc_init_device(ctx, (char *)table + 4, ntable, 8, (uint64_t *)d_uni, 3, NULL) != JB_EINVAL ||
        jb_colloc_init_device(ctx, table, ntable, 1024, NULL, 3, NULL) != JB_EINVAL ||
        jb_colloc_read(ctx, table, ntable, (const uint64_t *)d_uni, 3, JB_COLLOC_COUNT, 1, 0.0f, 0, NULL, NULL) != JB_EINVAL ||
        jb_colloc_read(ctx, NULL, ntable, (const uint64_t *)d_uni, 3, JB_COLLOC_COUNT, 1, 0.0f, 0, NULL, &r) != JB_EINVAL ||
        /* no vocabulary yet */
        jb_colloc_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, NULL, 0, 0, table, ntable, (uint64_t *)d_uni, 3) != JB_EINVAL) {
        fprintf(stderr, "an error return is wrong\n");
        ok = 0;
    }
    if (jb_vocab_set(ctx, (const uint8_t *)KEYS, KEY_OFF, 3) != JB_OK) {
        fprintf(stderr, "jb_vocab_set: %s\n", jb_last_error());
        return 2;
    }
    if (jb_colloc_batch(ctx, (const uint8_t *)TEXT, NULL, 3, 0, NULL, 0, 0, table, ntable, (uint64_t *)d_uni, 3) != JB_EINVAL ||
        jb_colloc_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, NULL, 0, 2, table, ntable, (uint64_t *)d_uni, 3) != JB_EINVAL ||
        jb_colloc_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, NULL, 0, 0, NULL, ntable, (uint64_t *)d_uni, 3) != JB_EINVAL) {
        fprintf(stderr, "an error return of jb_colloc_batch is wrong\n");
        ok = 0;
    }
    if (ok && jb_colloc_init_device(ctx, table, ntable, 1024, (uint64_t *)d_uni, 3, NULL) != JB_OK) {
        fprintf(stderr, "jb_colloc_init_device: %s\n", jb_last_error());
        ok = 0;
    }
    for (rep = 1; rep <= 2 && ok; rep++) { /* twice into one table: every count doubles */
        if (jb_colloc_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, NULL, 0, 0, table, ntable, (uint64_t *)d_uni, 3) != JB_OK ||
            jb_colloc_read(ctx, table, ntable, (const uint64_t *)d_uni, 3, JB_COLLOC_COUNT, 1, 0.0f, 0, NULL, &r) != JB_OK) {
            fprintf(stderr, "pass %d: %s\n", rep, jb_last_error());
            ok = 0;
            break;
        }
        if (!same(&r, A_ALL, B_ALL, rep == 1 ? C_ONE : C_TWO, 4) || r.tokens != 6u * (unsigned)rep || r.known != r.tokens ||
            r.pairs != 4u * (unsigned)rep || r.dropped != 0 || r.distinct != 4) {
            fprintf(stderr, "pass %d: %llu pairs of %llu tokens\n", rep, (unsigned long long)r.n, (unsigned long long)r.tokens);
            ok = 0;
        }
        printf("pass %d: %llu pairs of %llu tokens\n", rep, (unsigned long long)r.n, (unsigned long long)r.tokens);
        jb_colloc_result_free(&r);
    }
    /* NPMI on the device equals the host rule over the same counts (uni is 6 2 4 after two passes) */
    if (ok) {
        jb_colloc_result h;
        const uint64_t u2[3] = {6, 2, 4};
        if (jb_colloc_read(ctx, table, ntable, (const uint64_t *)d_uni, 3, JB_COLLOC_NPMI, 2, -1.0f, 0, NULL, &r) != JB_OK ||
            jb_colloc_score(A_ALL, B_ALL, C_TWO, 4, u2, 3, 12, JB_COLLOC_NPMI, 2, -1.0f, 0, &h) != JB_OK || r.n != 4 ||
            !same(&r, h.a, h.b, h.count, h.n) || memcmp(r.score, h.score, 4 * sizeof(float)) != 0) {
            fprintf(stderr, "NPMI: the device differs from the host rule\n");
            ok = 0;
        }
        jb_colloc_result_free(&r);
        jb_colloc_result_free(&h);
    }
    /* contiguous pairs only, into an emptied table; no document: nothing is added */
    if (ok && (jb_colloc_init_device(ctx, table, ntable, 8, (uint64_t *)d_uni, 3, NULL) != JB_OK ||
               jb_colloc_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 0, 1, NULL, 0, 0, table, ntable, (uint64_t *)d_uni, 3) != JB_OK ||
               jb_colloc_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, NULL, 0, JB_COLLOC_CONTIG, table, ntable, (uint64_t *)d_uni,
                               3) != JB_OK ||
               jb_colloc_read(ctx, table, ntable, (const uint64_t *)d_uni, 3, JB_COLLOC_COUNT, 1, 0.0f, 0, NULL, &r) != JB_OK ||
               !same(&r, A_CON, B_CON, C_ONE, 2) || r.tokens != 6)) {
        fprintf(stderr, "the contiguous batch: %s\n", jb_last_error());
        ok = 0;
    }
    jb_colloc_result_free(&r);
    jb_device_free(ctx, d_uni);
    jb_device_free(ctx, table);
    jb_close(ctx);
    if (ok) printf("colloc ok\n");
    return ok ? 0 : 1;
}
