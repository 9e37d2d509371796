/* A C99 consumer of the full-mode entry points of include/jiebahip.h: opens a small
 * dictionary, calls jb_cut_full and jb_cut_batch_full and compares the spans with the
 * hand-worked ones.  usage: c_abi_full <prob_emit.json>; exits non-zero on a mismatch. */
#include <stdio.h>
#include <string.h>

#include "jiebahip.h"

static const char DICT[] =
    "\xE7\x94\xB2 5\n"                                     /* 甲 */
    "\xE7\x94\xB2\xE4\xB9\x99 5\n"                         /* 甲乙 */
    "\xE7\x94\xB2\xE4\xB9\x99\xE4\xB8\x99 0\n"             /* 甲乙丙 */
    "\xE7\x94\xB2\xE4\xB9\x99\xE4\xB8\x99\xE4\xB8\x81 5\n" /* 甲乙丙丁 */
    "\xE4\xB9\x99 5\n"                                     /* 乙 */
    "\xE4\xB9\x99\xE4\xB8\x99 5\n"                         /* 乙丙 */
    "\xE4\xB8\x99 5\n"                                     /* 丙 */
    "\xE4\xB8\x81 5\n";                                    /* 丁 */

#define JIA "\xE7\x94\xB2"
#define YI "\xE4\xB9\x99"
#define BING "\xE4\xB8\x99"
#define DING "\xE4\xB8\x81"
#define WU "\xE6\x88\x8A"

static int same(const char *what, const jb_spans *sp, const uint64_t *s, const uint64_t *e, uint64_t n,
                const uint64_t *dt, uint32_t ndocs) {
    uint64_t k;
    uint32_t d;
    if (sp->ntokens != n || sp->ndocs != ndocs) {
        fprintf(stderr, "%s: %llu spans of %u documents, want %llu of %u\n", what, (unsigned long long)sp->ntokens,
                sp->ndocs, (unsigned long long)n, ndocs);
        return 0;
    }
    for (k = 0; k < n; k++)
        if (sp->start[k] != s[k] || sp->end[k] != e[k]) {
            fprintf(stderr, "%s: span %llu is [%llu, %llu), want [%llu, %llu)\n", what, (unsigned long long)k,
                    (unsigned long long)sp->start[k], (unsigned long long)sp->end[k], (unsigned long long)s[k],
                    (unsigned long long)e[k]);
            return 0;
        }
    for (d = 0; d <= ndocs; d++)
        if (sp->doc_tok[d] != dt[d]) {
            fprintf(stderr, "%s: doc_tok[%u] = %llu, want %llu\n", what, d, (unsigned long long)sp->doc_tok[d],
                    (unsigned long long)dt[d]);
            return 0;
        }
    return 1;
}

int main(int argc, char **argv) {
    /* 甲乙丙丁戊丁 -> 甲乙, 甲乙丙丁, 乙丙, 丁, 戊, 丁: 丙 is dropped (乙丙 reaches past it), the first 丁 is
     * not (the nearest rune with words is 乙, and 乙丙 ends before it) */
    static const char T1[] = JIA YI BING DING WU DING;
    static const uint64_t S1[] = {0, 0, 3, 9, 12, 15};
    static const uint64_t E1[] = {6, 12, 9, 12, 15, 18};
    static const uint64_t D1[] = {0, 6};
    /* documents x甲乙 and 丙丁y -> x, 甲乙 | 丙, 丁, y: no word crosses the document end */
    static const char T2[] = "x" JIA YI BING DING "y";
    static const uint64_t OFF2[] = {0, 7, 14};
    static const uint64_t S2[] = {0, 1, 7, 10, 13};
    static const uint64_t E2[] = {1, 7, 10, 13, 14};
    static const uint64_t D2[] = {0, 2, 5};
    jb_config cfg;
    jb_ctx *ctx = NULL;
    jb_spans sp;
    uint32_t *ds = NULL, *de = NULL;
    uint64_t *dd = NULL, *dn = NULL;
    int ok = 1, rep;
    if (argc < 2) {
        fprintf(stderr, "usage: %s prob_emit.json\n", argv[0]);
        return 2;
    }
    memset(&cfg, 0, sizeof cfg);
    cfg.dict_buf = DICT;
    cfg.dict_len = sizeof DICT - 1;
    cfg.dict_kind = JB_DICT_TXT;
    cfg.emit_path = argv[1];
    cfg.ndevices = 1;
    if (jb_open(&cfg, &ctx) != JB_OK) {
        fprintf(stderr, "jb_open: %s\n", jb_last_error());
        return 2;
    }
    if (jb_cut_full(NULL, (const uint8_t *)T1, sizeof T1 - 1, &sp) != JB_EINVAL ||
        jb_cut_device_full(NULL, NULL, 0, NULL, 0, NULL, &ds, &de, &dd, &dn) != JB_EINVAL ||
        jb_cut_device_full_into(ctx, NULL, 0, OFF2, 0, NULL, NULL, NULL, 0, NULL, NULL) != JB_EINVAL) {
        fprintf(stderr, "a null argument did not return JB_EINVAL\n");
        ok = 0;
    }
    for (rep = 0; rep < 2 && ok; rep++) {
        if (jb_cut_full(ctx, (const uint8_t *)T1, sizeof T1 - 1, &sp) != JB_OK) {
            fprintf(stderr, "jb_cut_full: %s\n", jb_last_error());
            ok = 0;
            break;
        }
        ok = same("jb_cut_full", &sp, S1, E1, sizeof S1 / sizeof *S1, D1, 1);
        jb_spans_free(&sp);
        if (!ok) break;
        if (jb_cut_batch_full(ctx, (const uint8_t *)T2, OFF2, 2, &sp) != JB_OK) {
            fprintf(stderr, "jb_cut_batch_full: %s\n", jb_last_error());
            ok = 0;
            break;
        }
        ok = same("jb_cut_batch_full", &sp, S2, E2, sizeof S2 / sizeof *S2, D2, 2);
        jb_spans_free(&sp);
    }
    jb_close(ctx);
    if (ok) printf("full ok\n");
    return ok ? 0 : 1;
}
