/* A C99 consumer of the search-mode entry points of include/jiebahip.h: opens a small
 * dictionary, calls jb_cut_search and jb_cut_batch_search and compares the spans with the
 * hand-checked ones.  usage: c_abi_search <prob_emit.json>; exits non-zero on a mismatch. */
#include <stdio.h>
#include <string.h>

#include "jiebahip.h"

static const char DICT[] =
    "\xE7\x94\xB2 10\n"                                     /* 甲 */
    "\xE7\x94\xB2\xE4\xB9\x99 20\n"                         /* 甲乙 */
    "\xE7\x94\xB2\xE4\xB9\x99\xE4\xB8\x99 30\n"             /* 甲乙丙 */
    "\xE7\x94\xB2\xE4\xB9\x99\xE4\xB8\x99\xE4\xB8\x81 40\n" /* 甲乙丙丁 */
    "\xE4\xB9\x99 0\n"                                      /* 乙 */
    "\xE4\xB9\x99\xE4\xB8\x99 50\n"                         /* 乙丙 */
    "\xE4\xB8\x99 5\n"                                      /* 丙 */
    "\xE4\xB8\x99\xE4\xB8\x81 60\n"                         /* 丙丁 */
    "\xE4\xB8\x81 7\n";                                     /* 丁 */

#define JIA "\xE7\x94\xB2"
#define YI "\xE4\xB9\x99"
#define BING "\xE4\xB8\x99"
#define DING "\xE4\xB8\x81"

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
    /* x甲乙丙丁y 甲乙丙丁丁 -> x, 甲乙, 丙丁, 甲乙丙, 甲乙丙丁, y, 甲乙, 丙丁, 甲乙丙, 甲乙丙丁, 丁 */
    static const char T1[] = "x" JIA YI BING DING "y " JIA YI BING DING DING;
    static const uint64_t S1[] = {0, 1, 7, 1, 1, 13, 15, 21, 15, 15, 27};
    static const uint64_t E1[] = {1, 7, 13, 10, 13, 14, 21, 27, 24, 27, 30};
    static const uint64_t D1[] = {0, 11};
    /* documents 甲乙丙丁 and 甲乙丙 -> 甲乙, 丙丁, 甲乙丙, 甲乙丙丁 | 甲乙, 甲乙丙 */
    static const char T2[] = JIA YI BING DING JIA YI BING;
    static const uint64_t OFF2[] = {0, 12, 21};
    static const uint64_t S2[] = {0, 6, 0, 0, 12, 12};
    static const uint64_t E2[] = {6, 12, 9, 12, 18, 21};
    static const uint64_t D2[] = {0, 4, 6};
    jb_config cfg;
    jb_ctx *ctx = NULL;
    jb_spans sp;
    int hmm, ok = 1;
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
    if (jb_cut_search(NULL, (const uint8_t *)T1, sizeof T1 - 1, 0, &sp) != JB_EINVAL) {
        fprintf(stderr, "jb_cut_search(NULL ctx) did not return JB_EINVAL\n");
        ok = 0;
    }
    for (hmm = 0; hmm <= 1 && ok; hmm++) {
        if (jb_cut_search(ctx, (const uint8_t *)T1, sizeof T1 - 1, hmm, &sp) != JB_OK) {
            fprintf(stderr, "jb_cut_search: %s\n", jb_last_error());
            ok = 0;
            break;
        }
        ok = same("jb_cut_search", &sp, S1, E1, sizeof S1 / sizeof *S1, D1, 1);
        jb_spans_free(&sp);
        if (!ok) break;
        if (jb_cut_batch_search(ctx, (const uint8_t *)T2, OFF2, 2, hmm, &sp) != JB_OK) {
            fprintf(stderr, "jb_cut_batch_search: %s\n", jb_last_error());
            ok = 0;
            break;
        }
        ok = same("jb_cut_batch_search", &sp, S2, E2, sizeof S2 / sizeof *S2, D2, 2);
        jb_spans_free(&sp);
    }
    jb_close(ctx);
    if (ok) printf("search ok\n");
    return ok ? 0 : 1;
}
