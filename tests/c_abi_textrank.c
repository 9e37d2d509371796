/* A C99 consumer of the TextRank entry points of include/jiebahip.h: attaches a vocabulary, runs
 * jb_textrank_batch on two documents, compares the records bit for bit with jb_textrank (the host form
 * of the rule) on the ids worked out by hand, and prints them; then the error returns.
 * usage: c_abi_textrank <mini_dict.txt> <prob_emit.json>; exits non-zero on a mismatch. */
#include <stdio.h>
#include <string.h>

#include "jiebahip.h"

#define U JB_ID_UNK

/* keys: abc | 今天 | U+FFFD | 一刹那 | 刹那 | 这 | 天天 */
static const char KEYS[] = "abc" "\xE4\xBB\x8A\xE5\xA4\xA9" "\xEF\xBF\xBD" "\xE4\xB8\x80\xE5\x88\xB9\xE9\x82\xA3"
                           "\xE5\x88\xB9\xE9\x82\xA3" "\xE8\xBF\x99" "\xE5\xA4\xA9\xE5\xA4\xA9";
static const uint64_t KEY_OFF[] = {0, 3, 9, 12, 21, 27, 30, 36};
#define NKEYS 7u
static const uint8_t KEEP[NKEYS] = {1, 1, 1, 1, 1, 0, 1}; /* 这 is a stop word */
#define TOPK 3u
#define SPAN 5u
#define ITERS 10u

int main(int argc, char **argv) {
    /* document 0: abc \xFF今天天氣 这一刹那 -> abc, U+FFFD, 今天, 天, 氣, 这, 一刹那 = ids 0 2 1 U U 5 3
     *   kept: 0 2 1 . . . 3; events within 5 positions: 0-2, 0-1, 2-1, 1-3 -> nodes 0 1 2 3
     * document 1: abc abc 今天 -> ids 0 0 1; events 0-0, 0-1, 0-1 -> nodes 0 1 */
    static const char TEXT[] = "abc \xFF" "\xE4\xBB\x8A\xE5\xA4\xA9\xE5\xA4\xA9\xE6\xB0\xA3 "
                               "\xE8\xBF\x99\xE4\xB8\x80\xE5\x88\xB9\xE9\x82\xA3"
                               "abc abc \xE4\xBB\x8A\xE5\xA4\xA9";
    static const uint64_t DOC_OFF[] = {0, 30, 44};
    static const uint32_t IDS[] = {0, 2, 1, U, U, 5, 3, 0, 0, 1};
    static const uint64_t DOC_TOK[] = {0, 7, 10};
    static const uint32_t TERM_ID[] = {0, 1, 2, 3, 5, 0, 1};
    static const uint64_t TERM_OFF[] = {0, 5, 7};
    jb_config cfg;
    jb_ctx *ctx = NULL;
    uint32_t kid[2 * TOPK], kn[2], hid[2 * TOPK], hn[2];
    float ksc[2 * TOPK], hsc[2 * TOPK];
    int ok = 1, rc;
    unsigned k, d;
    if (argc < 3) {
        fprintf(stderr, "usage: %s mini_dict.txt prob_emit.json\n", argv[0]);
        return 2;
    }
    if (jb_textrank_work_bytes(0, 0, 0) == 0 || jb_textrank_work_bytes(1, 1, 1) > jb_textrank_work_bytes(100000, 1, 1) ||
        jb_textrank_work_bytes(1, 1, 1) > jb_textrank_work_bytes(1, 100000, 1)) {
        fprintf(stderr, "jb_textrank_work_bytes is wrong\n");
        ok = 0;
    }
    /* the host form needs no ctx */
    rc = jb_textrank(IDS, 10, DOC_TOK, 10, 2, TERM_ID, TERM_OFF, 7, KEEP, NKEYS, SPAN, ITERS, TOPK, hid, hsc, hn);
    if (rc != JB_OK) {
        fprintf(stderr, "jb_textrank: %s\n", jb_last_error());
        return 1;
    }
    if (hn[0] != 3 || hn[1] != 2 || hid[5] != U || hsc[5] != 0.0f || hsc[0] != 1.0f || hsc[3] != 1.0f || hid[3] != 0) {
        fprintf(stderr, "jb_textrank: kw_n %u %u, first records %u %g, %u %g\n", hn[0], hn[1], hid[0], (double)hsc[0],
                hid[3], (double)hsc[3]);
        ok = 0;
    }
    if (jb_textrank(IDS, 10, DOC_TOK, 10, 2, TERM_ID, TERM_OFF, 7, KEEP, NKEYS, 1, ITERS, TOPK, hid, hsc, hn) != JB_EINVAL ||
        jb_textrank(IDS, 10, DOC_TOK, 10, 2, TERM_ID, TERM_OFF, 7, KEEP, NKEYS, JB_TR_MAXSPAN + 1, ITERS, TOPK, hid, hsc, hn) !=
            JB_ELIMIT ||
        jb_textrank(IDS, 10, DOC_TOK, 10, 2, TERM_ID, TERM_OFF, 7, KEEP, NKEYS, SPAN, JB_TR_MAXITER + 1, TOPK, hid, hsc, hn) !=
            JB_ELIMIT ||
        jb_textrank(IDS, 10, DOC_TOK, 10, 2, TERM_ID, TERM_OFF, 7, KEEP, NKEYS, SPAN, ITERS, JB_KW_MAXK + 1, hid, hsc, hn) !=
            JB_ELIMIT ||
        jb_textrank(NULL, 10, DOC_TOK, 10, 2, TERM_ID, TERM_OFF, 7, KEEP, NKEYS, SPAN, ITERS, TOPK, hid, hsc, hn) != JB_EINVAL) {
        fprintf(stderr, "an error return of jb_textrank is wrong\n");
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
    /* no vocabulary attached yet */
    if (jb_textrank_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, KEEP, NKEYS, SPAN, ITERS, TOPK, kid, ksc, kn) != JB_EINVAL) {
        fprintf(stderr, "jb_textrank_batch without a vocabulary did not return JB_EINVAL\n");
        ok = 0;
    }
    if (jb_vocab_set(ctx, (const uint8_t *)KEYS, KEY_OFF, NKEYS) != JB_OK) {
        fprintf(stderr, "jb_vocab_set: %s\n", jb_last_error());
        ok = 0;
    }
    if (jb_textrank_batch(NULL, (const uint8_t *)TEXT, DOC_OFF, 2, 0, KEEP, NKEYS, SPAN, ITERS, TOPK, kid, ksc, kn) != JB_EINVAL ||
        jb_textrank_batch(ctx, (const uint8_t *)TEXT, NULL, 2, 0, KEEP, NKEYS, SPAN, ITERS, TOPK, kid, ksc, kn) != JB_EINVAL ||
        jb_textrank_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, NULL, NKEYS, SPAN, ITERS, TOPK, kid, ksc, kn) != JB_EINVAL ||
        jb_textrank_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, KEEP, NKEYS, SPAN, ITERS, TOPK, NULL, ksc, kn) != JB_EINVAL ||
        jb_textrank_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, KEEP, NKEYS, SPAN, ITERS, 0, kid, ksc, kn) != JB_EINVAL ||
        jb_textrank_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, KEEP, NKEYS, 1, ITERS, TOPK, kid, ksc, kn) != JB_EINVAL ||
        jb_textrank_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, KEEP, NKEYS, SPAN, ITERS, JB_KW_MAXK + 1, kid, ksc, kn) !=
            JB_ELIMIT ||
        jb_textrank_device(ctx, NULL, 0, NULL, NULL, 1, NULL, NULL, 0, NULL, 0, SPAN, ITERS, TOPK, NULL, kid, ksc, kn, NULL, 0) !=
            JB_EINVAL) {
        fprintf(stderr, "an error return is wrong\n");
        ok = 0;
    }
    for (k = 0; k < 2 && ok; k++) { /* twice: the call leaves nothing behind */
        unsigned i;
        memset(kid, 0x55, sizeof kid);
        memset(ksc, 0x55, sizeof ksc);
        memset(kn, 0x55, sizeof kn);
        rc = jb_textrank_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, KEEP, NKEYS, SPAN, ITERS, TOPK, kid, ksc, kn);
        if (rc != JB_OK) {
            fprintf(stderr, "jb_textrank_batch: %s\n", jb_last_error());
            ok = 0;
            break;
        }
        for (i = 0; i < 2 * TOPK; i++)
            if (kid[i] != hid[i] || memcmp(&ksc[i], &hsc[i], sizeof(float)) != 0) {
                fprintf(stderr, "record %u is (%u, %g), jb_textrank says (%u, %g)\n", i, kid[i], (double)ksc[i], hid[i],
                        (double)hsc[i]);
                ok = 0;
            }
        if (kn[0] != hn[0] || kn[1] != hn[1]) {
            fprintf(stderr, "kw_n is %u %u\n", kn[0], kn[1]);
            ok = 0;
        }
    }
    for (d = 0; d < 2 && ok; d++) {
        printf("n %u %u\n", d, kn[d]);
        for (k = 0; k < TOPK; k++) {
            uint32_t bits;
            memcpy(&bits, &ksc[d * TOPK + k], 4);
            printf("rec %u %u %u %08x\n", d, k, kid[d * TOPK + k], bits);
        }
    }
    /* no document: nothing to do */
    if (ok && jb_textrank_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 0, 1, KEEP, NKEYS, SPAN, ITERS, TOPK, NULL, NULL, NULL) != JB_OK) {
        fprintf(stderr, "an empty batch: %s\n", jb_last_error());
        ok = 0;
    }
    jb_close(ctx);
    if (ok) printf("textrank ok\n");
    return ok ? 0 : 1;
}
