/* A C99 consumer of the keyword entry points of include/jiebahip.h: attaches a vocabulary, runs
 * jb_keywords_batch on two documents and compares the records with the hand-worked ones; then the
 * error returns.
 * usage: c_abi_keywords <mini_dict.txt> <prob_emit.json>; exits non-zero on a mismatch. */
#include <stdio.h>
#include <string.h>

#include "jiebahip.h"

#define U JB_ID_UNK

/* keys: abc | 今天 | U+FFFD | 一刹那 | 刹那 | 这 | 天天 */
static const char KEYS[] = "abc" "\xE4\xBB\x8A\xE5\xA4\xA9" "\xEF\xBF\xBD" "\xE4\xB8\x80\xE5\x88\xB9\xE9\x82\xA3"
                           "\xE5\x88\xB9\xE9\x82\xA3" "\xE8\xBF\x99" "\xE5\xA4\xA9\xE5\xA4\xA9";
static const uint64_t KEY_OFF[] = {0, 3, 9, 12, 21, 27, 30, 36};
#define NKEYS 7u
static const float WEIGHTS[NKEYS] = {1.0f, 1.5f, 0.5f, 2.0f, 1.0f, 0.0f, 1.0f};
#define TOPK 3u

int main(int argc, char **argv) {
    /* document 0: abc \xFF今天天氣 这一刹那 -> abc, U+FFFD, 今天, 天, 氣, 这, 一刹那 = ids 0 2 1 U U 5 3
     *   scores 1.0, 0.5, 1.5, -, -, (weight 0), 2.0          -> (3, 2.0, 1) (1, 1.5, 1) (0, 1.0, 1)
     * document 1: abc abc 今天 -> ids 0 0 1; scores 2 x 1.0, 1.5 -> (0, 2.0, 2) (1, 1.5, 1) and one empty slot */
    static const char TEXT[] = "abc \xFF" "\xE4\xBB\x8A\xE5\xA4\xA9\xE5\xA4\xA9\xE6\xB0\xA3 "
                               "\xE8\xBF\x99\xE4\xB8\x80\xE5\x88\xB9\xE9\x82\xA3"
                               "abc abc \xE4\xBB\x8A\xE5\xA4\xA9";
    static const uint64_t DOC_OFF[] = {0, 30, 44};
    static const uint32_t WANT_ID[] = {3, 1, 0, 0, 1, U}, WANT_CNT[] = {1, 1, 1, 2, 1, 0}, WANT_N[] = {3, 2};
    static const float WANT_SCORE[] = {2.0f, 1.5f, 1.0f, 2.0f, 1.5f, 0.0f};
    jb_config cfg;
    jb_ctx *ctx = NULL;
    uint32_t kid[2 * TOPK], kcnt[2 * TOPK], kn[2];
    float ksc[2 * TOPK];
    uint64_t one = 1;
    int ok = 1, rc;
    unsigned k;
    if (argc < 3) {
        fprintf(stderr, "usage: %s mini_dict.txt prob_emit.json\n", argv[0]);
        return 2;
    }
    if (sizeof TEXT - 1 != 44) {
        fprintf(stderr, "the text has %u bytes\n", (unsigned)(sizeof TEXT - 1));
        return 2;
    }
    if (jb_terms_work_bytes(1, 1) == 0 || jb_terms_work_bytes(1, 1) > jb_terms_work_bytes(100000, 1)) {
        fprintf(stderr, "jb_terms_work_bytes is wrong\n");
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
    if (jb_keywords_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, WEIGHTS, NKEYS, TOPK, kid, ksc, kcnt, kn) !=
        JB_EINVAL) {
        fprintf(stderr, "jb_keywords_batch without a vocabulary did not return JB_EINVAL\n");
        ok = 0;
    }
    if (jb_vocab_set(ctx, (const uint8_t *)KEYS, KEY_OFF, NKEYS) != JB_OK) {
        fprintf(stderr, "jb_vocab_set: %s\n", jb_last_error());
        ok = 0;
    }
    if (jb_keywords_batch(NULL, (const uint8_t *)TEXT, DOC_OFF, 2, 0, WEIGHTS, NKEYS, TOPK, kid, ksc, kcnt, kn) != JB_EINVAL ||
        jb_keywords_batch(ctx, (const uint8_t *)TEXT, NULL, 2, 0, WEIGHTS, NKEYS, TOPK, kid, ksc, kcnt, kn) != JB_EINVAL ||
        jb_keywords_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, WEIGHTS, NKEYS, TOPK, NULL, ksc, kcnt, kn) != JB_EINVAL ||
        jb_keywords_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, WEIGHTS, NKEYS, 0, kid, ksc, kcnt, kn) != JB_EINVAL ||
        jb_keywords_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, WEIGHTS, NKEYS, JB_KW_MAXK + 1, kid, ksc, kcnt, kn) !=
            JB_ELIMIT ||
        jb_keywords_device(ctx, NULL, NULL, NULL, 1, 0, NULL, 0, TOPK, NULL, kid, ksc, kcnt, kn) != JB_EINVAL ||
        jb_terms_device(ctx, NULL, 0, NULL, &one, 1, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0) != JB_EINVAL) {
        fprintf(stderr, "an error return is wrong\n");
        ok = 0;
    }
    for (k = 0; k < 2 && ok; k++) { /* twice: the call leaves nothing behind */
        unsigned i;
        memset(kid, 0x55, sizeof kid);
        memset(ksc, 0x55, sizeof ksc);
        memset(kcnt, 0x55, sizeof kcnt);
        memset(kn, 0x55, sizeof kn);
        rc = jb_keywords_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, WEIGHTS, NKEYS, TOPK, kid, ksc, kcnt, kn);
        if (rc != JB_OK) {
            fprintf(stderr, "jb_keywords_batch: %s\n", jb_last_error());
            ok = 0;
            break;
        }
        for (i = 0; i < 2 * TOPK; i++)
            if (kid[i] != WANT_ID[i] || kcnt[i] != WANT_CNT[i] || memcmp(&ksc[i], &WANT_SCORE[i], sizeof(float)) != 0) {
                fprintf(stderr, "record %u is (%u, %g, %u), want (%u, %g, %u)\n", i, kid[i], (double)ksc[i], kcnt[i],
                        WANT_ID[i], (double)WANT_SCORE[i], WANT_CNT[i]);
                ok = 0;
            }
        if (kn[0] != WANT_N[0] || kn[1] != WANT_N[1]) {
            fprintf(stderr, "kw_n is %u %u\n", kn[0], kn[1]);
            ok = 0;
        }
    }
    /* no document: nothing to do */
    if (ok && jb_keywords_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 0, 1, WEIGHTS, NKEYS, TOPK, NULL, NULL, NULL, NULL) != JB_OK) {
        fprintf(stderr, "an empty batch: %s\n", jb_last_error());
        ok = 0;
    }
    jb_close(ctx);
    if (ok) printf("keywords ok\n");
    return ok ? 0 : 1;
}
