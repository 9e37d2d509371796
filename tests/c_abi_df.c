/* A C99 consumer of the document-frequency entry points of include/jiebahip.h: attaches a vocabulary,
 * fits document frequencies on five documents in two batches with jb_df_batch, turns them into weights
 * with jb_idf and prints both (the test compares them with its reference); then the error returns.
 * usage: c_abi_df <mini_dict.txt> <prob_emit.json>; exits non-zero on a failure. */
#include <stdio.h>
#include <string.h>

#include "jiebahip.h"

/* keys: abc | 今天 | U+FFFD | 一刹那 | 刹那 | 这 | 天天 */
static const char KEYS[] = "abc" "\xE4\xBB\x8A\xE5\xA4\xA9" "\xEF\xBF\xBD" "\xE4\xB8\x80\xE5\x88\xB9\xE9\x82\xA3"
                           "\xE5\x88\xB9\xE9\x82\xA3" "\xE8\xBF\x99" "\xE5\xA4\xA9\xE5\xA4\xA9";
static const uint64_t KEY_OFF[] = {0, 3, 9, 12, 21, 27, 30, 36};
#define NKEYS 7u
#define NDOCS 5u

int main(int argc, char **argv) {
    /* abc abc 今天 | abc \xFF今天天氣 这一刹那 | 这一刹那 今天 | (empty) | 刹那 abc */
    static const char TEXT[] = "abc abc \xE4\xBB\x8A\xE5\xA4\xA9"
                               "abc \xFF" "\xE4\xBB\x8A\xE5\xA4\xA9\xE5\xA4\xA9\xE6\xB0\xA3 "
                               "\xE8\xBF\x99\xE4\xB8\x80\xE5\x88\xB9\xE9\x82\xA3"
                               "\xE8\xBF\x99\xE4\xB8\x80\xE5\x88\xB9\xE9\x82\xA3 \xE4\xBB\x8A\xE5\xA4\xA9"
                               "\xE5\x88\xB9\xE9\x82\xA3 abc";
    static const uint64_t DOC_OFF[NDOCS + 1] = {0, 14, 44, 63, 63, 73};
    jb_config cfg;
    jb_ctx *ctx = NULL;
    uint32_t df[NKEYS + 1], bits;
    float w[NKEYS + 1];
    int ok = 1;
    unsigned i;
    if (argc < 3) {
        fprintf(stderr, "usage: %s mini_dict.txt prob_emit.json\n", argv[0]);
        return 2;
    }
    if (sizeof TEXT - 1 != 73) {
        fprintf(stderr, "the text has %u bytes\n", (unsigned)(sizeof TEXT - 1));
        return 2;
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
    memset(df, 0, sizeof df);
    df[NKEYS] = 12345u; /* not one of the ndf counters */
    /* no vocabulary attached yet */
    if (jb_df_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, df, NKEYS) != JB_EINVAL) {
        fprintf(stderr, "jb_df_batch without a vocabulary did not return JB_EINVAL\n");
        ok = 0;
    }
    if (jb_vocab_set(ctx, (const uint8_t *)KEYS, KEY_OFF, NKEYS) != JB_OK) {
        fprintf(stderr, "jb_vocab_set: %s\n", jb_last_error());
        ok = 0;
    }
    if (jb_df_batch(NULL, (const uint8_t *)TEXT, DOC_OFF, 2, 0, df, NKEYS) != JB_EINVAL ||
        jb_df_batch(ctx, (const uint8_t *)TEXT, NULL, 2, 0, df, NKEYS) != JB_EINVAL ||
        jb_df_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, NULL, NKEYS) != JB_EINVAL ||
        jb_df_batch(ctx, NULL, DOC_OFF, 2, 0, df, NKEYS) != JB_EINVAL ||
        jb_df_device(ctx, NULL, NULL, 4, NULL, NKEYS, NULL) != JB_EINVAL ||
        jb_idf_device(ctx, NULL, NKEYS, NDOCS, 1, JB_DF_NOMAX, NULL, NULL, NULL) != JB_EINVAL ||
        jb_idf(df, NKEYS, (uint64_t)1 << 53, 1, JB_DF_NOMAX, NULL, w) != JB_ELIMIT ||
        jb_idf(NULL, NKEYS, NDOCS, 1, JB_DF_NOMAX, NULL, w) != JB_EINVAL) {
        fprintf(stderr, "an error return is wrong\n");
        ok = 0;
    }
    for (i = 0; i < NKEYS; i++)
        if (df[i] != 0) {
            fprintf(stderr, "a failed call changed df[%u]\n", i);
            ok = 0;
        }
    /* two batches into one array; no document and no counter are valid, too */
    if (jb_df_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, df, NKEYS) != JB_OK ||
        jb_df_batch(ctx, (const uint8_t *)TEXT, DOC_OFF + 2, 3, 0, df, NKEYS) != JB_OK ||
        jb_df_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 0, 0, df, NKEYS) != JB_OK ||
        jb_df_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 2, 0, NULL, 0) != JB_OK) {
        fprintf(stderr, "jb_df_batch: %s\n", jb_last_error());
        ok = 0;
    }
    if (df[NKEYS] != 12345u) {
        fprintf(stderr, "jb_df_batch wrote past df[ndf]\n");
        ok = 0;
    }
    if (jb_idf(df, NKEYS, NDOCS, 1, JB_DF_NOMAX, NULL, w) != JB_OK) {
        fprintf(stderr, "jb_idf: %s\n", jb_last_error());
        ok = 0;
    }
    printf("ndocs %u\n", NDOCS);
    for (i = 0; i < NKEYS; i++) printf("df %u %u\n", i, df[i]);
    for (i = 0; i < NKEYS; i++) {
        memcpy(&bits, &w[i], sizeof bits);
        printf("weight %u %08x\n", i, bits);
    }
    jb_close(ctx);
    if (ok) printf("df ok\n");
    return ok ? 0 : 1;
}
