/* A C99 consumer of the token-id entry points of include/jiebahip.h: builds a vocabulary on the
 * host, attaches one to a ctx, and compares the ids of jb_cut / jb_cut_search / jb_cut_full spans
 * (jb_spans_ids) with the hand-worked ones.
 * usage: c_abi_ids <mini_dict.txt> <prob_emit.json>; exits non-zero on a mismatch. */
#include <stdio.h>
#include <string.h>

#include "jiebahip.h"

#define U JB_ID_UNK

/* keys: abc | 今天 | U+FFFD | 一刹那 | 刹那 | 这 | 天天 */
static const char KEYS[] = "abc" "\xE4\xBB\x8A\xE5\xA4\xA9" "\xEF\xBF\xBD" "\xE4\xB8\x80\xE5\x88\xB9\xE9\x82\xA3"
                           "\xE5\x88\xB9\xE9\x82\xA3" "\xE8\xBF\x99" "\xE5\xA4\xA9\xE5\xA4\xA9";
static const uint64_t KEY_OFF[] = {0, 3, 9, 12, 21, 27, 30, 36};
#define NKEYS 7u

static int same(const char *what, const uint32_t *got, const uint32_t *want, uint64_t ngot, uint64_t n) {
    uint64_t k;
    if (ngot != n) {
        fprintf(stderr, "%s: %llu tokens, want %llu\n", what, (unsigned long long)ngot, (unsigned long long)n);
        return 0;
    }
    for (k = 0; k < n; k++)
        if (got[k] != want[k]) {
            fprintf(stderr, "%s: id %llu is %u, want %u\n", what, (unsigned long long)k, got[k], want[k]);
            return 0;
        }
    return 1;
}

int main(int argc, char **argv) {
    /* abc \xFF今天天氣 这一刹那 -> abc, U+FFFD, 今天, 天, 氣, 这, 一刹那 */
    static const char T1[] = "abc \xFF" "\xE4\xBB\x8A\xE5\xA4\xA9\xE5\xA4\xA9\xE6\xB0\xA3 "
                             "\xE8\xBF\x99\xE4\xB8\x80\xE5\x88\xB9\xE9\x82\xA3";
    static const uint32_t W1[] = {0, 2, 1, U, U, 5, 3};
    /* search mode: ... 这, 一刹, 刹那, 一刹那 */
    static const uint32_t W1S[] = {0, 2, 1, U, U, 5, U, 4, 3};
    /* full mode: abc, U+FFFD, 今天, 天天, 氣, 这, 一刹, 一刹那, 刹那 */
    static const uint32_t W1F[] = {0, 2, 1, 6, U, 5, U, 3, 4};
    jb_config cfg;
    jb_ctx *ctx = NULL;
    jb_vocab *v = NULL;
    jb_spans sp;
    uint32_t ids[16], id = 0, nkeys = 0, maxlen = 0;
    uint64_t nslots = 0, one = 1;
    int ok = 1, mode;
    if (argc < 3) {
        fprintf(stderr, "usage: %s mini_dict.txt prob_emit.json\n", argv[0]);
        return 2;
    }
    /* the host table */
    if (jb_vocab_build((const uint8_t *)KEYS, KEY_OFF, NKEYS, &v) != JB_OK) {
        fprintf(stderr, "jb_vocab_build: %s\n", jb_last_error());
        return 2;
    }
    if (jb_vocab_info(v, &nkeys, &maxlen, &nslots) != JB_OK || nkeys != NKEYS || maxlen != 9 || nslots < 2 * NKEYS ||
        (nslots & (nslots - 1)) != 0 || jb_vocab_lookup(v, (const uint8_t *)"abc", 3, &id) != 1 || id != 0 ||
        jb_vocab_lookup(v, (const uint8_t *)"\xE5\x88\xB9\xE9\x82\xA3", 6, &id) != 1 || id != 4 ||
        jb_vocab_lookup(v, (const uint8_t *)"ab", 2, &id) != 0 || id != JB_ID_UNK) {
        fprintf(stderr, "the host table is wrong\n");
        ok = 0;
    }
    jb_vocab_free(v);
    memset(&cfg, 0, sizeof cfg);
    cfg.dict_path = argv[1];
    cfg.dict_kind = JB_DICT_TXT;
    cfg.emit_path = argv[2];
    cfg.ndevices = 1;
    if (jb_open(&cfg, &ctx) != JB_OK) {
        fprintf(stderr, "jb_open: %s\n", jb_last_error());
        return 2;
    }
    memset(&sp, 0, sizeof sp);
    if (jb_vocab_set(NULL, (const uint8_t *)KEYS, KEY_OFF, NKEYS) != JB_EINVAL || jb_vocab_size(NULL) != -1 ||
        jb_vocab_size(ctx) != -1 || jb_spans_ids(NULL, (const uint8_t *)T1, &sp, ids) != JB_EINVAL ||
        jb_ids_device(NULL, NULL, 0, NULL, NULL, &one, 0, NULL, NULL) != JB_EINVAL) {
        fprintf(stderr, "a null argument did not return JB_EINVAL\n");
        ok = 0;
    }
    if (ok && jb_cut(ctx, (const uint8_t *)T1, sizeof T1 - 1, 0, &sp) == JB_OK) {
        if (jb_spans_ids(ctx, (const uint8_t *)T1, &sp, ids) != JB_EINVAL) { /* no vocabulary attached */
            fprintf(stderr, "jb_spans_ids without a vocabulary did not return JB_EINVAL\n");
            ok = 0;
        }
        jb_spans_free(&sp);
    }
    if (jb_vocab_set(ctx, (const uint8_t *)KEYS, KEY_OFF, NKEYS) != JB_OK || jb_vocab_size(ctx) != (int64_t)NKEYS) {
        fprintf(stderr, "jb_vocab_set: %s\n", jb_last_error());
        ok = 0;
    }
    for (mode = 0; mode < 3 && ok; mode++) {
        const uint32_t *want = mode == 0 ? W1 : mode == 1 ? W1S : W1F;
        const uint64_t n = mode == 0 ? sizeof W1 / sizeof *W1 : sizeof W1S / sizeof *W1S;
        const char *what = mode == 0 ? "jb_cut" : mode == 1 ? "jb_cut_search" : "jb_cut_full";
        const int rc = mode == 0   ? jb_cut(ctx, (const uint8_t *)T1, sizeof T1 - 1, 0, &sp)
                       : mode == 1 ? jb_cut_search(ctx, (const uint8_t *)T1, sizeof T1 - 1, 0, &sp)
                                   : jb_cut_full(ctx, (const uint8_t *)T1, sizeof T1 - 1, &sp);
        if (rc != JB_OK || sp.ntokens > sizeof ids / sizeof *ids) {
            fprintf(stderr, "%s: %s\n", what, jb_last_error());
            ok = 0;
            break;
        }
        if (jb_spans_ids(ctx, (const uint8_t *)T1, &sp, ids) != JB_OK) {
            fprintf(stderr, "jb_spans_ids: %s\n", jb_last_error());
            ok = 0;
        } else {
            ok = same(what, ids, want, sp.ntokens, n);
        }
        jb_spans_free(&sp);
    }
    /* removing it: the id calls refuse again */
    if (ok && (jb_vocab_set(ctx, NULL, NULL, 0) != JB_OK || jb_vocab_size(ctx) != -1)) {
        fprintf(stderr, "removing the vocabulary: %s\n", jb_last_error());
        ok = 0;
    }
    jb_close(ctx);
    if (ok) printf("ids ok\n");
    return ok ? 0 : 1;
}
