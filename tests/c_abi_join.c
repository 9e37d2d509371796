/* A C99 consumer of the joined-text entry points of include/jiebahip.h: jb_join (the host form of the rule)
 * on spans worked out by hand, jb_cut_batch_join on the same text in the three modes, compared byte for
 * byte, and the error returns.
 * usage: c_abi_join <mini_dict.txt> <prob_emit.json>; exits non-zero on a mismatch. */
#include <stdio.h>
#include <string.h>

#include "jiebahip.h"

/* document 0: abc \xFF 这一刹那 -> abc | U+FFFD | 这 | 一刹那 (search: 这 | 一刹 | 刹那 | 一刹那; full: 这 | 一刹 |
 * 一刹那 | 刹那); document 1 is empty; document 2: 2024 */
static const char TEXT[] = "abc \xFF\xE8\xBF\x99\xE4\xB8\x80\xE5\x88\xB9\xE9\x82\xA3" "2024";
static const uint64_t DOC_OFF[] = {0, 17, 17, 21};
static const uint32_t START[] = {0, 4, 5, 8, 17}, END[] = {3, 5, 8, 17, 21};
static const uint64_t DOC_TOK[] = {0, 4, 4, 5};
#define YI "\xE4\xB8\x80"
#define CHA "\xE5\x88\xB9"
#define NA "\xE9\x82\xA3"
#define ZHE "\xE8\xBF\x99"
static const char *WANT[3] = {
    "abc|\xEF\xBF\xBD|" ZHE "|" YI CHA NA "\n\n2024\n",
    "abc|\xEF\xBF\xBD|" ZHE "|" YI CHA "|" CHA NA "|" YI CHA NA "\n\n2024\n",
    "abc|\xEF\xBF\xBD|" ZHE "|" YI CHA "|" YI CHA NA "|" CHA NA "\n\n2024\n",
};

int main(int argc, char **argv) {
    jb_config cfg;
    jb_ctx *ctx = NULL;
    jb_joined j;
    uint8_t out[64];
    uint64_t off[4], nout = 0;
    int ok = 1, mode, rep;
    if (argc < 3) {
        fprintf(stderr, "usage: %s mini_dict.txt prob_emit.json\n", argv[0]);
        return 2;
    }
    if (jb_join_work_bytes(0, 0) == 0 || jb_join_work_bytes(1, 1) > jb_join_work_bytes(100000, 1) ||
        jb_join_work_bytes(1, 1) > jb_join_work_bytes(1, 100000)) {
        fprintf(stderr, "jb_join_work_bytes is wrong\n");
        ok = 0;
    }
    /* the host form needs no ctx */
    memset(out, 0x55, sizeof out);
    if (jb_join((const uint8_t *)TEXT, 21, START, END, DOC_TOK, 5, 5, 3, (const uint8_t *)"|", 1, (const uint8_t *)"\n", 1,
                out, sizeof out, off, &nout) != JB_OK) {
        fprintf(stderr, "jb_join: %s\n", jb_last_error());
        return 1;
    }
    if (nout != strlen(WANT[0]) || memcmp(out, WANT[0], nout) != 0 || out[nout] != 0x55 || off[0] != 0 || off[1] != 22 ||
        off[2] != 23 || off[3] != 28) {
        fprintf(stderr, "jb_join: %llu bytes, offsets %llu %llu %llu\n", (unsigned long long)nout, (unsigned long long)off[1],
                (unsigned long long)off[2], (unsigned long long)off[3]);
        ok = 0;
    }
    /* a small out_cap: the counts stay complete, nothing past it is written */
    memset(out, 0x55, sizeof out);
    if (jb_join((const uint8_t *)TEXT, 21, START, END, DOC_TOK, 5, 5, 3, (const uint8_t *)"|", 1, (const uint8_t *)"\n", 1,
                out, 6, off, &nout) != JB_OK || nout != 28 || memcmp(out, WANT[0], 6) != 0 || out[6] != 0x55) {
        fprintf(stderr, "jb_join with out_cap 6 is wrong\n");
        ok = 0;
    }
    if (jb_join((const uint8_t *)TEXT, 21, START, END, DOC_TOK, 5, 5, 3, (const uint8_t *)"123456789", 9, NULL, 0, out,
                sizeof out, off, &nout) != JB_ELIMIT ||
        jb_join((const uint8_t *)TEXT, 21, START, END, DOC_TOK, 5, 5, 3, NULL, 1, NULL, 0, out, sizeof out, off, &nout) !=
            JB_EINVAL ||
        jb_join((const uint8_t *)TEXT, 21, START, END, NULL, 5, 5, 3, NULL, 0, NULL, 0, out, sizeof out, off, &nout) !=
            JB_EINVAL) {
        fprintf(stderr, "an error return of jb_join is wrong\n");
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
    if (jb_cut_batch_join(NULL, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, NULL, 0, NULL, 0, &j) != JB_EINVAL ||
        jb_cut_batch_join(ctx, (const uint8_t *)TEXT, NULL, 3, 0, JB_MODE_CUT, NULL, 0, NULL, 0, &j) != JB_EINVAL ||
        jb_cut_batch_join(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, NULL, 0, NULL, 0, NULL) != JB_EINVAL ||
        jb_cut_batch_join(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, 3, NULL, 0, NULL, 0, &j) != JB_EINVAL ||
        jb_cut_batch_join(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, (const uint8_t *)"123456789", 9, NULL, 0, &j) !=
            JB_ELIMIT ||
        jb_join_device(ctx, NULL, 0, NULL, NULL, NULL, NULL, 0, 1, NULL, 0, NULL, 0, NULL, NULL, 0, NULL, NULL, NULL, 0) !=
            JB_EINVAL) {
        fprintf(stderr, "an error return is wrong\n");
        ok = 0;
    }
    for (rep = 0; rep < 2 && ok; rep++) /* twice: the call leaves nothing behind */
        for (mode = JB_MODE_CUT; mode <= JB_MODE_FULL; mode++) {
            if (jb_cut_batch_join(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, mode, (const uint8_t *)"|", 1, (const uint8_t *)"\n",
                                  1, &j) != JB_OK) {
                fprintf(stderr, "jb_cut_batch_join: %s\n", jb_last_error());
                ok = 0;
                break;
            }
            if (j.nbytes != strlen(WANT[mode]) || memcmp(j.text, WANT[mode], j.nbytes) != 0 || j.ndocs != 3 ||
                j.doc_off[0] != 0 || j.doc_off[3] != j.nbytes || j.doc_off[2] != j.doc_off[1] + 1) {
                fprintf(stderr, "mode %d: %llu bytes: %.*s\n", mode, (unsigned long long)j.nbytes, (int)j.nbytes,
                        (const char *)j.text);
                ok = 0;
            }
            printf("mode %d: %llu bytes\n", mode, (unsigned long long)j.nbytes);
            jb_joined_free(&j);
            if (j.text != NULL || j.doc_off != NULL) ok = 0;
        }
    /* no document: an empty result with one offset */
    if (ok && (jb_cut_batch_join(ctx, (const uint8_t *)TEXT, DOC_OFF, 0, 1, JB_MODE_CUT, NULL, 0, NULL, 0, &j) != JB_OK ||
               j.nbytes != 0 || j.ndocs != 0 || j.doc_off == NULL || j.doc_off[0] != 0)) {
        fprintf(stderr, "an empty batch: %s\n", jb_last_error());
        ok = 0;
    }
    jb_joined_free(&j);
    jb_joined_free(NULL);
    jb_close(ctx);
    if (ok) printf("join ok\n");
    return ok ? 0 : 1;
}
