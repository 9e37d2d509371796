/* A C99 consumer of the token filter's entry points of include/jiebahip.h: jb_filter (the host form of the rule)
 * on spans worked out by hand, with its outputs written out; then jb_stopwords_set, jb_cut_batch_filter on the
 * device in the three modes against the host rule, jb_batch_filter_set with jb_cut_batch_join, and the error
 * returns.  usage: c_abi_filter <mini_dict.txt> <prob_emit.json>; exits non-zero on a mismatch. */
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
static const uint32_t S_CUT[] = {0, 4, 5, 8, 18, 21}, E_CUT[] = {3, 5, 8, 17, 21, 24};
static const uint64_t T_CUT[] = {0, 5, 5, 6};
static const uint32_t S_SRCH[] = {0, 4, 5, 8, 11, 8, 18, 21}, E_SRCH[] = {3, 5, 8, 14, 17, 17, 21, 24};
static const uint32_t S_FULL[] = {0, 4, 5, 8, 8, 11, 18, 21}, E_FULL[] = {3, 5, 8, 14, 17, 17, 21, 24};
static const uint64_t T_ALL[] = {0, 7, 7, 8};
static const char STOPS[] = YI CHA NA "xyz";
static const uint64_t STOP_OFF[] = {0, 9, 12};

int main(int argc, char **argv) {
    jb_config cfg;
    jb_ctx *ctx = NULL;
    jb_vocab *stop = NULL;
    jb_filter_rule rule = {JB_FILTER_STOP, JB_TC_INVALID, 2, 0}, none = {0, 0, 0, 0}, bad;
    uint32_t os[8], oe[8], osrc[8], ds[8], de[8];
    uint64_t odt[4], n, stats[5], ddt[4], dn, dstats[5];
    jb_joined j;
    int ok = 1, mode;
    if (argc < 3) {
        fprintf(stderr, "usage: %s mini_dict.txt prob_emit.json\n", argv[0]);
        return 2;
    }
    if (jb_filter_work_bytes(0, 0) == 0 || jb_filter_work_bytes(1, 0) > jb_filter_work_bytes(100000, 0) ||
        jb_filter_work_bytes(100000, 0) < 100000 / 8 || jb_filter_work_bytes(100, 1) > jb_filter_work_bytes(100, 1000) ||
        jb_filter_work_bytes(~0ull, ~0u) == 0) {
        fprintf(stderr, "the size helper is wrong\n");
        ok = 0;
    }
    /* the host form needs no ctx: abc kept, U+FFFD dropped by class, 这 by length, 一刹那 by the stop set, abc, abc kept */
    if (jb_vocab_build((const uint8_t *)STOPS, STOP_OFF, 2, &stop) != JB_OK ||
        jb_filter((const uint8_t *)TEXT, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, &rule, stop, os, oe, osrc, 8, odt, &n, stats) != JB_OK) {
        fprintf(stderr, "jb_filter: %s\n", jb_last_error());
        return 1;
    }
    if (n != 3 || os[0] != 0 || oe[0] != 3 || os[1] != 18 || oe[1] != 21 || os[2] != 21 || oe[2] != 24 || osrc[0] != 0 ||
        osrc[1] != 4 || osrc[2] != 5 || odt[0] != 0 || odt[1] != 2 || odt[2] != 2 || odt[3] != 3 || stats[0] != 6 ||
        stats[1] != 0 || stats[2] != 1 || stats[3] != 1 || stats[4] != 1) {
        fprintf(stderr, "jb_filter differs from the rule written out\n");
        ok = 0;
    }
    bad = none;
    bad.flags = 2;
    if (jb_filter(NULL, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, &none, NULL, os, oe, osrc, 8, odt, &n, stats) != JB_EINVAL ||
        jb_filter((const uint8_t *)TEXT, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, NULL, NULL, os, oe, osrc, 8, odt, &n, stats) != JB_EINVAL ||
        jb_filter((const uint8_t *)TEXT, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, &rule, NULL, os, oe, osrc, 8, odt, &n, stats) != JB_EINVAL ||
        jb_filter((const uint8_t *)TEXT, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, &bad, NULL, os, oe, osrc, 8, odt, &n, stats) != JB_EINVAL ||
        jb_filter((const uint8_t *)TEXT, 1ull << 31, S_CUT, E_CUT, T_CUT, 6, 6, 3, &none, NULL, os, oe, osrc, 8, odt, &n, stats) != JB_ELIMIT) {
        fprintf(stderr, "an error return of the host call is wrong\n");
        ok = 0;
    }
    bad = none;
    bad.max_runes = 256;
    if (jb_filter((const uint8_t *)TEXT, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, &bad, NULL, os, oe, osrc, 8, odt, &n, stats) != JB_ELIMIT) ok = 0;
    memset(&cfg, 0, sizeof cfg);
    cfg.dict_path = argv[1];
    cfg.dict_kind = JB_DICT_TXT;
    cfg.emit_path = argv[2];
    cfg.ndevices = 1;
    if (jb_open(&cfg, &ctx) != JB_OK) {
        fprintf(stderr, "jb_open: %s\n", jb_last_error());
        return 2;
    }
    if (jb_stopwords_size(ctx) != -1 ||
        jb_cut_batch_filter(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, &rule, ds, de, 8, ddt, &dn, dstats) != JB_EINVAL ||
        jb_stopwords_set(ctx, (const uint8_t *)STOPS, STOP_OFF, 2) != JB_OK || jb_stopwords_size(ctx) != 2 ||
        jb_vocab_size(ctx) != -1) {
        fprintf(stderr, "the stop set: %s\n", jb_last_error());
        ok = 0;
    }
    if (jb_cut_batch_filter(NULL, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, &rule, ds, de, 8, ddt, &dn, dstats) != JB_EINVAL ||
        jb_cut_batch_filter(ctx, (const uint8_t *)TEXT, NULL, 3, 0, JB_MODE_CUT, &rule, ds, de, 8, ddt, &dn, dstats) != JB_EINVAL ||
        jb_cut_batch_filter(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, 3, &rule, ds, de, 8, ddt, &dn, dstats) != JB_EINVAL ||
        jb_cut_batch_filter(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, NULL, ds, de, 8, ddt, &dn, dstats) != JB_EINVAL ||
        jb_cut_batch_filter(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, &bad, ds, de, 8, ddt, &dn, dstats) != JB_ELIMIT ||
        jb_filter_device(ctx, NULL, 0, NULL, NULL, NULL, NULL, 0, 0, &none, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, 0) != JB_EINVAL ||
        jb_filter_device(ctx, NULL, 0, NULL, NULL, NULL, NULL, 0, 0, &bad, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, 0) != JB_ELIMIT ||
        jb_batch_filter_set(NULL, &none) != JB_EINVAL || jb_batch_filter_set(ctx, &bad) != JB_ELIMIT) {
        fprintf(stderr, "an error return is wrong\n");
        ok = 0;
    }
    for (mode = JB_MODE_CUT; mode <= JB_MODE_FULL && ok; mode++) {
        const uint32_t *s = mode == JB_MODE_CUT ? S_CUT : mode == JB_MODE_SEARCH ? S_SRCH : S_FULL;
        const uint32_t *e = mode == JB_MODE_CUT ? E_CUT : mode == JB_MODE_SEARCH ? E_SRCH : E_FULL;
        const uint64_t *t = mode == JB_MODE_CUT ? T_CUT : T_ALL;
        const uint64_t nt = t[3];
        memset(ds, 0x5A, sizeof ds);
        memset(de, 0x5A, sizeof de);
        if (jb_filter((const uint8_t *)TEXT, 24, s, e, t, nt, nt, 3, &rule, stop, os, oe, NULL, 8, odt, &n, stats) != JB_OK ||
            jb_cut_batch_filter(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, mode, &rule, ds, de, 8, ddt, &dn, dstats) != JB_OK) {
            fprintf(stderr, "mode %d: %s\n", mode, jb_last_error());
            ok = 0;
            break;
        }
        if (dn != n || memcmp(os, ds, n * 4) != 0 || memcmp(oe, de, n * 4) != 0 || memcmp(odt, ddt, sizeof odt) != 0 ||
            memcmp(stats, dstats, sizeof stats) != 0 || ds[n] != 0x5A5A5A5Au) {
            fprintf(stderr, "mode %d: the device's filtered spans are not the host rule's\n", mode);
            ok = 0;
        }
        /* the arrays too small: JB_ELIMIT with the count */
        if (jb_cut_batch_filter(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, mode, &rule, ds, de, n - 1, ddt, &dn, NULL) != JB_ELIMIT ||
            dn != n) {
            fprintf(stderr, "mode %d: the cap protocol\n", mode);
            ok = 0;
        }
        printf("mode %d: %u of %u tokens kept\n", mode, (unsigned)n, (unsigned)nt);
    }
    /* the batch filter and the joined text */
    if (ok) {
        if (jb_batch_filter_set(ctx, &rule) != JB_OK ||
            jb_cut_batch_join(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, (const uint8_t *)" ", 1, (const uint8_t *)"\n", 1, &j) != JB_OK) {
            fprintf(stderr, "the batch filter: %s\n", jb_last_error());
            ok = 0;
        } else {
            if (j.nbytes != 13 || memcmp(j.text, "abc abc\n\nabc\n", 13) != 0) {
                fprintf(stderr, "the filtered joined text is wrong\n");
                ok = 0;
            }
            jb_joined_free(&j);
        }
        if (jb_batch_filter_set(ctx, NULL) != JB_OK ||
            jb_cut_batch_join(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, (const uint8_t *)" ", 1, (const uint8_t *)"\n", 1, &j) != JB_OK) {
            ok = 0;
        } else {
            if (j.nbytes != 13 + 4 + 4 + 10 || memcmp(j.text, "abc \xEF\xBF\xBD " ZHE " " YI CHA NA " abc\n\nabc\n", j.nbytes) != 0) {
                fprintf(stderr, "the joined text after clearing the filter is wrong\n");
                ok = 0;
            }
            jb_joined_free(&j);
        }
    }
    /* no document: only the count, doc_tok[0] and the statistics are written */
    memset(ds, 0x5A, sizeof ds);
    if (ok && (jb_cut_batch_filter(ctx, (const uint8_t *)TEXT, DOC_OFF, 0, 1, JB_MODE_CUT, &rule, ds, de, 8, ddt, &dn, dstats) != JB_OK ||
               ds[0] != 0x5A5A5A5Au || dn != 0 || ddt[0] != 0)) {
        fprintf(stderr, "an empty batch: %s\n", jb_last_error());
        ok = 0;
    }
    if (jb_stopwords_set(ctx, NULL, NULL, 0) != JB_OK || jb_stopwords_size(ctx) != -1) ok = 0;
    jb_vocab_free(stop);
    jb_close(ctx);
    if (ok) printf("filter ok\n");
    return ok ? 0 : 1;
}
