/* A C99 consumer of the MinHash entry points of include/jiebahip.h: jb_minhash (the host form of the rule),
 * jb_minhash_params and jb_minhash_bands on spans worked out by hand, with one slot restated from the header's
 * constants; then jb_minhash_batch on the device in the three modes against the host rule, and the error returns.
 * usage: c_abi_minhash <mini_dict.txt> <prob_emit.json>; exits non-zero on a mismatch. */
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
#define K 16

static uint64_t mix(uint64_t h, uint64_t w) {
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 32);
}
static uint64_t init(uint64_t c) { return 0x243F6A8885A308D3ull ^ (c * 0xFF51AFD7ED558CCDull); }
static uint64_t fin(uint64_t h) {
    h *= 0xD6E8FEB86659FD93ull;
    return h ^ (h >> 32);
}

int main(int argc, char **argv) {
    jb_config cfg;
    jb_ctx *ctx = NULL;
    uint32_t sig[3 * K], dn[3], dsig[3 * K], ddn[3];
    uint64_t a[K], b[K], keys[3 * 4];
    int ok = 1, mode, i;
    if (argc < 3) {
        fprintf(stderr, "usage: %s mini_dict.txt prob_emit.json\n", argv[0]);
        return 2;
    }
    if (jb_minhash_work_bytes(0, 0) == 0 || jb_minhash_work_bytes(1, 0) > jb_minhash_work_bytes(100000, 0) ||
        jb_minhash_work_bytes(100000, 0) < 800000 || jb_minhash_work_bytes(100, 1) > jb_minhash_work_bytes(100, 1000) ||
        jb_minhash_work_bytes(~0ull, ~0u) == 0) {
        fprintf(stderr, "the size helper is wrong\n");
        ok = 0;
    }
    /* the host form needs no ctx */
    if (jb_minhash_params(1, K, a, b) != JB_OK || jb_minhash((const uint8_t *)TEXT, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, 2, K, 1,
                                                             sig, dn) != JB_OK) {
        fprintf(stderr, "jb_minhash: %s\n", jb_last_error());
        return 1;
    }
    if (dn[0] != 4 || dn[1] != 0 || dn[2] != 1 || !(a[0] & 1)) ok = 0;
    for (i = 0; i < K; i++)
        if (sig[K + i] != JB_MH_EMPTY) ok = 0;
    {
        /* document 2 is the one token abc, fewer than n = 2: one shingle over c = 1 token */
        const uint64_t t = fin(mix(init(3), 0x636261ull));
        const uint32_t x = (uint32_t)fin(mix(init(1), t));
        for (i = 0; i < K; i++)
            if (sig[2 * K + i] != (uint32_t)((a[i] * (uint64_t)x + b[i]) >> 32)) ok = 0;
        if (!ok) fprintf(stderr, "jb_minhash differs from the rule written out\n");
    }
    if (jb_minhash_bands(sig, dn, 3, K, 4, 4, keys) != JB_OK || keys[4] != JB_MH_NOKEY || keys[0] == JB_MH_NOKEY ||
        keys[0] == keys[1] || keys[8] == JB_MH_NOKEY) {
        fprintf(stderr, "jb_minhash_bands is wrong\n");
        ok = 0;
    }
    if (jb_minhash(NULL, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, 2, K, 1, sig, dn) != JB_EINVAL ||
        jb_minhash((const uint8_t *)TEXT, 24, S_CUT, E_CUT, NULL, 6, 6, 3, 2, K, 1, sig, dn) != JB_EINVAL ||
        jb_minhash((const uint8_t *)TEXT, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, 0, K, 1, sig, dn) != JB_EINVAL ||
        jb_minhash((const uint8_t *)TEXT, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, 2, 0, 1, sig, dn) != JB_EINVAL ||
        jb_minhash((const uint8_t *)TEXT, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, JB_MH_MAXN + 1, K, 1, sig, dn) != JB_ELIMIT ||
        jb_minhash((const uint8_t *)TEXT, 24, S_CUT, E_CUT, T_CUT, 6, 6, 3, 2, JB_MH_MAXK + 1, 1, sig, dn) != JB_ELIMIT ||
        jb_minhash((const uint8_t *)TEXT, 1ull << 31, S_CUT, E_CUT, T_CUT, 6, 6, 3, 2, K, 1, sig, dn) != JB_ELIMIT ||
        jb_minhash_bands(sig, dn, 3, K, 5, 4, keys) != JB_EINVAL || jb_minhash_bands(sig, dn, 3, K, 0, 4, keys) != JB_EINVAL ||
        jb_minhash_params(1, 0, a, b) != JB_EINVAL || jb_minhash_params(1, JB_MH_MAXK + 1, a, b) != JB_ELIMIT) {
        fprintf(stderr, "an error return of the host calls is wrong\n");
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
    if (jb_minhash_batch(NULL, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, 2, K, 1, dsig, ddn) != JB_EINVAL ||
        jb_minhash_batch(ctx, (const uint8_t *)TEXT, NULL, 3, 0, JB_MODE_CUT, 2, K, 1, dsig, ddn) != JB_EINVAL ||
        jb_minhash_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, 3, 2, K, 1, dsig, ddn) != JB_EINVAL ||
        jb_minhash_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, 2, K, 1, NULL, ddn) != JB_EINVAL ||
        jb_minhash_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, 0, K, 1, dsig, ddn) != JB_EINVAL ||
        jb_minhash_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, 9, K, 1, dsig, ddn) != JB_ELIMIT ||
        jb_minhash_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, JB_MODE_CUT, 2, 257, 1, dsig, ddn) != JB_ELIMIT ||
        jb_minhash_device(ctx, NULL, 0, NULL, NULL, NULL, NULL, 0, 0, 2, K, 1, NULL, NULL, NULL, NULL, 0) != JB_EINVAL ||
        jb_minhash_device(ctx, NULL, 0, NULL, NULL, NULL, NULL, 0, 0, 9, K, 1, NULL, NULL, NULL, NULL, 0) != JB_ELIMIT ||
        jb_minhash_bands_device(ctx, NULL, NULL, 3, K, 4, 4, NULL, NULL) != JB_EINVAL ||
        jb_minhash_bands_device(ctx, NULL, NULL, 0, K, 5, 4, NULL, NULL) != JB_EINVAL) {
        fprintf(stderr, "an error return is wrong\n");
        ok = 0;
    }
    for (mode = JB_MODE_CUT; mode <= JB_MODE_FULL && ok; mode++) {
        const uint32_t *s = mode == JB_MODE_CUT ? S_CUT : mode == JB_MODE_SEARCH ? S_SRCH : S_FULL;
        const uint32_t *e = mode == JB_MODE_CUT ? E_CUT : mode == JB_MODE_SEARCH ? E_SRCH : E_FULL;
        const uint64_t *t = mode == JB_MODE_CUT ? T_CUT : T_ALL;
        const uint64_t nt = t[3];
        uint32_t n;
        for (n = 1; n <= 3 && ok; n++) {
            memset(dsig, 0x5A, sizeof dsig);
            memset(ddn, 0x5A, sizeof ddn);
            if (jb_minhash((const uint8_t *)TEXT, 24, s, e, t, nt, nt, 3, n, K, 7, sig, dn) != JB_OK ||
                jb_minhash_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 3, 0, mode, n, K, 7, dsig, ddn) != JB_OK) {
                fprintf(stderr, "mode %d: %s\n", mode, jb_last_error());
                ok = 0;
                break;
            }
            if (memcmp(sig, dsig, sizeof sig) != 0 || memcmp(dn, ddn, sizeof dn) != 0) {
                fprintf(stderr, "mode %d, n %u: the device's signatures are not the host rule's\n", mode, n);
                ok = 0;
            }
        }
        printf("mode %d: %u shingles in document 0\n", mode, ddn[0]);
    }
    /* no document: nothing is written */
    memset(dsig, 0x5A, sizeof dsig);
    if (ok && (jb_minhash_batch(ctx, (const uint8_t *)TEXT, DOC_OFF, 0, 1, JB_MODE_CUT, 2, K, 1, dsig, ddn) != JB_OK ||
               dsig[0] != 0x5A5A5A5Au)) {
        fprintf(stderr, "an empty batch: %s\n", jb_last_error());
        ok = 0;
    }
    jb_close(ctx);
    if (ok) printf("minhash ok\n");
    return ok ? 0 : 1;
}
