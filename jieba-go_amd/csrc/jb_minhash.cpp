// jb_minhash.cpp — the host side of the MinHash signatures: jb_minhash, the rule of jiebahip.h on host arrays
// (what the kernels of jb_minhash.hip are pinned to, bit for bit), jb_minhash_params, jb_minhash_bands, the
// size helper and the argument checks shared with the device calls.  Host only, no HIP.
#include "jb_minhash.h"

#include <stdlib.h>

#include <algorithm>
#include <new>
#include <vector>

#include "jb_err.h"
#include "jiebahip.h"

namespace jb {

int minhash_args(const char* who, uint64_t nbytes, uint64_t cap, uint32_t n, uint32_t K) {
    if (n == 0 || K == 0) return fail(JB_EINVAL, "%s: n = %u, K = %u (each at least 1)", who, n, K);
    if (n > JB_MH_MAXN) return fail(JB_ELIMIT, "%s: shingles of %u tokens (limit JB_MH_MAXN = %u)", who, n, JB_MH_MAXN);
    if (K > JB_MH_MAXK) return fail(JB_ELIMIT, "%s: %u hash functions (limit JB_MH_MAXK = %u)", who, K, JB_MH_MAXK);
    if (nbytes >= (1ull << 31)) return fail(JB_ELIMIT, "%s: a text of %llu bytes (limit 2 GiB)", who, (unsigned long long)nbytes);
    if (cap >= (1ull << 32) - JB_MH_TILE)
        return fail(JB_ELIMIT, "%s: a span list of %llu entries (limit 2^32 - %u)", who, (unsigned long long)cap,
                    JB_MH_TILE);
    return JB_OK;
}

int minhash_band_args(const char* who, uint32_t K, uint32_t B, uint32_t R) {
    if (K == 0 || B == 0 || R == 0) return fail(JB_EINVAL, "%s: K = %u, B = %u, R = %u (each at least 1)", who, K, B, R);
    if ((uint64_t)B * R > K) return fail(JB_EINVAL, "%s: %u bands of %u rows do not fit %u slots", who, B, R, K);
    if (K > JB_MH_MAXK) return fail(JB_ELIMIT, "%s: %u hash functions (limit JB_MH_MAXK = %u)", who, K, JB_MH_MAXK);
    return JB_OK;
}

}  // namespace jb

extern "C" size_t jb_minhash_work_bytes(uint64_t max_tokens, uint32_t ndocs) {
    (void)ndocs;  // (the work buffer holds the token hashes alone today)
    if (max_tokens > (1ull << 59)) return SIZE_MAX;
    const uint64_t nb = (std::max<uint64_t>(max_tokens, 1u) * 8u + 255u) & ~(uint64_t)255u;
    return nb > (uint64_t)SIZE_MAX ? SIZE_MAX : (size_t)nb;
}

extern "C" int jb_minhash_params(uint64_t seed, uint32_t K, uint64_t* a, uint64_t* b) {
    if (K == 0 || !a || !b) return fail(JB_EINVAL, "jb_minhash_params: null argument or K = 0");
    if (K > JB_MH_MAXK) return fail(JB_ELIMIT, "jb_minhash_params: %u hash functions (limit JB_MH_MAXK = %u)", K, JB_MH_MAXK);
    for (uint32_t j = 0; j < K; j++) {
        a[j] = jb_mh_a(seed, j);
        b[j] = jb_mh_b(seed, j);
    }
    return JB_OK;
}

extern "C" int jb_minhash(const uint8_t* text, uint64_t nbytes, const uint32_t* start, const uint32_t* end,
                          const uint64_t* doc_tok, uint64_t ntok, uint64_t cap, uint32_t ndocs, uint32_t n, uint32_t K,
                          uint64_t seed, uint32_t* sig, uint32_t* doc_n) {
    if (!doc_tok || (nbytes && !text) || (cap && (!start || !end)) || (ndocs && (!sig || !doc_n)))
        return fail(JB_EINVAL, "jb_minhash: null argument");
    if (const int rc = jb::minhash_args("jb_minhash", nbytes, cap, n, K)) return rc;
    const uint64_t nt = std::min(ntok, cap);
    std::vector<uint64_t> t;
    try {
        t.resize(nt);
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "jb_minhash: out of host memory for %llu token hashes", (unsigned long long)nt);
    }
    static const uint8_t kRepl[3] = {0xEF, 0xBF, 0xBD};
    for (uint64_t k = 0; k < nt; k++) {
        const uint64_t s = start[k], e = end[k];
        const uint8_t* key = nullptr;
        uint32_t len = 0;  // (a malformed span: the empty key, no text byte is read)
        if (s < e && e <= nbytes) {
            key = text + s;
            len = (uint32_t)std::min<uint64_t>(e - s, JB_VOCAB_MAXKEY);
            if (e - s == 1 && text[s] >= 0x80) {
                key = kRepl;
                len = 3;
            }
        }
        uint32_t kw[6];
        jb_mh_words(key, len, kw);
        t[k] = jb_vocab_hash(kw, key, len);
    }
    uint64_t a[JB_MH_MAXK], b[JB_MH_MAXK];
    for (uint32_t j = 0; j < K; j++) {
        a[j] = jb_mh_a(seed, j);
        b[j] = jb_mh_b(seed, j);
    }
    for (uint32_t d = 0; d < ndocs; d++) {
        uint32_t* row = sig + (uint64_t)d * K;
        std::fill(row, row + K, JB_MH_EMPTY);
        const uint64_t lo = std::min(doc_tok[d], nt), hi = std::min(doc_tok[d + 1], nt);
        const uint64_t m = hi > lo ? hi - lo : 0;
        const uint32_t cnt = jb_mh_count(m, n), c = jb_mh_width(m, n);
        doc_n[d] = cnt;
        for (uint32_t i = 0; i < cnt; i++) {
            const uint32_t x = jb_mh_shingle(t.data() + lo + i, c);
            for (uint32_t j = 0; j < K; j++) row[j] = std::min(row[j], jb_mh_slot(a[j], b[j], x));
        }
    }
    return JB_OK;
}

extern "C" int jb_minhash_bands(const uint32_t* sig, const uint32_t* doc_n, uint32_t ndocs, uint32_t K, uint32_t B,
                                uint32_t R, uint64_t* keys) {
    if (ndocs && (!sig || !doc_n || !keys)) return fail(JB_EINVAL, "jb_minhash_bands: null argument");
    if (const int rc = jb::minhash_band_args("jb_minhash_bands", K, B, R)) return rc;
    for (uint32_t d = 0; d < ndocs; d++)
        for (uint32_t band = 0; band < B; band++)
            keys[(uint64_t)d * B + band] = doc_n[d] ? jb_mh_band(sig + (uint64_t)d * K, band, R) : JB_MH_NOKEY;
    return JB_OK;
}
