// jb_textrank.cpp — jb_textrank, the TextRank rule of jiebahip.h on host arrays, and the argument checks
// it shares with jb_textrank_device.  Host only, no HIP: the kernels of jb_textrank.hip are pinned to this
// function bit for bit, so every f64 operation here is a single IEEE operation (the unit is compiled
// with -ffp-contract=off) and every sum of the iteration is a u64.
#include "jb_textrank.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "jb_err.h"
#include "jiebahip.h"

namespace jb {

int textrank_args(const char* who, uint64_t ids_cap, uint64_t cap, uint32_t span, uint32_t iters, uint32_t topk) {
    if (topk == 0) return fail(JB_EINVAL, "%s: topk is 0", who);
    if (topk > JB_KW_MAXK) return fail(JB_ELIMIT, "%s: topk %u (limit JB_KW_MAXK = %u)", who, topk, JB_KW_MAXK);
    if (span < 2) return fail(JB_EINVAL, "%s: span %u (at least 2)", who, span);
    if (span > JB_TR_MAXSPAN) return fail(JB_ELIMIT, "%s: span %u (limit JB_TR_MAXSPAN = %u)", who, span, JB_TR_MAXSPAN);
    if (iters > JB_TR_MAXITER)
        return fail(JB_ELIMIT, "%s: iters %u (limit JB_TR_MAXITER = %u)", who, iters, JB_TR_MAXITER);
    if (ids_cap >= (1ull << 32) - JB_TERMS_TILE)
        return fail(JB_ELIMIT, "%s: an id list of %llu entries (limit 2^32 - %u)", who, (unsigned long long)ids_cap,
                    JB_TERMS_TILE);
    if (cap >= (1ull << 32) - JB_TERMS_TILE)
        return fail(JB_ELIMIT, "%s: a term list of %llu entries (limit 2^32 - %u)", who, (unsigned long long)cap,
                    JB_TERMS_TILE);
    return JB_OK;
}

}  // namespace jb

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

uint32_t bit_length(uint64_t n) {
    uint32_t b = 0;
    while (n) {
        b++;
        n >>= 1;
    }
    return b;
}

double pow2(int e) {  // 2^e for |e| <= 62, exactly
    const uint64_t bits = (uint64_t)(1023 + e) << 52;
    double d;
    std::memcpy(&d, &bits, 8);
    return d;
}

int textrank_host(const uint32_t* ids, uint64_t ids_cap, const uint64_t* doc_tok, uint64_t ntok, uint32_t ndocs,
                  const uint32_t* term_id, const uint64_t* term_off, uint64_t cap, const uint8_t* keep, uint32_t nkeep,
                  uint32_t span, uint32_t iters, uint32_t topk, uint32_t* kw_id, float* kw_score, uint32_t* kw_n) {
    const uint64_t n_all = std::min(ntok, ids_cap);
    std::vector<uint32_t> node;  // per token of the document: its term's index in the row, or kNone
    std::vector<uint64_t> out, r, acc;
    std::vector<double> ws;
    std::vector<uint64_t> keys;
    for (uint32_t d = 0; d < ndocs; d++) {
        uint32_t* oid = kw_id + (size_t)d * topk;
        float* osc = kw_score + (size_t)d * topk;
        for (uint32_t k = 0; k < topk; k++) {
            oid[k] = JB_ID_UNK;
            osc[k] = 0.0f;
        }
        kw_n[d] = 0;
        const uint64_t a = term_off[d], b = term_off[d + 1];
        if (b > cap || a > b) continue;  // a CSR that overflowed its arrays is not read past them
        const uint64_t t0 = std::min(doc_tok[d], n_all), t1 = std::min(doc_tok[d + 1], n_all);
        if (t0 >= t1) continue;
        const uint64_t len = t1 - t0, nt = b - a;
        node.assign(len, kNone);
        for (uint64_t k = 0; k < len; k++) {
            const uint32_t id = ids[t0 + k];
            if (id == JB_ID_UNK || id >= nkeep || keep[id] == 0) continue;
            uint64_t lo = a, hi = b;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (term_id[mid] < id) lo = mid + 1;
                else hi = mid;
            }
            if (lo < b && term_id[lo] == id) node[k] = (uint32_t)(lo - a);
        }
        // the kept tokens j != k of the same document with |j - k| < span
        auto window = [&](uint64_t k, uint64_t* lo, uint64_t* hi) {
            *lo = k >= span - 1u ? k - (span - 1u) : 0;
            *hi = std::min(len, k + span);
        };
        out.assign(nt, 0);
        for (uint64_t k = 0; k < len; k++) {
            if (node[k] == kNone) continue;
            uint64_t lo, hi, deg = 0;
            window(k, &lo, &hi);
            for (uint64_t j = lo; j < hi; j++) deg += j != k && node[j] != kNone;
            out[node[k]] += deg;
        }
        uint64_t n = 0;
        for (uint64_t t = 0; t < nt; t++) n += out[t] > 0;
        if (n == 0) continue;
        const int S = 62 - (int)bit_length(n);
        const double up = pow2(S), down = pow2(-S);
        ws.assign(nt, 0.0);
        r.assign(nt, 0);
        acc.assign(nt, 0);
        for (uint64_t t = 0; t < nt; t++)
            if (out[t] > 0) ws[t] = 1.0 / (double)n;
        for (uint32_t it = 0; it < iters; it++) {
            for (uint64_t t = 0; t < nt; t++) {
                acc[t] = 0;
                r[t] = out[t] > 0 ? (uint64_t)((ws[t] / (double)out[t]) * up) : 0;
            }
            for (uint64_t k = 0; k < len; k++) {
                if (node[k] == kNone) continue;
                uint64_t lo, hi, s = 0;
                window(k, &lo, &hi);
                for (uint64_t j = lo; j < hi; j++)
                    if (j != k && node[j] != kNone) s += r[node[j]];
                acc[node[k]] += s;
            }
            for (uint64_t t = 0; t < nt; t++)
                if (out[t] > 0) {
                    const double x = (double)acc[t] * down;
                    const double y = 0.85 * x;
                    ws[t] = (1.0 - 0.85) + y;
                }
        }
        double mn = 0, mx = 0;
        bool first = true;
        for (uint64_t t = 0; t < nt; t++) {
            if (out[t] == 0) continue;
            mn = first ? ws[t] : std::min(mn, ws[t]);
            mx = first ? ws[t] : std::max(mx, ws[t]);
            first = false;
        }
        const double base = mn / 10.0, den = mx - base;
        keys.clear();
        for (uint64_t t = 0; t < nt; t++) {
            if (out[t] == 0) continue;
            const float sc = (float)((ws[t] - base) / den);
            uint32_t bits;
            std::memcpy(&bits, &sc, 4);
            keys.push_back(((uint64_t)bits << 32) | (uint32_t)~term_id[a + t]);
        }
        const size_t take = std::min<size_t>(topk, keys.size());
        std::partial_sort(keys.begin(), keys.begin() + take, keys.end(), [](uint64_t x, uint64_t y) { return x > y; });
        for (size_t k = 0; k < take; k++) {
            const uint32_t bits = (uint32_t)(keys[k] >> 32);
            oid[k] = ~(uint32_t)keys[k];
            std::memcpy(&osc[k], &bits, 4);
        }
        kw_n[d] = (uint32_t)take;
    }
    return JB_OK;
}

}  // namespace

extern "C" int jb_textrank(const uint32_t* ids, uint64_t ids_cap, const uint64_t* doc_tok, uint64_t ntok, uint32_t ndocs,
                           const uint32_t* term_id, const uint64_t* term_off, uint64_t cap, const uint8_t* keep,
                           uint32_t nkeep, uint32_t span, uint32_t iters, uint32_t topk, uint32_t* kw_id,
                           float* kw_score, uint32_t* kw_n) {
    // (the limits come first, as in the keyword calls)
    if (const int rc = jb::textrank_args("jb_textrank", ids_cap, cap, span, iters, topk)) return rc;
    if (!doc_tok || !term_off || (ids_cap && !ids) || (cap && !term_id) || (nkeep && !keep) ||
        (ndocs && (!kw_id || !kw_score || !kw_n)))
        return fail(JB_EINVAL, "jb_textrank: null argument");
    try {
        return textrank_host(ids, ids_cap, doc_tok, ntok, ndocs, term_id, term_off, cap, keep, nkeep, span, iters, topk,
                             kw_id, kw_score, kw_n);
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "jb_textrank: out of host memory");
    }
}
