// jb_colloc.cpp — the host side of the collocation calls: jb_colloc_count and jb_colloc_score, the rule of
// jiebahip.h on host arrays (what the kernels of jb_colloc.hip are pinned to), the size helpers, the argument
// checks shared with the device calls and the sort of a result.  Host only, no HIP.
#include "jb_colloc.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <new>
#include <numeric>
#include <vector>

#include "jb_err.h"

static_assert(sizeof(JbClHeader) <= JB_CL_HDR_BYTES, "the header fits its block");

namespace jb {

int colloc_slots(const char* who, uint64_t nslots) {
    if (nslots < JB_CL_MIN_SLOTS || (nslots & (nslots - 1u)) != 0)
        return fail(JB_EINVAL, "%s: nslots %llu (a power of two >= %u)", who, (unsigned long long)nslots, JB_CL_MIN_SLOTS);
    if (nslots > JB_CL_MAX_SLOTS) return fail(JB_ELIMIT, "%s: nslots %llu (limit 2^30)", who, (unsigned long long)nslots);
    return JB_OK;
}

int colloc_table_args(const char* who, const void* d_table, size_t ntable, const void* d_uni, uint32_t nuni) {
    if (!d_table) return fail(JB_EINVAL, "%s: null table", who);
    if (((uintptr_t)d_table & 31u) != 0) return fail(JB_EINVAL, "%s: d_table must be 32-byte aligned", who);
    if (ntable < jb_cl_bytes(JB_CL_MIN_SLOTS))
        return fail(JB_EINVAL, "%s: a table buffer of %llu bytes, the smallest table has %llu", who,
                    (unsigned long long)ntable, (unsigned long long)jb_cl_bytes(JB_CL_MIN_SLOTS));
    if (nuni && !d_uni) return fail(JB_EINVAL, "%s: null d_uni", who);
    if (((uintptr_t)d_uni & 7u) != 0) return fail(JB_EINVAL, "%s: d_uni must be 8-byte aligned", who);
    return JB_OK;
}

int colloc_add_args(const char* who, const void* ids, uint64_t ids_cap, const void* doc_tok, const void* keep,
                    uint32_t nkeep, uint32_t flags, const void* start, const void* end, const void* uni, uint32_t nuni) {
    if (flags & ~JB_COLLOC_CONTIG) return fail(JB_EINVAL, "%s: flags %#x (JB_COLLOC_CONTIG)", who, flags);
    if (!doc_tok || (ids_cap && !ids) || (nkeep && !keep) || (nuni && !uni) ||
        ((flags & JB_COLLOC_CONTIG) && ids_cap && (!start || !end)))
        return fail(JB_EINVAL, "%s: null argument", who);
    if (ids_cap >= (1ull << 32) - JB_COLLOC_TILE)
        return fail(JB_ELIMIT, "%s: an id list of %llu entries (limit 2^32 - %u)", who, (unsigned long long)ids_cap,
                    JB_COLLOC_TILE);
    return JB_OK;
}

int colloc_score_args(const char* who, const void* uni, uint32_t nuni, int scorer, uint64_t min_count) {
    if (scorer != JB_COLLOC_NPMI && scorer != JB_COLLOC_RATIO && scorer != JB_COLLOC_COUNT)
        return fail(JB_EINVAL, "%s: scorer %d (JB_COLLOC_NPMI, JB_COLLOC_RATIO or JB_COLLOC_COUNT)", who, scorer);
    if (min_count == 0) return fail(JB_EINVAL, "%s: min_count is 0", who);
    if (nuni && !uni) return fail(JB_EINVAL, "%s: null uni", who);
    return JB_OK;
}

int colloc_alloc(const char* who, uint64_t n, jb_colloc_result* out) {
    const size_t m = (size_t)(n ? n : 1);
    out->a = (uint32_t*)malloc(m * sizeof(uint32_t));
    out->b = (uint32_t*)malloc(m * sizeof(uint32_t));
    out->count = (uint64_t*)malloc(m * sizeof(uint64_t));
    out->score = (float*)malloc(m * sizeof(float));
    if (!out->a || !out->b || !out->count || !out->score) {
        free(out->a);
        free(out->b);
        free(out->count);
        free(out->score);
        out->a = out->b = nullptr;
        out->count = nullptr;
        out->score = nullptr;
        return fail(JB_ENOMEM, "%s: out of host memory for %llu pairs", who, (unsigned long long)n);
    }
    out->n = n;
    return JB_OK;
}

void colloc_sort(jb_colloc_result* out, uint64_t topn) {
    const uint64_t n = out->n;
    std::vector<uint64_t> idx(n);
    std::iota(idx.begin(), idx.end(), (uint64_t)0);
    std::sort(idx.begin(), idx.end(), [&](uint64_t x, uint64_t y) {
        return jb_cl_before(out->score[x], out->count[x], jb_cl_key(out->a[x], out->b[x]), out->score[y], out->count[y],
                            jb_cl_key(out->a[y], out->b[y]));
    });
    const uint64_t keep = topn && topn < n ? topn : n;
    std::vector<uint32_t> a(keep), b(keep);
    std::vector<uint64_t> c(keep);
    std::vector<float> s(keep);
    for (uint64_t i = 0; i < keep; i++) {
        a[i] = out->a[idx[i]];
        b[i] = out->b[idx[i]];
        c[i] = out->count[idx[i]];
        s[i] = out->score[idx[i]];
    }
    if (keep) {
        memcpy(out->a, a.data(), keep * sizeof(uint32_t));
        memcpy(out->b, b.data(), keep * sizeof(uint32_t));
        memcpy(out->count, c.data(), keep * sizeof(uint64_t));
        memcpy(out->score, s.data(), keep * sizeof(float));
    }
    out->n = keep;
}

}  // namespace jb

static size_t sat(uint64_t x) { return x > (uint64_t)SIZE_MAX ? SIZE_MAX : (size_t)x; }

extern "C" size_t jb_colloc_table_bytes(uint64_t nslots) {
    uint64_t n = JB_CL_MIN_SLOTS;  // (the least valid slot count that is >= nslots, so that the size is monotone)
    while (n < nslots && n < (1ull << 62)) n <<= 1;
    if (n > (1ull << 40)) return SIZE_MAX;
    return sat(jb_cl_bytes(n));
}

extern "C" size_t jb_colloc_work_bytes(uint64_t max_tokens, uint32_t ndocs) {
    (void)ndocs;  // (the boundary bitmap is sized by the tokens)
    if (max_tokens > (1ull << 60)) return SIZE_MAX;
    return sat(jb_cl_work_slots(max_tokens) + jb_cl_r256(jb_cl_work_bitwords(max_tokens) * 4u));
}

extern "C" void jb_colloc_result_free(jb_colloc_result* r) {
    if (!r) return;
    free(r->a);
    free(r->b);
    free(r->count);
    free(r->score);
    memset(r, 0, sizeof *r);
}

extern "C" int jb_colloc_count(const uint32_t* ids, uint64_t ids_cap, const uint64_t* doc_tok, uint64_t ntok,
                               uint32_t ndocs, const uint8_t* keep, uint32_t nkeep, uint32_t flags, const uint32_t* start,
                               const uint32_t* end, uint64_t nslots, uint64_t* uni, uint32_t nuni, jb_colloc_result* out) {
    const char* who = "jb_colloc_count";
    if (!out) return fail(JB_EINVAL, "%s: null argument", who);
    memset(out, 0, sizeof *out);
    if (const int rc = jb::colloc_add_args(who, ids, ids_cap, doc_tok, keep, nkeep, flags, start, end, uni, nuni)) return rc;
    if (nslots)
        if (const int rc = jb::colloc_slots(who, nslots)) return rc;
    const uint64_t n = std::min(ntok, ids_cap);
    uint64_t lo, hi;
    jb_cl_range(doc_tok, ndocs, n, &lo, &hi);
    try {
        // the boundary bitmap of the kernels: bit p is set iff some doc_tok[d] == p (p <= n)
        std::vector<uint32_t> bits((size_t)jb_cl_work_bitwords(n), 0u);
        for (uint64_t d = 0; d <= ndocs; d++)
            if (doc_tok[d] <= n) bits[(size_t)(doc_tok[d] >> 5)] |= 1u << (doc_tok[d] & 31u);
        std::map<uint64_t, uint64_t> m;
        for (uint64_t k = lo; k < hi; k++) {
            const uint32_t a = ids[k];
            if (a < nuni) {
                uni[a]++;
                out->known++;
            }
            if (k + 1u >= hi) continue;
            const uint32_t b = ids[k + 1u];
            if (!jb_cl_pair(k, hi, jb_cl_bit(bits.data(), k + 1u), a, b, nuni, keep, nkeep, flags, start, end)) continue;
            out->pairs++;
            const uint64_t key = jb_cl_key(a, b);
            auto it = m.find(key);
            if (it != m.end()) {
                it->second++;
            } else if (nslots == 0 || m.size() < nslots / 2u) {
                m.emplace(key, 1u);
            } else {
                out->dropped++;
            }
        }
        out->tokens = n;
        out->distinct = m.size();
        if (const int rc = jb::colloc_alloc(who, m.size(), out)) return rc;
        uint64_t i = 0;
        for (const auto& kv : m) {  // (ascending by key)
            out->a[i] = (uint32_t)(kv.first >> 32);
            out->b[i] = (uint32_t)kv.first;
            out->count[i] = kv.second;
            out->score[i] = (float)(double)kv.second;
            i++;
        }
    } catch (const std::bad_alloc&) {
        jb_colloc_result_free(out);
        return fail(JB_ENOMEM, "%s: out of host memory", who);
    }
    return JB_OK;
}

extern "C" int jb_colloc_score(const uint32_t* a, const uint32_t* b, const uint64_t* count, uint64_t n, const uint64_t* uni,
                               uint32_t nuni, uint64_t N, int scorer, uint64_t min_count, float threshold, uint64_t topn,
                               jb_colloc_result* out) {
    const char* who = "jb_colloc_score";
    if (!out) return fail(JB_EINVAL, "%s: null argument", who);
    memset(out, 0, sizeof *out);
    if (const int rc = jb::colloc_score_args(who, uni, nuni, scorer, min_count)) return rc;
    if (n && (!a || !b || !count)) return fail(JB_EINVAL, "%s: null argument", who);
    try {
        std::vector<uint64_t> idx;
        std::vector<float> sc;
        for (uint64_t i = 0; i < n; i++) {
            float s;
            if (!jb_cl_score(jb_cl_key(a[i], b[i]), count[i], uni, nuni, N, min_count, scorer, threshold, &s)) continue;
            idx.push_back(i);
            sc.push_back(s);
        }
        if (const int rc = jb::colloc_alloc(who, idx.size(), out)) return rc;
        for (size_t j = 0; j < idx.size(); j++) {
            out->a[j] = a[idx[j]];
            out->b[j] = b[idx[j]];
            out->count[j] = count[idx[j]];
            out->score[j] = sc[j];
        }
        jb::colloc_sort(out, topn);
    } catch (const std::bad_alloc&) {
        jb_colloc_result_free(out);
        return fail(JB_ENOMEM, "%s: out of host memory", who);
    }
    return JB_OK;
}
