// jb_bm25.cpp — the host side of the BM25 calls: jb_bm25_avgdl, jb_bm25_norms, jb_bm25_idf and jb_bm25_search, the
// rule of jiebahip.h on host arrays (what the kernels of jb_bm25.hip are pinned to, on every output), the size
// helper, the work buffer's layout and the argument checks shared with the device calls.  Host only, no HIP.
#include "jb_bm25.h"

#include <stdlib.h>

#include <algorithm>
#include <new>
#include <vector>

#include "jb_err.h"

namespace jb {

int bm25_params(const char* who, double k1, double b) {
    if (!(k1 >= 0.0 && k1 <= 64.0)) return fail(JB_EINVAL, "%s: k1 = %g (want 0 <= k1 <= 64)", who, k1);
    if (!(b >= 0.0 && b <= 1.0)) return fail(JB_EINVAL, "%s: b = %g (want 0 <= b <= 1)", who, b);
    return JB_OK;
}

int bm25_avgdl_ok(const char* who, double avgdl) {
    if (!(avgdl > 0.0 && avgdl <= 1.7976931348623157e308))
        return fail(JB_EINVAL, "%s: avgdl = %g (want finite and > 0)", who, avgdl);
    return JB_OK;
}

int bm25_topk(const char* who, uint32_t topk) {
    if (topk == 0) return fail(JB_EINVAL, "%s: topk is 0", who);
    if (topk > JB_KW_MAXK) return fail(JB_ELIMIT, "%s: topk %u (limit JB_KW_MAXK = %u)", who, topk, JB_KW_MAXK);
    return JB_OK;
}

int bm25_search_args(const char* who, const void* post_doc, const void* post_tf, const void* post_off, uint64_t npost,
                     const void* norm, uint32_t ndocs, const void* weight, uint32_t nweights, const void* q_id,
                     uint64_t q_cap, const void* q_off, uint32_t nq, const void* res_doc, const void* res_score,
                     const void* res_n, const void* work) {
    if (!post_off || !q_off || (npost && (!post_doc || !post_tf)) || (ndocs && !norm) || (nweights && !weight) ||
        (q_cap && !q_id) || (nq && (!res_doc || !res_score || !res_n)))
        return fail(JB_EINVAL, "%s: null argument", who);
    const void* in[8] = {post_doc, post_tf, post_off, norm, weight, q_id, q_off, work};
    const void* out[3] = {res_doc, res_score, res_n};
    for (int i = 0; i < 3; i++) {
        if (!out[i]) continue;
        for (int j = 0; j < 8; j++)
            if (out[i] == in[j]) return fail(JB_EINVAL, "%s: an output array is an input array or the work buffer", who);
        for (int j = i + 1; j < 3; j++)
            if (out[i] == out[j]) return fail(JB_EINVAL, "%s: two output arrays are the same", who);
    }
    return JB_OK;
}

Bm25Work bm25_layout(uint32_t nq, uint32_t ndocs, uint32_t topk) {
    Bm25Work w;
    auto r256 = [](size_t x) { return (x + 255u) & ~(size_t)255u; };
    w.ntiles = ((uint64_t)ndocs + JB_BM25_TILE - 1u) / JB_BM25_TILE;  // <= 2^19
    const size_t pairs = std::max<size_t>((size_t)nq * (size_t)w.ntiles, 1u);  // < 2^51
    const size_t k = std::max<uint32_t>(std::min<uint32_t>(topk, JB_KW_MAXK), 1u);
    w.pscore = 0;
    w.pdoc = w.pscore + r256(pairs * k * 8u);
    w.pcnt = w.pdoc + r256(pairs * k * 4u);
    w.bytes1 = w.pcnt + r256(pairs * 4u);
    w.dense = w.bytes1;
    const size_t cells = std::max<size_t>((size_t)nq * (size_t)ndocs, 1u);  // < 2^64
    w.bytes = cells > (SIZE_MAX >> 4) || w.bytes1 > (SIZE_MAX >> 4) ? SIZE_MAX : w.dense + r256(cells * 8u);
    return w;
}

}  // namespace jb

extern "C" size_t jb_bm25_work_bytes(uint32_t nq, uint32_t ndocs, uint32_t topk) {
    return jb::bm25_layout(nq, ndocs, topk).bytes;
}

extern "C" int jb_bm25_avgdl(const uint32_t* doc_len, uint32_t ndocs, double* avgdl) {
    const char* who = "jb_bm25_avgdl";
    if (!avgdl || (ndocs && !doc_len)) return fail(JB_EINVAL, "%s: null argument", who);
    if (ndocs == 0) return fail(JB_EINVAL, "%s: no documents", who);
    uint64_t sum = 0;
    for (uint32_t d = 0; d < ndocs; d++) sum += doc_len[d];
    if (sum == 0) return fail(JB_EINVAL, "%s: every document is empty", who);
    *avgdl = (double)sum / (double)ndocs;
    return JB_OK;
}

extern "C" int jb_bm25_norms(const uint32_t* doc_len, uint32_t ndocs, double k1, double b, double avgdl, float* norm) {
    const char* who = "jb_bm25_norms";
    if (const int rc = jb::bm25_params(who, k1, b)) return rc;
    if (const int rc = jb::bm25_avgdl_ok(who, avgdl)) return rc;
    if (ndocs && (!doc_len || !norm)) return fail(JB_EINVAL, "%s: null argument", who);
    if (ndocs && (const void*)doc_len == (const void*)norm) return fail(JB_EINVAL, "%s: the output is the input", who);
    for (uint32_t d = 0; d < ndocs; d++) norm[d] = jb_bm25_norm(doc_len[d], k1, b, avgdl);
    return JB_OK;
}

extern "C" int jb_bm25_idf(const uint64_t* post_off, uint32_t nids, uint64_t ndocs_total, float* weight) {
    const char* who = "jb_bm25_idf";
    if (ndocs_total >= (1ull << 53))
        return fail(JB_ELIMIT, "%s: %llu documents (limit 2^53)", who, (unsigned long long)ndocs_total);
    if (!post_off || (nids && !weight)) return fail(JB_EINVAL, "%s: null argument", who);
    if ((const void*)post_off == (const void*)weight) return fail(JB_EINVAL, "%s: the output is the input", who);
    for (uint32_t t = 0; t < nids; t++) weight[t] = jb_bm25_weight(jb_bm25_df(post_off, t, ndocs_total), ndocs_total);
    return JB_OK;
}

extern "C" int jb_bm25_search(const uint32_t* post_doc, const uint32_t* post_tf, const uint64_t* post_off,
                              uint64_t npost, uint32_t nids, const float* norm, uint32_t ndocs, const float* weight,
                              uint32_t nweights, double k1, const uint32_t* q_id, uint64_t q_cap, const uint64_t* q_off,
                              uint32_t nq, uint32_t topk, uint32_t* res_doc, uint64_t* res_score, uint32_t* res_n) {
    const char* who = "jb_bm25_search";
    if (const int rc = jb::bm25_topk(who, topk)) return rc;
    if (const int rc = jb::bm25_params(who, k1, 0.0)) return rc;
    if (const int rc = jb::bm25_search_args(who, post_doc, post_tf, post_off, npost, norm, ndocs, weight, nweights, q_id,
                                            q_cap, q_off, nq, res_doc, res_score, res_n, nullptr))
        return rc;
    std::vector<uint64_t> acc;   // the dense row of one query, zero between queries
    std::vector<uint32_t> seen;  // the documents whose cell left zero
    try {
        acc.assign(ndocs, 0);
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "%s: out of host memory for %u scores", who, ndocs);
    }
    const double k1p1 = k1 + 1.0;
    const auto before = [&](uint32_t a, uint32_t b) { return jb_bm25_before(acc[a], a, acc[b], b); };
    for (uint32_t q = 0; q < nq; q++) {
        uint64_t qlo;
        const uint32_t n = jb_bm25_query(q_off, q, q_cap, &qlo);
        seen.clear();
        try {
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t t = q_id[qlo + j];
                const float w = jb_bm25_entry(t, nids, nweights, weight);
                if (!(w > 0.0f)) continue;
                uint64_t lo, hi;
                jb_bm25_list(post_off, t, npost, &lo, &hi);
                for (uint64_t i = lo; i < hi; i++) {
                    const uint32_t d = post_doc[i], tf = post_tf[i];
                    if (!jb_bm25_posting(d, tf, ndocs, norm)) continue;
                    const uint64_t c = jb_bm25_contrib(w, tf, norm[d], k1p1);
                    if (c == 0) continue;
                    if (acc[d] == 0) seen.push_back(d);
                    acc[d] += c;
                }
            }
        } catch (const std::bad_alloc&) {
            return fail(JB_ENOMEM, "%s: out of host memory for the candidates", who);
        }
        const uint32_t k = (uint32_t)std::min<size_t>(topk, seen.size());
        std::partial_sort(seen.begin(), seen.begin() + k, seen.end(), before);
        for (uint32_t r = 0; r < topk; r++) {
            res_doc[(size_t)q * topk + r] = r < k ? seen[r] : JB_ID_UNK;
            res_score[(size_t)q * topk + r] = r < k ? acc[seen[r]] : 0;
        }
        res_n[q] = k;
        for (const uint32_t d : seen) acc[d] = 0;
    }
    return JB_OK;
}
