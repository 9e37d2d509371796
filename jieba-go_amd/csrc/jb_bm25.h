// jb_bm25.h — the BM25 rule (jb_bm25_*, jiebahip.h): what the host rule (jb_bm25.cpp) and the gfx950 kernels
// (jb_bm25.hip) share: the norm of a document, the weight of an id, which query entries and postings take part,
// the contribution of a posting, the order of two records, the argument checks and the work buffer's layout.
//
// Every score is an integer in units of 2^-24: a posting's contribution is computed in f64, one rounding per
// operation (the build uses -ffp-contract=off -fno-fast-math), and truncated to a u64, and a document's score is
// the u64 sum of its contributions, so host and device agree whatever the order of the adds.
#pragma once
#include "jb_common.h"
#include "jiebahip.h"

// go_log (jb_image.cpp; jb_go_log) for a positive normal x, frexp by the bits: the same operations in the same
// order.  The weight's argument is 1 + (N - df + 0.5) / (df + 0.5), which lies in (1, 2^54).
JB_HD double jb_bm25_log(double x) {
    const double Ln2Hi = 6.93147180369123816490e-01, Ln2Lo = 1.90821492927058770002e-10,
                 L1 = 6.666666666666735130e-01, L2 = 3.999999999940941908e-01, L3 = 2.857142874366239149e-01,
                 L4 = 2.222219843214978396e-01, L5 = 1.818357216161805012e-01, L6 = 1.531383769920937332e-01,
                 L7 = 1.479819860511658591e-01;
    union {
        double d;
        uint64_t u;
    } v;
    v.d = x;
    int ki = (int)((v.u >> 52) & 0x7FFu) - 1022;
    v.u = (v.u & ~(0x7FFull << 52)) | (1022ull << 52);  // [0.5, 1)
    double f1 = v.d;
    if (f1 < 0.70710678118654752440) {  // Sqrt2/2
        f1 *= 2;
        ki--;
    }
    const double f = f1 - 1;
    const double k = (double)ki;
    const double s = f / (2 + f);
    const double s2 = s * s;
    const double s4 = s2 * s2;
    const double t1 = s2 * (L1 + s4 * (L3 + s4 * (L5 + s4 * L7)));
    const double t2 = s4 * (L2 + s4 * (L4 + s4 * L6));
    const double R = t1 + t2;
    const double hfsq = 0.5 * f * f;
    return k * Ln2Hi - ((hfsq - (s * (hfsq + R) + k * Ln2Lo)) - f);
}

// norm[d]: k1 * ((1 - b) + b * (len / avgdl)), each operation one f64 rounding, then one narrowing.
JB_HD float jb_bm25_norm(uint32_t len, double k1, double b, double avgdl) {
    const double r = (double)len / avgdl;
    const double br = b * r;
    const double ob = 1.0 - b;
    const double s = ob + br;
    return (float)(k1 * s);
}

// df of id t: the list's length, at most ndocs_total, 0 when the offsets decrease.
JB_HD uint64_t jb_bm25_df(const uint64_t* post_off, uint64_t t, uint64_t ndocs_total) {
    const uint64_t lo = post_off[t], hi = post_off[t + 1u];
    if (hi <= lo) return 0;
    return hi - lo < ndocs_total ? hi - lo : ndocs_total;
}

// weight[t] from df (Lucene's form, > 0 for df >= 1): 0 for df == 0.
JB_HD float jb_bm25_weight(uint64_t df, uint64_t ndocs_total) {
    if (df == 0) return 0.0f;
    const double num = (double)(ndocs_total - df) + 0.5;
    const double den = (double)df + 0.5;
    const double q = num / den;
    return (float)jb_bm25_log(1.0 + q);
}

// Query q's entries: [*lo, *lo + n) of q_id, n <= JB_BM25_MAXQ.
JB_HD uint32_t jb_bm25_query(const uint64_t* q_off, uint64_t q, uint64_t q_cap, uint64_t* lo) {
    const uint64_t a = q_off[q] < q_cap ? q_off[q] : q_cap;
    const uint64_t z = q_off[q + 1u] < q_cap ? q_off[q + 1u] : q_cap;
    *lo = a;
    if (z <= a) return 0;
    return z - a < JB_BM25_MAXQ ? (uint32_t)(z - a) : (uint32_t)JB_BM25_MAXQ;
}

// The weight of an entry with id t, or 0 when the entry does not take part.  No table is indexed by an id that
// is not checked.
JB_HD float jb_bm25_entry(uint32_t t, uint32_t nids, uint32_t nweights, const float* weight) {
    if (t >= nids || t >= nweights) return 0.0f;
    const float w = weight[t];
    return w > 0.0f && w <= JB_BM25_WMAX ? w : 0.0f;
}

// The list of id t < nids, clamped to [0, npost]: [*lo, *hi), empty when the offsets decrease.
JB_HD void jb_bm25_list(const uint64_t* post_off, uint32_t t, uint64_t npost, uint64_t* lo, uint64_t* hi) {
    const uint64_t a = post_off[t] < npost ? post_off[t] : npost;
    const uint64_t z = post_off[(uint64_t)t + 1u] < npost ? post_off[(uint64_t)t + 1u] : npost;
    *lo = a;
    *hi = z < a ? a : z;
}

// A posting takes part iff its document is below ndocs, its tf is positive and the document's norm is not
// negative (which excludes NaN): then den >= 1, num / den <= k1 + 1 <= 65 and the contribution is below 2^51.
JB_HD bool jb_bm25_posting(uint32_t doc, uint32_t tf, uint32_t ndocs, const float* norm) {
    return doc < ndocs && tf > 0u && norm[doc] >= 0.0f;
}

// The contribution of a participating posting under an entry of weight w, in units of 2^-24.
JB_HD uint64_t jb_bm25_contrib(float w, uint32_t tf, float nrm, double k1p1) {
    const double num = (double)tf * k1p1;
    const double den = (double)tf + (double)nrm;
    const double r = num / den;
    const double x = (double)w * r;
    return (uint64_t)(x * 16777216.0);
}

// The first i in [lo, hi) with post_doc[i] >= d, or hi (lists ascend by document).
JB_HD uint64_t jb_bm25_lb(const uint32_t* post_doc, uint64_t lo, uint64_t hi, uint64_t d) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)post_doc[mid] >= d) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// Record (sa, da) ranks before (sb, db): score descending, ties by document ascending.
JB_HD bool jb_bm25_before(uint64_t sa, uint32_t da, uint64_t sb, uint32_t db) {
    return sa > sb || (sa == sb && da < db);
}

// The host side (jb_bm25.cpp).
#pragma GCC visibility push(hidden)
namespace jb {

// The checks the host rules and the device calls share, in the order the calls report them: JB_OK, or
// JB_EINVAL / JB_ELIMIT with the thread's message set.  `who` names the entry point.
int bm25_params(const char* who, double k1, double b);
int bm25_avgdl_ok(const char* who, double avgdl);
int bm25_topk(const char* who, uint32_t topk);
// The null and aliasing checks of a search (work may be null: the host rule has none).
int bm25_search_args(const char* who, const void* post_doc, const void* post_tf, const void* post_off, uint64_t npost,
                     const void* norm, uint32_t ndocs, const void* weight, uint32_t nweights, const void* q_id,
                     uint64_t q_cap, const void* q_off, uint32_t nq, const void* res_doc, const void* res_score,
                     const void* res_n, const void* work);

// The work buffer of jb_bm25_search_device.  Both forms: per pair of query and document tile a count (u32) and
// topk partial records (u64 scores, u32 documents).  Form 0 also: a dense u64 row of ndocs per query.
struct Bm25Work {
    uint64_t ntiles;
    size_t pscore, pdoc, pcnt, dense;  // byte offsets
    size_t bytes1;                     // what form 1 needs (the partials)
    size_t bytes;                      // what form 0 needs: everything (SIZE_MAX when it overflows)
};
Bm25Work bm25_layout(uint32_t nq, uint32_t ndocs, uint32_t topk);

}  // namespace jb
#pragma GCC visibility pop
