// jb_filter.cpp — the host side of the token filter: jb_filter, the rule of jiebahip.h on host arrays (what the
// kernels of jb_filter.hip are pinned to, on every output), the size helper, the work buffer's layout and the
// argument checks shared with the device calls.  Host only, no HIP.
#include "jb_filter.h"

#include <stdlib.h>

#include <algorithm>
#include <new>
#include <vector>

#include "jb_err.h"

namespace jb {

int filter_args(const char* who, uint64_t nbytes, uint64_t cap, const jb_filter_rule* rule, bool have_stop) {
    if (!rule) return fail(JB_EINVAL, "%s: null rule", who);
    if (rule->flags & ~JB_FILTER_STOP) return fail(JB_EINVAL, "%s: unknown flags 0x%x", who, rule->flags);
    if (rule->drop_classes & ~JB_FILTER_ALLCLASSES)
        return fail(JB_EINVAL, "%s: unknown class bits 0x%x", who, rule->drop_classes);
    if ((rule->flags & JB_FILTER_STOP) && !have_stop)
        return fail(JB_EINVAL, "%s: JB_FILTER_STOP without a stop set", who);
    if (rule->min_runes > JB_FILTER_MAXRUNES || rule->max_runes > JB_FILTER_MAXRUNES)
        return fail(JB_ELIMIT, "%s: min_runes = %u, max_runes = %u (limit %u)", who, rule->min_runes, rule->max_runes,
                    JB_FILTER_MAXRUNES);
    if (nbytes >= (1ull << 31)) return fail(JB_ELIMIT, "%s: a text of %llu bytes (limit 2 GiB)", who, (unsigned long long)nbytes);
    if (cap >= (1ull << 32) - JB_FILTER_TILE)
        return fail(JB_ELIMIT, "%s: a span list of %llu entries (limit 2^32 - %u)", who, (unsigned long long)cap,
                    JB_FILTER_TILE);
    return JB_OK;
}

int filter_alias(const char* who, const void* start, const void* end, const void* doc_tok, const void* out_start,
                 const void* out_end, const void* out_src, const void* out_doc_tok) {
    const void* in[2] = {start, end};
    const void* out[3] = {out_start, out_end, out_src};
    for (int i = 0; i < 3; i++) {
        if (!out[i]) continue;
        for (int j = 0; j < 2; j++)
            if (out[i] == in[j]) return fail(JB_EINVAL, "%s: an output array is an input array", who);
        for (int j = i + 1; j < 3; j++)
            if (out[i] == out[j]) return fail(JB_EINVAL, "%s: two output arrays are the same", who);
    }
    if (out_doc_tok && out_doc_tok == doc_tok) return fail(JB_EINVAL, "%s: out_doc_tok is doc_tok", who);
    return JB_OK;
}

FilterWork filter_layout(uint64_t max_tokens) {
    FilterWork w;
    w.ntl = std::max<uint64_t>(1u, (max_tokens + JB_FILTER_TILE - 1u) / JB_FILTER_TILE);
    auto r256 = [](size_t x) { return (x + 255u) & ~(size_t)255u; };
    w.words = 0;
    w.cnt = w.words + r256((size_t)w.ntl * (JB_FILTER_TILE / 64u) * 8u);
    w.base = w.cnt + r256((size_t)w.ntl * 32u);
    w.bytes = w.base + r256(((size_t)w.ntl + 1u) * 8u);
    return w;
}

}  // namespace jb

extern "C" size_t jb_filter_work_bytes(uint64_t max_tokens, uint32_t ndocs) {
    (void)ndocs;  // (the document lanes need no room of their own today)
    if (max_tokens > (1ull << 40)) return SIZE_MAX;
    return jb::filter_layout(max_tokens).bytes;
}

extern "C" int jb_filter(const uint8_t* text, uint64_t nbytes, const uint32_t* start, const uint32_t* end,
                         const uint64_t* doc_tok, uint64_t ntok, uint64_t cap, uint32_t ndocs, const jb_filter_rule* rule,
                         const jb_vocab* stop, uint32_t* out_start, uint32_t* out_end, uint32_t* out_src, uint64_t out_cap,
                         uint64_t* out_doc_tok, uint64_t* out_ntok, uint64_t* stats) {
    const char* who = "jb_filter";
    if (const int rc = jb::filter_args(who, nbytes, cap, rule, stop != nullptr)) return rc;
    if (!doc_tok || !out_doc_tok || !out_ntok || !stats || (nbytes && !text) || (cap && (!start || !end)) ||
        (out_cap && (!out_start || !out_end)))
        return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = jb::filter_alias(who, start, end, doc_tok, out_start, out_end, out_src, out_doc_tok)) return rc;
    const uint64_t nt = std::min(ntok, cap);
    const JbVocabView sv = stop ? stop->v.view() : JbVocabView{nullptr, nullptr, 0u, 0u};
    uint64_t n[5] = {0, 0, 0, 0, 0};  // by reason; n[0] the kept ones
    uint32_t d = 0;                   // the next document offset to write
    // R(i) for the documents that start at i, before token i is looked at
    auto docs_at = [&](uint64_t i) {
        while (d <= ndocs && std::min(doc_tok[d], nt) == i) out_doc_tok[d++] = n[0];
    };
    // (doc_tok may be out of order: every entry is computed on its own when the sweep would miss one)
    bool sorted = true;
    for (uint32_t k = 0; k < ndocs; k++) sorted = sorted && doc_tok[k] <= doc_tok[k + 1];
    std::vector<uint64_t> R;
    if (!sorted) {
        try {
            R.resize(nt + 1);
        } catch (const std::bad_alloc&) {
            return fail(JB_ENOMEM, "%s: out of host memory for %llu prefix counts", who, (unsigned long long)nt);
        }
    }
    for (uint64_t k = 0; k < nt; k++) {
        if (sorted) docs_at(k);
        else R[k] = n[0];
        const uint64_t s = start[k], e = end[k];
        uint32_t why = JB_FR_BAD;
        if (!jb_filter_bad(s, e, nbytes)) {
            const uint8_t* p = text + s;
            const uint32_t len = (uint32_t)(e - s);
            uint32_t kw[6];
            jb_filter_words(p, len, kw);
            why = jb_filter_decide(*rule, sv, kw, p, len);
        }
        if (why == JB_FR_KEEP && n[0] < out_cap) {
            out_start[n[0]] = (uint32_t)s;
            out_end[n[0]] = (uint32_t)e;
            if (out_src) out_src[n[0]] = (uint32_t)k;
        }
        n[why]++;
    }
    if (sorted) {
        docs_at(nt);
    } else {
        R[nt] = n[0];
        for (uint32_t k = 0; k <= ndocs; k++) out_doc_tok[k] = R[std::min(doc_tok[k], nt)];
    }
    *out_ntok = n[0];
    stats[0] = nt;
    for (int i = 1; i < 5; i++) stats[i] = n[i];
    return JB_OK;
}
