// jb_postings.cpp — the host side of the postings call: jb_postings, the rule of jiebahip.h on host arrays (what
// the kernels of jb_postings.hip are pinned to, on every output), the size helper, the work buffer's layout and
// the argument checks shared with the device call.  Host only, no HIP.
#include "jb_postings.h"

#include <stdlib.h>

#include <algorithm>
#include <new>
#include <vector>

#include "jb_err.h"

namespace jb {

int postings_args(const char* who, uint64_t cap, uint32_t ndocs, uint32_t doc_base) {
    if (cap >= (1ull << 32) - JB_POSTINGS_TILE)
        return fail(JB_ELIMIT, "%s: a term list of %llu entries (limit 2^32 - %u)", who, (unsigned long long)cap,
                    JB_POSTINGS_TILE);
    if ((uint64_t)doc_base + ndocs > (1ull << 32))
        return fail(JB_ELIMIT, "%s: doc_base %u + %u documents pass 2^32", who, doc_base, ndocs);
    return JB_OK;
}

int postings_alias(const char* who, const void* term_id, const void* term_cnt, const void* term_off,
                   const void* nterms, const void* post_doc, const void* post_tf, const void* post_off,
                   const void* nposts, const void* work) {
    const void* in[5] = {term_id, term_cnt, term_off, nterms, work};
    const void* out[4] = {post_doc, post_tf, post_off, nposts};
    for (int i = 0; i < 4; i++) {
        if (!out[i]) continue;
        for (int j = 0; j < 5; j++)
            if (out[i] == in[j]) return fail(JB_EINVAL, "%s: an output array is an input array", who);
        for (int j = i + 1; j < 4; j++)
            if (out[i] == out[j]) return fail(JB_EINVAL, "%s: two output arrays are the same", who);
    }
    return JB_OK;
}

PostingsWork postings_layout(uint64_t max_terms) {
    PostingsWork w;
    w.ntl = std::max<uint64_t>(1u, (max_terms + JB_POSTINGS_TILE - 1u) / JB_POSTINGS_TILE);
    auto r256 = [](size_t x) { return (x + 255u) & ~(size_t)255u; };
    const size_t slots = (size_t)w.ntl * JB_POSTINGS_TILE;
    w.key[0] = 0;
    w.key[1] = w.key[0] + r256(slots * 4u);
    w.pay[0] = w.key[1] + r256(slots * 4u);
    w.pay[1] = w.pay[0] + r256(slots * 8u);
    w.cnt = w.pay[1] + r256(slots * 8u);
    w.tot = w.cnt + r256((size_t)w.ntl * 256u * 4u);
    w.bytes = w.tot + r256(256u * 4u);
    return w;
}

}  // namespace jb

extern "C" size_t jb_postings_work_bytes(uint64_t max_terms, uint64_t nids, uint32_t ndocs) {
    (void)nids;   // (the passes alternate between the same arrays however many there are)
    (void)ndocs;  // (rows are searched in term_off itself)
    if (max_terms > (1ull << 40)) return SIZE_MAX;
    return jb::postings_layout(max_terms).bytes;
}

extern "C" int jb_postings(const uint32_t* term_id, const uint32_t* term_cnt, const uint64_t* term_off, uint64_t nterms,
                           uint64_t cap, uint32_t ndocs, uint32_t nids, uint32_t doc_base, uint32_t* post_doc,
                           uint32_t* post_tf, uint64_t pcap, uint64_t* post_off, uint64_t* nposts) {
    const char* who = "jb_postings";
    if (const int rc = jb::postings_args(who, cap, ndocs, doc_base)) return rc;
    if (!term_off || !post_off || !nposts || (cap && (!term_id || !term_cnt)) || (pcap && (!post_doc || !post_tf)))
        return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = jb::postings_alias(who, term_id, term_cnt, term_off, nullptr, post_doc, post_tf, post_off, nposts,
                                          nullptr))
        return rc;
    const uint64_t n = std::min(std::min(nterms, cap), term_off[ndocs]);
    // a counting sort by id: the list lengths, their prefixes, then every entry at its list's next slot
    for (uint64_t t = 0; t <= nids; t++) post_off[t] = 0;
    for (uint64_t i = 0; i < n; i++)
        if (term_id[i] < nids) post_off[(uint64_t)term_id[i] + 1u]++;
    for (uint64_t t = 0; t < nids; t++) post_off[t + 1u] += post_off[t];
    *nposts = post_off[nids];
    if (pcap == 0 || *nposts == 0) return JB_OK;
    std::vector<uint64_t> next;
    try {
        next.assign(post_off, post_off + nids);
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "%s: out of host memory for %u list positions", who, nids);
    }
    // (term_off is trusted: on offsets that decrease the documents mean nothing, but they are only values)
    uint64_t d = 0;
    for (uint64_t i = 0; i < n; i++) {
        while (d < ndocs && term_off[d + 1u] <= i) d++;
        const uint32_t id = term_id[i];
        if (id >= nids) continue;
        const uint64_t at = next[id]++;
        if (at >= pcap) continue;
        post_doc[at] = doc_base + (uint32_t)d;
        post_tf[at] = term_cnt[i];
    }
    return JB_OK;
}
