// jb_postings.h — the postings rule (jb_postings*, jiebahip.h): what the host rule (jb_postings.cpp) and the
// gfx950 kernels (jb_postings.hip) share: the sort key of an entry, the row search, the number of digit
// passes, the argument checks and the work buffer's layout.
//
// n = min(nterms, cap, term_off[ndocs]) entries take part in the count; entry i is in the index iff i < n and
// term_id[i] < nids.  Its sort key is its id; every other entry (and every padding slot of the last tile) has
// the key nids, which sorts behind every id, so the index is the sorted list up to the first key nids.
#pragma once
#include "jb_common.h"
#include "jiebahip.h"

// The key of entry i.
JB_HD uint32_t jb_postings_key(uint32_t id, uint64_t i, uint64_t n, uint32_t nids) {
    return i < n && id < nids ? id : nids;
}

// The first j in [lo, hi) with term_off[j] > i, or hi: entry i lies in row j - 1 (doc_ub of jb_terms.hip).
JB_HD uint64_t jb_postings_row_ub(const uint64_t* term_off, uint64_t i, uint64_t lo, uint64_t hi) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (term_off[mid] > i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Passes of 8-bit digits that cover every key 0 .. nids: ceil(bit_width(nids) / 8), 1 .. 4 for nids >= 1.
JB_HD uint32_t jb_postings_passes(uint32_t nids) {
    uint32_t bits = 0;
    while (bits < 32u && (nids >> bits) != 0u) bits++;
    return bits == 0u ? 1u : (bits + 7u) / 8u;
}

// The host side (jb_postings.cpp).
#pragma GCC visibility push(hidden)
namespace jb {

// The checks the host rule and the device call share, in the order the calls report them: JB_OK, or
// JB_EINVAL / JB_ELIMIT with the thread's message set.  `who` names the entry point.
int postings_args(const char* who, uint64_t cap, uint32_t ndocs, uint32_t doc_base);
// Outputs must not alias inputs, each other or the work buffer: JB_EINVAL when two of the non-null pointers
// are equal.
int postings_alias(const char* who, const void* term_id, const void* term_cnt, const void* term_off,
                   const void* nterms, const void* post_doc, const void* post_tf, const void* post_off,
                   const void* nposts, const void* work);

// The work buffer of jb_postings_device: N = ntl * JB_POSTINGS_TILE slots; two key arrays (u32[N]) and two
// payload arrays (u64[N]: document << 32 | tf) that the passes alternate between, the tiles' digit counters
// (u32[256 * ntl], digit-major) and the 256 digit totals.
struct PostingsWork {
    uint64_t ntl;
    size_t key[2], pay[2], cnt, tot;  // byte offsets
    size_t bytes;
};
PostingsWork postings_layout(uint64_t max_terms);

}  // namespace jb
#pragma GCC visibility pop
