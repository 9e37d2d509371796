// jb_neardup.h — the near-duplicate rule (jb_neardup*, jiebahip.h): what the host rule (jb_neardup.cpp) and the
// gfx950 kernels (jb_neardup.hip) share: an entry's identity, the bucket match, the first-band test, the slot
// comparison of the agree count, the argument checks and the work buffer's layout.
//
// Entry e = d * B + b is document d in band b with the key key[e]; it is a member of the bucket (b, key[e])
// unless the key is JB_MH_NOKEY.  Sorted by (band, key) with the entries of equal (band, key) in the order of
// e, a bucket is a contiguous run with its documents ascending, so the member `w + 1` places before a member
// is the one whose rank is w + 1 lower.
#pragma once
#include "jb_common.h"
#include "jiebahip.h"

JB_HD uint32_t jb_nd_doc(uint32_t e, uint32_t B) { return e / B; }
JB_HD uint32_t jb_nd_band(uint32_t e, uint32_t B) { return e % B; }

// Entries ea (key ka) and eb (key kb) are members of one bucket.
JB_HD bool jb_nd_same(uint32_t ea, uint64_t ka, uint32_t eb, uint64_t kb, uint32_t B) {
    return ka == kb && ka != JB_MH_NOKEY && jb_nd_band(ea, B) == jb_nd_band(eb, B);
}

// Band b is the first band in which documents i and j share a bucket, given that they share one in band b.
JB_HD bool jb_nd_first(const uint64_t* key, uint32_t i, uint32_t j, uint32_t B, uint32_t b) {
    const uint64_t* ri = key + (uint64_t)i * B;
    const uint64_t* rj = key + (uint64_t)j * B;
    for (uint32_t c = 0; c < b; c++)
        if (ri[c] == rj[c] && ri[c] != JB_MH_NOKEY) return false;
    return true;
}

// Slot s of the agree count: 1 when s < K and documents i and j hold the same value there.
JB_HD uint32_t jb_nd_eq(const uint32_t* sig, uint32_t i, uint32_t j, uint32_t K, uint32_t s) {
    return s < K && sig[(uint64_t)i * K + s] == sig[(uint64_t)j * K + s] ? 1u : 0u;
}

// The host side (jb_neardup.cpp).
#pragma GCC visibility push(hidden)
namespace jb {

// The checks the host rule and the device call share, in the order the calls report them: JB_OK, or
// JB_EINVAL / JB_ELIMIT with the thread's message set.  `who` names the entry point.
int neardup_args(const char* who, uint32_t ndocs, uint32_t B, uint32_t K, uint32_t W, uint32_t min_agree);
// Outputs must not alias inputs, each other or the work buffer: JB_EINVAL when two of the non-null pointers
// are equal.
int neardup_alias(const char* who, const void* key, const void* sig, const void* pair_doc, const void* pair_agree,
                  const void* pair_off, const void* npairs, const void* stat, const void* work);

// The work buffer of jb_neardup_device: N = ntl * JB_ND_TILE slots; two key arrays (u64[N]) and two payload
// arrays (u32[N]: the entry) that the nine passes alternate between, the tiles' digit counters (u32[256 * ntl],
// digit-major), the 256 digit totals, and per tile the three counters of the mask pass (u32[3 * ntl]) and the
// offset of its first pair (u64[ntl]).  The last pass writes arrays 0; after it key[1] holds the keep masks
// (u64 per sorted position) and pay[1] the entries' pair counts, then their offsets inside their tile.
struct NeardupWork {
    uint64_t ntl;
    size_t key[2], pay[2], cnt, tot, part, tbase;  // byte offsets
    size_t bytes;
};
NeardupWork neardup_layout(uint64_t nentries);

}  // namespace jb
#pragma GCC visibility pop
