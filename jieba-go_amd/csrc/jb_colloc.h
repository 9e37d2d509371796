// jb_colloc.h — the collocation rule (jb_colloc_*, jiebahip.h): what the host rule (jb_colloc.cpp) and the gfx950
// kernels (jb_colloc.hip) share: the table's layout, the hash, the read-only probe, which tokens and pairs take
// part, the score of a pair and the order of two results.
//
// The table is one caller-owned device buffer:
//   header          JB_CL_HDR_BYTES: JbClHeader (the magic word, nslots, the five u64 totals)
//   key[nslots]     u64  (uint64_t)a << 32 | b of the slot's pair (JB_CL_EMPTY, all ones: the slot is empty; no
//                        pair has it, because a < nuni <= 2^32 - 1)
//   cnt[nslots]     u64  the pairs counted for the slot's key
// nslots is a power of two within jb_wc's limits; a new key is accepted while fewer than nslots / 2 slots are
// claimed (lanes that claim at the same moment can pass the half, so no probe relies on an empty slot: each is
// bounded by nslots steps).  A key sits at the first slot from jb_cl_home(key) on, stepping by one, that was
// empty when it came.  The whole key is the word the claim compares and swaps, so a slot never holds two keys.
#pragma once
#include "jb_bm25.h"  // jb_bm25_log, go_log's restatement for host and device
#include "jb_common.h"
#include "jiebahip.h"

#define JB_CL_HDR_BYTES 256u
#define JB_CL_MIN_SLOTS 8u
#define JB_CL_MAX_SLOTS (1u << 30)
#define JB_CL_SLOT_BYTES 16u
#define JB_CL_MAGIC 0x31544C43424Aull  // "JBCLT1"
#define JB_CL_EMPTY 0xFFFFFFFFFFFFFFFFull
// d_work codes of the tokens without a slot (slots are < JB_CL_MAX_SLOTS)
#define JB_CL_NOSLOT 0xFFFFFFFFu  // a pair that found and claimed no slot: looked up again by the count pass
#define JB_CL_NOPAIR 0xFFFFFFFEu  // (k, k + 1) takes no part

enum { JB_CL_TOKENS = 0, JB_CL_KNOWN, JB_CL_PAIRS, JB_CL_DROPPED, JB_CL_DISTINCT, JB_CL_NCTR };

struct JbClHeader {
    uint64_t magic, nslots;
    unsigned long long ctr[JB_CL_NCTR];  // JB_CL_*: totals over every batch added; DISTINCT counts the claims
};

struct JbClView {
    JbClHeader* hdr;
    uint64_t* key;
    uint64_t* cnt;
    uint32_t mask;  // nslots - 1
};

JB_HD uint64_t jb_cl_r256(uint64_t x) { return (x + 255u) & ~(uint64_t)255u; }
JB_HD uint64_t jb_cl_bytes(uint64_t nslots) { return JB_CL_HDR_BYTES + nslots * JB_CL_SLOT_BYTES; }
JB_HD bool jb_cl_slots_ok(uint64_t nslots) {
    return nslots >= JB_CL_MIN_SLOTS && nslots <= JB_CL_MAX_SLOTS && (nslots & (nslots - 1u)) == 0;
}
JB_HD JbClView jb_cl_view(void* base, uint64_t nslots) {
    uint8_t* b = (uint8_t*)base;
    JbClView v;
    v.hdr = (JbClHeader*)b;
    v.key = (uint64_t*)(b + JB_CL_HDR_BYTES);
    v.cnt = v.key + nslots;
    v.mask = (uint32_t)(nslots - 1u);
    return v;
}

// The work buffer: work[max_tokens] u32 (the slot of pair (k, k + 1), or a code), then a bitmap of max_tokens + 1
// bits in u32 words: bit p is set iff some doc_tok[d] == p, d in [0, ndocs].
JB_HD uint64_t jb_cl_work_slots(uint64_t max_tokens) { return jb_cl_r256((max_tokens ? max_tokens : 1u) * 4u); }
JB_HD uint64_t jb_cl_work_bitwords(uint64_t max_tokens) { return max_tokens / 32u + 1u; }

JB_HD uint64_t jb_cl_key(uint32_t a, uint32_t b) { return (uint64_t)a << 32 | b; }
// splitmix64's finalizer: the home slot of a key.
JB_HD uint32_t jb_cl_home(uint64_t key, uint32_t mask) {
    uint64_t x = key + 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)x & mask;
}
JB_HD uint32_t jb_cl_next(uint32_t s, uint32_t mask) { return (s + 1u) & mask; }

// The slot that holds key, or JB_CL_NOSLOT: a read-only probe of at most nslots steps that ends at the first
// empty slot.
JB_HD uint32_t jb_cl_find(const uint64_t* keyv, uint32_t mask, uint64_t key) {
    uint32_t s = jb_cl_home(key, mask);
    for (uint32_t i = 0; i <= mask; i++, s = jb_cl_next(s, mask)) {
        const uint64_t f = keyv[s];
        if (f == key) return s;
        if (f == JB_CL_EMPTY) break;
    }
    return JB_CL_NOSLOT;
}

// Tokens lo <= k < hi belong to a document: lo = doc_tok[0], hi = doc_tok[ndocs], both clamped to n, the tokens
// that exist.
JB_HD void jb_cl_range(const uint64_t* doc_tok, uint32_t ndocs, uint64_t n, uint64_t* lo, uint64_t* hi) {
    const uint64_t a = doc_tok[0], z = doc_tok[ndocs];
    *lo = a < n ? a : n;
    *hi = z < n ? z : n;
}
JB_HD bool jb_cl_bit(const uint32_t* bits, uint64_t p) { return (bits[p >> 5] >> (p & 31u)) & 1u; }

// Does id take part in pairs?  Below nuni, and kept.  keep is read only below nkeep.
JB_HD bool jb_cl_kept(uint32_t id, uint32_t nuni, const uint8_t* keep, uint32_t nkeep) {
    if (id >= nuni) return false;
    if (nkeep == 0) return true;
    return id < nkeep && keep[id] != 0;
}

// Does (k, k + 1) take part, for a token k in [lo, hi) with ids a and b?  bound: the bitmap's bit of k + 1.
JB_HD bool jb_cl_pair(uint64_t k, uint64_t hi, bool bound, uint32_t a, uint32_t b, uint32_t nuni, const uint8_t* keep,
                      uint32_t nkeep, uint32_t flags, const uint32_t* start, const uint32_t* end) {
    if (k + 1u >= hi || bound) return false;
    if (!jb_cl_kept(a, nuni, keep, nkeep) || !jb_cl_kept(b, nuni, keep, nkeep)) return false;
    if ((flags & JB_COLLOC_CONTIG) && end[k] != start[k + 1u]) return false;
    return true;
}

// The score of a pair with count c under uni / N; false when the pair is no candidate.  f64, one rounding per
// operation (the build uses -ffp-contract=off -fno-fast-math), then one narrowing.  Every argument of the
// logarithm is a positive normal number: 1 <= c < N < 2^53 and 1 <= ca, cb < 2^53.
JB_HD bool jb_cl_score(uint64_t key, uint64_t c, const uint64_t* uni, uint32_t nuni, uint64_t N, uint64_t m, int scorer,
                       float threshold, float* score) {
    const uint32_t a = (uint32_t)(key >> 32), b = (uint32_t)key;
    if (a >= nuni || b >= nuni || c < m) return false;
    const uint64_t ca = uni[a], cb = uni[b], lim = 1ull << 53;
    if (ca == 0 || cb == 0 || c >= N || c >= lim || ca >= lim || cb >= lim || N >= lim) return false;
    double s;
    if (scorer == JB_COLLOC_NPMI) {
        const double dn = (double)N;
        const double pa = (double)ca / dn;
        const double pb = (double)cb / dn;
        const double pab = (double)c / dn;
        const double papb = pa * pb;
        const double r = pab / papb;
        const double num = jb_bm25_log(r);
        const double den = 0.0 - jb_bm25_log(pab);
        s = num / den;
    } else if (scorer == JB_COLLOC_RATIO) {
        const double x = (double)(c - m) / (double)ca;
        const double y = x / (double)cb;
        s = y * (double)N;
    } else {
        s = (double)c;
    }
    const float f = (float)s;
    *score = f;
    return f >= threshold;  // (false for NaN)
}

// Result (sa, ca, ka) ranks before (sb, cb, kb): score descending, count descending, then the key ascending.
JB_HD bool jb_cl_before(float sa, uint64_t ca, uint64_t ka, float sb, uint64_t cb, uint64_t kb) {
    if (sa != sb) return sa > sb;
    if (ca != cb) return ca > cb;
    return ka < kb;
}

// The host side (jb_colloc.cpp).
#pragma GCC visibility push(hidden)
namespace jb {

// The checks the host rule and the device calls share: JB_OK, or JB_EINVAL / JB_ELIMIT with the thread's message set.
int colloc_slots(const char* who, uint64_t nslots);
// What every call that is handed a table checks: JB_OK, or JB_EINVAL with the thread's message set.
int colloc_table_args(const char* who, const void* d_table, size_t ntable, const void* d_uni, uint32_t nuni);
int colloc_add_args(const char* who, const void* ids, uint64_t ids_cap, const void* doc_tok, const void* keep,
                    uint32_t nkeep, uint32_t flags, const void* start, const void* end, const void* uni, uint32_t nuni);
int colloc_score_args(const char* who, const void* uni, uint32_t nuni, int scorer, uint64_t min_count);
// out's arrays allocated for n entries (the totals untouched): JB_OK or JB_ENOMEM.
int colloc_alloc(const char* who, uint64_t n, ::jb_colloc_result* out);
// out's n entries sorted into the rule's order and cut to the first topn (0: all).
void colloc_sort(::jb_colloc_result* out, uint64_t topn);

}  // namespace jb
#pragma GCC visibility pop
