// jb_terms.hip — gfx950 kernels of the term-count and keyword calls (jb_terms_device,
// jb_keywords_device): a unit of its own, it shares nothing with the cut pipeline.
//
// jb_terms_device: an id list (one u32 per token, any mode) and its per-document offsets become the
// document-term matrix as CSR: per document its distinct ids, ascending, each with its count.
//   k_terms_sort   per tile of kTermsTile consecutive tokens, whatever documents they belong to: the keys
//                  (document << 32 | id; unknown ids and tokens of no document are all-ones) are sorted
//                  (bitonic, in registers and LDS) and run-length counted.  The runs of document d go to the work list
//                  W0 at [max(first token of d, tile start), ...): every document's runs lie inside its
//                  own token range, and the first run of each group carries a flag.  A document inside
//                  one tile is finished here.
//   k_terms_merge / k_terms_copy   a document that spans several tiles has one sorted list per tile.
//                  Pass p joins, for every aligned group of 2^(p+1) tiles whose middle boundary lies
//                  inside one document, that document's list left of the boundary with the one right of
//                  it: each entry finds its rank in the other list by binary search (equal ids stay
//                  side by side, left first), the merged list is written to W1 and copied back.  The
//                  number of passes depends on the capacity alone; a pass without such a document ends
//                  after a few loads per group.
//   k_terms_count / k_terms_scan / k_terms_write   an entry starts a term when it is flagged or its id
//                  differs from the entry before it.  The terms in list order are the CSR in order, so a
//                  count per tile and one scan give every term its index and every document its offset;
//                  the writer sums the counts of the equal ids that follow a term's first entry.
// jb_keywords_device: k_keywords, one wave per document.  The wave keeps the 64 best keys
// (score bits << 32 | ~id, so that the order is score descending, then id ascending) sorted over its
// lanes, reads the document's terms 64 at a time, and joins a batch that holds a better key by a
// bitonic sort of the batch and one bitonic merge.
//
// jb_df_device: k_df / k_df_combine add 1 to df[id] for every entry of a CSR's flat id list, the
// document frequencies of the batch (a row holds each id once).  k_df is one global atomic per entry;
// k_df_combine gives each workgroup a contiguous share of the list and a direct-mapped table in LDS
// (id tag and count per slot), and flushes the table with one global atomic per occupied slot.
// jb_idf_device: k_idf, one thread per id, the rule of jb_idf with go_log restated for the device.
//
// Nothing here synchronises, allocates or reads on the host; the launch counts depend on host values.
#include <hip/hip_runtime.h>

#include "jb_kstages.h"

#include <algorithm>

namespace jb {

namespace {

constexpr uint32_t T = kTermsTile;
constexpr uint32_t kNone = 0xFFFFFFFFu;    // no document
constexpr uint64_t kFlag = 0x80000000ull;  // entry: id << 32 | flag << 31 | count (31 bits, never 0)
constexpr uint64_t kCntMask = 0x7FFFFFFFull;
static_assert(T == 4096, "k_terms_sort's thread layout: 256 threads x 16 tokens");

__device__ __forceinline__ uint32_t ent_id(uint64_t e) { return (uint32_t)(e >> 32); }
__device__ __forceinline__ uint32_t ent_cnt(uint64_t e) { return (uint32_t)(e & kCntMask); }

// First j in [lo, hi) with doc_tok[j] > k, else hi.
__device__ __forceinline__ uint64_t doc_ub(const uint64_t* __restrict__ doc_tok, uint64_t k, uint64_t lo, uint64_t hi) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (doc_tok[mid] > k) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Inclusive scan over the 64 lanes of a wave.
__device__ __forceinline__ uint32_t wave_incl(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// Exclusive scan of one value per thread over a workgroup of NW waves; *total receives the sum.
template <uint32_t NW>
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t* sh /* NW + 1 */, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t inc = wave_incl(v, lane);
    __syncthreads();  // (sh may still be read from an earlier call)
    if (lane == 63u) sh[w] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < NW; k++) {
        const uint32_t x = sh[k];
        if (k < w) before += x;
        all += x;
    }
    *total = all;
    return before + inc - v;
}

// ---------------------------------------------------------------------------
// k_terms_sort
// ---------------------------------------------------------------------------
// The tile's keys in LDS: index i lives at i + i / 16 (one pad slot per 16 keys), which keeps the three
// register layouts below free of bank conflicts.
constexpr uint32_t kKeySlots = T + T / 16;
__device__ __forceinline__ uint32_t kslot(uint32_t i) { return i + (i >> 4); }
// Layout B (0, 4 or 8): thread t holds in register r the key of index
// (t >> B) << (B + 4) | r << B | (t & (2^B - 1)), so the bitonic stages j = 2^B .. 2^(B+3) pair registers
// of one thread.
template <uint32_t B>
__device__ __forceinline__ uint32_t key_index(uint32_t t, uint32_t r) {
    return ((t >> B) << (B + 4u)) | (r << B) | (t & ((1u << B) - 1u));
}
template <uint32_t B>
__device__ __forceinline__ void keys_store(const uint64_t (&v)[16], uint64_t* key, uint32_t t) {
#pragma unroll
    for (uint32_t r = 0; r < 16; r++) key[kslot(key_index<B>(t, r))] = v[r];
}
template <uint32_t B>
__device__ __forceinline__ void keys_load(uint64_t (&v)[16], const uint64_t* key, uint32_t t) {
#pragma unroll
    for (uint32_t r = 0; r < 16; r++) v[r] = key[kslot(key_index<B>(t, r))];
}
// The stages of phase k (blocks of k keys, ascending where index & k == 0) that layout B holds:
// j = min(k / 2, 2^(B+3)) down to 2^B.
template <uint32_t B>
__device__ __forceinline__ void keys_stages(uint64_t (&v)[16], uint32_t t, uint32_t k) {
    const uint32_t i0 = key_index<B>(t, 0), jjmax = std::min(k >> (B + 1u), 8u);
#pragma unroll
    for (uint32_t jj = 8; jj > 0; jj >>= 1) {
        if (jj > jjmax) continue;
#pragma unroll
        for (uint32_t r = 0; r < 16; r++) {
            if (r & jj) continue;
            const bool asc = ((i0 | (r << B)) & k) == 0;
            const uint64_t x = v[r], y = v[r | jj];
            const bool sw = (x > y) == asc;
            v[r] = sw ? y : x;
            v[r | jj] = sw ? x : y;
        }
    }
}

__global__ __launch_bounds__(256) void k_terms_sort(const uint32_t* __restrict__ ids, uint64_t ids_cap,
                                                    const uint64_t* __restrict__ doc_tok,
                                                    const uint64_t* __restrict__ ntok, uint32_t ndocs,
                                                    uint64_t* __restrict__ W0, uint32_t* __restrict__ headcnt,
                                                    uint32_t* __restrict__ tailcnt, uint32_t* __restrict__ fdoc,
                                                    uint32_t* __restrict__ ldoc) {
    __shared__ uint64_t key[kKeySlots];
    __shared__ uint16_t pos[T + 2];
    __shared__ uint32_t cnt64[64], off64[64];
    __shared__ uint64_t s_j[2], dmask[64], s_nz;
    __shared__ uint32_t s_nvalid, s_nr, s_head, s_tail;
    const uint32_t th = threadIdx.x, lane = th & 63u, w = th >> 6;
    const uint64_t t = blockIdx.x, base = t * T;
    const uint64_t n = std::min(*ntok, ids_cap);
    if (base >= n) {  // (the work buffer holds whole tiles: an unused one is empty)
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) W0[base + j * 256u + th] = 0;
        if (th == 0) {
            headcnt[t] = 0;
            tailcnt[t] = 0;
            fdoc[t] = kNone;
            ldoc[t] = kNone;
        }
        return;
    }
    const uint32_t lim = (uint32_t)std::min<uint64_t>(T, n - base);
    if (th < 2) s_j[th] = doc_ub(doc_tok, th == 0 ? base : base + lim - 1u, 0, (uint64_t)ndocs + 1u);
    if (th == 0) {
        s_nvalid = 0;
        s_head = 0;
        s_tail = 0;
    }
    __syncthreads();
    const uint64_t jF = s_j[0], jL = s_j[1];
    const uint32_t dF = jF >= 1 && jF <= ndocs ? (uint32_t)(jF - 1) : kNone;
    const uint32_t dL = jL >= 1 && jL <= ndocs ? (uint32_t)(jL - 1) : kNone;
    // the keys, 16 per thread (a coalesced read; which register gets which token does not matter)
    uint64_t v[16];
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        const uint32_t i = j * 256u + th;
        uint64_t kk = ~0ull;
        if (i < lim) {
            const uint32_t id = ids[base + i];
            if (id != JB_VOCAB_UNK) {
                const uint64_t u = jF < jL ? doc_ub(doc_tok, base + i, jF, jL) : jF;
                if (u >= 1 && u <= ndocs) kk = ((u - 1) << 32) | id;
            }
        }
        v[j] = kk;
    }
    // bitonic sort, ascending (the all-ones keys end up last): the stages below 16 in registers, the
    // others after a trip through LDS into the layout that makes them register pairs.  A thread stores
    // to the slots it loaded, so one barrier per change of layout is enough.
    for (uint32_t k = 2; k <= 16; k <<= 1) keys_stages<0>(v, th, k);
    for (uint32_t k = 32; k <= T; k <<= 1) {
        keys_store<0>(v, key, th);
        __syncthreads();
        if (k >= 512) {
            keys_load<8>(v, key, th);
            keys_stages<8>(v, th, k);
            keys_store<8>(v, key, th);
            __syncthreads();
        }
        keys_load<4>(v, key, th);
        keys_stages<4>(v, th, k);
        keys_store<4>(v, key, th);
        __syncthreads();
        keys_load<0>(v, key, th);
        keys_stages<0>(v, th, k);
    }
    keys_store<0>(v, key, th);
    __syncthreads();
    // run heads: positions whose key differs from the one before
    uint32_t hm = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        const uint32_t i = j * 256u + th;
        const uint64_t kv = key[kslot(i)];
        const bool valid = kv != ~0ull;
        const bool head = valid && (i == 0 || key[kslot(i - 1)] != kv);
        hm |= (uint32_t)head << j;
        const uint64_t bh = __ballot(head), bv = __ballot(valid);
        if (lane == 0) {
            cnt64[j * 4u + w] = (uint32_t)__popcll(bh);
            if (bv) atomicAdd(&s_nvalid, (uint32_t)__popcll(bv));
        }
    }
    __syncthreads();
    if (th < 64) {
        const uint32_t v = cnt64[th], inc = wave_incl(v, th);
        off64[th] = inc - v;
        if (th == 63) s_nr = inc;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        const bool head = (hm >> j) & 1u;
        const uint64_t bh = __ballot(head);
        if (head) pos[off64[j * 4u + w] + (uint32_t)__popcll(bh & ((1ull << lane) - 1ull))] = (uint16_t)(j * 256u + th);
    }
    const uint32_t nr = s_nr;
    if (th == 0) pos[nr] = (uint16_t)s_nvalid;
    __syncthreads();
    // the runs that start a document's group, as a bit per run (64 words) and a bit per non-empty word
#pragma unroll 4
    for (uint32_t q = 0; q < 16; q++) {
        const uint32_t r = q * 256u + th;
        const bool first = r < nr && (r == 0 || (uint32_t)(key[kslot(pos[r])] >> 32) != (uint32_t)(key[kslot(pos[r - 1])] >> 32));
        const uint64_t bf = __ballot(first);
        if (lane == 0) dmask[q * 4u + w] = bf;
    }
    __syncthreads();
    if (th < 64) {
        const uint64_t nz = __ballot(dmask[th] != 0);
        if (th == 0) s_nz = nz;
    }
    __syncthreads();
    const uint64_t nzw = s_nz;
    // each run's slot in the tile and its entry, in registers: the tile is then put together in LDS, over
    // the keys, and written out whole, every slot once
    uint32_t oslot[16];
    uint64_t oval[16];
#pragma unroll
    for (uint32_t q = 0; q < 16; q++) {
        const uint32_t r = q * 256u + th;
        oslot[q] = T;
        oval[q] = 0;
        if (r >= nr) continue;
        const uint32_t i = pos[r];
        const uint64_t kv = key[kslot(i)];
        const uint32_t cnt = pos[r + 1] - i, d = (uint32_t)(kv >> 32);
        // the first run of document d: the last group start at or before r (run 0 is one)
        uint32_t w0 = r >> 6;
        uint64_t m = dmask[w0] & (~0ull >> (63u - (r & 63u)));
        if (!m) {
            w0 = 63u - (uint32_t)__clzll((long long)(nzw & ((1ull << w0) - 1ull)));
            m = dmask[w0];
        }
        const uint32_t g = w0 * 64u + 63u - (uint32_t)__clzll((long long)m);
        const uint64_t s = std::min(doc_tok[d], n);
        const uint64_t out = std::max(s, base) + (r - g);
        if (out < base + lim) {
            oslot[q] = (uint32_t)(out - base);
            oval[q] = ((uint64_t)(uint32_t)kv << 32) | cnt | (r == g ? kFlag : 0ull);
        }
        if (r == g && (d == dF || d == dL)) {
            // the first run of a later document: the next group start after r, or nr
            uint32_t w1 = r >> 6, ge = nr;
            uint64_t m1 = (r & 63u) == 63u ? 0ull : dmask[w1] & (~0ull << ((r & 63u) + 1u));
            if (!m1) {
                const uint64_t later = w1 == 63u ? 0ull : nzw & (~0ull << (w1 + 1u));
                if (later) {
                    w1 = (uint32_t)__ffsll((long long)later) - 1u;
                    m1 = dmask[w1];
                }
            }
            if (m1) ge = w1 * 64u + (uint32_t)__ffsll((long long)m1) - 1u;
            if (d == dF) s_head = ge - g;
            if (d == dL) s_tail = ge - g;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) key[kslot(j * 256u + th)] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < 16; q++)
        if (oslot[q] < T) key[kslot(oslot[q])] = oval[q];
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) W0[base + j * 256u + th] = key[kslot(j * 256u + th)];
    __syncthreads();
    if (th == 0) {
        headcnt[t] = s_head;
        tailcnt[t] = s_tail;
        fdoc[t] = dF;
        ldoc[t] = dL;
    }
}

// ---------------------------------------------------------------------------
// k_terms_merge / k_terms_copy
// ---------------------------------------------------------------------------
// The lists a group joins in pass p.  Tiles [L0, m) are its left half, m is the boundary tile; the
// document d owns the tokens m * T - 1 and m * T.  Its list left of the boundary starts at posA and has
// *locA entries: the length is kept with the tile the list starts in, as that tile's head count when d
// began before the half and as its tail count when d begins inside it.  The list right of the boundary
// starts at m * T and has headcnt[m] entries.
struct MergeJob {
    uint64_t m, posA, posB;
    uint32_t* locA;
    uint32_t lenA, lenB;
    bool go;
};

__device__ __forceinline__ MergeJob merge_job(uint32_t p, uint64_t g, uint64_t ntl, uint64_t n,
                                              const uint64_t* __restrict__ doc_tok, uint32_t* headcnt,
                                              uint32_t* tailcnt, const uint32_t* fdoc, const uint32_t* ldoc) {
    MergeJob j;
    const uint64_t L0 = g << (p + 1u);
    j.m = L0 + (1ull << p);
    j.go = false;
    j.posA = j.posB = 0;
    j.locA = nullptr;
    j.lenA = j.lenB = 0;
    if (j.m >= ntl || j.m * T >= n) return j;
    const uint32_t d = ldoc[j.m - 1];
    if (d == kNone || d != fdoc[j.m]) return j;
    const uint64_t s = std::min(doc_tok[d], n);
    if (s >= j.m * T) return j;  // (doc_tok out of order)
    j.posB = j.m * T;
    j.posA = std::max(s, L0 * T);
    j.locA = s < L0 * T ? headcnt + L0 : tailcnt + s / T;
    j.lenA = (uint32_t)std::min<uint64_t>(*j.locA, j.posB - j.posA);
    j.lenB = (uint32_t)std::min<uint64_t>(headcnt[j.m], std::min<uint64_t>((uint64_t)T << p, (ntl - j.m) * T));
    j.go = j.lenB != 0;  // (nothing right of the boundary: the left list stays as it is)
    return j;
}

__global__ __launch_bounds__(256) void k_terms_merge(uint32_t p, uint32_t chunks, uint64_t ntl, uint64_t ids_cap,
                                                     const uint64_t* __restrict__ doc_tok,
                                                     const uint64_t* __restrict__ ntok,
                                                     const uint64_t* __restrict__ W0, uint64_t* __restrict__ W1,
                                                     uint32_t* headcnt, uint32_t* tailcnt, const uint32_t* fdoc,
                                                     const uint32_t* ldoc, uint32_t* __restrict__ newlen) {
    const uint64_t g = blockIdx.x / chunks;
    const uint32_t c = blockIdx.x % chunks;
    const uint64_t n = std::min(*ntok, ids_cap);
    const MergeJob j = merge_job(p, g, ntl, n, doc_tok, headcnt, tailcnt, fdoc, ldoc);
    if (j.m >= ntl) return;
    if (!j.go) {
        if (c == 0 && threadIdx.x == 0) newlen[j.m] = 0;
        return;
    }
    const uint64_t* A = W0 + j.posA;
    const uint64_t* B = W0 + j.posB;
    const uint32_t total = j.lenA + j.lenB;
    for (uint32_t idx = c * 256u + threadIdx.x; idx < total; idx += chunks * 256u) {
        uint64_t e;
        uint32_t o;
        if (idx < j.lenA) {  // + the entries of B with a smaller id
            e = A[idx];
            const uint32_t x = ent_id(e);
            uint32_t lo = 0, hi = j.lenB;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (ent_id(B[mid]) < x) lo = mid + 1;
                else hi = mid;
            }
            o = idx + lo;
        } else {  // + the entries of A with a smaller or equal id
            const uint32_t k = idx - j.lenA;
            e = B[k];
            const uint32_t x = ent_id(e);
            uint32_t lo = 0, hi = j.lenA;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (ent_id(A[mid]) <= x) lo = mid + 1;
                else hi = mid;
            }
            o = k + lo;
        }
        W1[j.posA + o] = (e & ~kFlag) | (o == 0 ? kFlag : 0ull);
    }
    if (c == 0 && threadIdx.x == 0) newlen[j.m] = total;
}

__global__ __launch_bounds__(256) void k_terms_copy(uint32_t p, uint32_t chunks, uint64_t ntl, uint64_t ids_cap,
                                                    const uint64_t* __restrict__ doc_tok,
                                                    const uint64_t* __restrict__ ntok, uint64_t* __restrict__ W0,
                                                    const uint64_t* __restrict__ W1, uint32_t* headcnt,
                                                    uint32_t* tailcnt, const uint32_t* fdoc, const uint32_t* ldoc,
                                                    const uint32_t* __restrict__ newlen) {
    const uint64_t g = blockIdx.x / chunks;
    const uint32_t c = blockIdx.x % chunks;
    const uint64_t m = (g << (p + 1u)) + (1ull << p);
    if (m >= ntl) return;
    const uint32_t total = newlen[m];
    if (total == 0) return;
    const uint64_t n = std::min(*ntok, ids_cap);
    // (locA's old value is not used here: this kernel's other workgroups never read it)
    const MergeJob j = merge_job(p, g, ntl, n, doc_tok, headcnt, tailcnt, fdoc, ldoc);
    if (!j.go) return;
    for (uint32_t idx = c * 256u + threadIdx.x; idx < total; idx += chunks * 256u) W0[j.posA + idx] = W1[j.posA + idx];
    // what is left of the right list's old place is empty again
    const uint64_t c0 = std::max(j.posA + total, j.posB), c1 = j.posB + j.lenB;
    for (uint64_t i = c0 + c * 256u + threadIdx.x; i < c1; i += chunks * 256u) W0[i] = 0;
    if (c == 0 && threadIdx.x == 0) *j.locA = total;
}

// ---------------------------------------------------------------------------
// k_terms_count / k_terms_scan / k_terms_write
// ---------------------------------------------------------------------------
// Entry i of the list (e; 0 at or past n) starts a term: it is flagged, or its id differs from the entry
// before it.  The lanes of a wave hold consecutive entries, so only lane 0 loads its predecessor.
__device__ __forceinline__ bool term_head(const uint64_t* __restrict__ W0, uint64_t i, uint64_t n, uint64_t e,
                                          uint32_t lane) {
    uint64_t prev = ((uint64_t)(uint32_t)__shfl_up((uint32_t)(e >> 32), 1, 64) << 32) |
                    (uint32_t)__shfl_up((uint32_t)e, 1, 64);
    if (lane == 0) prev = i > 0 && i < n ? W0[i - 1] : 0;
    return (e & kCntMask) != 0 && ((e & kFlag) || (prev & kCntMask) == 0 || ent_id(e) != ent_id(prev));
}

__global__ __launch_bounds__(256) void k_terms_count(const uint64_t* __restrict__ W0, uint64_t ids_cap,
                                                     const uint64_t* __restrict__ ntok,
                                                     uint32_t* __restrict__ tilecnt) {
    __shared__ uint32_t sh[5];
    const uint64_t n = std::min(*ntok, ids_cap), t0 = (uint64_t)blockIdx.x * T;
    uint32_t c = 0;
    if (t0 < n) {
#pragma unroll 4
        for (uint32_t j = 0; j < 16; j++) {
            const uint64_t i = t0 + j * 256u + threadIdx.x;
            const uint64_t e = i < n ? W0[i] : 0;
            c += term_head(W0, i, n, e, threadIdx.x & 63u);
        }
    }
    uint32_t total;
    (void)block_excl<4>(c, sh, &total);
    if (threadIdx.x == 0) tilecnt[blockIdx.x] = total;
}

// One workgroup: base[t] = terms before tile t (ntl + 1 entries), *nterms = all of them.
__global__ __launch_bounds__(1024) void k_terms_scan(const uint32_t* __restrict__ tilecnt, uint64_t ntl,
                                                     uint64_t* __restrict__ base, uint64_t* __restrict__ nterms) {
    __shared__ uint32_t sh[17];
    uint64_t carry = 0;
    for (uint64_t c0 = 0; c0 < ntl; c0 += 1024u) {
        const uint64_t i = c0 + threadIdx.x;
        const uint32_t v = i < ntl ? tilecnt[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl<16>(v, sh, &total);
        if (i < ntl) base[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        base[ntl] = carry;
        *nterms = carry;
    }
}

__global__ __launch_bounds__(256) void k_terms_write(const uint64_t* __restrict__ W0, uint64_t ids_cap,
                                                     const uint64_t* __restrict__ doc_tok,
                                                     const uint64_t* __restrict__ ntok, uint32_t ndocs,
                                                     const uint64_t* __restrict__ base, uint32_t* __restrict__ term_id,
                                                     uint32_t* __restrict__ term_cnt, uint64_t cap,
                                                     uint64_t* __restrict__ term_off) {
    // per 64 consecutive entries (trip j, wave w: index j * 4 + w): their heads as a mask, and the heads before them
    __shared__ uint64_t bal[64];
    __shared__ uint32_t off64[65];
    __shared__ uint64_t s_d[2];
    const uint32_t th = threadIdx.x, lane = th & 63u, w = th >> 6;
    const uint64_t t = blockIdx.x, t0 = t * T;
    const uint64_t n = std::min(*ntok, ids_cap);
    if (t > 0 && t0 >= n) return;
    uint32_t hm = 0;
#pragma unroll 4
    for (uint32_t j = 0; j < 16; j++) {
        const uint64_t i = t0 + j * 256u + th;
        const uint64_t e = i < n ? W0[i] : 0;
        const bool head = term_head(W0, i, n, e, lane);
        hm |= (uint32_t)head << j;
        const uint64_t b = __ballot(head);
        if (lane == 0) bal[j * 4u + w] = b;
    }
    if (th == 0) {
        // the documents whose first token position lies in (t0, t0 + T] (tile 0: [0, T])
        s_d[0] = t == 0 ? 0 : doc_ub(doc_tok, t0, 0, (uint64_t)ndocs + 1u);
        s_d[1] = n <= t0 + T ? (uint64_t)ndocs + 1u : doc_ub(doc_tok, t0 + T, 0, (uint64_t)ndocs + 1u);
    }
    __syncthreads();
    if (th < 64) {
        const uint32_t c = (uint32_t)__popcll(bal[th]), inc = wave_incl(c, th);
        off64[th] = inc - c;
        if (th == 63) off64[64] = inc;
    }
    __syncthreads();
    const uint64_t b0 = base[t];
    for (uint64_t d = s_d[0] + th; d < s_d[1]; d += 256u) {
        const uint64_t s = std::min(doc_tok[d], n);
        if (s < t0 || s > t0 + T) continue;  // (doc_tok out of order)
        const uint32_t p = (uint32_t)(s - t0);
        term_off[d] = b0 + (p == T ? off64[64] : off64[p >> 6] + (uint32_t)__popcll(bal[p >> 6] & ((1ull << (p & 63u)) - 1ull)));
    }
    for (uint32_t j = 0; j < 16; j++) {
        if (!((hm >> j) & 1u)) continue;
        const uint64_t idx = b0 + off64[j * 4u + w] + (uint32_t)__popcll(bal[j * 4u + w] & ((1ull << lane) - 1ull));
        if (idx >= cap) continue;
        const uint64_t i = t0 + j * 256u + th, e0 = W0[i];
        const uint32_t id = ent_id(e0);
        uint32_t c = ent_cnt(e0);
        // the entries of the same id that follow (one per tile the document spans, at most)
        for (uint64_t k = i + 1u; k < n; k++) {
            const uint64_t e = W0[k];
            if ((e & kCntMask) == 0 || (e & kFlag) || ent_id(e) != id) break;
            c += ent_cnt(e);
        }
        term_id[idx] = id;
        term_cnt[idx] = c;
    }
}

// ---------------------------------------------------------------------------
// k_keywords
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
    const uint32_t lo = __shfl((uint32_t)v, (int)src, 64), hi = __shfl((uint32_t)(v >> 32), (int)src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// compare-exchange with the lane `j` away: the lower lane of a pair keeps the larger key when `desc`
__device__ __forceinline__ uint64_t cmpx(uint64_t v, uint32_t lane, uint32_t j, bool desc) {
    const uint64_t o = shfl64(v, lane ^ j);
    const bool keepmax = ((lane & j) == 0) == desc;
    return keepmax ? std::max(v, o) : std::min(v, o);
}

__global__ __launch_bounds__(256) void k_keywords(const uint32_t* __restrict__ term_id,
                                                  const uint32_t* __restrict__ term_cnt,
                                                  const uint64_t* __restrict__ term_off, uint32_t ndocs, uint64_t cap,
                                                  const float* __restrict__ weight, uint32_t nweights, uint32_t topk,
                                                  uint32_t* __restrict__ kw_id, float* __restrict__ kw_score,
                                                  uint32_t* __restrict__ kw_cnt, uint32_t* __restrict__ kw_n) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t d = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (d >= ndocs) return;
    uint64_t a = term_off[d], b = term_off[d + 1];
    if (b > cap || a > b) a = b = 0;  // a CSR that overflowed its arrays is not read past them
    uint64_t top = 0;                 // lane l: the l-th best key so far, 0 = none
    for (uint64_t i0 = a; i0 < b; i0 += 64u) {
        const uint64_t i = i0 + lane;
        uint64_t k = 0;
        if (i < b) {
            const uint32_t id = term_id[i];
            if (id < nweights) {
                const float w = weight[id];
                if (w > 0.0f) k = ((uint64_t)__float_as_uint((float)term_cnt[i] * w) << 32) | (uint32_t)~id;
            }
        }
        const uint64_t thr = shfl64(top, topk - 1u);
        if (__ballot(k > thr) == 0) continue;
        // the batch, sorted descending
        for (uint32_t kk = 2; kk <= 64; kk <<= 1)
            for (uint32_t j = kk >> 1; j > 0; j >>= 1) k = cmpx(k, lane, j, (lane & kk) == 0 || kk == 64);
        // max(top[l], batch[63 - l]) holds the 64 best of both and is bitonic: one merge sorts it
        top = std::max(top, shfl64(k, 63u - lane));
        for (uint32_t j = 32; j > 0; j >>= 1) top = cmpx(top, lane, j, true);
    }
    const bool have = lane < topk && top != 0;
    const uint32_t id = ~(uint32_t)top;
    uint32_t cnt = 0;
    if (have) {  // the term's count: its id is in the document's ascending id list
        uint64_t lo = a, hi = b;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (term_id[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        cnt = term_cnt[lo];
    }
    const uint64_t nk = __ballot(have);
    if (lane < topk) {
        const uint64_t o = d * topk + lane;
        kw_id[o] = have ? id : JB_VOCAB_UNK;
        kw_score[o] = have ? __uint_as_float((uint32_t)(top >> 32)) : 0.0f;
        kw_cnt[o] = cnt;
    }
    if (lane == 0) kw_n[d] = (uint32_t)__popcll(nk);
}

// ---------------------------------------------------------------------------
// k_df / k_df_combine
// ---------------------------------------------------------------------------
// The list as both kernels read it: `head` leading entries up to the first 16-byte boundary, `nv` whole
// uint4 after them, and up to 3 entries after those.  The list is never read at or past n.
struct DfSpan {
    uint64_t n, nv, tail0;
    uint32_t head;
    const uint4* vec;
};

__device__ __forceinline__ DfSpan df_span(const uint32_t* __restrict__ term_id, const uint64_t* __restrict__ nterms,
                                          uint64_t cap) {
    DfSpan s;
    s.n = std::min(*nterms, cap);
    s.head = (uint32_t)std::min<uint64_t>(s.n, ((16u - ((uintptr_t)term_id & 15u)) & 15u) >> 2);
    s.nv = (s.n - s.head) >> 2;
    s.tail0 = s.head + 4u * s.nv;
    s.vec = (const uint4*)(term_id + s.head);
    return s;
}

// The entry that thread th of workgroup 0 owns outside the vectors (the head, then the tail), or kNone.
__device__ __forceinline__ uint32_t df_edge(const uint32_t* __restrict__ term_id, const DfSpan& s, uint32_t th) {
    if (th < s.head) return term_id[th];
    if (th >= 4u && th < 8u && s.tail0 + (th - 4u) < s.n) return term_id[s.tail0 + (th - 4u)];
    return kNone;
}

// The plain form: one relaxed device-scope add per entry (an id of kNone is never < ndf).
__global__ __launch_bounds__(256) void k_df(const uint32_t* __restrict__ term_id, const uint64_t* __restrict__ nterms,
                                            uint64_t cap, uint32_t* __restrict__ df, uint32_t ndf) {
    const DfSpan s = df_span(term_id, nterms, cap);
    const uint32_t th = threadIdx.x;
    if (blockIdx.x == 0 && th < 8u) {
        const uint32_t id = df_edge(term_id, s, th);
        if (id < ndf) atomicAdd(&df[id], 1u);
    }
    const uint64_t stride = (uint64_t)gridDim.x * 1024u;
    for (uint64_t v0 = (uint64_t)blockIdx.x * 1024u; v0 < s.nv; v0 += stride) {
        uint4 x[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint64_t v = v0 + j * 256u + th;
            x[j] = v < s.nv ? s.vec[v] : make_uint4(kNone, kNone, kNone, kNone);
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            if (x[j].x < ndf) atomicAdd(&df[x[j].x], 1u);
            if (x[j].y < ndf) atomicAdd(&df[x[j].y], 1u);
            if (x[j].z < ndf) atomicAdd(&df[x[j].z], 1u);
            if (x[j].w < ndf) atomicAdd(&df[x[j].w], 1u);
        }
    }
}

// The combining form.  Workgroup b owns the vectors [b * share, (b + 1) * share), share = the vectors
// divided evenly over the grid, in whole trips of 1024 and at least kDfMinShare.  A slot's tag is kNone
// until an id claims it (no id < ndf is kNone); the id that finds another id's tag there goes to the
// global counter itself.
constexpr uint32_t kDfSlots = 4096;      // 32 KiB of LDS: five workgroups per CU
constexpr uint32_t kDfMinShare = 1024;   // vectors: 4096 entries

__device__ __forceinline__ void df_add(uint32_t id, uint32_t ndf, uint32_t* tag, uint32_t* cnt,
                                       uint32_t* __restrict__ df) {
    if (id >= ndf) return;
    const uint32_t slot = id & (kDfSlots - 1u);
    uint32_t t = __hip_atomic_load(&tag[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (t == kNone) {
        t = atomicCAS(&tag[slot], kNone, id);
        if (t == kNone) t = id;
    }
    if (t == id) atomicAdd(&cnt[slot], 1u);
    else atomicAdd(&df[id], 1u);
}

__global__ __launch_bounds__(256) void k_df_combine(const uint32_t* __restrict__ term_id,
                                                    const uint64_t* __restrict__ nterms, uint64_t cap,
                                                    uint32_t* __restrict__ df, uint32_t ndf) {
    __shared__ uint32_t tag[kDfSlots], cnt[kDfSlots];
    const DfSpan s = df_span(term_id, nterms, cap);
    const uint32_t th = threadIdx.x;
    uint64_t share = (s.nv + gridDim.x - 1u) / gridDim.x;
    share = std::max<uint64_t>((share + 1023u) & ~(uint64_t)1023u, kDfMinShare);
    const uint64_t b0 = (uint64_t)blockIdx.x * share;
    if (b0 >= s.nv && blockIdx.x != 0) return;  // (workgroup 0 also owns the head and the tail)
    const uint64_t b1 = std::min(b0 + share, s.nv);
    for (uint32_t i = th; i < kDfSlots; i += 256u) {
        tag[i] = kNone;
        cnt[i] = 0;
    }
    __syncthreads();
    if (blockIdx.x == 0 && th < 8u) df_add(df_edge(term_id, s, th), ndf, tag, cnt, df);
    for (uint64_t v0 = b0; v0 < b1; v0 += 1024u) {
        uint4 x[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint64_t v = v0 + j * 256u + th;
            x[j] = v < b1 ? s.vec[v] : make_uint4(kNone, kNone, kNone, kNone);
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            df_add(x[j].x, ndf, tag, cnt, df);
            df_add(x[j].y, ndf, tag, cnt, df);
            df_add(x[j].z, ndf, tag, cnt, df);
            df_add(x[j].w, ndf, tag, cnt, df);
        }
    }
    __syncthreads();
    for (uint32_t i = th; i < kDfSlots; i += 256u) {
        const uint32_t c = cnt[i];
        if (c) atomicAdd(&df[tag[i]], c);  // (a counted slot has a tag < ndf)
    }
}

// ---------------------------------------------------------------------------
// k_idf
// ---------------------------------------------------------------------------
// go_log (jb_image.cpp) for a positive normal x: the same operations in the same order, frexp by the bits.
__device__ __forceinline__ double dev_go_log(double x) {
    const double Ln2Hi = 6.93147180369123816490e-01, Ln2Lo = 1.90821492927058770002e-10,
                 L1 = 6.666666666666735130e-01, L2 = 3.999999999940941908e-01, L3 = 2.857142874366239149e-01,
                 L4 = 2.222219843214978396e-01, L5 = 1.818357216161805012e-01, L6 = 1.531383769920937332e-01,
                 L7 = 1.479819860511658591e-01;
    const uint64_t bits = (uint64_t)__double_as_longlong(x);
    int ki = (int)((bits >> 52) & 0x7FFu) - 1022;
    double f1 = __longlong_as_double((long long)((bits & ~(0x7FFull << 52)) | (1022ull << 52)));  // [0.5, 1)
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

__global__ __launch_bounds__(256) void k_idf(const uint32_t* __restrict__ df, uint32_t ndf, uint64_t ndocs_total,
                                             uint32_t min_df, uint32_t max_df, const uint8_t* __restrict__ keep,
                                             float* __restrict__ weight) {
    const uint64_t id = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (id >= ndf) return;
    const uint32_t f = df[id];
    float w = 0.0f;
    if (f != 0 && f >= min_df && f <= max_df && (keep == nullptr || keep[id] != 0))
        w = (float)(dev_go_log((double)(ndocs_total + 1u) / (double)((uint64_t)f + 1u)) + 1.0);
    weight[id] = w;
}

struct TermsWork {
    uint64_t ntl;
    uint64_t *W0, *W1, *base;
    uint32_t *headcnt, *tailcnt, *fdoc, *ldoc, *newlen, *tilecnt;
    size_t bytes;
};

TermsWork terms_layout(uint64_t max_tokens, void* p) {
    TermsWork w;
    w.ntl = std::max<uint64_t>(1u, (max_tokens + T - 1u) / T);
    uint8_t* b = (uint8_t*)p;
    size_t off = 0;
    auto take = [&](size_t nb) -> uint8_t* {
        const size_t o = off;
        off += (nb + 255u) & ~(size_t)255u;
        return b ? b + o : nullptr;
    };
    w.W0 = (uint64_t*)take(w.ntl * T * 8u);
    w.W1 = (uint64_t*)take(w.ntl * T * 8u);
    w.base = (uint64_t*)take((w.ntl + 1u) * 8u);
    uint32_t** u[6] = {&w.headcnt, &w.tailcnt, &w.fdoc, &w.ldoc, &w.newlen, &w.tilecnt};
    for (auto pp : u) *pp = (uint32_t*)take(w.ntl * 4u);
    w.bytes = off;
    return w;
}

}  // namespace

size_t terms_work_bytes(uint64_t max_tokens, uint32_t /*ndocs*/) { return terms_layout(max_tokens, nullptr).bytes; }

hipError_t run_terms(const uint32_t* d_ids, uint64_t ids_cap, const uint64_t* d_doc_tok, const uint64_t* d_ntok,
                     uint32_t ndocs, uint32_t* d_term_id, uint32_t* d_term_cnt, uint64_t cap, uint64_t* d_term_off,
                     uint64_t* d_nterms, void* d_work, hipStream_t stream, KernelTimer* timer) {
    const TermsWork w = terms_layout(ids_cap, d_work);
    const uint32_t ntl = (uint32_t)w.ntl;
    JB_TIMED(K_TERMS_SORT, hipLaunchKernelGGL(k_terms_sort, dim3(ntl), dim3(256), 0, stream, d_ids, ids_cap, d_doc_tok,
                                              d_ntok, ndocs, w.W0, w.headcnt, w.tailcnt, w.fdoc, w.ldoc));
    for (uint32_t p = 0; (1ull << p) < w.ntl; p++) {
        const uint64_t groups = (w.ntl + (2ull << p) - 1u) >> (p + 1u);
        const uint32_t chunks = (uint32_t)std::min<uint64_t>(2ull << p, 128u);
        const uint32_t grid = (uint32_t)(groups * chunks);
        JB_TIMED(K_TERMS_MERGE,
                 hipLaunchKernelGGL(k_terms_merge, dim3(grid), dim3(256), 0, stream, p, chunks, w.ntl, ids_cap, d_doc_tok,
                                    d_ntok, w.W0, w.W1, w.headcnt, w.tailcnt, w.fdoc, w.ldoc, w.newlen);
                 hipLaunchKernelGGL(k_terms_copy, dim3(grid), dim3(256), 0, stream, p, chunks, w.ntl, ids_cap, d_doc_tok,
                                    d_ntok, w.W0, w.W1, w.headcnt, w.tailcnt, w.fdoc, w.ldoc, w.newlen));
    }
    JB_TIMED(K_TERMS_COUNT,
             hipLaunchKernelGGL(k_terms_count, dim3(ntl), dim3(256), 0, stream, w.W0, ids_cap, d_ntok, w.tilecnt));
    JB_TIMED(K_TERMS_SCAN,
             hipLaunchKernelGGL(k_terms_scan, dim3(1), dim3(1024), 0, stream, w.tilecnt, w.ntl, w.base, d_nterms));
    JB_TIMED(K_TERMS_WRITE, hipLaunchKernelGGL(k_terms_write, dim3(ntl), dim3(256), 0, stream, w.W0, ids_cap, d_doc_tok,
                                               d_ntok, ndocs, w.base, d_term_id, d_term_cnt, cap, d_term_off));
    return hipGetLastError();
}

hipError_t run_keywords(const uint32_t* d_term_id, const uint32_t* d_term_cnt, const uint64_t* d_term_off,
                        uint32_t ndocs, uint64_t cap, const float* d_weight, uint32_t nweights, uint32_t topk,
                        uint32_t* d_kw_id, float* d_kw_score, uint32_t* d_kw_cnt, uint32_t* d_kw_n,
                        hipStream_t stream, KernelTimer* timer) {
    const uint32_t grid = (uint32_t)(((uint64_t)ndocs + 3u) / 4u);
    JB_TIMED(K_KEYWORDS, hipLaunchKernelGGL(k_keywords, dim3(grid), dim3(256), 0, stream, d_term_id, d_term_cnt,
                                            d_term_off, ndocs, cap, d_weight, nweights, topk, d_kw_id, d_kw_score,
                                            d_kw_cnt, d_kw_n));
    return hipGetLastError();
}

hipError_t run_df(const uint32_t* d_term_id, const uint64_t* d_nterms, uint64_t cap, uint32_t* d_df, uint32_t ndf,
                  bool combine, uint32_t ncu, hipStream_t stream, KernelTimer* timer) {
    // the grid follows cap (a host value), up to a few workgroups per CU; the kernels loop or share
    const uint64_t trips = std::max<uint64_t>(1u, (cap / 4u + 1023u) / 1024u);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(trips, (uint64_t)std::max(ncu, 1u) * (combine ? 5u : 8u));
    if (combine)
        JB_TIMED(K_DF, hipLaunchKernelGGL(k_df_combine, dim3(grid), dim3(256), 0, stream, d_term_id, d_nterms, cap, d_df,
                                          ndf));
    else
        JB_TIMED(K_DF, hipLaunchKernelGGL(k_df, dim3(grid), dim3(256), 0, stream, d_term_id, d_nterms, cap, d_df, ndf));
    return hipGetLastError();
}

hipError_t run_idf(const uint32_t* d_df, uint32_t ndf, uint64_t ndocs_total, uint32_t min_df, uint32_t max_df,
                   const uint8_t* d_keep, float* d_weight, hipStream_t stream, KernelTimer* timer) {
    const uint32_t grid = (uint32_t)(((uint64_t)ndf + 255u) / 256u);
    JB_TIMED(K_IDF, hipLaunchKernelGGL(k_idf, dim3(grid), dim3(256), 0, stream, d_df, ndf, ndocs_total, min_df, max_df,
                                       d_keep, d_weight));
    return hipGetLastError();
}

}  // namespace jb
