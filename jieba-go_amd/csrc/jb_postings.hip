// jb_postings.hip — gfx950 kernels of the postings call (jb_postings_device; the rule is jb_postings',
// jb_postings.cpp; the code shared with the host is jb_postings.h's).
//
// The document-term CSR of jb_terms_device (rows = documents) becomes the index (rows = ids): a stable LSD
// radix sort of the entries by id, 8 bits per pass, with the payload (document, tf).  With n = min(*nterms, cap,
// term_off[ndocs]), the N = ceil(n / kPostTile) * kPostTile slots of the tiles that hold an entry are sorted:
// slot i carries the key jb_postings_key (its id when it takes part, nids otherwise, also for the padding of
// the last such tile), so the index is the sorted list up to the first key nids and every position a pass
// computes is below N <= ntl * kPostTile.  The grid covers the ntl tiles of cap, whatever n is; the workgroup of
// a tile past n writes zero counters and nothing else, so the cost follows n, not cap.  P = jb_postings_passes(nids) passes of three launches, then one more:
//   k_post_hist     per tile, the 256 digit counts -> cnt[digit * ntl + tile] (every counter is written).  A
//                   wave matches its 64 digits by 8 ballots and the lowest lane of each group adds the group's
//                   size to a counter in LDS: a tile of one digit value does 64 adds, not 4096.
//   k_post_scan     workgroup d scans cnt[d * ntl ..] over the tiles in place (exclusive) and writes tot[d].
//   k_post_scatter  per tile: rank every entry among the tile's entries of its digit, then write key and
//                   payload at  (sum of tot[< digit]) + cnt[digit][tile] + rank.  The 256 totals are scanned
//                   again in every workgroup.  Pass 0 builds keys and payloads from the CSR (the row of an
//                   entry by a search in term_off between the rows of the tile's first and last entry, doc_ub
//                   of jb_terms.hip); the last pass writes post_doc / post_tf (positions below pcap, keys
//                   below nids) instead of the payload array.
//   k_post_off      one lane per t in 0 .. nids: post_off[t] = the first sorted position whose key is >= t, by
//                   binary search; the lane of t = nids also writes *nposts.
// Why the rank is stable.  Wave w of the workgroup owns the tile's slots [w * 1024, (w + 1) * 1024) and takes
// them in 16 rounds of 64, lane l of round r holding slot w * 1024 + r * 64 + l: slot order is (w, r, l).  In a
// round the lanes of equal digit are found by the ballot match; a lane's rank inside the round is the number
// of lower lanes of its group, and the group's lowest lane reads the wave's counter of the digit and adds the
// group's size, so rounds are counted in order r and lanes in order l.  Only the wave itself touches its 256
// counters (s_c[w]), and a wave's LDS accesses complete in program order, so no atomic is needed.  After a
// barrier thread d turns the four waves' counts of digit d into exclusive prefixes in order w.  Rank =
// prefix(w) + count of earlier rounds + lower lanes = the number of slots of the same digit before this one
// in the tile.  Counters are u32 and count at most kPostTile.
// Form 0 writes every slot from its lane to its global position.  Form 1 first moves keys and payloads to
// their rank-sorted place in LDS (position = the tile's exclusive digit prefix + rank) and then writes LDS
// slot q to global position gbase[digit] + q - lstart[digit]: consecutive lanes write consecutive addresses
// inside a digit's run.  Both compute the same positions, so their outputs are the same bytes.
// Measured on the 1 GiB corpus (profiles/postings_bench.json; 77.3M entries, nids = 350,000, 3 passes): form 0
// 3.26 ms (k_post_scatter 2.49 ms over the three passes), form 1 3.37 ms (2.59 ms); form 0 is the default.
// No lane waits for another workgroup and there are no global atomics; every value is an integer, so the
// outputs are the same from run to run.  Reads of the CSR are at indices below min(*nterms, cap, term_off[
// ndocs]) <= cap and of term_off at indices <= ndocs; writes to the work arrays are at positions checked
// against N, to post_doc / post_tf below pcap, to post_off at t <= nids.
#include <hip/hip_runtime.h>

#include "jb_kstages.h"
#include "jb_postings.h"

#include <algorithm>

namespace jb {

namespace {

constexpr uint32_t T = kPostTile;
constexpr uint32_t WSLOTS = T / 4u;    // slots per wave
constexpr uint32_t RPW = WSLOTS / 64u;  // rounds per wave
static_assert(kPostTile == JB_POSTINGS_TILE, "the header's constant");
static_assert(RPW * 256u == T, "four waves, RPW rounds of 64 slots each");

// The lanes of the wave whose digit equals this lane's (all 64 lanes take part).
__device__ __forceinline__ uint64_t match8(uint32_t dg) {
    uint64_t m = ~0ull;
#pragma unroll
    for (uint32_t b = 0; b < 8u; b++) {
        const bool bit = (dg >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

__device__ __forceinline__ uint32_t popc64(uint64_t v) { return (uint32_t)__popcll((unsigned long long)v); }

// Inclusive scan over the 64 lanes of a wave.
__device__ __forceinline__ uint32_t wave_incl(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// The exclusive scan of one u32 per thread over the NW waves of the workgroup; *total is the sum.
template <uint32_t NW>
__device__ __forceinline__ uint32_t block_excl32(uint32_t v, uint32_t* sh /* NW */, uint32_t* total) {
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

// n of the rule: the entries that take part in the count.
__device__ __forceinline__ uint64_t post_n(const uint64_t* __restrict__ nterms, uint64_t cap,
                                           const uint64_t* __restrict__ term_off, uint32_t ndocs) {
    return std::min(std::min(*nterms, cap), term_off[ndocs]);
}

// The key of slot i: pass 0 from the CSR, later passes from the keys the pass before wrote.
__device__ __forceinline__ uint32_t slot_key(bool first, const uint32_t* __restrict__ src, uint64_t i, uint64_t n,
                                             uint32_t nids) {
    if (!first) return src[i];
    return i < n ? jb_postings_key(src[i], i, n, nids) : nids;
}

__global__ __launch_bounds__(256) void k_post_hist(const uint32_t* __restrict__ src, uint32_t first,
                                                   const uint64_t* __restrict__ nterms, uint64_t cap,
                                                   const uint64_t* __restrict__ term_off, uint32_t ndocs,
                                                   uint32_t nids, uint32_t shift, uint32_t ntl,
                                                   uint32_t* __restrict__ cnt) {
    __shared__ uint32_t s_h[256];
    const uint32_t th = threadIdx.x, lane = th & 63u, w = th >> 6;
    const uint64_t n = post_n(nterms, cap, term_off, ndocs);
    if ((uint64_t)blockIdx.x * T >= n) {  // a tile past the list: it is not sorted
        cnt[(uint64_t)th * ntl + blockIdx.x] = 0;
        return;
    }
    s_h[th] = 0;
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * T + w * WSLOTS + lane;
    // (the ballots stand outside every divergent branch: all 64 lanes take part)
#pragma unroll 4
    for (uint32_t r = 0; r < RPW; r++) {
        const uint32_t dg = (slot_key(first != 0, src, t0 + r * 64u, n, nids) >> shift) & 255u;
        const uint64_t m = match8(dg);
        if (lane == (uint32_t)__ffsll((unsigned long long)m) - 1u) atomicAdd(&s_h[dg], popc64(m));
    }
    __syncthreads();
    cnt[(uint64_t)th * ntl + blockIdx.x] = s_h[th];
}

__global__ __launch_bounds__(1024) void k_post_scan(uint32_t* __restrict__ cnt, uint32_t ntl,
                                                    uint32_t* __restrict__ tot) {
    __shared__ uint32_t sh[16];
    uint32_t* c = cnt + (uint64_t)blockIdx.x * ntl;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < ntl; c0 += 1024u) {
        const uint32_t i = c0 + threadIdx.x;
        const uint32_t v = i < ntl ? c[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl32<16>(v, sh, &total);
        if (i < ntl) c[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

template <uint32_t FORM>
__global__ __launch_bounds__(256, FORM == 0 ? 4 : 2) void k_post_scatter(
    const uint32_t* __restrict__ src, const uint64_t* __restrict__ pay_in, const uint32_t* __restrict__ term_cnt,
    uint32_t first, uint32_t last, const uint64_t* __restrict__ nterms, uint64_t cap,
    const uint64_t* __restrict__ term_off, uint32_t ndocs, uint32_t nids, uint32_t doc_base, uint32_t shift,
    uint32_t ntl, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ tot, uint32_t* __restrict__ key_out,
    uint64_t* __restrict__ pay_out, uint32_t* __restrict__ post_doc, uint32_t* __restrict__ post_tf, uint64_t pcap) {
    __shared__ uint32_t s_c[4][256];  // per wave: the digit's count so far, then the wave's base for the digit
    __shared__ uint32_t s_g[256];     // form 1: the digit's global base minus its start in the tile
    __shared__ uint32_t s_sc[4];
    __shared__ uint64_t s_j[2];
    const uint32_t th = threadIdx.x, lane = th & 63u, w = th >> 6;
    const uint64_t nslots = (uint64_t)ntl * T, tb = (uint64_t)blockIdx.x * T;
    const uint64_t n = post_n(nterms, cap, term_off, ndocs);
    if (tb >= n) return;  // a tile past the list: it is not sorted
    if (first && th < 2u)  // the rows of the tile's first and last entry
        s_j[th] = jb_postings_row_ub(term_off, th == 0 ? tb : std::min(tb + T, n) - 1u, 0, (uint64_t)ndocs + 1u);
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) s_c[k][th] = 0;
    __syncthreads();
    uint32_t key[RPW], rank[RPW];
    uint64_t pay[RPW];
    const uint64_t t0 = tb + w * WSLOTS + lane;
    if (first) {
        const uint64_t jF = s_j[0], jL = s_j[1];
#pragma unroll
        for (uint32_t r = 0; r < RPW; r++) {
            const uint64_t i = t0 + r * 64u;
            key[r] = nids;
            pay[r] = 0;
            if (i < n) {
                key[r] = jb_postings_key(src[i], i, n, nids);
                if (key[r] != nids) {
                    const uint64_t u = jF < jL ? jb_postings_row_ub(term_off, i, jF, jL) : jF;
                    pay[r] = ((uint64_t)(doc_base + (uint32_t)(u - 1u)) << 32) | term_cnt[i];
                }
            }
        }
    } else {
#pragma unroll
        for (uint32_t r = 0; r < RPW; r++) {
            key[r] = src[t0 + r * 64u];
            pay[r] = pay_in[t0 + r * 64u];
        }
    }
    // the ranks inside the wave, round by round (the header comment: why this is the slot order)
    volatile uint32_t* cw = s_c[w];
#pragma unroll
    for (uint32_t r = 0; r < RPW; r++) {
        const uint32_t dg = (key[r] >> shift) & 255u;
        const uint64_t m = match8(dg);
        const uint32_t lead = (uint32_t)__ffsll((unsigned long long)m) - 1u;
        uint32_t old = 0;
        if (lane == lead) {
            old = cw[dg];
            cw[dg] = old + popc64(m);
        }
        rank[r] = (uint32_t)__shfl((int)old, (int)lead, 64) + popc64(m & ((1ull << lane) - 1ull));
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // thread d: the digit's global base, and the waves' counts as exclusive prefixes in wave order
    uint32_t total;
    const uint32_t c0 = s_c[0][th], c1 = s_c[1][th], c2 = s_c[2][th], c3 = s_c[3][th];
    const uint32_t g = block_excl32<4>(tot[th], s_sc, &total) + cnt[(uint64_t)th * ntl + blockIdx.x];
    uint32_t b = g;
    if constexpr (FORM == 1) {
        b = block_excl32<4>(c0 + c1 + c2 + c3, s_sc, &total);  // the digit's start in the tile
        s_g[th] = g - b;
    }
    s_c[0][th] = b;
    s_c[1][th] = b + c0;
    s_c[2][th] = b + c0 + c1;
    s_c[3][th] = b + c0 + c1 + c2;
    __syncthreads();
    auto put = [&](uint64_t pos, uint32_t k, uint64_t p) {
        if (pos >= nslots) return;  // (never, while the CSR is the one k_post_hist counted)
        key_out[pos] = k;
        if (!last) {
            pay_out[pos] = p;
        } else if (k != nids && pos < pcap) {
            post_doc[pos] = (uint32_t)(p >> 32);
            post_tf[pos] = (uint32_t)p;
        }
    };
    if constexpr (FORM == 0) {
#pragma unroll
        for (uint32_t r = 0; r < RPW; r++) put((uint64_t)s_c[w][(key[r] >> shift) & 255u] + rank[r], key[r], pay[r]);
    } else {
        __shared__ uint32_t s_key[T];
        __shared__ uint64_t s_pay[T];
#pragma unroll
        for (uint32_t r = 0; r < RPW; r++) {
            const uint32_t lp = (s_c[w][(key[r] >> shift) & 255u] + rank[r]) & (T - 1u);
            s_key[lp] = key[r];
            s_pay[lp] = pay[r];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < RPW; j++) {
            const uint32_t q = j * 256u + th, k = s_key[q];
            put((uint64_t)(uint32_t)(s_g[(k >> shift) & 255u] + q), k, s_pay[q]);
        }
    }
}

__global__ __launch_bounds__(256) void k_post_off(const uint32_t* __restrict__ keys,
                                                  const uint64_t* __restrict__ nterms, uint64_t cap,
                                                  const uint64_t* __restrict__ term_off, uint32_t ndocs, uint32_t nids,
                                                  uint64_t* __restrict__ post_off, uint64_t* __restrict__ nposts) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t > nids) return;
    const uint64_t nslots = (post_n(nterms, cap, term_off, ndocs) + T - 1u) / T * T;  // the sorted slots
    uint64_t lo = 0, hi = nslots;  // the first position whose key is >= t
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] >= t) hi = mid;
        else lo = mid + 1;
    }
    post_off[t] = lo;
    if (t == nids) *nposts = lo;
}

}  // namespace

hipError_t run_postings(const uint32_t* d_term_id, const uint32_t* d_term_cnt, const uint64_t* d_term_off,
                        const uint64_t* d_nterms, uint64_t cap, uint32_t ndocs, uint32_t nids, uint32_t doc_base,
                        uint32_t form, uint32_t* d_post_doc, uint32_t* d_post_tf, uint64_t pcap, uint64_t* d_post_off,
                        uint64_t* d_nposts, void* d_work, hipStream_t stream, KernelTimer* timer) {
    if (cap == 0 || nids == 0) {  // no entry takes part: the zero outputs, no launch
        hipError_t e = hipMemsetAsync(d_post_off, 0, ((size_t)nids + 1u) * 8u, stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_nposts, 0, 8, stream);
        return e;
    }
    const PostingsWork w = postings_layout(cap);
    uint8_t* b = (uint8_t*)d_work;
    uint32_t* key[2] = {(uint32_t*)(b + w.key[0]), (uint32_t*)(b + w.key[1])};
    uint64_t* pay[2] = {(uint64_t*)(b + w.pay[0]), (uint64_t*)(b + w.pay[1])};
    uint32_t* cnt = (uint32_t*)(b + w.cnt);
    uint32_t* tot = (uint32_t*)(b + w.tot);
    const uint32_t ntl = (uint32_t)w.ntl, P = jb_postings_passes(nids);
    for (uint32_t p = 0; p < P; p++) {
        const uint32_t first = p == 0, last = p + 1u == P, shift = 8u * p;
        const uint32_t* src = first ? d_term_id : key[(p - 1u) & 1u];
        const uint64_t* pin = first ? nullptr : pay[(p - 1u) & 1u];
        JB_TIMED(K_POST_HIST, hipLaunchKernelGGL(k_post_hist, dim3(ntl), dim3(256), 0, stream, src, first, d_nterms, cap,
                                                 d_term_off, ndocs, nids, shift, ntl, cnt));
        JB_TIMED(K_POST_SCAN, hipLaunchKernelGGL(k_post_scan, dim3(256), dim3(1024), 0, stream, cnt, ntl, tot));
        if (form)
            JB_TIMED(K_POST_SCATTER,
                     hipLaunchKernelGGL(k_post_scatter<1>, dim3(ntl), dim3(256), 0, stream, src, pin, d_term_cnt, first,
                                        last, d_nterms, cap, d_term_off, ndocs, nids, doc_base, shift, ntl, cnt, tot,
                                        key[p & 1u], pay[p & 1u], d_post_doc, d_post_tf, pcap));
        else
            JB_TIMED(K_POST_SCATTER,
                     hipLaunchKernelGGL(k_post_scatter<0>, dim3(ntl), dim3(256), 0, stream, src, pin, d_term_cnt, first,
                                        last, d_nterms, cap, d_term_off, ndocs, nids, doc_base, shift, ntl, cnt, tot,
                                        key[p & 1u], pay[p & 1u], d_post_doc, d_post_tf, pcap));
    }
    const uint32_t goff = (uint32_t)(((uint64_t)nids + 1u + 255u) / 256u);
    JB_TIMED(K_POST_OFF, hipLaunchKernelGGL(k_post_off, dim3(goff), dim3(256), 0, stream, key[(P - 1u) & 1u],
                                            d_nterms, cap, d_term_off, ndocs, nids, d_post_off, d_nposts));
    return hipGetLastError();
}

}  // namespace jb
