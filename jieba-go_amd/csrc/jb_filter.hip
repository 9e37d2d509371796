// jb_filter.hip — gfx950 kernels of the token filter (jb_filter_device; the rule is jb_filter's, jb_filter.cpp;
// the code shared with the host is jb_filter.h's).
//
// A span list of any mode and its per-document offsets become the shorter list of the tokens a rule keeps,
// in their order, with its own per-document offsets and count.  n_t = min(*ntok, cap) tokens take part.
// Tile = kFiltTile consecutive tokens, one workgroup of 4 waves each; on trip j (0 .. 7) wave w owns the 64
// tokens of the tile's word j * 4 + w, one lane per token, so a wave ballot is that word of the keep bitmap.
//   k_filt_mark   the key from aligned dwords (ids_one's reads), jb_filter_decide; each wave's ballot goes to
//                 words[] (zero bits past n_t: every word of every tile is written), ballots of the four
//                 reasons are counted per wave, and the workgroup sums them into cnt[tile][0..4].
//   k_filt_scan   one workgroup, looping over the tiles (k_join_scan's pattern): base[i] = the kept tokens
//                 before tile i (ntl + 1 entries), the five totals, *out_ntok and stats.
//   k_filt_write  the token tiles: a kept token's rank is base[tile] + the popcounts of the tile's earlier
//                 words + the popcount of its own word below its lane; out_start, out_end and out_src are
//                 written at ranks below out_cap.  The workgroups past the token tiles take 256 documents
//                 each: out_doc_tok[d] = R(min(doc_tok[d], n_t)) from the same words and prefixes.
// No lane waits for another and there are no global atomics; every value is an integer sum, so the outputs
// are the same from run to run.  Text bytes are read only for spans with start < end <= nbytes, in
// [start & ~3, start + 28) or inside the span, and at most JB_FILTER_SCAN of them for a count: never at or
// past nbytes + 64.  Every write index into out_* is a rank below out_cap or a document index <= ndocs;
// words[], cnt[] and base[] are written inside jb_filter_work_bytes(cap, ndocs).
#include <hip/hip_runtime.h>

#include "jb_filter.h"
#include "jb_kstages.h"

#include <algorithm>

namespace jb {

namespace {

constexpr uint32_t T = kFiltTile;
constexpr uint32_t PER = T / 256u;  // trips per workgroup: tokens per thread
constexpr uint32_t WPT = T / 64u;   // bitmap words per tile
static_assert(kFiltTile == JB_FILTER_TILE, "the header's constant");
static_assert(WPT == 32 && PER * 4u == WPT, "wave w of trip j owns word j * 4 + w; 32 lanes prefix a tile's words");

__device__ __forceinline__ uint32_t filt_word_mask(uint32_t len, uint32_t w) {
    if (len >= 4u * w + 4u) return 0xFFFFFFFFu;
    return len > 4u * w ? (1u << (8u * (len - 4u * w))) - 1u : 0u;
}

// The reason of span [s, e) (JB_FR_*).  A bad span reads nothing.
__device__ __forceinline__ uint32_t filt_one(const uint8_t* __restrict__ text, uint32_t nbytes, const jb_filter_rule& r,
                                             const DevVocab& stop, uint32_t s, uint32_t e) {
    if (jb_filter_bad(s, e, nbytes)) return JB_FR_BAD;
    const uint32_t len = e - s;
    const uint32_t* a = reinterpret_cast<const uint32_t*>(text + (s & ~3u));
    const uint32_t sh = s & 3u;
    uint32_t kw[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    const uint32_t d0 = a[0], d1 = a[1], d2 = a[2];
    kw[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
    kw[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
    if (len > 8u) {
        const uint32_t d3 = a[3], d4 = a[4];
        kw[2] = __builtin_amdgcn_alignbyte(d3, d2, sh);
        kw[3] = __builtin_amdgcn_alignbyte(d4, d3, sh);
        if (len > 16u) {
            const uint32_t d5 = a[5], d6 = a[6];
            kw[4] = __builtin_amdgcn_alignbyte(d5, d4, sh);
            kw[5] = __builtin_amdgcn_alignbyte(d6, d5, sh);
        }
    }
#pragma unroll
    for (uint32_t w = 0; w < 6u; w++) kw[w] &= filt_word_mask(len, w);
    return jb_filter_decide(r, stop, kw, text + s, len);
}

__device__ __forceinline__ uint32_t popc64(uint64_t v) { return (uint32_t)__popcll((unsigned long long)v); }

__global__ __launch_bounds__(256) void k_filt_mark(const uint8_t* __restrict__ text, uint32_t nbytes,
                                                   const uint32_t* __restrict__ ts, const uint32_t* __restrict__ te,
                                                   const uint64_t* __restrict__ ntok, uint64_t cap, jb_filter_rule rule,
                                                   DevVocab stop, uint64_t* __restrict__ words,
                                                   uint32_t* __restrict__ cnt) {
    __shared__ uint32_t s_c[4][5];
    const uint32_t th = threadIdx.x, lane = th & 63u, w = th >> 6;
    const uint64_t n = std::min(*ntok, cap), t0 = (uint64_t)blockIdx.x * T;
    uint32_t why[PER];
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        const uint64_t k = t0 + j * 256u + th;
        why[j] = 0xFFu;  // (past the list: no reason, and not kept)
        if (k < n) why[j] = filt_one(text, nbytes, rule, stop, ts[k], te[k]);
    }
    // (the ballots stand outside every divergent branch: all 64 lanes take part)
    uint32_t c[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        const uint64_t keep = __ballot(why[j] == JB_FR_KEEP);
        if (lane == 0) words[(uint64_t)blockIdx.x * WPT + j * 4u + w] = keep;
        c[0] += popc64(keep);
#pragma unroll
        for (uint32_t q = 1; q < 5u; q++) c[q] += popc64(__ballot(why[j] == q));
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t q = 0; q < 5u; q++) s_c[w][q] = c[q];
    }
    __syncthreads();
    if (th < 5u) cnt[(uint64_t)blockIdx.x * 8u + th] = s_c[0][th] + s_c[1][th] + s_c[2][th] + s_c[3][th];
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, uint32_t o) {
    const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

// k_join_scan's block scan: the exclusive scan of one u64 per thread over 16 waves; *total is the sum.
__device__ __forceinline__ uint64_t block_excl64(uint64_t v, uint64_t* sh /* 16 */, uint64_t* total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint64_t u = shfl_up64(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();  // (sh may still be read from an earlier call)
    if (lane == 63u) sh[w] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) {
        const uint64_t x = sh[k];
        if (k < w) before += x;
        all += x;
    }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(1024) void k_filt_scan(const uint32_t* __restrict__ cnt, uint64_t ntl,
                                                    const uint64_t* __restrict__ ntok, uint64_t cap,
                                                    uint64_t* __restrict__ base, uint64_t* __restrict__ out_ntok,
                                                    uint64_t* __restrict__ stats) {
    __shared__ uint64_t sh[16];
    uint64_t carry = 0, r[4] = {0, 0, 0, 0};  // (r: this thread's share of the four reasons)
    for (uint64_t c0 = 0; c0 < ntl; c0 += 1024u) {
        const uint64_t i = c0 + threadIdx.x;
        uint64_t v = 0;
        if (i < ntl) {
            const uint32_t* c = cnt + i * 8u;  // (d_work is 8-byte aligned: no 16-byte load)
            v = c[0];
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) r[q] += c[1u + q];
        }
        uint64_t total;
        const uint64_t ex = block_excl64(v, sh, &total);
        if (i < ntl) base[i] = carry + ex;
        carry += total;
    }
    uint64_t tot[4];
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) (void)block_excl64(r[q], sh, &tot[q]);
    if (threadIdx.x == 0) {
        base[ntl] = carry;
        *out_ntok = carry;
        stats[0] = std::min(*ntok, cap);
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) stats[1u + q] = tot[q];
    }
}

__global__ __launch_bounds__(256) void k_filt_write(const uint32_t* __restrict__ ts, const uint32_t* __restrict__ te,
                                                    const uint64_t* __restrict__ doc_tok,
                                                    const uint64_t* __restrict__ ntok, uint64_t cap, uint32_t ndocs,
                                                    uint32_t ntl, const uint64_t* __restrict__ words,
                                                    const uint64_t* __restrict__ base, uint32_t* __restrict__ out_start,
                                                    uint32_t* __restrict__ out_end, uint32_t* __restrict__ out_src,
                                                    uint64_t out_cap, uint64_t* __restrict__ out_doc_tok) {
    __shared__ uint64_t s_w[WPT];
    __shared__ uint32_t s_pre[WPT];  // the set bits of the tile's words before each word
    const uint32_t th = threadIdx.x, lane = th & 63u, w = th >> 6;
    const uint64_t n = std::min(*ntok, cap);
    if (blockIdx.x >= ntl) {  // a document tile
        const uint64_t d = (uint64_t)(blockIdx.x - ntl) * 256u + th;
        if (d > ndocs) return;
        const uint64_t a = std::min(doc_tok[d], n);
        uint64_t R;
        if (a >= n) {
            R = base[ntl];  // (no bit is set at or past n)
        } else {
            const uint64_t tile = a / T;  // (a < n <= cap: a tile below ntl)
            const uint32_t in = (uint32_t)(a - tile * T), wi = in >> 6, bit = in & 63u;
            const uint64_t* tw = words + tile * WPT;
            R = base[tile];
            for (uint32_t i = 0; i < wi; i++) R += popc64(tw[i]);
            R += popc64(tw[wi] & ((1ull << bit) - 1ull));
        }
        out_doc_tok[d] = R;
        return;
    }
    const uint64_t t0 = (uint64_t)blockIdx.x * T;
    if (t0 >= n) return;
    if (th < WPT) {
        const uint64_t* tw = words + (uint64_t)blockIdx.x * WPT;
        s_w[th] = tw[th];
        uint32_t p = 0;
        for (uint32_t i = 0; i < th; i++) p += popc64(tw[i]);
        s_pre[th] = p;
    }
    __syncthreads();
    const uint64_t tb = base[blockIdx.x];
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        const uint64_t k = t0 + j * 256u + th;
        const uint32_t wi = j * 4u + w;
        const uint64_t word = s_w[wi];
        if (!((word >> lane) & 1ull)) continue;  // (a set bit's token lies below n)
        const uint64_t rank = tb + s_pre[wi] + popc64(word & ((1ull << lane) - 1ull));
        if (rank >= out_cap) continue;
        out_start[rank] = ts[k];
        out_end[rank] = te[k];
        if (out_src) out_src[rank] = (uint32_t)k;
    }
}

}  // namespace

hipError_t run_filter(const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start, const uint32_t* d_end,
                      const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint64_t cap, uint32_t ndocs,
                      const jb_filter_rule& rule, const DevVocab& stop, uint32_t* d_out_start, uint32_t* d_out_end,
                      uint32_t* d_out_src, uint64_t out_cap, uint64_t* d_out_doc_tok, uint64_t* d_out_ntok,
                      uint64_t* d_stats, void* d_work, hipStream_t stream, KernelTimer* timer) {
    if (cap == 0) {  // no token takes part: the zero outputs, no launch
        hipError_t e = hipMemsetAsync(d_out_doc_tok, 0, ((size_t)ndocs + 1u) * 8u, stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_out_ntok, 0, 8, stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_stats, 0, 40, stream);
        return e;
    }
    const FilterWork w = filter_layout(cap);
    uint8_t* b = (uint8_t*)d_work;
    uint64_t* words = (uint64_t*)(b + w.words);
    uint32_t* cnt = (uint32_t*)(b + w.cnt);
    uint64_t* base = (uint64_t*)(b + w.base);
    const uint32_t ntl = (uint32_t)w.ntl, ndt = (uint32_t)(((uint64_t)ndocs + 1u + 255u) / 256u);
    JB_TIMED(K_FILT_MARK, hipLaunchKernelGGL(k_filt_mark, dim3(ntl), dim3(256), 0, stream, d_text, (uint32_t)nbytes,
                                             d_start, d_end, d_ntok, cap, rule, stop, words, cnt));
    JB_TIMED(K_FILT_SCAN, hipLaunchKernelGGL(k_filt_scan, dim3(1), dim3(1024), 0, stream, cnt, w.ntl, d_ntok, cap, base,
                                             d_out_ntok, d_stats));
    JB_TIMED(K_FILT_WRITE, hipLaunchKernelGGL(k_filt_write, dim3(ntl + ndt), dim3(256), 0, stream, d_start, d_end,
                                              d_doc_tok, d_ntok, cap, ndocs, ntl, words, base, d_out_start, d_out_end,
                                              d_out_src, out_cap, d_out_doc_tok));
    return hipGetLastError();
}

}  // namespace jb
