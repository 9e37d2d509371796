// jb_k_tok.hip — the span kernels (token bitmaps -> spans, per-document first tokens),
// the boundary-mask merge, and the utility kernels k_snap, k_zero and k_span_pack.
#include "jb_kdev.h"
#include "jb_kstages.h"

#include <algorithm>

namespace jb {

// k_sup: the (x, y) sums of each group of 256 consecutive tile counts.
__global__ __launch_bounds__(256) void k_sup(const uint2* __restrict__ cnt, uint32_t n, uint2* __restrict__ sup) {
    __shared__ uint32_t lds[8];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    PrefixLoads p{0u, 0u};
    if (i < n) {
        const uint2 c = cnt[i];
        p.x = c.x;
        p.y = c.y;
    }
    const uint2 s = pf_sum(p, lds);
    if (threadIdx.x == 0) sup[blockIdx.x] = s;
}

// ---------------------------------------------------------------------------
// token bitmaps -> spans
// ---------------------------------------------------------------------------
#ifndef JB_TOK_CAP
#define JB_TOK_CAP 3072
#endif
constexpr uint32_t kTokCap = JB_TOK_CAP;  // tokens per tile staged in LDS (k_tok's write pass)
// block `blk` of `nblk` (the write pass: token tile blk; the count pass: tiles 2 blk, 2 blk + 1)
template <bool WRITE>
__device__ __forceinline__ void tok_body(const uint32_t* __restrict__ sbits, const uint32_t* __restrict__ ebits,
                                         uint64_t nwords, uint2* __restrict__ tile_cnt,
                                         const uint2* __restrict__ supt, uint32_t* __restrict__ counters,
                                         uint32_t* __restrict__ tok_start, uint32_t* __restrict__ tok_end,
                                         uint32_t blk, uint32_t nblk, uint32_t* lds, uint32_t* s_s, uint32_t* s_e) {
    // bitmap words per lane: the write pass takes a token tile per workgroup, the count
    // pass two (16-byte loads, half the workgroups; a tile's count is the half's sum)
    constexpr uint32_t W = (WRITE ? 1u : 2u) * (kTokTileWords / 256);
    constexpr uint32_t kCap = kTokCap;
    const uint64_t w0 = ((uint64_t)blk * 256u + threadIdx.x) * W;
    PrefixLoads pl{0u, 0u};
    if (WRITE) pl = pf_load(tile_cnt, supt, blk);
    uint32_t s[W], e[W];
    if (w0 + W <= nwords) {
        if constexpr (W == 4u) {
            const uint4 a = *reinterpret_cast<const uint4*>(sbits + w0);
            const uint4 b = *reinterpret_cast<const uint4*>(ebits + w0);
            s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
            e[0] = b.x; e[1] = b.y; e[2] = b.z; e[3] = b.w;
        } else {
            const uint2 a = *reinterpret_cast<const uint2*>(sbits + w0);
            const uint2 b = *reinterpret_cast<const uint2*>(ebits + w0);
            s[0] = a.x; s[1] = a.y;
            e[0] = b.x; e[1] = b.y;
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < W; k++) {
            s[k] = w0 + k < nwords ? sbits[w0 + k] : 0u;
            e[k] = w0 + k < nwords ? ebits[w0 + k] : 0u;
        }
    }
    uint32_t cs = 0, ce = 0;
#pragma unroll
    for (uint32_t k = 0; k < W; k++) {
        cs += __popc(s[k]);
        ce += __popc(e[k]);
    }
    uint32_t ts, te;
    const uint32_t xs = block_scan_u32(cs, lds, &ts);
    const uint32_t xe = block_scan_u32(ce, lds, &te);
    if (!WRITE) {  // lanes 0-127 hold the first tile: its count is lane 128's exclusive prefix
        if (threadIdx.x == 128u) {
            tile_cnt[2u * blk] = make_uint2(xs, xe);
            tile_cnt[2u * blk + 1u] = make_uint2(ts - xs, te - xe);
        }
        return;
    }
    const uint2 to = pf_sum(pl, lds);
    if (blk == nblk - 1u && threadIdx.x == 0) {  // token totals
        counters[CNT_NTOK] = to.x + ts;
        counters[CNT_NTOKE] = to.y + te;
        *reinterpret_cast<uint64_t*>(counters + CNT_NWORDS) = to.x + ts;
    }
    // spans go to LDS in tile order, then out in one coalesced pass (a lane's own
    // tokens are ~60 bytes apart in the output: direct stores touch a line each)
    const bool staged = ts <= kCap && te <= kCap;
    // staged at LDS index (output index mod 4) + k, so that LDS and output share their
    // 16-byte alignment and the copy-out moves four spans per lane and store
    // (k_tok_write 0.298 -> 0.288 ms at 1 GiB; caller arrays not 16-byte aligned: one each)
    const bool v4 = (((uintptr_t)tok_start | (uintptr_t)tok_end) & 15u) == 0u;
    const uint32_t shs = v4 ? (to.x & 3u) : 0u, she = v4 ? (to.y & 3u) : 0u;
    uint32_t* os = staged ? s_s + shs : tok_start + to.x;
    uint32_t* oe = staged ? s_e + she : tok_end + to.y;
    uint32_t gs = xs, ge = xe;
#pragma unroll
    for (uint32_t k = 0; k < W; k++) {
        const uint32_t base = (uint32_t)((w0 + k) << 5);
        uint32_t m = s[k];
        while (m) {
            os[gs++] = base + (uint32_t)__builtin_ctz(m);
            m &= m - 1;
        }
        m = e[k];
        while (m) {
            oe[ge++] = base + (uint32_t)__builtin_ctz(m) + 1u;
            m &= m - 1;
        }
    }
    if (staged) {
        __syncthreads();
        if (v4) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            auto out = [&](const uint32_t* a, uint32_t sh, uint32_t n, uint32_t* g) {  // g: output at LDS index 0
                const uint32_t lo = (sh + 3u) & ~3u, hi = (sh + n) & ~3u;  // whole vectors: [lo, hi)
                if (lo < hi) {
                    for (uint32_t p = lo + 4u * threadIdx.x; p < hi; p += 1024u)
                        __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(a + p), reinterpret_cast<u32x4*>(g + p));
                    if (threadIdx.x < lo - sh) __builtin_nontemporal_store(a[sh + threadIdx.x], g + sh + threadIdx.x);
                    if (threadIdx.x < sh + n - hi) __builtin_nontemporal_store(a[hi + threadIdx.x], g + hi + threadIdx.x);
                } else if (threadIdx.x < n) {
                    __builtin_nontemporal_store(a[sh + threadIdx.x], g + sh + threadIdx.x);
                }
            };
            out(s_s, shs, ts, tok_start + to.x - shs);
            out(s_e, she, te, tok_end + to.y - she);
            return;
        }
        for (uint32_t k = threadIdx.x; k < ts; k += 256u) __builtin_nontemporal_store(s_s[k], tok_start + to.x + k);
        for (uint32_t k = threadIdx.x; k < te; k += 256u) __builtin_nontemporal_store(s_e[k], tok_end + to.y + k);
    }
}
template <bool WRITE>
__global__ __launch_bounds__(256) void k_tok(const uint32_t* __restrict__ sbits, const uint32_t* __restrict__ ebits,
                                             uint64_t nwords, uint2* __restrict__ tile_cnt,
                                             const uint2* __restrict__ supt, uint32_t* __restrict__ counters,
                                             uint32_t* __restrict__ tok_start, uint32_t* __restrict__ tok_end) {
    __shared__ uint32_t lds[8];
    __shared__ __attribute__((aligned(16))) uint32_t s_s[WRITE ? kTokCap + 4 : 1], s_e[WRITE ? kTokCap + 4 : 1];
    tok_body<WRITE>(sbits, ebits, nwords, tile_cnt, supt, counters, tok_start, tok_end, blockIdx.x, gridDim.x, lds, s_s,
                    s_e);
}

// tokens of document d: [doc_tok[d], doc_tok[d+1]) = lower_bound over starts.
// G lanes per document.  G = 16 (a small batch: few documents, so the kernel's time
// is one search's dependent loads): each trip, lane k probes the last start of the
// k-th sixteenth of the range and a ballot counts the sixteenths wholly before the
// target, log16 loads instead of log2.  G = 1 (many documents: their searches hide
// each other's latency, and 16 lanes each would cost more loads in all): binary.
template <uint32_t G>
__device__ __forceinline__ void doc_tok_body(const uint64_t* __restrict__ doc_off, uint32_t ndocs,
                                             const uint32_t* __restrict__ tok_start,
                                             const uint32_t* __restrict__ counters, uint64_t* __restrict__ doc_tok,
                                             uint32_t g) {
    static_assert(G == 1u || G == 16u, "binary or 16-ary");
    const uint32_t d = g / G, k = threadIdx.x & (G - 1u), gsh = threadIdx.x & (63u & ~(G - 1u));
    if (d > ndocs) return;  // (whole groups: a group is one document)
    const uint32_t n = counters[CNT_NTOK];
    const uint64_t target = doc_off[d];
    uint32_t lo = 0, hi = n;  // the answer is in [lo, hi]
    if constexpr (G == 1u) {
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((uint64_t)tok_start[mid] < target) lo = mid + 1;
            else hi = mid;
        }
    } else {
        while (lo < hi) {
            const uint32_t s = (hi - lo + 15u) >> 4;  // a sixteenth, rounded up
            const uint32_t i = lo + (k + 1u) * s - 1u;
            const bool before = i < hi && (uint64_t)tok_start[i] < target;
            const uint32_t c = (uint32_t)__popcll((__ballot(before) >> gsh) & 0xFFFFull);
            const uint32_t nlo = lo + c * s;
            if (s == 1u || nlo >= hi) {
                lo = min(nlo, hi);
                break;
            }
            hi = min(hi, nlo + s - 1u);  // (the probe ending the c-th sixteenth is >= target)
            lo = nlo;
        }
    }
    if (k == 0u) doc_tok[d] = lo;
}
template <uint32_t G>
__global__ __launch_bounds__(256) void k_doc_tok(const uint64_t* __restrict__ doc_off, uint32_t ndocs,
                                                 const uint32_t* __restrict__ tok_start,
                                                 const uint32_t* __restrict__ counters, uint64_t* __restrict__ doc_tok) {
    doc_tok_body<G>(doc_off, ndocs, tok_start, counters, doc_tok, blockIdx.x * blockDim.x + threadIdx.x);
}
constexpr uint32_t kDocTokWide = 16384;  // documents from which k_doc_tok searches one lane each

// k_tok1: the span kernels in one pass (round 5): k_tok's count pass, k_sup, its write
// pass and k_doc_tok.  A workgroup takes the next token tile by a ticket (tiles in
// claim order), counts its tokens, publishes the count, and finds its exclusive prefix
// by looking back over the tiles before it (decoupled look-back: a tile's status word is
// its count, flag 1, or its inclusive prefix, flag 2; it waits only on tiles claimed
// before it, so by running workgroups).  Then it writes its spans as k_tok's write pass
// does, and the per-document first tokens of the documents that start in its bytes
// (k_doc_tok's lower bound, here over the tile's own starts in LDS).
// Status: flag << 62 | starts prefix (31 bits) << 31 | ends prefix (31 bits).
__device__ __forceinline__ uint64_t ts_pack(uint32_t f, uint32_t x, uint32_t y) {
    return ((uint64_t)f << 62) | ((uint64_t)x << 31) | (uint64_t)y;
}
__global__ __launch_bounds__(256) void k_tok1(const uint32_t* __restrict__ sbits, const uint32_t* __restrict__ ebits,
                                              uint64_t nwords, uint32_t ntt, uint64_t* __restrict__ tstat,
                                              uint32_t* __restrict__ counters, uint32_t* __restrict__ tok_start,
                                              uint32_t* __restrict__ tok_end, const uint64_t* __restrict__ doc_off,
                                              uint32_t ndocs, uint64_t* __restrict__ doc_tok) {
    constexpr uint32_t W = kTokTileWords / 256u;
    constexpr uint32_t kCap = kTokCap;
    constexpr uint64_t TB = (uint64_t)kTokTileWords * 32u;  // bytes per token tile
    __shared__ uint32_t lds[8];
    __shared__ uint32_t s_t, s_d0;
    __shared__ uint2 s_to;
    __shared__ __attribute__((aligned(16))) uint32_t s_s[kCap + 4], s_e[kCap + 4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0u) s_t = __hip_atomic_fetch_add(counters + CNT_TOKT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint32_t t = s_t;
    const uint64_t w0 = ((uint64_t)t * 256u + threadIdx.x) * W;
    uint32_t s[W], e[W];
    if (w0 + W <= nwords) {
        const uint2 a = *reinterpret_cast<const uint2*>(sbits + w0);
        const uint2 b = *reinterpret_cast<const uint2*>(ebits + w0);
        s[0] = a.x; s[1] = a.y;
        e[0] = b.x; e[1] = b.y;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < W; k++) {
            s[k] = w0 + k < nwords ? sbits[w0 + k] : 0u;
            e[k] = w0 + k < nwords ? ebits[w0 + k] : 0u;
        }
    }
    // the first document that starts in the tile (or after it): a JB_TOK1_ARY-ary lower bound
    // over doc_off (wave 1, its loads beside the bitmap loads)
#ifndef JB_TOK1_ARY
#define JB_TOK1_ARY 64
#endif
    static_assert(JB_TOK1_ARY == 16 || JB_TOK1_ARY == 64, "k_tok1's search: 16 or 64 lanes");
    if (wave == 1u) {
        constexpr uint32_t AR = JB_TOK1_ARY, SH = AR == 64u ? 6u : 4u;
        const uint64_t target = (uint64_t)t * TB;
        const uint32_t k = lane & (AR - 1u);
        uint32_t lo = 0, hi = ndocs + 1u;  // the answer in [lo, hi]
        while (lo < hi) {
            const uint32_t sx = (hi - lo + AR - 1u) >> SH;
            const uint32_t i = lo + (k + 1u) * sx - 1u;
            const bool before = i < hi && doc_off[i] < target;
            const uint32_t c = (uint32_t)__popcll(__ballot(before) & (AR == 64u ? ~0ull : 0xFFFFull));
            const uint32_t nlo = lo + c * sx;
            if (sx == 1u || nlo >= hi) {
                lo = min(nlo, hi);
                break;
            }
            hi = min(hi, nlo + sx - 1u);
            lo = nlo;
        }
        if (lane == 0u) s_d0 = lo;
    }
    uint32_t cs = 0, ce = 0;
#pragma unroll
    for (uint32_t k = 0; k < W; k++) {
        cs += __popc(s[k]);
        ce += __popc(e[k]);
    }
    uint32_t ts, te;
    const uint32_t xs = block_scan_u32(cs, lds, &ts);
    const uint32_t xe = block_scan_u32(ce, lds, &te);
    // publish the count, then look back (wave 0)
    if (threadIdx.x == 0u)
        __hip_atomic_store(tstat + t, ts_pack(t == 0u ? 2u : 1u, ts, te), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (wave == 0u) {
        uint32_t px = 0, py = 0;
        for (int64_t base = (int64_t)t - 1; base >= 0;) {
            const int64_t j = base - (int64_t)lane;
            uint64_t v = j >= 0 ? __hip_atomic_load(tstat + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ts_pack(2u, 0u, 0u);
            const uint64_t incl = __ballot((v >> 62) == 2u), ready = __ballot((v >> 62) != 0u);
            // the nearest inclusive prefix, and every tile between ready
            const uint32_t k2 = incl ? (uint32_t)__builtin_ctzll(incl) : 64u;
            const uint64_t need = k2 == 64u ? ~0ull : ((2ull << k2) - 1ull);
            if ((ready & need) != need) {
                __builtin_amdgcn_s_sleep(1);
                continue;  // (a tile before is still counting: read again)
            }
            uint32_t x = lane <= k2 ? (uint32_t)(v >> 31) & 0x7FFFFFFFu : 0u;
            uint32_t y = lane <= k2 ? (uint32_t)v & 0x7FFFFFFFu : 0u;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                x += (uint32_t)__shfl_xor((int)x, d, 64);
                y += (uint32_t)__shfl_xor((int)y, d, 64);
            }
            px += x;
            py += y;
            if (k2 < 64u) break;
            base -= 64;
        }
        if (lane == 0u) {
            s_to = make_uint2(px, py);
            if (t > 0u)
                __hip_atomic_store(tstat + t, ts_pack(2u, px + ts, py + te), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    const uint2 to = s_to;
    if (t == ntt - 1u && threadIdx.x == 0) {  // token totals
        counters[CNT_NTOK] = to.x + ts;
        counters[CNT_NTOKE] = to.y + te;
        *reinterpret_cast<uint64_t*>(counters + CNT_NWORDS) = to.x + ts;
    }
    // the spans (k_tok's write pass)
    const bool staged = ts <= kCap && te <= kCap;
    const bool v4 = (((uintptr_t)tok_start | (uintptr_t)tok_end) & 15u) == 0u;
    const uint32_t shs = v4 ? (to.x & 3u) : 0u, she = v4 ? (to.y & 3u) : 0u;
    uint32_t* os = staged ? s_s + shs : tok_start + to.x;
    uint32_t* oe = staged ? s_e + she : tok_end + to.y;
    uint32_t gs = xs, ge = xe;
#pragma unroll
    for (uint32_t k = 0; k < W; k++) {
        const uint32_t base = (uint32_t)((w0 + k) << 5);
        uint32_t m = s[k];
        while (m) {
            os[gs++] = base + (uint32_t)__builtin_ctz(m);
            m &= m - 1;
        }
        m = e[k];
        while (m) {
            oe[ge++] = base + (uint32_t)__builtin_ctz(m) + 1u;
            m &= m - 1;
        }
    }
    __syncthreads();  // (the staged starts, or this workgroup's global ones, for the documents below)
    // the documents that start in the tile (the last tile: all that are left, with the end
    // sentinel d = ndocs): their first token is the first start >= their offset
    {
        const uint32_t d0 = s_d0;
        const uint64_t hiB = t == ntt - 1u ? ~0ull : ((uint64_t)t + 1u) * TB;
        for (uint32_t d = d0 + threadIdx.x; d <= ndocs; d += 256u) {
            const uint64_t o = doc_off[d];
            if (o >= hiB) break;
            const uint32_t* st = staged ? s_s + shs : tok_start + to.x;
            uint32_t lo = 0, hi = ts;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((uint64_t)st[mid] < o) lo = mid + 1;
                else hi = mid;
            }
            doc_tok[d] = to.x + lo;
        }
    }
    if (!staged) return;
    if (v4) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        auto out = [&](const uint32_t* a, uint32_t sh, uint32_t n, uint32_t* g) {  // g: output at LDS index 0
            const uint32_t lo = (sh + 3u) & ~3u, hi = (sh + n) & ~3u;  // whole vectors: [lo, hi)
            if (lo < hi) {
                for (uint32_t p = lo + 4u * threadIdx.x; p < hi; p += 1024u)
                    __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(a + p), reinterpret_cast<u32x4*>(g + p));
                if (threadIdx.x < lo - sh) __builtin_nontemporal_store(a[sh + threadIdx.x], g + sh + threadIdx.x);
                if (threadIdx.x < sh + n - hi) __builtin_nontemporal_store(a[hi + threadIdx.x], g + hi + threadIdx.x);
            } else if (threadIdx.x < n) {
                __builtin_nontemporal_store(a[sh + threadIdx.x], g + sh + threadIdx.x);
            }
        };
        out(s_s, shs, ts, tok_start + to.x - shs);
        out(s_e, she, te, tok_end + to.y - she);
        return;
    }
    for (uint32_t k = threadIdx.x; k < ts; k += 256u) __builtin_nontemporal_store(s_s[k], tok_start + to.x + k);
    for (uint32_t k = threadIdx.x; k < te; k += 256u) __builtin_nontemporal_store(s_e[k], tok_end + to.y + k);
}

// A pipeline run's counters and summed tile block counts, written straight into
// mapped pinned host memory (cut_range: no copy-engine transfer on the kernels'
// stream, where it would queue behind the bulk copies of later pieces).
// out: u32[kSnapWords]: counters[0..CNT_CLEAR), then u64 blocks, u64 zh blocks.
__global__ __launch_bounds__(256) void k_snap(const uint32_t* __restrict__ counters, const uint2* __restrict__ tile_cnt,
                                              uint32_t ntiles, uint32_t* __restrict__ out) {
    __shared__ unsigned long long red[8];
    unsigned long long b = 0, z = 0;
    for (uint32_t t = threadIdx.x; t < ntiles; t += 256u) {
        const uint2 c = tile_cnt[t];
        b += c.x;
        z += c.y;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        b += (unsigned long long)__shfl_xor((long long)b, d, 64);
        z += (unsigned long long)__shfl_xor((long long)z, d, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        red[threadIdx.x >> 6] = b;
        red[4 + (threadIdx.x >> 6)] = z;
    }
    __syncthreads();
    if (threadIdx.x < CNT_CLEAR) out[threadIdx.x] = counters[threadIdx.x];
    if (threadIdx.x == 0) {
        const unsigned long long bs = red[0] + red[1] + red[2] + red[3], zs = red[4] + red[5] + red[6] + red[7];
        out[CNT_CLEAR] = (uint32_t)bs;
        out[CNT_CLEAR + 1] = (uint32_t)(bs >> 32);
        out[CNT_CLEAR + 2] = (uint32_t)zs;
        out[CNT_CLEAR + 3] = (uint32_t)(zs >> 32);
    }
    __threadfence_system();
}

// Zero n u32 words (instead of hipMemsetAsync, which may go to the copy engine and
// queue there behind the host pipeline's bulk transfers).
__global__ __launch_bounds__(256) void k_zero(uint32_t* __restrict__ p, uint64_t n, bool v4,
                                             uint32_t* __restrict__ p2, uint32_t n2) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u, t0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t0 < n2) p2[t0] = 0u;  // a second, small range (n2 <= 256) in the same launch
    const uint64_t n4 = v4 ? n / 4u : 0u;
    uint4* p4 = reinterpret_cast<uint4*>(p);
    for (uint64_t i = t0; i < n4; i += stride) p4[i] = make_uint4(0u, 0u, 0u, 0u);
    for (uint64_t i = 4u * n4 + t0; i < n; i += stride) p[i] = 0u;
}

hipError_t run_zero(void* p, uint64_t bytes, hipStream_t stream, void* p2, uint32_t bytes2) {
    const uint64_t n = bytes / 4u;  // (callers pass whole words)
    if (!n && !bytes2) return hipSuccess;
    const bool v4 = ((uintptr_t)p & 15u) == 0;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(2048u, (n / 4u + 255u) / 256u + 1u);
    hipLaunchKernelGGL(k_zero, dim3(grid), dim3(256), 0, stream, reinterpret_cast<uint32_t*>(p), n, v4,
                       reinterpret_cast<uint32_t*>(p2), bytes2 / 4u);
    return hipGetLastError();
}

hipError_t run_snap(const Work& w, uint64_t nbytes, uint32_t* out, hipStream_t stream) {
    const uint32_t ntiles = (uint32_t)((nbytes + kTileBytes - 1) / kTileBytes);
    hipLaunchKernelGGL(k_snap, dim3(1), dim3(256), 0, stream, w.counters, w.tile_cnt, ntiles, out);
    return hipGetLastError();
}

// Spans packed for the trip back to the host (jb_cut_batch's spans mode): token i as
// one u16, the gap from the previous token's end (0 for the first) in the low 6 bits and
// its length in the high 10, so the host link carries 2 bytes per token instead of 8 (on
// the C_syn corpus gaps stay under 63 bytes and tokens under 1,023: 0 escapes in 4.36M
// tokens).  A gap of 63 or more or a length of 1,023 or more is written as 0xFFFF, with
// the token's (index, start, end) appended to a side list.  hdr[b] is the end of the token
// before token b x kPackBlock (0 for b = 0), so the host decodes blocks of kPackBlock
// tokens independently.
__global__ __launch_bounds__(256) void k_span_pack(const uint32_t* __restrict__ ts, const uint32_t* __restrict__ te,
                                                   uint32_t* __restrict__ counters, uint16_t* __restrict__ pk,
                                                   uint32_t* __restrict__ hdr, uint4* __restrict__ side,
                                                   uint32_t side_cap) {
    const uint32_t nt = counters[CNT_NWORDS];  // (the u64 token count's low word: a piece has < 2^31 tokens)
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nt; i += gridDim.x * 256u) {
        const uint32_t a = ts[i], b = te[i], p = i ? te[i - 1u] : 0u;
        const uint32_t g = a - p, l = b - a;
        uint32_t x = g | (l << kPackGapBits);
        if (g >= kPackGapEsc || l >= kPackLenEsc) {
            x = 0xFFFFu;
            const uint32_t k = atomicAdd(counters + CNT_SIDE, 1u);
            if (k < side_cap) side[k] = make_uint4(i, a, b, 0u);
            else atomicOr(counters + CNT_ERR, 4u);  // (cannot happen: side_cap bounds the escapes)
        }
        pk[i] = (uint16_t)x;
        if ((i & (kPackBlock - 1u)) == 0u) hdr[i / kPackBlock] = p;
    }
}

hipError_t run_span_pack(const uint32_t* ts, const uint32_t* te, uint32_t* counters, uint16_t* pk, uint32_t* hdr,
                         uint4* side, uint32_t side_cap, uint64_t max_tokens, hipStream_t stream) {
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(4096u, (max_tokens + 255u) / 256u));
    hipLaunchKernelGGL(k_span_pack, dim3(grid), dim3(256), 0, stream, ts, te, counters, pk, hdr, side, side_cap);
    return hipGetLastError();
}

// Boundary-mask output (jb_cut_batch_mask): a piece's token bitmaps (bit j = byte j
// of the piece, u32 words) into the range's u64 bitmaps at bit offset `rel`, bits
// of other pieces untouched: a word the piece shares with its neighbours (its first
// and last) is ORed in, the others stored.  Pieces of one range run in order on one
// stream over bitmaps cleared at the start.  Counts the piece's token starts and
// ends into the counters (the spans kernels do not run in this mode).
constexpr uint32_t kMergeWords = 16;  // k_mask_merge: output words per thread
__global__ __launch_bounds__(256) void k_mask_merge(const uint32_t* __restrict__ sbits,
                                                    const uint32_t* __restrict__ ebits, uint64_t n, uint64_t rel,
                                                    uint64_t* __restrict__ ms, uint64_t* __restrict__ me,
                                                    uint32_t* __restrict__ counters) {
    __shared__ uint32_t red[8];
    const uint32_t sh = (uint32_t)(rel & 63u);
    const uint64_t nout = (sh + n + 63u) >> 6, nw32 = (n + 31u) >> 5;
    auto piece64 = [&](const uint32_t* b, int64_t i) -> uint64_t {  // piece bits [64i, 64i + 64)
        if (i < 0) return 0ull;
        const uint64_t lo = 2u * (uint64_t)i, hi = lo + 1u;
        return (lo < nw32 ? (uint64_t)b[lo] : 0ull) | ((hi < nw32 ? (uint64_t)b[hi] : 0ull) << 32);
    };
    uint32_t cs = 0, ce = 0;
    const uint64_t t0 = (uint64_t)blockIdx.x * (256u * kMergeWords) + threadIdx.x;
#pragma unroll 4
    for (uint32_t j = 0; j < kMergeWords; j++) {
        const uint64_t t = t0 + 256u * j;  // (consecutive threads: consecutive words)
        if (t >= nout) break;
        uint64_t os = piece64(sbits, (int64_t)t), oe = piece64(ebits, (int64_t)t);
        if (sh) {
            os = (os << sh) | (piece64(sbits, (int64_t)t - 1) >> (64u - sh));
            oe = (oe << sh) | (piece64(ebits, (int64_t)t - 1) >> (64u - sh));
        }
        const uint64_t w = (rel >> 6) + t;
        if (t == 0 || t == nout - 1u) {
            if (os) atomicOr(reinterpret_cast<unsigned long long*>(ms + w), (unsigned long long)os);
            if (oe) atomicOr(reinterpret_cast<unsigned long long*>(me + w), (unsigned long long)oe);
        } else {
            ms[w] = os;
            me[w] = oe;
        }
        cs += (uint32_t)__popcll(os);
        ce += (uint32_t)__popcll(oe);
    }
    // one set of counter atomics per workgroup (one per wave serialised on three addresses)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        cs += (uint32_t)__shfl_xor((int)cs, d, 64);
        ce += (uint32_t)__shfl_xor((int)ce, d, 64);
    }
    const uint32_t wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        red[wv] = cs;
        red[4 + wv] = ce;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        cs = red[0] + red[1] + red[2] + red[3];
        ce = red[4] + red[5] + red[6] + red[7];
        if (cs | ce) {
            atomicAdd(counters + CNT_NTOK, cs);
            atomicAdd(counters + CNT_NTOKE, ce);
            atomicAdd(reinterpret_cast<unsigned long long*>(counters + CNT_NWORDS), (unsigned long long)cs);
        }
    }
}

void enq_sup(const uint2* cnt, uint32_t n, uint2* sup, hipStream_t stream) {
    hipLaunchKernelGGL(k_sup, dim3((n + 255u) / 256u), dim3(256), 0, stream, cnt, n, sup);
}

void enq_tok_count(const Work& w, uint64_t nwords, uint32_t nttiles, hipStream_t stream) {
    hipLaunchKernelGGL((k_tok<false>), dim3((nttiles + 1u) / 2u), dim3(256), 0, stream, w.sbits, w.ebits, nwords,
                       w.ttile_cnt, w.supt, w.counters, nullptr, nullptr);
}

void enq_tok_write(const Work& w, uint64_t nwords, uint32_t nttiles, hipStream_t stream) {
    hipLaunchKernelGGL((k_tok<true>), dim3(nttiles), dim3(256), 0, stream, w.sbits, w.ebits, nwords, w.ttile_cnt,
                       w.supt, w.counters, w.tok_start, w.tok_end);
}

void enq_doc_tok(const Work& w, const uint64_t* d_doc_off, uint32_t ndocs, hipStream_t stream) {
    if (ndocs >= kDocTokWide)
        hipLaunchKernelGGL(k_doc_tok<1>, dim3((ndocs + 1 + 255) / 256), dim3(256), 0, stream, d_doc_off, ndocs,
                           w.tok_start, w.counters, w.doc_tok);
    else
        hipLaunchKernelGGL(k_doc_tok<16>, dim3((16u * (ndocs + 1) + 255) / 256), dim3(256), 0, stream, d_doc_off,
                           ndocs, w.tok_start, w.counters, w.doc_tok);
}

void enq_tok1(const Work& w, uint64_t nwords, uint32_t nttiles, const uint64_t* d_doc_off, uint32_t ndocs,
              hipStream_t stream) {
    hipLaunchKernelGGL(k_tok1, dim3(nttiles), dim3(256), 0, stream, w.sbits, w.ebits, nwords, nttiles,
                       reinterpret_cast<uint64_t*>(w.ttile_cnt), w.counters, w.tok_start, w.tok_end, d_doc_off, ndocs,
                       w.doc_tok);
}

void enq_mask_merge(const Work& w, uint64_t nbytes, const MaskOut& mask, hipStream_t stream) {
    const uint64_t nout = ((mask.rel & 63u) + nbytes + 63u) >> 6;
    hipLaunchKernelGGL(k_mask_merge, dim3((uint32_t)((nout + 256u * kMergeWords - 1u) / (256u * kMergeWords))),
                       dim3(256), 0, stream, w.sbits, w.ebits, nbytes, mask.rel, mask.s, mask.e, w.counters);
}

}  // namespace jb
