// jb_textrank.hip — gfx950 kernels of jb_textrank_device: TextRank keywords per document, the rule of
// jiebahip.h ("TextRank keywords").  A unit of its own beside jb_terms.hip; it shares nothing with the cut
// pipeline and takes only the timing macros of jb_kstages.h.
//
// A term's index t in the CSR's flat lists is its node.  The work buffer holds, per token, its node
// (all-ones: not kept) and its reach (how many positions of its window lie on each side inside its
// document); per term its document, out, r and acc (ws lives in registers: a round's ws is a function of
// its acc); per document its node count n.
//   k_tr_init    per term below the CSR's length (term_off[ndocs], at most cap; the per-term kernels all
//                stop there): its document (binary search in term_off; none for a term of no valid row),
//                out = 0; per document: n = 0.
//   k_tr_setup   per chunk of kTrChunk consecutive tokens and a halo of span - 1 on each side: each
//                token's document (as k_terms_sort finds it), its node by binary search in the row, into
//                LDS; then per token of the chunk the kept tokens of its window are counted there, and
//                that degree goes to out[node] with one integer atomic.  Node and reach are written once
//                per call.
//   k_tr_count   per term with out > 0: n[document] += 1 (one add per wave where the wave's terms share
//                a document).
//   k_tr_step    per term: ws (1 / n before the first round, else 0.15 + 0.85 * acc * 2^-S), then
//                r = trunc(ws / out * 2^S), acc = 0.  ws itself is not stored.
//   k_tr_push / k_tr_push_win   acc[node(k)] += the sum of r[node(j)] over the kept j != k of k's window.
//                The plain form gathers r from memory and does one global atomic per kept token.  The
//                windowed form gathers each token's r once into an LDS tile with the halo, sums the
//                windows there, and combines the adds to one node within the workgroup in a
//                direct-mapped table in LDS (node tag and sum per slot) before one global atomic per
//                occupied slot.  The sums are u64 integers: the same whatever the order, in both forms.
//   k_tr_final   one wave per document: ws of the last round, its minimum and maximum over the nodes,
//                the f32 score, and the topk best keys (score bits << 32 | ~id) as k_keywords keeps them.
// Every f64 operation is a single IEEE operation (the unit is compiled with -ffp-contract=off), the same
// ones in the same order as jb_textrank.cpp.
//
// Nothing here synchronises, allocates or reads on the host; the launch count depends on iters alone.
#include <hip/hip_runtime.h>

#include "jb_kstages.h"

#include <algorithm>

namespace jb {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t C = kTrChunk;
constexpr uint32_t kHalo = kTrMaxSpan - 1u;
constexpr uint32_t kTileMax = C + 2u * kHalo;
static_assert(C == 1024, "the chunk kernels' thread layout: 256 threads x 4 tokens");

// First j in [lo, hi) with doc_tok[j] > k, else hi.
__device__ __forceinline__ uint64_t doc_ub(const uint64_t* __restrict__ doc_tok, uint64_t k, uint64_t lo, uint64_t hi) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (doc_tok[mid] > k) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ double pow2(int e) {  // 2^e for |e| <= 62, exactly
    return __longlong_as_double((long long)((uint64_t)(1023 + e) << 52));
}
// S = 62 - bit_length(n), n >= 1
__device__ __forceinline__ int scale_of(uint32_t n) { return 62 - (32 - (int)__clz((int)n)); }

__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
    const uint32_t lo = __shfl((uint32_t)v, (int)src, 64), hi = __shfl((uint32_t)(v >> 32), (int)src, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ double shfl_xor_f64(double v, uint32_t m, uint32_t lane) {
    return __longlong_as_double((long long)shfl64((uint64_t)__double_as_longlong(v), lane ^ m));
}
// compare-exchange with the lane `j` away: the lower lane of a pair keeps the larger key when `desc`
__device__ __forceinline__ uint64_t cmpx(uint64_t v, uint32_t lane, uint32_t j, bool desc) {
    const uint64_t o = shfl64(v, lane ^ j);
    const bool keepmax = ((lane & j) == 0) == desc;
    return keepmax ? std::max(v, o) : std::min(v, o);
}

// ---------------------------------------------------------------------------
// k_tr_init
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tr_init(const uint64_t* __restrict__ term_off, uint32_t ndocs, uint64_t cap,
                                                 uint32_t* __restrict__ tdoc, uint64_t* __restrict__ out,
                                                 uint32_t* __restrict__ docn) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t < ndocs) docn[t] = 0;
    if (t >= std::min(term_off[ndocs], cap)) return;
    // the last row that starts at or before t: rows are consecutive, so it is the one that holds t
    const uint64_t u = doc_ub(term_off, t, 0, (uint64_t)ndocs + 1u);
    uint32_t d = kNone;
    if (u >= 1 && u <= ndocs) {
        const uint64_t a = term_off[u - 1], b = term_off[u];
        if (a <= t && t < b && b <= cap) d = (uint32_t)(u - 1);
    }
    tdoc[t] = d;
    out[t] = 0;
}

// ---------------------------------------------------------------------------
// k_tr_setup
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tr_setup(const uint32_t* __restrict__ ids, uint64_t ids_cap,
                                                  const uint64_t* __restrict__ doc_tok,
                                                  const uint64_t* __restrict__ ntok, uint32_t ndocs,
                                                  const uint32_t* __restrict__ term_id,
                                                  const uint64_t* __restrict__ term_off, uint64_t cap,
                                                  const uint8_t* __restrict__ keep, uint32_t nkeep, uint32_t span,
                                                  uint32_t* __restrict__ node, uint16_t* __restrict__ reach,
                                                  uint64_t* __restrict__ out) {
    __shared__ uint32_t s_node[kTileMax];
    __shared__ uint16_t s_reach[kTileMax];
    __shared__ uint64_t s_j[2];
    const uint32_t th = threadIdx.x, H = span - 1u;
    const uint64_t n = std::min(*ntok, ids_cap), c0 = (uint64_t)blockIdx.x * C;
    if (c0 >= n) return;  // (tokens at or past n do not exist: nothing of theirs is read later)
    const uint64_t p0 = c0 >= H ? c0 - H : 0, p1 = std::min(n, c0 + C + H);  // the tile
    const uint32_t off0 = (uint32_t)(c0 - p0), len = (uint32_t)(p1 - p0);
    if (th < 2) s_j[th] = doc_ub(doc_tok, th == 0 ? p0 : p1 - 1u, 0, (uint64_t)ndocs + 1u);
    __syncthreads();
    const uint64_t jF = s_j[0], jL = s_j[1];
    for (uint32_t i = th; i < len; i += 256u) {
        const uint64_t p = p0 + i;
        uint32_t nd = kNone, rc = 0;
        const uint64_t u = jF < jL ? doc_ub(doc_tok, p, jF, jL) : jF;
        if (u >= 1 && u <= ndocs) {
            const uint64_t s = std::min(doc_tok[u - 1], n), e = std::min(doc_tok[u], n);
            if (s <= p && p < e) {  // (always, when doc_tok is non-decreasing)
                rc = (uint32_t)std::min<uint64_t>(H, p - s) | ((uint32_t)std::min<uint64_t>(H, e - 1u - p) << 8);
                const uint32_t id = ids[p];
                if (id != JB_VOCAB_UNK && id < nkeep && keep[id] != 0) {
                    const uint64_t a = term_off[u - 1], b = term_off[u];
                    if (a <= b && b <= cap) {  // a CSR that overflowed its arrays is not read past them
                        uint64_t lo = a, hi = b;
                        while (lo < hi) {
                            const uint64_t mid = lo + ((hi - lo) >> 1);
                            if (term_id[mid] < id) lo = mid + 1;
                            else hi = mid;
                        }
                        if (lo < b && term_id[lo] == id) nd = (uint32_t)lo;
                    }
                }
            }
        }
        s_node[i] = nd;
        s_reach[i] = (uint16_t)rc;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t q = j * 256u + th, i = off0 + q;
        if (c0 + q >= n) continue;
        const uint32_t nd = s_node[i], rc = s_reach[i];
        node[c0 + q] = nd;
        reach[c0 + q] = (uint16_t)rc;
        if (nd == kNone) continue;
        const uint32_t lo = i - (rc & 0xFFu), hi = i + (rc >> 8);  // (inside the tile: the reach is at most H)
        uint32_t deg = 0;
        for (uint32_t x = lo; x <= hi; x++) deg += x != i && s_node[x] != kNone;
        if (deg) atomicAdd((unsigned long long*)&out[nd], (unsigned long long)deg);
    }
}

// ---------------------------------------------------------------------------
// k_tr_count / k_tr_step
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tr_count(const uint32_t* __restrict__ tdoc, const uint64_t* __restrict__ out,
                                                  const uint64_t* __restrict__ term_off, uint32_t ndocs, uint64_t cap,
                                                  uint32_t* __restrict__ docn) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t d = kNone;
    if (t < std::min(term_off[ndocs], cap)) {
        d = tdoc[t];
        if (d != kNone && out[t] == 0) d = kNone;
    }
    // the wave's nodes mostly share a document: one add for those of the first node's document
    const uint64_t live = __ballot(d != kNone);
    if (live == 0) return;
    const uint32_t lead = (uint32_t)__ffsll((long long)live) - 1u;
    const uint32_t d0 = (uint32_t)__shfl((int)d, (int)lead, 64);
    const uint64_t same = __ballot(d == d0);
    if (d == d0) {
        if ((threadIdx.x & 63u) == lead) atomicAdd(&docn[d0], (uint32_t)__popcll(same));
    } else if (d != kNone) {
        atomicAdd(&docn[d], 1u);
    }
}

__global__ __launch_bounds__(256) void k_tr_step(const uint32_t* __restrict__ tdoc, const uint64_t* __restrict__ out,
                                                 const uint32_t* __restrict__ docn,
                                                 const uint64_t* __restrict__ term_off, uint32_t ndocs, uint64_t cap,
                                                 uint32_t first, uint64_t* __restrict__ r, uint64_t* __restrict__ acc) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= std::min(term_off[ndocs], cap)) return;  // (no token's node: r and acc there are never touched)
    const uint32_t d = tdoc[t];
    uint64_t rr = 0;
    if (d != kNone) {
        const uint64_t o = out[t];
        if (o != 0) {
            const uint32_t n = docn[d];  // (>= 1: this term is one of the nodes)
            const int S = scale_of(n);
            double w;
            if (first) {
                w = 1.0 / (double)n;
            } else {
                const double x = (double)acc[t] * pow2(-S);
                const double y = 0.85 * x;
                w = (1.0 - 0.85) + y;
            }
            rr = (uint64_t)((w / (double)o) * pow2(S));
        }
    }
    r[t] = rr;
    acc[t] = 0;
}

// ---------------------------------------------------------------------------
// k_tr_push / k_tr_push_win
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tr_push(const uint32_t* __restrict__ node, const uint16_t* __restrict__ reach,
                                                 uint64_t ids_cap, const uint64_t* __restrict__ ntok,
                                                 const uint64_t* __restrict__ r, uint64_t* __restrict__ acc) {
    const uint64_t n = std::min(*ntok, ids_cap), k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint32_t nd = node[k];
    if (nd == kNone) return;
    const uint32_t rc = reach[k];
    const uint64_t lo = k - (rc & 0xFFu), hi = k + (rc >> 8);  // (inside the document, so inside [0, n))
    uint64_t s = 0;
    for (uint64_t j = lo; j <= hi; j++) {
        if (j == k) continue;
        const uint32_t x = node[j];
        if (x != kNone) s += r[x];
    }
    if (s) atomicAdd((unsigned long long*)&acc[nd], (unsigned long long)s);
}

constexpr uint32_t kTrSlots = 1024;  // one per token of the chunk: 12 KiB of LDS beside the 9 KiB tile

__global__ __launch_bounds__(256) void k_tr_push_win(const uint32_t* __restrict__ node,
                                                     const uint16_t* __restrict__ reach, uint64_t ids_cap,
                                                     const uint64_t* __restrict__ ntok, uint32_t span,
                                                     const uint64_t* __restrict__ r, uint64_t* __restrict__ acc) {
    __shared__ uint64_t s_r[kTileMax];
    __shared__ uint32_t tag[kTrSlots];
    __shared__ uint64_t sum[kTrSlots];
    const uint32_t th = threadIdx.x, H = span - 1u;
    const uint64_t n = std::min(*ntok, ids_cap), c0 = (uint64_t)blockIdx.x * C;
    if (c0 >= n) return;
    const uint64_t p0 = c0 >= H ? c0 - H : 0, p1 = std::min(n, c0 + C + H);
    const uint32_t off0 = (uint32_t)(c0 - p0), len = (uint32_t)(p1 - p0);
    uint32_t mynode[4];
    for (uint32_t i = th; i < len; i += 256u) {
        const uint32_t x = node[p0 + i];
        s_r[i] = x != kNone ? r[x] : 0;  // (a token that is not kept adds nothing to a window)
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t q = j * 256u + th;
        mynode[j] = c0 + q < n ? node[c0 + q] : kNone;
        tag[q] = kNone;
        sum[q] = 0;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t nd = mynode[j];
        if (nd == kNone) continue;
        const uint32_t q = j * 256u + th, i = off0 + q, rc = reach[c0 + q];
        const uint32_t lo = i - (rc & 0xFFu), hi = i + (rc >> 8);
        uint64_t s = 0;
        for (uint32_t x = lo; x <= hi; x++) s += s_r[x];
        s -= s_r[i];
        if (s == 0) continue;
        const uint32_t slot = nd & (kTrSlots - 1u);
        uint32_t t = __hip_atomic_load(&tag[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (t == kNone) {
            t = atomicCAS(&tag[slot], kNone, nd);
            if (t == kNone) t = nd;
        }
        if (t == nd) atomicAdd((unsigned long long*)&sum[slot], (unsigned long long)s);
        else atomicAdd((unsigned long long*)&acc[nd], (unsigned long long)s);  // another node holds the slot
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t q = j * 256u + th;
        const uint64_t s = sum[q];
        if (s) atomicAdd((unsigned long long*)&acc[tag[q]], (unsigned long long)s);  // (a summed slot has a node's tag)
    }
}

// ---------------------------------------------------------------------------
// k_tr_final
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tr_final(const uint32_t* __restrict__ term_id,
                                                  const uint64_t* __restrict__ term_off, uint32_t ndocs, uint64_t cap,
                                                  const uint64_t* __restrict__ out, const uint64_t* __restrict__ acc,
                                                  const uint32_t* __restrict__ docn, uint32_t iters,
                                                  uint32_t topk, uint32_t* __restrict__ kw_id,
                                                  float* __restrict__ kw_score, uint32_t* __restrict__ kw_n) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t d = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (d >= ndocs) return;
    uint64_t a = term_off[d], b = term_off[d + 1];
    if (b > cap || a > b) a = b = 0;  // a CSR that overflowed its arrays is not read past them
    const uint32_t n = docn[d];
    uint64_t top = 0;  // lane l: the l-th best key so far, 0 = none
    if (n != 0 && a < b) {
        const int S = scale_of(n);
        const double down = pow2(-S), w0 = 1.0 / (double)n;
        // the last round's ws of node i
        auto ws_of = [&](uint64_t i) -> double {
            if (iters == 0) return w0;
            const double x = (double)acc[i] * down;
            const double y = 0.85 * x;
            return (1.0 - 0.85) + y;
        };
        // its bounds over the nodes (a lane keeps its own terms' bounds first)
        double mn = 0, mx = 0;
        bool have = false;
        for (uint64_t i = a + lane; i < b; i += 64u) {
            if (out[i] == 0) continue;
            const double w = ws_of(i);
            mn = have ? std::min(mn, w) : w;
            mx = have ? std::max(mx, w) : w;
            have = true;
        }
        // (n != 0: some lane has a node; a lane without one takes the bounds of one that has)
        const uint64_t hv = __ballot(have);
        const uint32_t src = (uint32_t)__ffsll((long long)hv) - 1u;
        const double fm = __longlong_as_double((long long)shfl64((uint64_t)__double_as_longlong(mn), src));
        const double fx = __longlong_as_double((long long)shfl64((uint64_t)__double_as_longlong(mx), src));
        if (!have) {
            mn = fm;
            mx = fx;
        }
#pragma unroll
        for (uint32_t m = 32; m > 0; m >>= 1) {
            mn = std::min(mn, shfl_xor_f64(mn, m, lane));
            mx = std::max(mx, shfl_xor_f64(mx, m, lane));
        }
        const double base = mn / 10.0, den = mx - base;
        for (uint64_t i0 = a; i0 < b; i0 += 64u) {
            const uint64_t i = i0 + lane;
            uint64_t k = 0;
            if (i < b && out[i] != 0) {
                const float sc = (float)((ws_of(i) - base) / den);
                k = ((uint64_t)__float_as_uint(sc) << 32) | (uint32_t)~term_id[i];
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
    }
    const bool got = lane < topk && top != 0;
    const uint64_t nk = __ballot(got);
    if (lane < topk) {
        const uint64_t o = d * topk + lane;
        kw_id[o] = got ? ~(uint32_t)top : JB_VOCAB_UNK;
        kw_score[o] = got ? __uint_as_float((uint32_t)(top >> 32)) : 0.0f;
    }
    if (lane == 0) kw_n[d] = (uint32_t)__popcll(nk);
}

struct TrWork {
    uint32_t *node, *tdoc, *docn;
    uint16_t* reach;
    uint64_t *out, *r, *acc;
    size_t bytes;
};

TrWork tr_layout(uint64_t max_tokens, uint64_t max_terms, uint32_t ndocs, void* p) {
    TrWork w;
    uint8_t* b = (uint8_t*)p;
    size_t off = 0;
    auto take = [&](size_t nb) -> uint8_t* {
        const size_t o = off;
        off += (std::max<size_t>(nb, 1u) + 255u) & ~(size_t)255u;
        return b ? b + o : nullptr;
    };
    w.out = (uint64_t*)take(max_terms * 8u);
    w.r = (uint64_t*)take(max_terms * 8u);
    w.acc = (uint64_t*)take(max_terms * 8u);
    w.tdoc = (uint32_t*)take(max_terms * 4u);
    w.node = (uint32_t*)take(max_tokens * 4u);
    w.docn = (uint32_t*)take((size_t)ndocs * 4u);
    w.reach = (uint16_t*)take(max_tokens * 2u);
    w.bytes = off;
    return w;
}

}  // namespace

size_t textrank_work_bytes(uint64_t max_tokens, uint64_t max_terms, uint32_t ndocs) {
    return tr_layout(max_tokens, max_terms, ndocs, nullptr).bytes;
}

hipError_t run_textrank(const uint32_t* d_ids, uint64_t ids_cap, const uint64_t* d_doc_tok, const uint64_t* d_ntok,
                        uint32_t ndocs, const uint32_t* d_term_id, const uint64_t* d_term_off, uint64_t cap,
                        const uint8_t* d_keep, uint32_t nkeep, uint32_t span, uint32_t iters, uint32_t topk,
                        bool window, uint32_t* d_kw_id, float* d_kw_score, uint32_t* d_kw_n, void* d_work,
                        hipStream_t stream, KernelTimer* timer) {
    const TrWork w = tr_layout(ids_cap, cap, ndocs, d_work);
    const uint32_t gterm = (uint32_t)((cap + 255u) / 256u);
    const uint32_t ginit = (uint32_t)((std::max<uint64_t>(cap, ndocs) + 255u) / 256u);
    const uint32_t gchunk = (uint32_t)((ids_cap + C - 1u) / C), gtok = (uint32_t)((ids_cap + 255u) / 256u);
    JB_TIMED(K_TR_INIT,
             hipLaunchKernelGGL(k_tr_init, dim3(ginit), dim3(256), 0, stream, d_term_off, ndocs, cap, w.tdoc, w.out, w.docn));
    if (gchunk && gterm) {
        JB_TIMED(K_TR_SETUP,
                 hipLaunchKernelGGL(k_tr_setup, dim3(gchunk), dim3(256), 0, stream, d_ids, ids_cap, d_doc_tok, d_ntok, ndocs,
                                    d_term_id, d_term_off, cap, d_keep, nkeep, span, w.node, w.reach, w.out));
        JB_TIMED(K_TR_COUNT, hipLaunchKernelGGL(k_tr_count, dim3(gterm), dim3(256), 0, stream, w.tdoc, w.out, d_term_off,
                                                ndocs, cap, w.docn));
        for (uint32_t it = 0; it < iters; it++) {
            JB_TIMED(K_TR_STEP, hipLaunchKernelGGL(k_tr_step, dim3(gterm), dim3(256), 0, stream, w.tdoc, w.out, w.docn,
                                                   d_term_off, ndocs, cap, it == 0 ? 1u : 0u, w.r, w.acc));
            if (window)
                JB_TIMED(K_TR_PUSH, hipLaunchKernelGGL(k_tr_push_win, dim3(gchunk), dim3(256), 0, stream, w.node, w.reach,
                                                       ids_cap, d_ntok, span, w.r, w.acc));
            else
                JB_TIMED(K_TR_PUSH, hipLaunchKernelGGL(k_tr_push, dim3(gtok), dim3(256), 0, stream, w.node, w.reach, ids_cap,
                                                       d_ntok, w.r, w.acc));
        }
    }
    const uint32_t gdoc = (uint32_t)(((uint64_t)ndocs + 3u) / 4u);
    JB_TIMED(K_TR_FINAL, hipLaunchKernelGGL(k_tr_final, dim3(gdoc), dim3(256), 0, stream, d_term_id, d_term_off, ndocs, cap,
                                            w.out, w.acc, w.docn, iters, topk, d_kw_id, d_kw_score, d_kw_n));
    return hipGetLastError();
}

}  // namespace jb
