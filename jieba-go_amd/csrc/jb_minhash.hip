// jb_minhash.hip — gfx950 kernels of the MinHash signatures (jb_minhash_device, jb_minhash_bands_device; the
// rule is jb_minhash's, jb_minhash.cpp; the code shared with the host is jb_minhash.h's).
//
// A span list of any mode and its per-document offsets become K u32 slots per document: the least value of
// hash function j over the document's shingles of n consecutive tokens.  n_t = min(*ntok, cap) tokens take part.
//   k_mh_init  every slot of sig = JB_MH_EMPTY, and doc_n from doc_tok alone (a grid-stride loop).
//   k_mh_hash  one lane per token (k_ids' tile loop): the key in registers from aligned dwords (k_wc_*'s
//              reads), cut to 255 bytes, empty for a malformed span; work[k] = jb_vocab_hash of it.
//   k_mh_sig   the minima.  A shingle belongs to its first token k, whose document d comes from a search over
//              doc_tok; it exists when k + n <= the document's end, or when k is the first of fewer than n
//              tokens.  Two forms with identical bits (a minimum does not depend on the order):
//              plain   one lane per token folds its shingle from work[] and walks the K functions: a load of
//                      the slot, and an atomicMin only where the value is below what the load shows (a
//                      stale load costs an atomic, never a result: slots only fall).
//              staged  one workgroup per tile of kMhTile tokens: the tile's hashes and a halo of n - 1 go to
//                      LDS, then each shingle's x and document.  A lane owns function j = thread % Kw for
//                      one share of the tile's shingles (Kw = K rounded up to whole waves, 256 / Kw shares),
//                      so a wave reads one LDS address at a time, a broadcast; it keeps a running minimum
//                      per run of one document and flushes it with one atomicMin.
// No lane waits for another.  Text bytes are read only for spans with start < end <= nbytes, in
// [start & ~3, start + 28) or inside the span: never at or past nbytes + 64.  Every write index into sig
// and doc_n is a document index below ndocs; work[] is written below n_t only.
#include <hip/hip_runtime.h>

#include "jb_kstages.h"
#include "jb_minhash.h"
#include "jiebahip.h"

#include <algorithm>

namespace jb {

namespace {

constexpr uint32_t T = kMhTile;
constexpr uint32_t PER = T / 256u;  // shingles per thread of the staging
static_assert(kMhTile == JB_MH_TILE && kMhMaxN == JB_MH_MAXN && kMhMaxK == JB_MH_MAXK, "the header's constants");
static_assert(T % 1024u == 0, "a share of the tile is whole for 1, 2 and 4 shares");

// First j in [lo, hi) with doc_tok[j] > k, else hi (k_join_write's search).
__device__ __forceinline__ uint64_t doc_ub(const uint64_t* __restrict__ doc_tok, uint64_t k, uint64_t lo, uint64_t hi) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (doc_tok[mid] > k) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ uint32_t mh_word_mask(uint32_t len, uint32_t w) {
    if (len >= 4u * w + 4u) return 0xFFFFFFFFu;
    return len > 4u * w ? (1u << (8u * (len - 4u * w))) - 1u : 0u;
}

// The hash of span [s, e)'s key.  k_wc_claim's reads; a malformed span reads nothing.
__device__ __forceinline__ uint64_t mh_token(const uint8_t* __restrict__ text, uint32_t nbytes, uint32_t s, uint32_t e) {
    uint32_t kw[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (s >= e || e > nbytes) return jb_vocab_hash(kw, text, 0u);
    uint32_t len = std::min(e - s, (uint32_t)JB_VOCAB_MAXKEY);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(text + (s & ~3u));
    const uint32_t sh = s & 3u;
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
    if (len == 1u && (kw[0] & 0x80u)) {  // an invalid UTF-8 byte: the key is "\xEF\xBF\xBD"
        kw[0] = 0x00BDBFEFu;
        kw[1] = 0u;
        len = 3u;
    } else {
#pragma unroll
        for (uint32_t w = 0; w < 6u; w++) kw[w] &= mh_word_mask(len, w);
    }
    return jb_vocab_hash(kw, text + s, len);
}

__global__ __launch_bounds__(256) void k_mh_init(const uint64_t* __restrict__ doc_tok, const uint64_t* __restrict__ ntok,
                                                 uint64_t cap, uint32_t ndocs, uint32_t nn, uint32_t K,
                                                 uint32_t* __restrict__ sig, uint32_t* __restrict__ doc_n) {
    const uint64_t n = std::min(*ntok, cap);
    const uint64_t stride = (uint64_t)gridDim.x * 256u, first = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t nslots = (uint64_t)ndocs * K;
    for (uint64_t i = first; i < nslots; i += stride) sig[i] = JB_MH_EMPTY;
    for (uint64_t d = first; d < ndocs; d += stride) {
        const uint64_t lo = std::min(doc_tok[d], n), hi = std::min(doc_tok[d + 1], n);
        doc_n[d] = jb_mh_count(hi > lo ? hi - lo : 0u, nn);
    }
}

__global__ __launch_bounds__(256) void k_mh_hash(const uint8_t* __restrict__ text, uint32_t nbytes,
                                                 const uint32_t* __restrict__ ts, const uint32_t* __restrict__ te,
                                                 const uint64_t* __restrict__ ntok, uint64_t cap,
                                                 uint64_t* __restrict__ work) {
    const uint64_t n = std::min(*ntok, cap), step = (uint64_t)gridDim.x * 256u;
    uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t s1 = 0, e1 = 0;  // (the next span is loaded one trip ahead)
    if (i < n) {
        s1 = ts[i];
        e1 = te[i];
    }
    for (; i < n; i += step) {
        const uint32_t s = s1, e = e1;
        if (i + step < n) {
            s1 = ts[i + step];
            e1 = te[i + step];
        }
        work[i] = mh_token(text, nbytes, s, e);
    }
}

// The shingle that starts at token k (k < n): its document and the tokens it folds, or c = 0 when there is
// none.  u is doc_ub(k): k's document is u - 1.  Whatever doc_tok holds, *d < ndocs and k + c <= n.
__device__ __forceinline__ uint32_t mh_shingle_of(const uint64_t* __restrict__ doc_tok, uint64_t k, uint64_t u,
                                                  uint64_t n, uint32_t ndocs, uint32_t nn, uint32_t* d) {
    if (u == 0 || u > ndocs) return 0u;  // (before the first document or past the last)
    *d = (uint32_t)(u - 1u);
    const uint64_t lo = std::min(doc_tok[u - 1u], n), hi = std::min(doc_tok[u], n);
    if (k < lo || k >= hi) return 0u;  // (doc_tok out of order)
    if (k + nn <= hi) return nn;
    return k == lo ? (uint32_t)(hi - lo) : 0u;  // (fewer than n tokens: one shingle over all of them)
}

__global__ __launch_bounds__(256) void k_mh_sig_plain(const uint64_t* __restrict__ doc_tok,
                                                      const uint64_t* __restrict__ ntok, uint64_t cap, uint32_t ndocs,
                                                      uint32_t nn, uint32_t K, uint64_t seed,
                                                      const uint64_t* __restrict__ work, uint32_t* __restrict__ sig) {
    const uint64_t n = std::min(*ntok, cap);
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    uint32_t d = 0;
    const uint32_t c = mh_shingle_of(doc_tok, k, doc_ub(doc_tok, k, 0, (uint64_t)ndocs + 1u), n, ndocs, nn, &d);
    if (c == 0u) return;
    uint64_t t[kMhMaxN];
#pragma unroll
    for (uint32_t i = 0; i < kMhMaxN; i++) t[i] = i < c ? work[k + i] : 0u;
    const uint32_t x = jb_mh_shingle(t, c);
    uint32_t* row = sig + (uint64_t)d * K;
    for (uint32_t j = 0; j < K; j++) {
        const uint32_t v = jb_mh_slot(jb_mh_a(seed, j), jb_mh_b(seed, j), x);
        if (v < row[j]) atomicMin(&row[j], v);
    }
}

constexpr uint32_t kNoDoc = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void k_mh_sig_staged(const uint64_t* __restrict__ doc_tok,
                                                       const uint64_t* __restrict__ ntok, uint64_t cap, uint32_t ndocs,
                                                       uint32_t nn, uint32_t K, uint64_t seed,
                                                       const uint64_t* __restrict__ work, uint32_t* __restrict__ sig) {
    __shared__ uint64_t s_t[T + kMhMaxN];  // the tile's token hashes and the halo
    __shared__ uint32_t s_x[T];            // x of the shingle that starts at each token
    __shared__ uint32_t s_doc[T];          // its document, or kNoDoc
    __shared__ uint64_t s_d[2];
    const uint32_t th = threadIdx.x;
    const uint64_t n = std::min(*ntok, cap), t0 = (uint64_t)blockIdx.x * T;
    if (t0 >= n) return;
    const uint64_t hi_k = std::min(t0 + T, n);
    for (uint32_t i = th; i < T + nn - 1u; i += 256u) s_t[i] = t0 + i < n ? work[t0 + i] : 0u;
    if (th == 0) {
        // token k's document is doc_ub(k) - 1, and doc_ub(k) lies in [s_d[0], s_d[1]] for the tile's tokens
        s_d[0] = doc_ub(doc_tok, t0, 0, (uint64_t)ndocs + 1u);
        s_d[1] = doc_ub(doc_tok, hi_k - 1u, s_d[0], (uint64_t)ndocs + 1u);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t p = 0; p < PER; p++) {
        const uint32_t i = p * 256u + th;
        const uint64_t k = t0 + i;
        uint32_t d = kNoDoc, c = 0u;
        if (k < n) c = mh_shingle_of(doc_tok, k, doc_ub(doc_tok, k, s_d[0], s_d[1]), n, ndocs, nn, &d);
        s_doc[i] = c ? d : kNoDoc;
        s_x[i] = c ? jb_mh_shingle(&s_t[i], c) : 0u;  // (i + c <= T + nn - 1: the halo holds the tokens)
    }
    __syncthreads();
    // thread th owns function j for the share `part` of the tile; a wave's lanes have one `part`
    const uint32_t Kw = K <= 64u ? 64u : K <= 128u ? 128u : 256u, share = T / (256u / Kw);
    const uint32_t j = th % Kw, part = th / Kw;
    if (j >= K) return;
    const uint64_t a = jb_mh_a(seed, j), b = jb_mh_b(seed, j);
    const uint32_t i1 = (uint32_t)std::min<uint64_t>((uint64_t)(part + 1u) * share, hi_k - t0);
    uint32_t cur = kNoDoc, mn = JB_MH_EMPTY;
    for (uint32_t i = part * share; i < i1; i++) {
        const uint32_t d = s_doc[i];
        if (d != cur) {
            if (cur != kNoDoc) atomicMin(&sig[(uint64_t)cur * K + j], mn);
            cur = d;
            mn = JB_MH_EMPTY;
        }
        if (d != kNoDoc) mn = std::min(mn, jb_mh_slot(a, b, s_x[i]));
    }
    if (cur != kNoDoc) atomicMin(&sig[(uint64_t)cur * K + j], mn);
}

__global__ __launch_bounds__(256) void k_mh_bands(const uint32_t* __restrict__ sig, const uint32_t* __restrict__ doc_n,
                                                  uint32_t ndocs, uint32_t K, uint32_t B, uint32_t R,
                                                  uint64_t* __restrict__ keys) {
    const uint64_t total = (uint64_t)ndocs * B, stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += stride) {
        const uint64_t d = i / B;
        keys[i] = doc_n[d] ? jb_mh_band(sig + d * K, (uint32_t)(i - d * B), R) : JB_MH_NOKEY;
    }
}

}  // namespace

hipError_t run_minhash(const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start, const uint32_t* d_end,
                       const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint64_t cap, uint32_t ndocs, uint32_t n,
                       uint32_t K, uint64_t seed, bool staged, uint32_t* d_sig, uint32_t* d_doc_n, uint64_t* d_work,
                       uint32_t ncu, hipStream_t stream, KernelTimer* timer) {
    const uint32_t cus = std::max(1u, ncu);
    const uint64_t nslots = std::max<uint64_t>((uint64_t)ndocs * K, 1u);
    const uint32_t g0 = (uint32_t)std::min<uint64_t>((nslots + 255u) / 256u, (uint64_t)cus * 8u);
    JB_TIMED(K_MH_INIT, hipLaunchKernelGGL(k_mh_init, dim3(g0), dim3(256), 0, stream, d_doc_tok, d_ntok, cap, ndocs, n, K,
                                           d_sig, d_doc_n));
    if (cap == 0 || ndocs == 0) return hipGetLastError();  // (no token takes part, or no slot receives one)
    const uint32_t g1 = (uint32_t)std::min<uint64_t>((cap + 255u) / 256u, (uint64_t)cus * kIdsWgPerCu);
    JB_TIMED(K_MH_HASH, hipLaunchKernelGGL(k_mh_hash, dim3(g1), dim3(256), 0, stream, d_text, (uint32_t)nbytes, d_start,
                                           d_end, d_ntok, cap, d_work));
    if (staged) {
        const uint32_t g2 = (uint32_t)((cap + T - 1u) / T);
        JB_TIMED(K_MH_SIG, hipLaunchKernelGGL(k_mh_sig_staged, dim3(g2), dim3(256), 0, stream, d_doc_tok, d_ntok, cap,
                                              ndocs, n, K, seed, d_work, d_sig));
    } else {
        const uint32_t g2 = (uint32_t)((cap + 255u) / 256u);
        JB_TIMED(K_MH_SIG, hipLaunchKernelGGL(k_mh_sig_plain, dim3(g2), dim3(256), 0, stream, d_doc_tok, d_ntok, cap,
                                              ndocs, n, K, seed, d_work, d_sig));
    }
    return hipGetLastError();
}

hipError_t run_minhash_bands(const uint32_t* d_sig, const uint32_t* d_doc_n, uint32_t ndocs, uint32_t K, uint32_t B,
                             uint32_t R, uint64_t* d_keys, uint32_t ncu, hipStream_t stream, KernelTimer* timer) {
    const uint64_t total = std::max<uint64_t>((uint64_t)ndocs * B, 1u);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((total + 255u) / 256u, (uint64_t)std::max(1u, ncu) * 8u);
    JB_TIMED(K_MH_BANDS, hipLaunchKernelGGL(k_mh_bands, dim3(grid), dim3(256), 0, stream, d_sig, d_doc_n, ndocs, K, B, R,
                                            d_keys));
    return hipGetLastError();
}

}  // namespace jb
