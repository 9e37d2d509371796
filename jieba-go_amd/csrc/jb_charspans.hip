// jb_charspans.hip — gfx950 kernels of the character-offset call (jb_charspans_device; the rule is
// jb_charspans', jb_charspans.cpp).
//
// Byte spans become spans in runes or in UTF-16 code units, per document.  With S the bitmap of rune starts
// (one u64 word per 64 text bytes), A the bitmap of the starts that count 2 (UTF-16: valid runes of four
// bytes), P[w] the units of the words before w inside w's tile and B[t] the units of the tiles before t,
//   pos(p) = B[p >> 12] + P[p >> 6] + popc(S[p >> 6] & below(p)) + popc(A[p >> 6] & below(p))
// is the number of units that start before byte p in the whole batch, and a token [s, e) of document d is
// [pos(s) - pos(doc_off[d]), pos(e) - pos(doc_off[d])).
//
// Whether a byte starts a rune is a local question.  A byte below 0x80 or from 0xC0 on always does: Go's
// DecodeRune skips only the tail of a valid sequence, and tails are continuation bytes.  So every lead byte
// is decoded exactly where it stands, with the bytes left in its document as the limit, and the bytes it
// covers are the only ones that start nothing.  A lane therefore needs its 16 bytes, the three before them,
// the three after them and the document boundaries among those, and nothing else.
//   k_cs_class   one workgroup per tile of kCsTile bytes: the tile and its halo staged in LDS, the document
//                boundaries that fall into it as bits in LDS (two searches over doc_off per workgroup; of
//                equal offsets only the first is marked), S, A and the tile-local P, and the tile's sum.
//   k_cs_scan    one workgroup: B, the exclusive scan of the tile sums.  No workgroup waits for another.
//   k_cs_lookup  one lane per token: its document by a search over the doc_tok entries of its workgroup's
//                tokens, three positions, two stores; the workgroups past the token tiles write doc_units,
//                one lane per document.
// No text byte at or past nbytes rounded up to 4 is read.  Always 3 launches; nothing here synchronises,
// allocates or reads on the host.
#include "jb_kdev.h"
#include "jb_kstages.h"

#include <algorithm>

namespace jb {

namespace {

constexpr uint32_t T = kCsTile;
constexpr uint32_t WPT = T / 64u;  // bitmap words per tile
constexpr uint32_t TT = kCsTokTile;
constexpr uint32_t PER = TT / 256u;  // tokens per lane
constexpr uint32_t kHead = 4;        // staged bytes before the tile (3 are needed; 4 keeps dwords aligned)
constexpr uint32_t kStage = T + 16u; // staged bytes: the head, the tile, 3 after it, and lds4's 8-byte reach
constexpr uint32_t kNone = 0xFFFFFFFFu;  // JB_CHAR_NONE
static_assert(T == 256u * 16u && WPT == 64u, "a lane takes 16 bytes, and wave 0 one bitmap word per lane");

// First j in [lo, hi) with a[j] >= v, else hi.
__device__ __forceinline__ uint64_t lower_bound64(const uint64_t* __restrict__ a, uint64_t v, uint64_t lo, uint64_t hi) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] >= v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// First j in [lo, hi) with doc_tok[j] > k, else hi (k_join_write's search).
__device__ __forceinline__ uint64_t doc_ub(const uint64_t* __restrict__ doc_tok, uint64_t k, uint64_t lo, uint64_t hi) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (doc_tok[mid] > k) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// ---------------------------------------------------------------------------
// k_cs_class
// ---------------------------------------------------------------------------
template <bool UTF16>
__global__ __launch_bounds__(256) void k_cs_class(const uint8_t* __restrict__ text, uint64_t nbytes,
                                                  const uint64_t* __restrict__ doc_off, uint32_t ndocs,
                                                  uint64_t* __restrict__ S, uint64_t* __restrict__ A,
                                                  uint32_t* __restrict__ P, uint32_t* __restrict__ tilesum) {
    __shared__ __attribute__((aligned(16))) uint32_t tx[kStage / 4u];  // staged byte r is text byte t0 - kHead + r
    __shared__ uint32_t bnd[kStage / 32u + 2u];                        // bit r: a document boundary at that byte
    __shared__ __attribute__((aligned(8))) uint16_t sS[256], sA[256];  // a lane's 16 bits; four lanes make a word
    __shared__ uint64_t s_d[2];
    const uint32_t th = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * T;
    // the bytes [lo, hi) are staged (lo is t0 - kHead but for the first tile)
    const uint64_t lo = t0 >= kHead ? t0 - kHead : 0u, hi = t0 + (kStage - kHead);
    for (uint32_t q = th; q < kStage / 4u; q += 256u) {
        const uint64_t g = t0 + 4u * q;  // (the dword's text offset + kHead)
        tx[q] = (g >= kHead && g - kHead < nbytes) ? ((const uint32_t*)text)[(g - kHead) >> 2] : 0u;
    }
    for (uint32_t q = th; q < kStage / 32u + 2u; q += 256u) bnd[q] = 0;
    if (th == 0) {
        s_d[0] = lower_bound64(doc_off, lo, 0, (uint64_t)ndocs + 1u);
        s_d[1] = lower_bound64(doc_off, hi, s_d[0], (uint64_t)ndocs + 1u);
    }
    __syncthreads();
    for (uint64_t d = s_d[0] + th; d < s_d[1]; d += 256u) {
        const uint64_t o = doc_off[d];
        if (o < lo || o >= hi) continue;                // (doc_off out of order)
        if (d > s_d[0] && doc_off[d - 1u] == o) continue;  // (empty documents at one offset: one bit)
        const uint32_t r = (uint32_t)(o + kHead - t0);
        atomicOr(&bnd[r >> 5], 1u << (r & 31u));
    }
    if (th == 0 && nbytes >= lo && nbytes < hi) {  // the text's end bounds the last document whatever doc_off says
        const uint32_t r = (uint32_t)(nbytes + kHead - t0);
        atomicOr(&bnd[r >> 5], 1u << (r & 31u));
    }
    __syncthreads();
    // The lane's bytes are the staged bytes r0 + 3 .. r0 + 18; the leads that can cover one of them stand at
    // r0 .. r0 + 18.  Bit j of the masks below is the staged byte r0 + j.
    const uint8_t* txb = (const uint8_t*)tx;
    const uint32_t r0 = th * 16u + (kHead - 3u);
    const uint32_t bw = r0 >> 5;
    const uint32_t win = (uint32_t)((((uint64_t)bnd[bw + 1u] << 32) | bnd[bw]) >> (r0 & 31u));  // boundaries at r0 + j
    uint32_t tail = 0, two = 0;
#pragma unroll
    for (uint32_t j = 0; j < 19u; j++) {
        if (txb[r0 + j] < 0xC0u) continue;
        const uint32_t b3 = (win >> (j + 1u)) & 7u;  // boundaries 1, 2 and 3 bytes after the lead
        const uint32_t lim = (b3 & 1u) ? 1u : (b3 & 2u) ? 2u : (b3 & 4u) ? 3u : 4u;
        uint32_t rune;
        const uint32_t w = dec_lead(lds4(txb, r0 + j), lim, &rune);
        tail |= ((1u << w) - 2u) << j;  // the bytes j + 1 .. j + w - 1
        if (UTF16 && w == 4u) two |= 1u << j;  // (a valid four-byte form is U+10000 or above)
    }
    const uint64_t i0 = t0 + th * 16u;
    const uint32_t have = i0 >= nbytes ? 0u : (uint32_t)std::min<uint64_t>(16u, nbytes - i0);
    const uint32_t live = (1u << have) - 1u;
    sS[th] = (uint16_t)(~(tail >> 3) & live);
    sA[th] = (uint16_t)((two >> 3) & live);
    __syncthreads();
    if (th < WPT) {  // (wave 0: one bitmap word per lane)
        const uint64_t s = ((const uint64_t*)sS)[th], a = UTF16 ? ((const uint64_t*)sA)[th] : 0ull;
        const uint32_t cnt = (uint32_t)__popcll(s) + (uint32_t)__popcll(a);
        const uint32_t inc = wave_incl_scan(cnt);
        const uint64_t w = (uint64_t)blockIdx.x * WPT + th;
        S[w] = s;
        if (UTF16) A[w] = a;
        P[w] = inc - cnt;
        if (th == WPT - 1u) tilesum[blockIdx.x] = inc;
    }
}

// ---------------------------------------------------------------------------
// k_cs_scan: one workgroup; tilebase[i] = the sum of tilesum[0 .. i), ntl + 1 entries, 4 tiles per lane a trip
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_cs_scan(const uint32_t* __restrict__ tilesum, uint64_t ntl,
                                                  uint32_t* __restrict__ tilebase) {
    __shared__ uint32_t sh[16];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint64_t c0 = 0; c0 < ntl; c0 += 4096u) {
        const uint64_t i = c0 + 4u * threadIdx.x;
        uint32_t v[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) v[k] = i + k < ntl ? tilesum[i + k] : 0u;
        const uint32_t sum = v[0] + v[1] + v[2] + v[3];
        const uint32_t inc = wave_incl_scan(sum);
        __syncthreads();  // (sh may still be read from the trip before)
        if (lane == 63u) sh[wv] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t x = sh[k];
            if (k < wv) before += x;
            all += x;
        }
        uint32_t run = carry + before + inc - sum;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            if (i + k < ntl) tilebase[i + k] = run;
            run += v[k];
        }
        carry += all;
    }
    if (threadIdx.x == 0) tilebase[ntl] = carry;
}

// ---------------------------------------------------------------------------
// k_cs_lookup
// ---------------------------------------------------------------------------
template <bool UTF16>
__device__ __forceinline__ uint32_t cs_pos(const uint64_t* __restrict__ S, const uint64_t* __restrict__ A,
                                           const uint32_t* __restrict__ P, const uint32_t* __restrict__ tilebase,
                                           uint64_t p) {
    const uint64_t w = p >> 6, below = (1ull << (p & 63u)) - 1ull;
    uint32_t r = tilebase[p / T] + P[w] + (uint32_t)__popcll(S[w] & below);
    if (UTF16) r += (uint32_t)__popcll(A[w] & below);
    return r;
}

// (start / cstart and end / cend may be the same arrays: no __restrict__ on them, and a lane reads its
// token's two inputs before it writes its two outputs)
template <bool UTF16>
__global__ __launch_bounds__(256) void k_cs_lookup(const uint64_t* __restrict__ S, const uint64_t* __restrict__ A,
                                                   const uint32_t* __restrict__ P,
                                                   const uint32_t* __restrict__ tilebase, uint64_t nbytes,
                                                   const uint64_t* __restrict__ doc_off, uint32_t ndocs,
                                                   const uint32_t* start, const uint32_t* end,
                                                   const uint64_t* __restrict__ doc_tok,
                                                   const uint64_t* __restrict__ ntok, uint64_t cap, uint32_t ntb,
                                                   uint32_t* cstart, uint32_t* cend,
                                                   uint32_t* __restrict__ doc_units) {
    __shared__ uint64_t s_d[2];
    const uint32_t th = threadIdx.x;
    if (blockIdx.x >= ntb) {  // a document tile: the documents' lengths
        const uint64_t d = (uint64_t)(blockIdx.x - ntb) * 256u + th;
        if (d >= ndocs) return;
        const uint64_t so = doc_off[d], eo = doc_off[d + 1u];
        doc_units[d] = (so <= eo && eo <= nbytes)
                           ? cs_pos<UTF16>(S, A, P, tilebase, eo) - cs_pos<UTF16>(S, A, P, tilebase, so)
                           : 0u;
        return;
    }
    const uint64_t n = std::min(*ntok, cap), t0 = (uint64_t)blockIdx.x * TT;
    if (t0 >= n) return;
    const uint64_t hi_k = std::min(t0 + TT, n);
    if (th == 0) {
        // token k's document is doc_ub(k) - 1, and doc_ub(k) lies in [s_d[0], s_d[1]] for the tile's tokens
        s_d[0] = doc_ub(doc_tok, t0, 0, (uint64_t)ndocs + 1u);
        s_d[1] = doc_ub(doc_tok, hi_k - 1u, s_d[0], (uint64_t)ndocs + 1u);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        const uint64_t k = t0 + j * 256u + th;
        if (k >= n) continue;
        const uint64_t s = start[k], e = end[k];
        uint32_t cs = kNone, ce = kNone;
        const uint64_t u = doc_ub(doc_tok, k, s_d[0], s_d[1]);
        if (u != 0 && u <= ndocs) {  // (else before the first document or past the last)
            const uint64_t so = doc_off[u - 1u], eo = doc_off[u];
            if (so <= s && s <= e && e <= eo && eo <= nbytes) {
                const uint32_t base = cs_pos<UTF16>(S, A, P, tilebase, so);
                cs = cs_pos<UTF16>(S, A, P, tilebase, s) - base;
                ce = cs_pos<UTF16>(S, A, P, tilebase, e) - base;
            }
        }
        cstart[k] = cs;
        cend[k] = ce;
    }
}

struct CsWork {
    uint64_t ntl;  // tiles: the byte nbytes itself has a word, so that pos(nbytes) reads inside the arrays
    uint64_t *S, *A;
    uint32_t *P, *tilesum, *tilebase;
    size_t bytes;
};

CsWork cs_layout(uint64_t nbytes, void* p) {
    CsWork w;
    w.ntl = nbytes / T + 1u;
    const size_t nw = (size_t)w.ntl * WPT;
    uint8_t* b = (uint8_t*)p;
    size_t off = 0;
    auto take = [&](size_t nb) -> void* {
        const size_t o = off;
        off += (nb + 255u) & ~(size_t)255u;
        return b ? (void*)(b + o) : nullptr;
    };
    w.S = (uint64_t*)take(nw * 8u);
    w.A = (uint64_t*)take(nw * 8u);
    w.P = (uint32_t*)take(nw * 4u);
    w.tilesum = (uint32_t*)take((size_t)w.ntl * 4u);
    w.tilebase = (uint32_t*)take(((size_t)w.ntl + 1u) * 4u);
    w.bytes = off;
    return w;
}

}  // namespace

size_t charspans_work_bytes(uint64_t nbytes, uint32_t) { return cs_layout(nbytes, nullptr).bytes; }

hipError_t run_charspans(const uint8_t* d_text, uint64_t nbytes, const uint64_t* d_doc_off, uint32_t ndocs,
                         const uint32_t* d_start, const uint32_t* d_end, const uint64_t* d_doc_tok,
                         const uint64_t* d_ntok, uint64_t cap, bool utf16, uint32_t* d_cstart, uint32_t* d_cend,
                         uint32_t* d_doc_units, void* d_work, hipStream_t stream, KernelTimer* timer) {
    const CsWork w = cs_layout(nbytes, d_work);
    const uint32_t ntl = (uint32_t)w.ntl;
    const uint32_t ntb = (uint32_t)((cap + TT - 1u) / TT), ndb = (uint32_t)(((uint64_t)ndocs + 255u) / 256u);
    const uint32_t grid = std::max(1u, ntb + ndb);
    if (utf16) {
        JB_TIMED(K_CS_CLASS, hipLaunchKernelGGL(k_cs_class<true>, dim3(ntl), dim3(256), 0, stream, d_text, nbytes, d_doc_off,
                                                ndocs, w.S, w.A, w.P, w.tilesum));
    } else {
        JB_TIMED(K_CS_CLASS, hipLaunchKernelGGL(k_cs_class<false>, dim3(ntl), dim3(256), 0, stream, d_text, nbytes,
                                                d_doc_off, ndocs, w.S, w.A, w.P, w.tilesum));
    }
    JB_TIMED(K_CS_SCAN, hipLaunchKernelGGL(k_cs_scan, dim3(1), dim3(1024), 0, stream, w.tilesum, w.ntl, w.tilebase));
    if (utf16) {
        JB_TIMED(K_CS_LOOKUP, hipLaunchKernelGGL(k_cs_lookup<true>, dim3(grid), dim3(256), 0, stream, w.S, w.A, w.P,
                                                 w.tilebase, nbytes, d_doc_off, ndocs, d_start, d_end, d_doc_tok, d_ntok,
                                                 cap, ntb, d_cstart, d_cend, d_doc_units));
    } else {
        JB_TIMED(K_CS_LOOKUP, hipLaunchKernelGGL(k_cs_lookup<false>, dim3(grid), dim3(256), 0, stream, w.S, w.A, w.P,
                                                 w.tilebase, nbytes, d_doc_off, ndocs, d_start, d_end, d_doc_tok, d_ntok,
                                                 cap, ntb, d_cstart, d_cend, d_doc_units));
    }
    return hipGetLastError();
}

}  // namespace jb
