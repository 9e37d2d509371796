// jb_join.hip — gfx950 kernels of the joined-text call (jb_join_device; the rule is jb_join's, jb_join.cpp).
//
// A span list of any mode, its per-document offsets, a separator and a terminator become one contiguous
// buffer: per document key_0 sep key_1 ... key_{n-1} term.  With L[k] = len(key_k) + seplen and A its
// exclusive scan over the tokens k < n = min(*ntok, cap), E[d] the number of non-empty documents before
// d and a_d = min(doc_tok[d], n),
//   out_doc_off[d] = A[a_d] - A[a_0] + d * termlen - seplen * E[d]
//   token k of document d starts at A[k] + D[d],  D[d] = out_doc_off[d] - A[a_d]
// and the separator follows every token but a document's last.  Tile = kJoinTile consecutive tokens, one
// workgroup each, whatever documents they belong to; thread t owns the tokens j * 256 + t of its tile.
//   k_join_count  per tile the sum of L (tilesum), and for every document whose first token lies in the
//                 tile the sum of L before that token inside the tile (aloc); the workgroups past the
//                 token tiles count the non-empty documents of 256 documents each (doccnt).
//   k_join_scan   one workgroup: the exclusive scans of tilesum and doccnt.  No workgroup waits for
//                 another anywhere here.
//   k_join_doc    one thread per document: out_doc_off, D, *nout and the document's terminator.
//   k_join_write  the keys and separators of a tile.  It scans L again (the spans are read anyway), finds
//                 each token's document by a search over the few doc_tok entries of its tile, and then
//                 either copies byte by byte, one lane per token (the plain form), or assembles the
//                 tile's output in LDS, kJoinStage bytes at a time, with one bit per staged byte, and
//                 streams it out: 16 bytes per store where all 16 bits of an aligned unit are set, byte
//                 by byte elsewhere (a tile's head and tail, the neighbours of a terminator, the edge
//                 of out_cap), so no byte is written that the tile does not own.  Keys of kJoinLong
//                 bytes or more are not staged: the workgroup copies them from the text together.
// Text bytes are read only inside spans with start < end <= nbytes; output bytes are written only below
// out_cap.  Nothing here synchronises, allocates or reads on the host; there are always 4 launches.
#include <hip/hip_runtime.h>

#include "jb_kstages.h"

#include <algorithm>

namespace jb {

namespace {

constexpr uint32_t T = kJoinTile;
constexpr uint32_t PER = T / 256u;  // tokens per thread
constexpr uint32_t CH = kJoinStage;
constexpr uint32_t kMaskWords = CH / 32u;
constexpr uint32_t kDocTile = 256;  // documents per workgroup of the document passes
static_assert(T == 2048, "the tile scan reads 8 consecutive lengths per thread as two uint4");
static_assert(CH % 512u == 0 && CH >= (T + 1u) * 8u, "the staging buffer also holds the tile scan");
static_assert(kJoinLong > 3, "a replaced byte is never a long key");

// First j in [lo, hi) with doc_tok[j] > k, else hi.
__device__ __forceinline__ uint64_t doc_ub(const uint64_t* __restrict__ doc_tok, uint64_t k, uint64_t lo, uint64_t hi) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (doc_tok[mid] > k) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, uint32_t o) {
    const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

// Exclusive scan of one u64 per thread over a workgroup of NW waves; *total receives the sum.
template <uint32_t NW>
__device__ __forceinline__ uint64_t block_excl64(uint64_t v, uint64_t* sh /* NW */, uint64_t* total) {
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
    for (uint32_t k = 0; k < NW; k++) {
        const uint64_t x = sh[k];
        if (k < w) before += x;
        all += x;
    }
    *total = all;
    return before + inc - v;
}

// The key length of span [s, e): 0 for a malformed span (no text byte is read), 3 for a replaced byte.
__device__ __forceinline__ uint32_t key_len(const uint8_t* __restrict__ text, uint64_t nbytes, uint32_t s, uint32_t e,
                                            bool* repl) {
    *repl = false;
    if (s >= e || e > nbytes) return 0;
    if (e - s == 1u && text[s] >= 0x80u) {
        *repl = true;
        return 3;
    }
    return e - s;
}

// The tile's exclusive scan: v[j] is L of token j * 256 + t (0 past the list).  X (T + 1 entries in LDS)
// receives the sum of L before each token of the tile and, at T, the tile's sum, which is returned.  X is
// valid after the call; a caller that reuses its memory synchronises first.
__device__ __forceinline__ uint64_t tile_scan(const uint32_t (&v)[PER], uint64_t* X, uint64_t* sh) {
    const uint32_t th = threadIdx.x;
    uint32_t* Lsh = (uint32_t*)X;
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) Lsh[j * 256u + th] = v[j];
    __syncthreads();
    const uint4 a = ((const uint4*)Lsh)[th * 2u], b = ((const uint4*)Lsh)[th * 2u + 1u];
    const uint32_t l[PER] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < PER; i++) sum += l[i];
    uint64_t total;
    uint64_t run = block_excl64<4>(sum, sh, &total);  // (its first barrier also ends the reads of Lsh)
#pragma unroll
    for (uint32_t i = 0; i < PER; i++) {
        X[th * PER + i] = run;
        run += l[i];
    }
    if (th == 255u) X[T] = total;
    __syncthreads();
    return total;
}

// ---------------------------------------------------------------------------
// k_join_count
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_join_count(const uint8_t* __restrict__ text, uint64_t nbytes,
                                                    const uint32_t* __restrict__ start,
                                                    const uint32_t* __restrict__ end,
                                                    const uint64_t* __restrict__ doc_tok,
                                                    const uint64_t* __restrict__ ntok, uint64_t cap, uint32_t ndocs,
                                                    uint32_t seplen, uint32_t ntl, uint64_t* __restrict__ tilesum,
                                                    uint64_t* __restrict__ aloc, uint64_t* __restrict__ doccnt) {
    __shared__ __attribute__((aligned(16))) uint64_t X[T + 1];
    __shared__ uint64_t sh[4];
    __shared__ uint64_t s_d[2];
    const uint32_t th = threadIdx.x;
    const uint64_t n = std::min(*ntok, cap);
    if (blockIdx.x >= ntl) {  // a document tile: its non-empty documents
        const uint64_t d = (uint64_t)(blockIdx.x - ntl) * kDocTile + th;
        const uint64_t f = d < ndocs && std::min(doc_tok[d + 1], n) > std::min(doc_tok[d], n);
        uint64_t total;
        (void)block_excl64<4>(f, sh, &total);
        if (th == 0) doccnt[blockIdx.x - ntl] = total;
        return;
    }
    const uint64_t t0 = (uint64_t)blockIdx.x * T;
    uint32_t v[PER];
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        const uint64_t k = t0 + j * 256u + th;
        v[j] = 0;
        if (k < n) {
            bool repl;
            v[j] = key_len(text, nbytes, start[k], end[k], &repl) + seplen;
        }
    }
    const uint64_t total = tile_scan(v, X, sh);
    const uint64_t hi_k = std::min(t0 + T, n);
    if (th == 0) {
        tilesum[blockIdx.x] = total;
        // the documents whose first token lies in [t0, hi_k)
        s_d[0] = s_d[1] = 0;
        if (hi_k > t0) {
            s_d[0] = t0 == 0 ? 0 : doc_ub(doc_tok, t0 - 1u, 0, (uint64_t)ndocs + 1u);
            s_d[1] = doc_ub(doc_tok, hi_k - 1u, s_d[0], (uint64_t)ndocs + 1u);
        }
    }
    __syncthreads();
    for (uint64_t d = s_d[0] + th; d < s_d[1]; d += 256u) {
        const uint64_t a = doc_tok[d];
        if (a < t0 || a >= hi_k) continue;  // (doc_tok out of order)
        aloc[d] = X[a - t0];
    }
}

// ---------------------------------------------------------------------------
// k_join_scan: one workgroup; base[i] = the sum of cnt[0 .. i), n + 1 entries (tiles) or n (documents)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_join_scan(const uint64_t* __restrict__ tilesum, uint64_t ntl,
                                                    uint64_t* __restrict__ tilebase,
                                                    const uint64_t* __restrict__ doccnt, uint64_t ndt,
                                                    uint64_t* __restrict__ docbase) {
    __shared__ uint64_t sh[16];
    uint64_t carry = 0;
    for (uint64_t c0 = 0; c0 < ntl; c0 += 1024u) {
        const uint64_t i = c0 + threadIdx.x;
        const uint64_t v = i < ntl ? tilesum[i] : 0u;
        uint64_t total;
        const uint64_t ex = block_excl64<16>(v, sh, &total);
        if (i < ntl) tilebase[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tilebase[ntl] = carry;
    carry = 0;
    for (uint64_t c0 = 0; c0 < ndt; c0 += 1024u) {
        const uint64_t i = c0 + threadIdx.x;
        const uint64_t v = i < ndt ? doccnt[i] : 0u;
        uint64_t total;
        const uint64_t ex = block_excl64<16>(v, sh, &total);
        if (i < ndt) docbase[i] = carry + ex;
        carry += total;
    }
}

// ---------------------------------------------------------------------------
// k_join_doc
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_join_doc(const uint64_t* __restrict__ doc_tok,
                                                  const uint64_t* __restrict__ ntok, uint64_t cap, uint32_t ndocs,
                                                  uint32_t ntl, const uint64_t* __restrict__ tilebase,
                                                  const uint64_t* __restrict__ aloc,
                                                  const uint64_t* __restrict__ docbase, uint32_t seplen,
                                                  uint64_t term8, uint32_t termlen, uint8_t* __restrict__ out,
                                                  uint64_t out_cap, uint64_t* __restrict__ out_doc_off,
                                                  uint64_t* __restrict__ nout, uint64_t* __restrict__ D) {
    __shared__ uint64_t sh[4];
    const uint64_t n = std::min(*ntok, cap);
    const uint64_t d = (uint64_t)blockIdx.x * kDocTile + threadIdx.x;
    // A at document dd's first token (the whole list's sum when the document starts at or past its end)
    auto a_at = [&](uint64_t dd) -> uint64_t {
        const uint64_t a = doc_tok[dd];
        return a >= n ? tilebase[ntl] : tilebase[a / T] + aloc[dd];
    };
    const bool nonempty = d < ndocs && std::min(doc_tok[d + 1], n) > std::min(doc_tok[d], n);
    uint64_t total;
    const uint64_t E = docbase[blockIdx.x] + block_excl64<4>(nonempty, sh, &total);
    if (d > ndocs) return;
    const uint64_t A0 = a_at(0), Ad = a_at(d);
    const uint64_t off = Ad - A0 + d * termlen - E * seplen;
    out_doc_off[d] = off;
    if (d == ndocs) {
        *nout = off;
        return;
    }
    D[d] = off - Ad;
    const uint64_t tpos = off + (a_at(d + 1u) - Ad) - (nonempty ? seplen : 0u);
    for (uint32_t i = 0; i < termlen; i++)
        if (tpos + i < out_cap) out[tpos + i] = (uint8_t)(term8 >> (8u * i));
}

// ---------------------------------------------------------------------------
// k_join_write
// ---------------------------------------------------------------------------
struct LongKey {
    uint64_t q;  // where it goes (output position + the output pointer's low 4 bits)
    uint32_t s, len;
};

template <bool STAGED>
__global__ __launch_bounds__(256) void k_join_write(const uint8_t* __restrict__ text, uint64_t nbytes,
                                                    const uint32_t* __restrict__ start,
                                                    const uint32_t* __restrict__ end,
                                                    const uint64_t* __restrict__ doc_tok,
                                                    const uint64_t* __restrict__ ntok, uint64_t cap, uint32_t ndocs,
                                                    const uint64_t* __restrict__ tilebase,
                                                    const uint64_t* __restrict__ D, uint64_t sep8, uint32_t seplen,
                                                    uint8_t* __restrict__ out, uint64_t out_cap) {
    // the tile scan (T + 1 u64), then the staged bytes or the list of long keys
    __shared__ __attribute__((aligned(16))) uint8_t buf[CH];
    __shared__ uint32_t mask[STAGED ? kMaskWords : 1];  // one bit per staged byte: the tile placed it
    __shared__ uint64_t sh[4];
    __shared__ uint64_t s_d[2];
    __shared__ unsigned long long s_q[2];  // the least start and the greatest end of what the tile places
    __shared__ uint32_t s_nl;
    const uint32_t th = threadIdx.x;
    const uint64_t n = std::min(*ntok, cap), t0 = (uint64_t)blockIdx.x * T;
    if (t0 >= n) return;
    const uint64_t hi_k = std::min(t0 + T, n);
    uint32_t s[PER], len[PER], v[PER];
    bool repl[PER];
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        const uint64_t k = t0 + j * 256u + th;
        s[j] = len[j] = v[j] = 0;
        repl[j] = false;
        if (k < n) {
            s[j] = start[k];
            len[j] = key_len(text, nbytes, s[j], end[k], &repl[j]);
            v[j] = len[j] + seplen;
        }
    }
    if (th == 0) {
        // token k's document is doc_ub(k) - 1, and doc_ub(k) lies in [s_d[0], s_d[1]] for the tile's tokens
        s_d[0] = doc_ub(doc_tok, t0, 0, (uint64_t)ndocs + 1u);
        s_d[1] = doc_ub(doc_tok, hi_k - 1u, s_d[0], (uint64_t)ndocs + 1u);
        s_q[0] = ~0ull;
        s_q[1] = 0;
    }
    if (STAGED)
        for (uint32_t w = th; w < kMaskWords; w += 256u) mask[w] = 0;
    uint64_t* X = (uint64_t*)buf;
    (void)tile_scan(v, X, sh);
    const uint64_t tb = tilebase[blockIdx.x];
    // q: the token's output position, plus the output pointer's low 4 bits in the staged form (so that q
    // is a multiple of 16 where the address is); w: the bytes it places there, key and separator
    const uint32_t al = STAGED ? (uint32_t)((uintptr_t)out & 15u) : 0u;
    const uint64_t limit = out_cap + al;
    uint64_t q[PER];
    uint32_t sepn[PER];
    bool has[PER];
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        const uint64_t k = t0 + j * 256u + th;
        has[j] = false;
        q[j] = 0;
        sepn[j] = 0;
        if (k >= n) continue;
        const uint64_t u = doc_ub(doc_tok, k, s_d[0], s_d[1]);
        if (u == 0 || u > ndocs) continue;  // (before the first document or past the last)
        has[j] = true;
        sepn[j] = (k + 1u == n || doc_tok[u] == k + 1u) ? 0u : seplen;
        q[j] = tb + X[j * 256u + th] + D[u - 1u] + al;
    }
    if (!STAGED) {
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) {
            if (!has[j]) continue;
            const uint64_t p = q[j];
            for (uint32_t i = 0; i < len[j] && p + i < out_cap; i++)
                out[p + i] = repl[j] ? (uint8_t)(0xBDBFEFu >> (8u * i)) : text[s[j] + i];
            for (uint32_t i = 0; i < sepn[j] && p + len[j] + i < out_cap; i++)
                out[p + len[j] + i] = (uint8_t)(sep8 >> (8u * i));
        }
        return;
    }
    // ---- the staged form ----
    bool anylong = false;
    {
        uint64_t lo = ~0ull, hi = 0;
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) {
            if (!has[j]) continue;
            const bool lng = len[j] >= kJoinLong;
            anylong |= lng;
            const uint64_t a = lng ? q[j] + len[j] : q[j], b = q[j] + len[j] + sepn[j];
            if (a < b) {
                lo = std::min(lo, a);
                hi = std::max(hi, b);
            }
        }
        if (lo < hi) {
            atomicMin(&s_q[0], (unsigned long long)lo);
            atomicMax(&s_q[1], (unsigned long long)hi);
        }
    }
    __syncthreads();  // (s_q complete; every thread has read X, whose memory now stages bytes)
    const uint64_t qend = std::min((uint64_t)s_q[1], limit);
    for (uint64_t c0 = (uint64_t)s_q[0] & ~15ull; c0 < qend; c0 += CH) {
        const uint64_t c1 = std::min(c0 + CH, qend);
        bool any = false;
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) {
            if (!has[j]) continue;
            const uint32_t kl = len[j];
            const bool lng = kl >= kJoinLong;
            const uint64_t lo = std::max(lng ? q[j] + kl : q[j], c0), hi = std::min(q[j] + kl + sepn[j], c1);
            if (lo >= hi) continue;
            any = true;
            for (uint64_t g = lo; g < hi; g++) {
                const uint64_t i = g - q[j];  // (the byte's index in key + separator)
                buf[g - c0] = i >= kl ? (uint8_t)(sep8 >> (8u * (uint32_t)(i - kl)))
                                      : repl[j] ? (uint8_t)(0xBDBFEFu >> (8u * (uint32_t)i)) : text[s[j] + i];
            }
            const uint32_t b0 = (uint32_t)(lo - c0), b1 = (uint32_t)(hi - c0);  // bits [b0, b1)
            for (uint32_t w = b0 >> 5; w <= (b1 - 1u) >> 5; w++) {
                const uint32_t f = w == (b0 >> 5) ? b0 & 31u : 0u, l = w == ((b1 - 1u) >> 5) ? ((b1 - 1u) & 31u) + 1u : 32u;
                atomicOr(&mask[w], (l == 32u ? ~0u : (1u << l) - 1u) & ~((1u << f) - 1u));
            }
        }
        if (!__syncthreads_or(any)) continue;  // (a chunk inside a long key, or between far documents)
        for (uint32_t w = th; w < kMaskWords; w += 256u) {
            const uint32_t m = mask[w];
            if (m == 0) continue;
            mask[w] = 0;
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t mm = (m >> (16u * h)) & 0xFFFFu, u = 2u * w + h;
                uint8_t* dst = out + (c0 + 16u * u - al);  // (only the bytes whose bits are set are touched)
                if (mm == 0xFFFFu) {
                    *(uint4*)dst = *(const uint4*)(buf + 16u * u);
                } else {
                    for (uint32_t b = 0; b < 16; b++)
                        if ((mm >> b) & 1u) dst[b] = buf[16u * u + b];
                }
            }
        }
        __syncthreads();
    }
    // the long keys, trip by trip: their owners list them, the workgroup copies them
    if (!__syncthreads_or(anylong)) return;
    LongKey* list = (LongKey*)buf;
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        if (th == 0) s_nl = 0;
        __syncthreads();
        if (has[j] && len[j] >= kJoinLong) list[atomicAdd(&s_nl, 1u)] = LongKey{q[j], s[j], len[j]};
        __syncthreads();
        const uint32_t nl = s_nl;
        for (uint32_t e = 0; e < nl; e++) {
            const LongKey lk = list[e];
            if (lk.q >= limit) continue;
            const uint64_t m = std::min<uint64_t>(lk.len, limit - lk.q);
            for (uint64_t b = th; b < m; b += 256u) out[lk.q + b - al] = text[lk.s + b];
        }
        __syncthreads();
    }
}

struct JoinWork {
    uint64_t ntl, ndt;
    uint64_t *tilesum, *tilebase, *doccnt, *docbase, *aloc, *D;
    size_t bytes;
};

JoinWork join_layout(uint64_t max_tokens, uint32_t ndocs, void* p) {
    JoinWork w;
    w.ntl = std::max<uint64_t>(1u, (max_tokens + T - 1u) / T);
    w.ndt = ((uint64_t)ndocs + 1u + kDocTile - 1u) / kDocTile;
    uint8_t* b = (uint8_t*)p;
    size_t off = 0;
    auto take = [&](size_t nb) -> uint64_t* {
        const size_t o = off;
        off += (nb + 255u) & ~(size_t)255u;
        return b ? (uint64_t*)(b + o) : nullptr;
    };
    w.tilesum = take(w.ntl * 8u);
    w.tilebase = take((w.ntl + 1u) * 8u);
    w.doccnt = take(w.ndt * 8u);
    w.docbase = take(w.ndt * 8u);
    w.aloc = take(((size_t)ndocs + 1u) * 8u);
    w.D = take(((size_t)ndocs + 1u) * 8u);
    w.bytes = off;
    return w;
}

uint64_t pack8(const uint8_t* p, uint32_t len) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < len; i++) v |= (uint64_t)p[i] << (8u * i);
    return v;
}

}  // namespace

size_t join_work_bytes(uint64_t max_tokens, uint32_t ndocs) { return join_layout(max_tokens, ndocs, nullptr).bytes; }

hipError_t run_join(const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start, const uint32_t* d_end,
                    const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint64_t cap, uint32_t ndocs, const uint8_t* sep,
                    uint32_t seplen, const uint8_t* term, uint32_t termlen, bool staged, uint8_t* d_out,
                    uint64_t out_cap, uint64_t* d_out_doc_off, uint64_t* d_nout, void* d_work, hipStream_t stream,
                    KernelTimer* timer) {
    const JoinWork w = join_layout(cap, ndocs, d_work);
    const uint32_t ntl = (uint32_t)w.ntl, ndt = (uint32_t)w.ndt;
    const uint64_t sep8 = pack8(sep, seplen), term8 = pack8(term, termlen);
    JB_TIMED(K_JOIN_COUNT, hipLaunchKernelGGL(k_join_count, dim3(ntl + ndt), dim3(256), 0, stream, d_text, nbytes, d_start,
                                              d_end, d_doc_tok, d_ntok, cap, ndocs, seplen, ntl, w.tilesum, w.aloc,
                                              w.doccnt));
    JB_TIMED(K_JOIN_SCAN, hipLaunchKernelGGL(k_join_scan, dim3(1), dim3(1024), 0, stream, w.tilesum, w.ntl, w.tilebase,
                                             w.doccnt, w.ndt, w.docbase));
    JB_TIMED(K_JOIN_DOC, hipLaunchKernelGGL(k_join_doc, dim3(ndt), dim3(256), 0, stream, d_doc_tok, d_ntok, cap, ndocs,
                                            ntl, w.tilebase, w.aloc, w.docbase, seplen, term8, termlen, d_out, out_cap,
                                            d_out_doc_off, d_nout, w.D));
    if (staged)
        JB_TIMED(K_JOIN_WRITE, hipLaunchKernelGGL(k_join_write<true>, dim3(ntl), dim3(256), 0, stream, d_text, nbytes,
                                                  d_start, d_end, d_doc_tok, d_ntok, cap, ndocs, w.tilebase, w.D, sep8,
                                                  seplen, d_out, out_cap));
    else
        JB_TIMED(K_JOIN_WRITE, hipLaunchKernelGGL(k_join_write<false>, dim3(ntl), dim3(256), 0, stream, d_text, nbytes,
                                                  d_start, d_end, d_doc_tok, d_ntok, cap, ndocs, w.tilebase, w.D, sep8,
                                                  seplen, d_out, out_cap));
    return hipGetLastError();
}

}  // namespace jb
