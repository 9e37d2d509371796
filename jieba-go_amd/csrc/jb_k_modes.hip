// jb_k_modes.hip — the passes over a finished run's spans: search mode, full mode, token ids.
#include "jb_kdev.h"
#include "jb_kstages.h"

#include <algorithm>

namespace jb {

// ---------------------------------------------------------------------------
// Search mode (jieba's cut_for_search on this reference's DAG): a pass over the
// spans of a finished run.  For a Han token of n runes at bytes p_0 < ... < p_n:
// n > 2: [p_i, p_i+2) for every i with a 2-rune edge in buildDag's DAG of the
// token, ascending; n > 3: then [p_i, p_i+3) likewise; then the token.  Every
// other token is copied.  An edge of rune i is read from its record erec[p_i / 3]
// (k_mark_walk: bit L-1 of the mask = an edge of L runes; the record was built on
// the whole Han run, so the caller keeps only grams that end inside the token); a
// zero record (overflowed, or DevImage::plainw == 0) is answered by two trie steps
// with dp_walk_rune's rules.  Nearly every token takes the fast form (srch_masks): no 4-byte rune
// near it, so its runes and records sit at fixed strides and all its loads are issued at once.
// Three launches, no waits between workgroups: k_srch_count (spans per token and
// per tile of kSrchTile tokens), k_sup over the tile sums, k_srch_write (the tile's
// prefix as k_tok's write pass finds it, pf_load / pf_sum; the spans); then
// k_srch_doc maps doc_tok through the offsets.
// Thread t of a tile owns tokens j * 256 + t (j < kSrchPer): every load and
// store of the token arrays is coalesced, and the scan runs over (j, t) in that order.
// ---------------------------------------------------------------------------
constexpr uint32_t kSrchNone = 0xFFFFFFFFu;
// the byte after the Han rune at p, or kSrchNone when no whole rune starts at p inside [.., e)
__device__ __forceinline__ uint32_t srch_next(const uint8_t* __restrict__ text, uint32_t p, uint32_t e) {
    if (p >= e) return kSrchNone;  // (also p == kSrchNone)
    const uint32_t q = p + (text[p] >= 0xF0u ? 4u : 3u);
    return q <= e ? q : kSrchNone;
}
__device__ __forceinline__ uint32_t srch_rune(const uint8_t* __restrict__ text, uint32_t p) {  // valid UTF-8, 3 or 4 bytes
    const uint32_t x = ld4(text, p), b0 = x & 0xFFu;
    const uint32_t r3 = ((b0 & 0x0Fu) << 12) | (((x >> 8) & 0x3Fu) << 6) | ((x >> 16) & 0x3Fu);
    const uint32_t r4 = ((b0 & 0x07u) << 18) | (((x >> 8) & 0x3Fu) << 12) | (((x >> 16) & 0x3Fu) << 6) |
                        ((x >> 24) & 0x3Fu);
    return b0 >= 0xF0u ? r4 : r3;
}
// bit 0: E(i, 2), bit 1: E(i, 3) for the rune at a, whose next two runes start at b and (third
// == true) at c, all inside the token.  rc: the rune's record.
__device__ __forceinline__ uint32_t srch_edges(const uint8_t* __restrict__ text, const DevImage& im, uint64_t rc,
                                               uint32_t a, uint32_t b, uint32_t c, bool third) {
    if (rc) return (uint32_t)(rc >> 1) & 3u;
    const uint32_t r0 = srch_rune(text, a), r1 = srch_rune(text, b);
    if (r0 >= 0x110000u || r1 >= 0x110000u) return 0u;  // (not in a Han token)
    const uint32_t id = rune_code(im, r0);
    const uint64_t cc = im.cells[id];
    if (jb_cell_check(cc) != JB_CHECK_ROOT || jb_cell_fc(cc) == JB_FC_ZERO || !jb_cell_hc(cc)) return 0u;
    const uint32_t t1 = dat_slot(im, cc, r1);
    const uint64_t c1 = im.cells[t1];
    if (!dat_hit(c1, id)) return 0u;
    uint32_t m = jb_cell_fc(c1) == JB_FC_POS ? 1u : 0u;
    if (third && jb_cell_hc(c1)) {
        const uint32_t r2 = srch_rune(text, c);
        if (r2 < 0x110000u) {
            const uint32_t t2 = dat_slot(im, c1, r2);
            const uint64_t c2 = im.cells[t2];
            if (dat_hit(c2, t1) && jb_cell_fc(c2) == JB_FC_POS) m |= 2u;
        }
    }
    return m;
}
// Does a token of at least nine bytes (three runes) whose first four bytes are x start with a Han rune?
__device__ __forceinline__ bool srch_han(uint32_t x) {
    uint32_t w;
    return (x & 0x80u) != 0u && han_rune(x, 4u, &w) != 0u;
}
// The fast form.  A token whose tiles hold no 4-byte Han rune (tile4) has rune i at s + 3 i and its
// records at consecutive slots, so no load waits for another: the edges of its runes as two masks,
// bit i of m2 = E(i, 2) (i <= n - 2), bit i of m3 = E(i, 3) (n > 3, i <= n - 3).  han: the token starts
// with a Han rune (the caller's load; only then may a zero record be walked).  False: the token has more
// than kSrchFastN runes or may hold a 4-byte rune, and takes the general form (srch_grams).
constexpr uint32_t kSrchFastN = 32;
__device__ __forceinline__ bool srch_masks(const uint8_t* __restrict__ text, const DevImage& im,
                                           const uint64_t* __restrict__ erec, const uint32_t* __restrict__ tile4,
                                           uint32_t s, uint32_t e, bool han, uint32_t& m2, uint32_t& m3) {
    const uint32_t n = (e - s) / 3u;
    if (n * 3u != e - s || n > kSrchFastN) return false;
    const bool all3 = (tile4[s / kTileBytes] | tile4[(e - 1u) / kTileBytes]) == 0u;
    const uint64_t* const rp = erec + s / 3u;
    uint32_t a2 = 0, a3 = 0;
    for (uint32_t i = 0; i + 1u < n; i += 4u) {  // runes i .. i+3 of 0 .. n-2
        uint64_t r[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) r[k] = rp[i + k];  // (slots past the last rune are read and dropped)
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t q = i + k, a = s + 3u * q;
            if (q + 1u < n) {
                uint32_t m = (uint32_t)(r[k] >> 1) & 3u;
                if (r[k] == 0ull) m = han && all3 ? srch_edges(text, im, 0ull, a, a + 3u, a + 6u, q + 2u < n) : 0u;
                a2 |= (m & 1u) << q;
                a3 |= (m >> 1) << q;
            }
        }
    }
    m2 = a2;
    m3 = n > 3u ? a3 & ((1u << (n - 2u)) - 1u) : 0u;
    return all3;
}
// The grams of one length (L = 2, 3) or both (L = 0) of the Han token [s, e), in text order:
// f(L, from, to).  A token of n runes has 2-grams when n > 2 and 3-grams when n > 3.
template <uint32_t L, class F>
__device__ __forceinline__ void srch_grams(const uint8_t* __restrict__ text, const DevImage& im,
                                           const uint64_t* __restrict__ erec, uint32_t s, uint32_t e, F&& f) {
    uint32_t a = s, b = srch_next(text, a, e), c = srch_next(text, b, e), d = srch_next(text, c, e);
    if (c == kSrchNone || c >= e) return;  // n <= 2
    const bool n3 = d != kSrchNone && d < e;  // n > 3
    if (L == 3u && !n3) return;
    while (c != kSrchNone) {  // the rune at a has a next rune [b, c)
        const uint32_t m = srch_edges(text, im, erec[a / 3u], a, b, c, d != kSrchNone);
        if (L != 3u && (m & 1u)) f(2u, a, c);
        if (L != 2u && n3 && (m & 2u) && d != kSrchNone) f(3u, a, d);
        a = b;
        b = c;
        c = d;
        d = srch_next(text, d, e);
    }
}

// (96 SGPRs at most: the image's pointers would otherwise cost the eighth wave per SIMD)
#define JB_SRCH_ATTR __attribute__((amdgpu_num_sgpr(96)))
__global__ __launch_bounds__(256) JB_SRCH_ATTR void k_srch_count(const uint8_t* __restrict__ text, DevImage im,
                                                    const uint64_t* __restrict__ erec,
                                                    const uint32_t* __restrict__ ts, const uint32_t* __restrict__ te,
                                                    const uint32_t* __restrict__ counters, uint32_t* __restrict__ off,
                                                    uint2* __restrict__ tile, const uint32_t* __restrict__ tile4) {
    __shared__ uint32_t lds[8];
    const uint32_t n = counters[CNT_NTOK], i0 = blockIdx.x * kSrchTile + threadIdx.x;
    uint32_t sum = 0;
    if (blockIdx.x * kSrchTile < n) {
        uint32_t s1 = 0, e1 = 0;  // the next token's span, loaded one trip ahead
        if (i0 < n) {
            s1 = ts[i0];
            e1 = te[i0];
        }
        for (uint32_t j = 0; j < kSrchPer; j++) {
            const uint32_t i = i0 + j * 256u;
            if (i >= n) break;
            const uint32_t s = s1, e = e1;
            if (j + 1u < kSrchPer && i + 256u < n) {
                s1 = ts[i + 256u];
                e1 = te[i + 256u];
            }
            uint32_t cnt = 1u;
            if (e - s >= 9u) {
                const bool han = srch_han(ld4(text, s));
                uint32_t m2, m3;
                const bool fast = srch_masks(text, im, erec, tile4, s, e, han, m2, m3);
                if (han && fast) cnt += __popc(m2) + __popc(m3);
                else if (han) srch_grams<0u>(text, im, erec, s, e, [&](uint32_t, uint32_t, uint32_t) { cnt++; });
            }
            off[i] = cnt;
            sum += cnt;
        }
    }
    const uint2 t = pf_sum(PrefixLoads{sum, 0u}, lds);
    if (threadIdx.x == 0) tile[blockIdx.x] = make_uint2(t.x, 0u);  // (0 for the tiles past the last token)
}

__global__ __launch_bounds__(256) JB_SRCH_ATTR void k_srch_write(const uint8_t* __restrict__ text, DevImage im,
                                                    const uint64_t* __restrict__ erec,
                                                    const uint32_t* __restrict__ ts, const uint32_t* __restrict__ te,
                                                    uint32_t* __restrict__ counters, uint32_t* __restrict__ off,
                                                    const uint2* __restrict__ tile, const uint2* __restrict__ sup,
                                                    uint32_t* __restrict__ os, uint32_t* __restrict__ oe,
                                                    uint64_t* ontok, const uint32_t* __restrict__ tile4) {
    __shared__ uint32_t lds[8];
    __shared__ uint32_t s_tot[kSrchPer * 4u], s_pre[kSrchPer * 4u];
    static_assert(kSrchPer * 4u == 64u, "the (row, wave) totals are scanned by one wave");
    const uint32_t n = counters[CNT_NTOK], t0 = blockIdx.x * kSrchTile, i0 = t0 + threadIdx.x;
    if (t0 >= n && blockIdx.x != 0u) return;  // (the whole workgroup)
    const PrefixLoads pl = pf_load(tile, sup, blockIdx.x);
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint32_t c[kSrchPer], x[kSrchPer];
#pragma unroll
    for (uint32_t j = 0; j < kSrchPer; j++) c[j] = i0 + j * 256u < n ? off[i0 + j * 256u] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < kSrchPer; j++) {
        x[j] = wave_incl_scan(c[j]);
        if (lane == 63u) s_tot[j * 4u + wid] = x[j];
    }
    const uint2 tb = pf_sum(pl, lds);  // (its barriers also publish s_tot)
    if (threadIdx.x < 64u) {
        const uint32_t v = s_tot[threadIdx.x];
        s_pre[threadIdx.x] = wave_incl_scan(v) - v;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kSrchPer; j++)
        if (i0 + j * 256u < n) off[i0 + j * 256u] = tb.x + s_pre[j * 4u + wid] + x[j] - c[j];
    if (threadIdx.x == 0 && t0 + kSrchTile >= n) {  // the last tile: the expanded count
        const uint64_t tot = (uint64_t)tb.x + s_pre[63] + s_tot[63];
        *reinterpret_cast<uint64_t*>(counters + CNT_NSRCH) = tot;
        *ontok = tot;
    }
    uint32_t s1 = 0, e1 = 0, k1 = 0;  // the next token's span and offset, loaded one trip ahead
    if (i0 < n) {
        s1 = ts[i0];
        e1 = te[i0];
        k1 = off[i0];  // (this thread's own store)
    }
    for (uint32_t j = 0; j < kSrchPer; j++) {
        const uint32_t i = i0 + j * 256u;
        if (i >= n) break;
        const uint32_t s = s1, e = e1;
        uint32_t k = k1;
        if (j + 1u < kSrchPer && i + 256u < n) {
            s1 = ts[i + 256u];
            e1 = te[i + 256u];
            k1 = off[i + 256u];
        }
        bool han = false, fast = false;
        uint32_t m2 = 0, m3 = 0;
        if (e - s >= 9u) {
            han = srch_han(ld4(text, s));
            fast = srch_masks(text, im, erec, tile4, s, e, han, m2, m3);
        }
        if (han && fast) {
            for (; m2; m2 &= m2 - 1u, k++) {
                const uint32_t a = s + 3u * (uint32_t)__builtin_ctz(m2);
                os[k] = a;
                oe[k] = a + 6u;
            }
            for (; m3; m3 &= m3 - 1u, k++) {
                const uint32_t a = s + 3u * (uint32_t)__builtin_ctz(m3);
                os[k] = a;
                oe[k] = a + 9u;
            }
        } else if (han) {
            srch_grams<2u>(text, im, erec, s, e, [&](uint32_t, uint32_t a, uint32_t b) {
                os[k] = a;
                oe[k] = b;
                k++;
            });
            srch_grams<3u>(text, im, erec, s, e, [&](uint32_t, uint32_t a, uint32_t b) {
                os[k] = a;
                oe[k] = b;
                k++;
            });
        }
        os[k] = s;
        oe[k] = e;
    }
}

// doc_tok of the expanded list: the first span of each document's first token
__global__ __launch_bounds__(256) void k_srch_doc(const uint64_t* __restrict__ doc_tok, uint32_t ndocs,
                                                  const uint32_t* __restrict__ counters,
                                                  const uint32_t* __restrict__ off, uint64_t* __restrict__ out) {
    const uint32_t d = blockIdx.x * 256u + threadIdx.x;
    if (d > ndocs) return;
    const uint64_t t = doc_tok[d];
    out[d] = t < counters[CNT_NTOK] ? (uint64_t)off[t] : *reinterpret_cast<const uint64_t*>(counters + CNT_NSRCH);
}

hipError_t run_search(const DevImage& im, const Work& w, const SearchOut& so, const uint8_t* d_text, uint64_t nbytes,
                      uint32_t ndocs, hipStream_t stream, KernelTimer* timer) {
    if (nbytes == 0)  // (run_pipeline left the counters and the plain doc_tok all zeros)
        return run_zero(so.doc_tok, (ndocs + 1) * sizeof(uint64_t), stream, so.ntok, sizeof(uint64_t));
    const uint32_t ntt = (uint32_t)srch_tiles(nbytes);
    JB_TIMED(K_SRCH_COUNT, hipLaunchKernelGGL(k_srch_count, dim3(ntt), dim3(256), 0, stream, d_text, im,
                                              w.erec + kErecPad, w.tok_start, w.tok_end, w.counters, so.off, so.tile,
                                              w.tile4));
    if (ntt > 256u)  // (k_srch_write reads the sums of whole groups of 256 tiles only)
        JB_TIMED(K_SRCH_SCAN, enq_sup(so.tile, ntt, so.sup, stream));
    JB_TIMED(K_SRCH_WRITE, hipLaunchKernelGGL(k_srch_write, dim3(ntt), dim3(256), 0, stream, d_text, im,
                                              w.erec + kErecPad, w.tok_start, w.tok_end, w.counters, so.off, so.tile,
                                              so.sup, so.start, so.end, so.ntok, w.tile4));
    JB_TIMED(K_SRCH_DOC, hipLaunchKernelGGL(k_srch_doc, dim3((ndocs + 1u + 255u) / 256u), dim3(256), 0, stream,
                                            w.doc_tok, ndocs, w.counters, so.off, so.doc_tok));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Full mode (jieba's cut_all on this reference's DAG): every dictionary word of
// two or more runes in a Han block, by start then by length, and the single runes
// that no such word accounts for.  A pass over the plain spans of a finished run
// with hmm = 0, in the search pass's shape: k_full_count (spans per plain token and
// per tile of kSrchTile tokens), k_sup64, k_full_write, k_full_doc.  A Han rune's
// spans belong to the plain token that holds the rune; they may end past that
// token but never past the Han run.  A non-Han token is copied.
// For the rune i at byte p with record rc = erec[p / 3]: rc != 0 gives M(i) = rc & 0xFE
// (bit L-1 = a word of L runes); rc == 0 (overflowed, or DevImage::plainw == 0) is
// walked through the trie by dp_walk_rune's rules up to the end of the Han run,
// which is the token's end or, past it, the next block start of k_mark_walk's lane
// masks (found once per token, only when a walk gets that far).  A rune with M = {}
// is emitted alone unless the nearest earlier rune of its block that has words
// reaches past it (cov); at the head of a token that rune is found by stepping back
// through the records, up to maxlen - 1 runes or the block's start (full_back).
// The output may be longer than the input, so tile sums, the total and the output
// index are 64 bits wide; spans with an index >= cap are counted and not written,
// and CNT_ERR bit 3 reports that.
// ---------------------------------------------------------------------------
struct FullCtx {
    const uint8_t* text;
    const uint64_t* erec;
    const uint32_t* lanemask;
    const uint2* tile_cnt;
    const uint32_t* tile4;
    uint32_t ntiles, nbytes, maxlen;
};
constexpr uint32_t kFullUnk = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t full_w(const uint8_t* __restrict__ text, uint32_t p) {  // width of the Han rune at p
    return text[p] >= 0xF0u ? 4u : 3u;
}
// A walk's limit: lim is a byte up to which the Han run is known to go on, real once
// `known` is set (the first block start at or after the token's end).
struct FullLim {
    uint32_t lim;
    bool known;
};
// The words of two or more runes that start at the Han rune at p, by a trie walk:
// f(end byte) in ascending length.  Returns the last end, 0 when there is none.
template <class F>
__device__ __forceinline__ uint32_t full_walk(const FullCtx& c, const DevImage& im, uint32_t p, FullLim& fl, F&& f) {
    const uint32_t r0 = srch_rune(c.text, p);
    uint32_t id = rune_code(im, r0);
    uint64_t cc = im.cells[id];
    if (jb_cell_check(cc) != JB_CHECK_ROOT || jb_cell_fc(cc) == JB_FC_ZERO) return 0u;  // (:468-471)
    uint32_t qq = p + (r0 >= 0x10000u ? 4u : 3u), last = 0u;
    bool go = jb_cell_hc(cc) != 0u;
    while (go) {
        if (qq >= fl.lim) {
            if (!fl.known) {
                fl.lim = block_end_at(c.lanemask, c.tile_cnt, c.ntiles, c.nbytes, fl.lim - 1u);
                fl.known = true;
            }
            if (qq >= fl.lim) break;
        }
        const uint32_t r = srch_rune(c.text, qq);
        const uint32_t tt = dat_slot(im, cc, r);
        const uint64_t ch = im.cells[tt];
        if (!dat_hit(ch, id)) break;  // (:475-478)
        qq += r >= 0x10000u ? 4u : 3u;
        if (jb_cell_fc(ch) == JB_FC_POS) {
            f(qq);
            last = qq;
        }
        go = jb_cell_hc(ch) != 0u;
        id = tt;
        cc = ch;
    }
    return last;
}
// cov for the rune at p, the first of its token: the end of the longest word of the
// nearest earlier rune of the block that has words, 0 when there is none in reach.
// The fast form covers the eight runes before p when no 4-byte Han rune is near: they
// then sit at a stride of three bytes, so their records and the lane masks that bound
// the block are loaded at once instead of rune by rune.
__device__ __forceinline__ uint32_t full_back(const FullCtx& c, const DevImage& im, uint32_t p, FullLim& fl) {
    uint32_t q = p, k = 1u;
    if (p >= 32u) {
        const uint32_t c0 = p >> 4, base = (c0 - 2u) << 4;
        const uint32_t l0 = c.lanemask[c0], l1 = c.lanemask[c0 - 1u], l2 = c.lanemask[c0 - 2u];
        const uint32_t t4 = c.tile4[(p - 24u) / kTileBytes] | c.tile4[(p - 1u) / kTileBytes];
        const uint64_t* const rp = c.erec + p / 3u;
        uint64_t r[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) r[j] = rp[-(int)(j + 1u)];
        if (t4 == 0u) {
            // block starts at bytes base .. p (bit b = byte base + b): the nearest one bounds the steps
            uint64_t bm = ((uint64_t)(l0 & 0xFFFFu) << 32) | ((uint64_t)(l1 & 0xFFFFu) << 16) | (uint64_t)(l2 & 0xFFFFu);
            bm &= (2ull << (p - base)) - 1ull;
            uint32_t steps = bm ? (p - (base + 63u - (uint32_t)__builtin_clzll(bm))) / 3u : 8u;
            const bool open = steps >= 8u && c.maxlen > 9u;  // neither the block's start nor maxlen - 1 in these eight
            steps = min(min(steps, 8u), c.maxlen - 1u);
            bool zero = false;
#pragma unroll
            for (uint32_t j = 0; j < 8u; j++) {
                if (j < steps && !zero) {
                    const uint64_t rc = r[j];
                    if (rc == 0ull) {
                        zero = true;  // a walk: the general form goes on from this rune
                    } else {
                        const uint32_t m = (uint32_t)rc & 0xFEu;
                        if (m) return p - 3u * (j + 1u) + 3u * (32u - (uint32_t)__builtin_clz(m));
                        q = p - 3u * (j + 1u);
                        k = j + 2u;
                    }
                }
            }
            if (!zero && !open) return 0u;
        }
    }
    for (; k < c.maxlen; k++) {
        if (q < 3u || ((c.lanemask[q >> 4] >> (q & 15u)) & 1u)) return 0u;  // the block starts at q
        const uint32_t wp = (c.text[q - 3u] & 0xF0u) == 0xE0u ? 3u : 4u;  // (the rune before q is a Han rune)
        if (q < wp) return 0u;
        q -= wp;
        const uint64_t rc = c.erec[q / 3u];
        uint32_t last = 0u;
        if (rc) {
            const uint32_t m = (uint32_t)rc & 0xFEu;
            if (m) {
                last = q;
                for (uint32_t L = 32u - (uint32_t)__builtin_clz(m); L; L--) last += full_w(c.text, last);
            }
        } else {
            last = full_walk(c, im, q, fl, [](uint32_t) {});
        }
        if (last) return last;
    }
    return 0u;
}
// The full-mode spans of the plain token [s, e), in output order: f(from, to).
template <class F>
__device__ __forceinline__ void full_token(const FullCtx& c, const DevImage& im, uint32_t s, uint32_t e, F&& f) {
    // every load that depends on the span alone is issued before any is used: the first bytes, the
    // two tile flags and the records of the first four runes at a stride of three bytes (right when
    // all3 below holds; slots that belong to no rune of the token are read and dropped)
    const uint32_t lastb = min(e + 23u, c.nbytes - 1u);
    const uint64_t* const rp = c.erec + s / 3u;
    const uint32_t x0 = ld4(c.text, s);
    const uint32_t t4 = c.tile4[s / kTileBytes] | c.tile4[lastb / kTileBytes];
    uint64_t r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
    uint32_t w0 = 0;
    const bool han = e - s >= 3u && han_rune(x0, min(e - s, 4u), &w0) != 0u;
    if (!han) {
        f(s, e);
        return;
    }
    // no 4-byte Han rune in reach (the token and the eight runes a record's words may span): runes and
    // records sit at fixed strides, and four records are loaded at once
    const bool all3 = t4 == 0u;
    FullLim fl{e, false};
    uint32_t cov = kFullUnk;
    for (uint32_t p = s, q = 0; p < e; q++) {
        uint64_t rc;
        uint32_t w = 3u;
        if (all3) {
            if (q && (q & 3u) == 0u) {  // (slots past the token's last rune are read and dropped)
                r0 = rp[q];
                r1 = rp[q + 1u];
                r2 = rp[q + 2u];
                r3 = rp[q + 3u];
            }
            const uint32_t k = q & 3u;
            rc = k == 0u ? r0 : (k == 1u ? r1 : (k == 2u ? r2 : r3));
        } else {
            w = full_w(c.text, p);
            rc = c.erec[p / 3u];
        }
        uint32_t last = 0u;
        if (rc) {
            uint32_t m = (uint32_t)rc & 0xFEu;
            if (all3) {
                for (; m; m &= m - 1u) {
                    last = p + 3u * ((uint32_t)__builtin_ctz(m) + 1u);
                    f(p, last);
                }
            } else {
                uint32_t qq = p + w, L = 1u;
                for (; m; m &= m - 1u) {
                    for (const uint32_t t = (uint32_t)__builtin_ctz(m) + 1u; L < t; L++) qq += full_w(c.text, qq);
                    f(p, qq);
                    last = qq;
                }
            }
        } else {
            last = full_walk(c, im, p, fl, [&](uint32_t to) { f(p, to); });
        }
        if (last) {
            cov = last;
        } else {
            if (cov == kFullUnk) cov = full_back(c, im, p, fl);
            if (p >= cov) f(p, p + w);
        }
        p += w;
    }
}

// the sum of v over a 256-thread workgroup, 64 bits wide: three 24-bit limbs by DPP wave scans
__device__ uint64_t wg_sum64(uint64_t v, uint64_t* lds) {
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan((uint32_t)v & 0xFFFFFFu), 63);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan((uint32_t)(v >> 24) & 0xFFFFFFu), 63);
    const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan((uint32_t)(v >> 48)), 63);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = (uint64_t)a + ((uint64_t)b << 24) + ((uint64_t)h << 48);
    __syncthreads();
    const uint64_t out = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return out;
}
// k_sup and pf_load for 64-bit tile counts
__global__ __launch_bounds__(256) void k_sup64(const uint64_t* __restrict__ cnt, uint32_t n, uint64_t* __restrict__ sup) {
    __shared__ uint64_t lds[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint64_t s = wg_sum64(i < n ? cnt[i] : 0ull, lds);
    if (threadIdx.x == 0) sup[blockIdx.x] = s;
}
__device__ __forceinline__ uint64_t pf_load64(const uint64_t* __restrict__ cnt, const uint64_t* __restrict__ sup,
                                              uint32_t t) {
    uint64_t p = 0;
    const uint32_t sn = t >> 8, r = t & 255u;
    for (uint32_t i = threadIdx.x; i < sn; i += 256u) p += sup[i];
    if (threadIdx.x < r) p += cnt[(t & ~255u) + threadIdx.x];
    return p;
}

__global__ __launch_bounds__(256) JB_SRCH_ATTR void k_full_count(FullCtx c, DevImage im,
                                                    const uint32_t* __restrict__ ts, const uint32_t* __restrict__ te,
                                                    const uint32_t* __restrict__ counters, uint32_t* __restrict__ off,
                                                    uint64_t* __restrict__ tile) {
    __shared__ uint32_t lds[8];
    const uint32_t n = counters[CNT_NTOK], i0 = blockIdx.x * kSrchTile + threadIdx.x;
    uint32_t sum = 0;  // (a tile's tokens are dictionary words: at most 4096 x 255 runes x 254 spans)
    if (blockIdx.x * kSrchTile < n) {
        uint32_t s1 = 0, e1 = 0;  // the next token's span, loaded one trip ahead
        if (i0 < n) {
            s1 = ts[i0];
            e1 = te[i0];
        }
        for (uint32_t j = 0; j < kSrchPer; j++) {
            const uint32_t i = i0 + j * 256u;
            if (i >= n) break;
            const uint32_t s = s1, e = e1;
            if (j + 1u < kSrchPer && i + 256u < n) {
                s1 = ts[i + 256u];
                e1 = te[i + 256u];
            }
            uint32_t cnt = 0u;
            full_token(c, im, s, e, [&](uint32_t, uint32_t) { cnt++; });
            off[i] = cnt;
            sum += cnt;
        }
    }
    const uint2 t = pf_sum(PrefixLoads{sum, 0u}, lds);
    if (threadIdx.x == 0) tile[blockIdx.x] = t.x;  // (0 for the tiles past the last token)
}

__global__ __launch_bounds__(256) JB_SRCH_ATTR void k_full_write(FullCtx c, DevImage im,
                                                    const uint32_t* __restrict__ ts, const uint32_t* __restrict__ te,
                                                    uint32_t* __restrict__ counters, uint32_t* __restrict__ off,
                                                    const uint64_t* __restrict__ tile, const uint64_t* __restrict__ sup,
                                                    uint64_t* __restrict__ tbase, uint32_t* __restrict__ os,
                                                    uint32_t* __restrict__ oe, uint64_t cap, uint64_t* ontok) {
    __shared__ uint64_t lds[4];
    __shared__ uint32_t s_tot[kSrchPer * 4u], s_pre[kSrchPer * 4u];
    static_assert(kSrchPer * 4u == 64u, "the (row, wave) totals are scanned by one wave");
    const uint32_t n = counters[CNT_NTOK], t0 = blockIdx.x * kSrchTile, i0 = t0 + threadIdx.x;
    if (t0 >= n && blockIdx.x != 0u) return;  // (the whole workgroup)
    const uint64_t pl = pf_load64(tile, sup, blockIdx.x);
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint32_t cn[kSrchPer], x[kSrchPer];
#pragma unroll
    for (uint32_t j = 0; j < kSrchPer; j++) cn[j] = i0 + j * 256u < n ? off[i0 + j * 256u] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < kSrchPer; j++) {
        x[j] = wave_incl_scan(cn[j]);
        if (lane == 63u) s_tot[j * 4u + wid] = x[j];
    }
    const uint64_t tb = wg_sum64(pl, lds);  // (its barriers also publish s_tot)
    if (threadIdx.x < 64u) {
        const uint32_t v = s_tot[threadIdx.x];
        s_pre[threadIdx.x] = wave_incl_scan(v) - v;
    }
    __syncthreads();
    // off: the token's first span, counted from the tile's (tbase)
#pragma unroll
    for (uint32_t j = 0; j < kSrchPer; j++)
        if (i0 + j * 256u < n) off[i0 + j * 256u] = s_pre[j * 4u + wid] + x[j] - cn[j];
    if (threadIdx.x == 0) {
        tbase[blockIdx.x] = tb;
        if (t0 + kSrchTile >= n) {  // the last tile: the count of the complete list
            const uint64_t tot = tb + s_pre[63] + s_tot[63];
            *reinterpret_cast<uint64_t*>(counters + CNT_NSRCH) = tot;
            *ontok = tot;
            if (tot > cap) atomicOr(counters + CNT_ERR, 8u);
        }
    }
    uint32_t s1 = 0, e1 = 0, k1 = 0;  // the next token's span and offset, loaded one trip ahead
    if (i0 < n) {
        s1 = ts[i0];
        e1 = te[i0];
        k1 = off[i0];  // (this thread's own store)
    }
    for (uint32_t j = 0; j < kSrchPer; j++) {
        const uint32_t i = i0 + j * 256u;
        if (i >= n) break;
        const uint32_t s = s1, e = e1;
        uint64_t k = tb + k1;
        if (j + 1u < kSrchPer && i + 256u < n) {
            s1 = ts[i + 256u];
            e1 = te[i + 256u];
            k1 = off[i + 256u];
        }
        full_token(c, im, s, e, [&](uint32_t a, uint32_t b) {
            if (k < cap) {
                os[k] = a;
                oe[k] = b;
            }
            k++;
        });
    }
}

// doc_tok of the full-mode list: the first span of each document's first token
__global__ __launch_bounds__(256) void k_full_doc(const uint64_t* __restrict__ doc_tok, uint32_t ndocs,
                                                  const uint32_t* __restrict__ counters,
                                                  const uint32_t* __restrict__ off, const uint64_t* __restrict__ tbase,
                                                  uint64_t* __restrict__ out) {
    const uint32_t d = blockIdx.x * 256u + threadIdx.x;
    if (d > ndocs) return;
    const uint64_t t = doc_tok[d];
    out[d] = t < counters[CNT_NTOK] ? tbase[t / kSrchTile] + off[t]
                                    : *reinterpret_cast<const uint64_t*>(counters + CNT_NSRCH);
}

hipError_t run_full(const DevImage& im, const Work& w, const FullOut& fo, const uint8_t* d_text, uint64_t nbytes,
                    uint32_t ndocs, hipStream_t stream, KernelTimer* timer) {
    if (nbytes == 0)  // (run_pipeline left the counters and the plain doc_tok all zeros)
        return run_zero(fo.doc_tok, (ndocs + 1) * sizeof(uint64_t), stream, fo.ntok, sizeof(uint64_t));
    const uint32_t ntt = (uint32_t)srch_tiles(nbytes);
    const FullCtx c{d_text, w.erec + kErecPad, w.lanemask, w.tile_cnt, w.tile4,
                    (uint32_t)((nbytes + kTileBytes - 1) / kTileBytes), (uint32_t)nbytes, fo.maxlen};
    JB_TIMED(K_FULL_COUNT, hipLaunchKernelGGL(k_full_count, dim3(ntt), dim3(256), 0, stream, c, im, w.tok_start,
                                              w.tok_end, w.counters, fo.off, fo.tile));
    if (ntt > 256u)  // (k_full_write reads the sums of whole groups of 256 tiles only)
        JB_TIMED(K_FULL_SCAN, hipLaunchKernelGGL(k_sup64, dim3((ntt + 255u) / 256u), dim3(256), 0, stream, fo.tile, ntt,
                                                 fo.sup));
    JB_TIMED(K_FULL_WRITE, hipLaunchKernelGGL(k_full_write, dim3(ntt), dim3(256), 0, stream, c, im, w.tok_start,
                                              w.tok_end, w.counters, fo.off, fo.tile, fo.sup, fo.tbase, fo.start, fo.end,
                                              fo.cap, fo.ntok));
    JB_TIMED(K_FULL_DOC, hipLaunchKernelGGL(k_full_doc, dim3((ndocs + 1u + 255u) / 256u), dim3(256), 0, stream,
                                            w.doc_tok, ndocs, w.counters, fo.off, fo.tbase, fo.doc_tok));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Token ids: every span of a span list looked up in the caller's vocabulary (jb_vocab.h).
// One lane per span, tiles of kIdsTile consecutive spans (coalesced span loads and id
// stores; neighbouring spans are neighbouring text, so a wave's text reads share lines).
// The span count is on the device, so a fixed grid loops over the tiles.  A lane reads its
// token's bytes into registers (8, 16 or 24 of them by its length, from aligned dwords),
// hashes them and probes: jb_vocab_find, the host lookup's code.  No atomics, no waits.
// ---------------------------------------------------------------------------
// Bytes [4 w, 4 w + 4) of a key of len bytes that are inside it, as a mask over the word.
__device__ __forceinline__ uint32_t ids_word_mask(uint32_t len, uint32_t w) {
    if (len >= 4u * w + 4u) return 0xFFFFFFFFu;
    return len > 4u * w ? (1u << (8u * (len - 4u * w))) - 1u : 0u;
}

// The id of the span [s, e) of the text.  The spans are not trusted: one that is empty, reversed
// or past nbytes, or longer than the longest key, is unknown without a text read; every other
// read lies in [s & ~3, s + 28) with s < nbytes, or inside the span.
__device__ __forceinline__ uint32_t ids_one(const uint8_t* __restrict__ text, uint32_t nbytes, const DevVocab& v,
                                            uint32_t s, uint32_t e) {
    if (s >= e || e > nbytes) return JB_VOCAB_UNK;
    uint32_t len = e - s;
    if (len > v.maxlen) return JB_VOCAB_UNK;
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
    // a 1-byte span whose byte is >= 0x80 is an invalid UTF-8 byte: the token is "\xEF\xBF\xBD"
    if (len == 1u && (kw[0] & 0x80u)) {
        kw[0] = 0x00BDBFEFu;
        kw[1] = 0u;
        len = 3u;
    } else {
#pragma unroll
        for (uint32_t w = 0; w < 6u; w++) kw[w] &= ids_word_mask(len, w);
    }
    return jb_vocab_find(v, kw, text + s, len);
}

__global__ __launch_bounds__(256) JB_SRCH_ATTR void k_ids(const uint8_t* __restrict__ text, uint32_t nbytes, DevVocab v,
                                                          const uint32_t* __restrict__ ts,
                                                          const uint32_t* __restrict__ te,
                                                          const uint64_t* __restrict__ ntok, uint64_t cap,
                                                          uint32_t* __restrict__ ids) {
    const uint64_t n = std::min(*ntok, cap), step = (uint64_t)gridDim.x * kIdsTile;
    uint64_t i = (uint64_t)blockIdx.x * kIdsTile + threadIdx.x;
    uint32_t s1 = 0, e1 = 0;  // the next span, loaded one trip ahead
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
        ids[i] = ids_one(text, nbytes, v, s, e);
    }
}

hipError_t run_ids(const DevVocab& v, const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start,
                   const uint32_t* d_end, const uint64_t* d_ntok, uint64_t cap, uint32_t* d_ids, uint32_t ncu,
                   hipStream_t stream, KernelTimer* timer) {
    if (cap == 0) return hipSuccess;  // (nothing to write)
    const uint64_t tiles = (cap + kIdsTile - 1u) / kIdsTile;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)std::max(1u, ncu) * kIdsWgPerCu);
    JB_TIMED(K_IDS, hipLaunchKernelGGL(k_ids, dim3(grid), dim3(256), 0, stream, d_text, (uint32_t)nbytes, v, d_start,
                                       d_end, d_ntok, cap, d_ids));
    return hipGetLastError();
}

}  // namespace jb
