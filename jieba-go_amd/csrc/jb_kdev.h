// jb_kdev.h — device helpers every kernel unit uses (internal to csrc/): text and LDS
// loads, the token-bitmap emitters, wave and workgroup scans, the UTF-8 and Han decode,
// the double-array trie steps, the DAG-record layout and the block bounds from
// k_mark_walk's lane masks.
#pragma once
#include <hip/hip_runtime.h>

#include "jb_kernels.h"

#ifndef JB_STAMPS
#define JB_STAMPS 0
#endif

namespace jb {

// ---------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------
// 4 bytes at any offset: one 8-byte load at the dword below + v_alignbyte.  The
// text buffer is 4-byte aligned and readable 8 bytes past every offset used.
__device__ __forceinline__ uint32_t ld4(const uint8_t* __restrict__ t, uint64_t q) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2), aligned(4)));
    const u32x2 a = *reinterpret_cast<const u32x2*>(t + (q & ~3ull));
    return __builtin_amdgcn_alignbyte(a.y, a.x, (uint32_t)(q & 3));
}

// 4 bytes at window offset k of staged text (k + 8 readable).
__device__ __forceinline__ uint32_t lds4(const uint8_t* tx, uint32_t k) {
    const uint32_t* a = reinterpret_cast<const uint32_t*>(tx + (k & ~3u));
    return __builtin_amdgcn_alignbyte(a[1], a[0], k & 3u);
}

// Token bitmaps: bits are accumulated per 32-byte word in registers and
// flushed with one atomicOr per word (neighbouring blocks may share a word).
struct Emitter {
    uint32_t* sb;
    uint32_t* eb;
    uint32_t word, s, e;
    uint32_t ties = 0;  // exact Viterbi route ties seen by this lane (Q12)
    bool off = false;   // drop the bits instead of flushing them (k_zh_long: only lane 0 writes)
    __device__ Emitter(uint32_t* s_, uint32_t* e_) : sb(s_), eb(e_), word(0xFFFFFFFFu), s(0), e(0) {}
    __device__ __forceinline__ void flush() {
        if (!off) {
            if (s) atomicOr(sb + word, s);
            if (e) atomicOr(eb + word, e);
        }
        s = e = 0;
    }
    __device__ __forceinline__ void at(uint32_t pos) {
        const uint32_t w = pos >> 5;
        if (w != word) {
            flush();
            word = w;
        }
    }
    // token = bytes [a, b)
    __device__ __forceinline__ void token(uint32_t a, uint32_t b) {
        at(a);
        s |= 1u << (a & 31u);
        at(b - 1u);
        e |= 1u << ((b - 1u) & 31u);
    }
    // start / end bits sm, em_ of bitmap word w
    __device__ __forceinline__ void bits(uint32_t w, uint32_t sm, uint32_t em_) {
        if (!(sm | em_)) return;
        if (w != word) {
            flush();
            word = w;
        }
        s |= sm;
        e |= em_;
    }
};

// The same for a wave's LDS token bitmaps: word index = global word - w0.
struct LdsEmitter {
    uint32_t* sb;
    uint32_t* eb;
    uint32_t w0;
    uint32_t word, s, e;
    uint32_t ties = 0;  // exact Viterbi route ties seen by this lane (Q12)
    __device__ LdsEmitter(uint32_t* s_, uint32_t* e_, uint32_t w0_)
        : sb(s_), eb(e_), w0(w0_), word(0xFFFFFFFFu), s(0), e(0) {}
    __device__ __forceinline__ void flush() {
        if (s) atomicOr(sb + (word - w0), s);
        if (e) atomicOr(eb + (word - w0), e);
        s = e = 0;
    }
    __device__ __forceinline__ void at(uint32_t pos) {
        const uint32_t w = pos >> 5;
        if (w != word) {
            flush();
            word = w;
        }
    }
    __device__ __forceinline__ void token(uint32_t a, uint32_t b) {
        at(a);
        s |= 1u << (a & 31u);
        at(b - 1u);
        e |= 1u << ((b - 1u) & 31u);
    }
};

// Inclusive prefix sum over a wave's 64 lanes with DPP moves (VALU, no LDS round
// trips): row_shr 1/2/4/8 scans each row of 16 lanes, row_bcast15/31 carry the row
// totals into the rows above.  Lanes a move cannot source keep 0 (old = 0, bound_ctrl off).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);  // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);  // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);  // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);  // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    return x;
}

__device__ __forceinline__ uint32_t block_scan_u32(uint32_t v, uint32_t* lds, uint32_t* total) {
    // exclusive scan over a 256-thread workgroup
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t x = wave_incl_scan(v);
    if (lane == 63) lds[wid] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    const uint32_t nw = blockDim.x >> 6;
    for (uint32_t k = 0; k < nw; k++) {
        const uint32_t t = lds[k];
        if (k < wid) base += t;
        tot += t;
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

// Exclusive prefix of tile t's (x, y) counts, by a 256-thread workgroup: the
// 256-tile sums (k_sup) before t's group of 256, plus the counts of the tiles
// before t in its own group.  The loads are issued first (pf_load) and summed
// later (pf_sum), so their latency hides under the caller's own loads.
// Replaces a single-workgroup scan launch.
struct PrefixLoads {
    uint32_t x, y;
};
__device__ __forceinline__ PrefixLoads pf_load(const uint2* __restrict__ cnt, const uint2* __restrict__ sup,
                                               uint32_t t) {
    PrefixLoads p{0u, 0u};
    const uint32_t sn = t >> 8, r = t & 255u;
    for (uint32_t i = threadIdx.x; i < sn; i += 256u) {
        const uint2 v = sup[i];
        p.x += v.x;
        p.y += v.y;
    }
    if (threadIdx.x < r) {
        const uint2 c = cnt[(t & ~255u) + threadIdx.x];
        p.x += c.x;
        p.y += c.y;
    }
    return p;
}
__device__ inline uint2 pf_sum(PrefixLoads p, uint32_t* lds) {
    // wave sums by DPP scans (a shuffle reduction was twelve LDS round trips)
    const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(p.x), 63);
    const uint32_t y = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(p.y), 63);
    const uint32_t wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        lds[wid] = x;
        lds[4u + wid] = y;
    }
    __syncthreads();
    const uint2 out = make_uint2(lds[0] + lds[1] + lds[2] + lds[3], lds[4] + lds[5] + lds[6] + lds[7]);
    __syncthreads();
    return out;
}

// \p{Han} (unicode.Han, Unicode 13) with the common ranges first: the two
// big BMP blocks, a bitmask for U+3000-303F (CJK punctuation: only 3005,
// 3007, 3021-3029, 3038-303B are Han), and the full table only for the rare
// rest (radicals, compatibility ideographs, the supplementary planes).
__device__ __forceinline__ bool han_cp(uint32_t r) {
    constexpr uint64_t k3000 = (1ull << 5) | (1ull << 7) | (0x1FFull << 0x21) | (0xFull << 0x38);
    bool h = (r - 0x4E00u <= 0x9FFCu - 0x4E00u) | (r - 0x3400u <= 0x4DBFu - 0x3400u);
    const uint32_t o = r - 0x3000u;
    h |= o < 64u && ((k3000 >> (o & 63u)) & 1ull);
    const bool rare = (r - 0x2E80u < 0x180u) | (r - 0xF900u < 0x200u) | (r >= 0x16FF0u);
    if (rare) h = jb_is_han(r);
    return h;
}

constexpr uint32_t kEdgeMaxL = 8;     // edge lengths a record holds
constexpr uint32_t kEdgeIdxBits = 14;  // a record field: weight index + 1 (0: phantom edge)
constexpr uint32_t kRecIdxMax = (1u << kEdgeIdxBits) - 2u;  // the largest weight index a record holds
constexpr uint32_t kRecTop = 8u + 3u * kEdgeIdxBits;         // bit of the last field (a new edge enters there)

// utf8.DecodeRune (Go rules, as jb_decode) at a lead byte (>= 0xC0), without
// branches: the phase-1 lead loop runs every lane's leads in step, so a
// branchy decode diverged on every byte class (k_mark_walk 0.601 -> 0.598 ms).
__device__ __forceinline__ uint32_t dec_lead(uint32_t x, uint32_t lim, uint32_t* rune) {
    const uint32_t b0 = x & 0xFFu, b1 = (x >> 8) & 0xFFu, b2 = (x >> 16) & 0xFFu, b3 = x >> 24;
    const uint32_t n = b0 >= 0xF0u ? 4u : (b0 >= 0xE0u ? 3u : 2u);
    uint32_t lo = b0 == 0xE0u ? 0xA0u : 0x80u;
    lo = b0 == 0xF0u ? 0x90u : lo;
    uint32_t hi = b0 == 0xEDu ? 0x9Fu : 0xBFu;
    hi = b0 == 0xF4u ? 0x8Fu : hi;
    const bool ok = (b0 - 0xC2u <= 0xF4u - 0xC2u) & (b1 >= lo) & (b1 <= hi) &
                    ((n < 3u) | ((b2 & 0xC0u) == 0x80u)) & ((n < 4u) | ((b3 & 0xC0u) == 0x80u)) & (n <= lim);
    const uint32_t m0 = n == 2u ? 0x1Fu : (n == 3u ? 0x0Fu : 0x07u);
    uint32_t cp = ((b0 & m0) << 6) | (b1 & 0x3Fu);
    cp = n >= 3u ? ((cp << 6) | (b2 & 0x3Fu)) : cp;
    cp = n == 4u ? ((cp << 6) | (b3 & 0x3Fu)) : cp;
    *rune = ok ? cp : 0xFFFDu;
    return ok ? n : 1u;
}

// The Han rune encoded by x (Go-valid, within `lim` bytes), or 0.  A 3-byte
// form with a Han value cannot be overlong (E0: below U+0800) or a surrogate
// (ED), so its bit pattern suffices.  A 4-byte form can be overlong with a
// Han value (F0 84 B8 80 has the value U+4E00; Go decodes four invalid
// bytes), hence the test r >= 0x10000: every overlong F0 form lies below it
// and no valid one does.  F5..F7 and F4 90.. lie past U+10FFFF, where
// han_cp has nothing.
__device__ __forceinline__ uint32_t han_rune(uint32_t x, uint32_t lim, uint32_t* w) {
    const uint32_t b0 = x & 0xFFu;
    if ((x & 0x00C0C0F0u) == 0x008080E0u) {
        const uint32_t r = ((b0 & 0x0Fu) << 12) | (((x >> 8) & 0x3Fu) << 6) | ((x >> 16) & 0x3Fu);
        if (lim < 3u || !han_cp(r)) return 0u;
        *w = 3u;
        return r;
    }
    if ((x & 0xC0C0C0F8u) == 0x808080F0u) {
        const uint32_t r =
            ((b0 & 0x07u) << 18) | (((x >> 8) & 0x3Fu) << 12) | (((x >> 16) & 0x3Fu) << 6) | ((x >> 24) & 0x3Fu);
        if (lim < 4u || r < 0x10000u || !han_cp(r)) return 0u;
        *w = 4u;
        return r;
    }
    return 0u;
}

// One trie step in the double array: the cell that holds rune r (code k) under
// the node whose cell is c; a hit when its check names that node.
__device__ __forceinline__ uint32_t rune_code(const DevImage& im, uint32_t r) {
    return im.code[jb_row(im.pagemap, r)];
}
__device__ __forceinline__ uint32_t dat_slot_k(uint64_t c, uint32_t k) { return jb_cell_base(c) + k; }
__device__ __forceinline__ uint32_t dat_slot(const DevImage& im, uint64_t c, uint32_t r) {
    return dat_slot_k(c, rune_code(im, r));
}
__device__ __forceinline__ bool dat_hit(uint64_t child, uint32_t id) { return jb_cell_check(child) == id + 1u; }

// The first block start after chunk c (16 bytes each), or nbytes: the rest of c's
// tile chunk by chunk, then whole tiles by their block counts (tile_cnt.x).
__device__ inline uint32_t nz_block_end(const uint32_t* __restrict__ lanemask, const uint2* __restrict__ tile_cnt,
                                 uint32_t ntiles, uint32_t nbytes, uint32_t c) {
    const uint32_t nch = ntiles * 256u;
    uint32_t k = c + 1u;
    while (k < nch) {
        if ((k & 255u) == 0u) {
            uint32_t t = k >> 8;
            while (t < ntiles && tile_cnt[t].x == 0u) t++;
            if (t >= ntiles) break;
            k = t * 256u;
        }
        const uint32_t m = lanemask[k] & 0xFFFFu;
        if (m) return min(nbytes, k * 16u + (uint32_t)__builtin_ctz(m));
        k++;
    }
    return nbytes;
}

// The end of the block that starts at byte bs: the next block start of any kind
// (k_mark_walk's lane masks), or nbytes.
__device__ inline uint32_t block_end_at(const uint32_t* __restrict__ lanemask, const uint2* __restrict__ tile_cnt,
                                 uint32_t ntiles, uint32_t nbytes, uint32_t bs) {
    const uint32_t c = bs >> 4;
    const uint32_t above = lanemask[c] & 0xFFFFu & ~((2u << (bs & 15u)) - 1u);
    if (above) return c * 16u + (uint32_t)__builtin_ctz(above);
    return nz_block_end(lanemask, tile_cnt, ntiles, nbytes, c);
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// c ? a : b for a mask c of all ones or zero, as two v_bfi_b32 (a select the compiler
// keeps: it turns ternaries whose arms are loads into exec-mask branches)
__device__ __forceinline__ double bitsel64(uint32_t m, double a, double b) {
    const uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
    uint32_t lo, hi;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(lo) : "v"(m), "v"((uint32_t)ua), "v"((uint32_t)ub));
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(hi) : "v"(m), "v"((uint32_t)(ua >> 32)), "v"((uint32_t)(ub >> 32)));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

}  // namespace jb
