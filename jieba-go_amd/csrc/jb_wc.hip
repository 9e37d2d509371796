// jb_wc.hip — gfx950 kernels of the word counts (jb_wc_init_device, jb_wc_add_device; the rule is
// jb_wc_count's, jb_wc.cpp; the table and the code shared with the host are jb_wc.h's).
//
// A batch is added by three passes over its tokens k < n = min(*ntok, cap), one lane per token, tiles of
// kWcTile consecutive tokens under a fixed grid (k_ids' loop).  No lane waits for another anywhere: there
// is no spin and no lock, every probe is bounded by nslots steps, and what one pass hands to the next
// travels across the kernel boundary.
//   k_wc_claim  builds the key in registers (ids_one's reads), hashes it and finds the slot of its
//               fingerprint from the home slot on: a plain load first, so the words the table already
//               holds cost reads only; an empty slot is confirmed by a load that bypasses the L1 and then,
//               while fewer than nslots / 2 slots are counted as claimed, claimed by one atomicCAS (the
//               count follows the claim, so no lane is turned away while there is room; lanes that claim
//               at the same moment can take the table past the half, never past nslots).  work[k] = the
//               slot, or JB_WC_NOSLOT.  While the slot's bytes are not stored, rep = min(rep, k) (an
//               atomicMin only when k is below what a load shows).
//   k_wc_store  the token with k == rep of a slot without bytes writes them (jb_wc_put); a key over 24
//               bytes takes its place in the pool by one atomicAdd, and the slot is dead when there is none.
//   k_wc_count  every token compares its bytes with its slot's (jb_wc_same): equal adds 1 to the slot's
//               count, different is a collision; a dead slot's token is dropped.  A token without a slot
//               looks its fingerprint up once more (the table no longer changes: a lane that saw the half
//               full while another claimed its key finds it now), and is dropped when it is not there.
//               The five totals are summed per workgroup in LDS and added once.
//               Form 0: one global u64 atomic per token.  Form 1 (k_df_combine's shape): a workgroup owns a
//               contiguous share of the tiles and a direct-mapped table in LDS keyed by slot, which it adds
//               to the counts at its end; a slot that finds another one's tag goes to memory itself.
// Stale reads cost an atomic and never a result: a slot only goes from empty to its fingerprint, rep only
// falls, and every decision that matters is an atomic's return value.  Text bytes are read only for spans
// with start < end <= nbytes, in [start & ~3, start + 28) or inside the span: never at or past nbytes + 64.
#include <hip/hip_runtime.h>

#include "jb_kstages.h"
#include "jb_wc.h"

#include <algorithm>

namespace jb {

namespace {

constexpr uint32_t T = kWcTile;

// The table of a buffer of ntable bytes, by its own header; mask == 0 when there is none (a buffer that
// jb_wc_init_device did not fill, or one shorter than its sizes ask for): the kernels then do nothing.
__device__ __forceinline__ JbWcView wc_table(void* table, uint64_t ntable) {
    const JbWcHeader* h = (const JbWcHeader*)table;
    const uint64_t nslots = h->nslots, pool = h->pool_bytes;
    const bool ok = h->magic == JB_WC_MAGIC && nslots >= JB_WC_MIN_SLOTS && nslots <= JB_WC_MAX_SLOTS &&
                    (nslots & (nslots - 1u)) == 0 && pool < (1ull << 32) && jb_wc_bytes(nslots, pool) <= ntable;
    JbWcView v = jb_wc_view(table, ok ? nslots : 1u, pool);
    return v;
}

__device__ __forceinline__ uint32_t wc_word_mask(uint32_t len, uint32_t w) {
    if (len >= 4u * w + 4u) return 0xFFFFFFFFu;
    return len > 4u * w ? (1u << (8u * (len - 4u * w))) - 1u : 0u;
}

// The key of span [s, e): 0 and (kw, *len) as jb_vocab_hash takes them (the tail is text + s), or
// JB_WC_BADSPAN / JB_WC_LONGKEY without a text read.  ids_one's reads.
__device__ __forceinline__ uint32_t wc_key(const uint8_t* __restrict__ text, uint32_t nbytes, uint32_t s, uint32_t e,
                                           uint32_t kw[6], uint32_t* plen) {
    if (s >= e || e > nbytes) return JB_WC_BADSPAN;
    uint32_t len = e - s;
    if (len > JB_VOCAB_MAXKEY) return JB_WC_LONGKEY;
    const uint32_t* a = reinterpret_cast<const uint32_t*>(text + (s & ~3u));
    const uint32_t sh = s & 3u;
#pragma unroll
    for (uint32_t w = 0; w < 6u; w++) kw[w] = 0u;
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
        for (uint32_t w = 0; w < 6u; w++) kw[w] &= wc_word_mask(len, w);
    }
    *plen = len;
    return 0u;
}

// k_ids' tile loop: body(i, s, e) for every token i < n this workgroup owns from `first` on in steps of
// `step` tokens; the next span is loaded one trip ahead.
template <class Body>
__device__ __forceinline__ void wc_tiles(const uint32_t* __restrict__ ts, const uint32_t* __restrict__ te, uint64_t first,
                                         uint64_t n, uint64_t step, Body body) {
    uint64_t i = first + threadIdx.x;
    uint32_t s1 = 0, e1 = 0;
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
        body(i, s, e);
    }
}

__device__ __forceinline__ uint64_t ld_agent64(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_agent32(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The slot of fp, claimed if need be, or JB_WC_NOSLOT.  At most nslots steps.
__device__ __forceinline__ uint32_t wc_claim(const JbWcView& v, uint64_t fp) {
    const uint32_t limit = (v.mask + 1u) / 2u;
    uint32_t s = jb_wc_home(fp, v.mask);
    for (uint32_t step = 0; step <= v.mask; step++, s = jb_vocab_next(s, v.mask)) {
        uint64_t f = v.fp[s];
        if (f == 0u) f = ld_agent64(&v.fp[s]);  // (the L1 may hold the line from before the claim)
        if (f == 0u) {
            if (ld_agent32(&v.hdr->nclaimed) >= limit) return JB_WC_NOSLOT;  // no new keys any more
            f = atomicCAS((unsigned long long*)&v.fp[s], 0ull, (unsigned long long)fp);
            if (f == 0u) {
                atomicAdd(&v.hdr->nclaimed, 1u);
                return s;
            }
        }
        if (f == fp) return s;
    }
    return JB_WC_NOSLOT;
}

__global__ __launch_bounds__(256) void k_wc_claim(const uint8_t* __restrict__ text, uint32_t nbytes, void* table,
                                                  uint64_t ntable, const uint32_t* __restrict__ ts,
                                                  const uint32_t* __restrict__ te, const uint64_t* __restrict__ ntok,
                                                  uint64_t cap, uint32_t bits, uint32_t* __restrict__ work) {
    const JbWcView v = wc_table(table, ntable);
    if (v.mask == 0u) return;
    const uint64_t n = std::min(*ntok, cap);
    wc_tiles(ts, te, (uint64_t)blockIdx.x * T, n, (uint64_t)gridDim.x * T, [&](uint64_t i, uint32_t s, uint32_t e) {
        uint32_t kw[6], len = 0;
        const uint32_t code = wc_key(text, nbytes, s, e, kw, &len);
        if (code) {
            work[i] = code;
            return;
        }
        const uint64_t fp = jb_wc_fp_of(jb_vocab_hash(kw, text + s, len), bits);
        const uint32_t slot = wc_claim(v, fp);
        work[i] = slot;
        if (slot == JB_WC_NOSLOT) return;
        uint32_t* q = v.key + (uint64_t)slot * JB_VOCAB_SLOT_WORDS;
        if (q[0] != 0u) return;  // the bytes are stored (or the slot is dead): an earlier batch's slot
        const uint32_t k = (uint32_t)i;
        if (q[1] > k && ld_agent32(&q[1]) > k) atomicMin(&q[1], k);
    });
}

__global__ __launch_bounds__(256) void k_wc_store(const uint8_t* __restrict__ text, uint32_t nbytes, void* table,
                                                  uint64_t ntable, const uint32_t* __restrict__ ts,
                                                  const uint32_t* __restrict__ te, const uint64_t* __restrict__ ntok,
                                                  uint64_t cap, const uint32_t* __restrict__ work) {
    const JbWcView v = wc_table(table, ntable);
    if (v.mask == 0u) return;
    const uint64_t n = std::min(*ntok, cap);
    wc_tiles(ts, te, (uint64_t)blockIdx.x * T, n, (uint64_t)gridDim.x * T, [&](uint64_t i, uint32_t s, uint32_t e) {
        const uint32_t slot = work[i];
        if (slot > v.mask) return;
        uint32_t* q = v.key + (uint64_t)slot * JB_VOCAB_SLOT_WORDS;
        if (q[1] != (uint32_t)i || q[0] != 0u) return;  // (exactly one token of the batch passes, per new slot)
        uint32_t kw[6], len = 0;
        if (wc_key(text, nbytes, s, e, kw, &len)) return;
        uint32_t off = 0;
        if (len > JB_VOCAB_INLINE) {
            const unsigned long long o = atomicAdd(&v.hdr->pool_used, (unsigned long long)len);
            if (o + len > v.pool_bytes) {
                q[0] = JB_WC_DEAD;
                return;
            }
            off = (uint32_t)o;
        }
        jb_wc_put(q, v.pool, kw, text + s, len, jb_vocab_hash(kw, text + s, len), off);
    });
}

constexpr uint32_t kWcLds = 4096;  // form 1's table: 32 KiB of LDS, five workgroups per CU
constexpr uint32_t kWcNone = 0xFFFFFFFFu;

template <bool COMBINE>
__global__ __launch_bounds__(256) void k_wc_count(const uint8_t* __restrict__ text, uint32_t nbytes, void* table,
                                                  uint64_t ntable, const uint32_t* __restrict__ ts,
                                                  const uint32_t* __restrict__ te, const uint64_t* __restrict__ ntok,
                                                  uint64_t cap, uint32_t bits, const uint32_t* __restrict__ work) {
    __shared__ uint32_t tag[COMBINE ? kWcLds : 1], cnt[COMBINE ? kWcLds : 1];
    __shared__ uint32_t s_ctr[4];
    const JbWcView v = wc_table(table, ntable);
    if (v.mask == 0u) return;
    const uint64_t n = std::min(*ntok, cap);
    const uint32_t th = threadIdx.x;
    if (th < 4u) s_ctr[th] = 0u;
    if (COMBINE)
        for (uint32_t i = th; i < kWcLds; i += 256u) {
            tag[i] = kWcNone;
            cnt[i] = 0u;
        }
    __syncthreads();
    uint32_t c[4] = {0u, 0u, 0u, 0u};  // JB_WC_BAD .. JB_WC_COLLIDED of this lane's tokens
    auto body = [&](uint64_t i, uint32_t s, uint32_t e) {
        uint32_t kw[6], len = 0;
        const uint32_t code = wc_key(text, nbytes, s, e, kw, &len);
        if (code) {
            c[code == JB_WC_BADSPAN ? JB_WC_BAD : JB_WC_LONG]++;
            return;
        }
        const uint64_t h = jb_vocab_hash(kw, text + s, len);
        uint32_t slot = work[i];
        if (slot > v.mask) slot = jb_wc_find(v.fp, v.mask, jb_wc_fp_of(h, bits));
        if (slot == JB_WC_NOSLOT) {
            c[JB_WC_DROPPED]++;
            return;
        }
        const uint32_t* q = v.key + (uint64_t)slot * JB_VOCAB_SLOT_WORDS;
        const uint32_t head = q[0];
        if (head == JB_WC_DEAD || head == 0u) {
            c[JB_WC_DROPPED]++;
            return;
        }
        if (!jb_wc_same(q, v.pool, kw, text + s, len, h)) {
            c[JB_WC_COLLIDED]++;
            return;
        }
        if (COMBINE) {
            const uint32_t ls = slot & (kWcLds - 1u);
            uint32_t t = __hip_atomic_load(&tag[ls], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (t == kWcNone) {
                t = atomicCAS(&tag[ls], kWcNone, slot);
                if (t == kWcNone) t = slot;
            }
            if (t == slot) {
                atomicAdd(&cnt[ls], 1u);
                return;
            }
        }
        atomicAdd((unsigned long long*)&v.cnt[slot], 1ull);
    };
    if (COMBINE) {
        // a contiguous share of whole tiles (under 2^32 tokens, so an LDS count fits 32 bits)
        const uint64_t tiles = (n + T - 1u) / T, share = (tiles + gridDim.x - 1u) / gridDim.x;
        const uint64_t first = (uint64_t)blockIdx.x * share * T;
        wc_tiles(ts, te, first, std::min(n, first + share * T), T, body);
    } else {
        wc_tiles(ts, te, (uint64_t)blockIdx.x * T, n, (uint64_t)gridDim.x * T, body);
    }
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++)
        if (c[j]) atomicAdd(&s_ctr[j], c[j]);
    __syncthreads();
    if (th < 4u && s_ctr[th]) atomicAdd((unsigned long long*)&v.hdr->ctr[th], (unsigned long long)s_ctr[th]);
    if (blockIdx.x == 0 && th == 4u && n) atomicAdd((unsigned long long*)&v.hdr->ctr[JB_WC_TOKENS], (unsigned long long)n);
    if (COMBINE)
        for (uint32_t i = th; i < kWcLds; i += 256u) {
            const uint32_t k = cnt[i];
            if (k) atomicAdd((unsigned long long*)&v.cnt[tag[i]], (unsigned long long)k);
        }
}

__global__ __launch_bounds__(256) void k_wc_init(void* table, uint64_t nslots, uint64_t pool_bytes) {
    const JbWcView v = jb_wc_view(table, nslots, pool_bytes);
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < nslots; s += stride) {
        v.fp[s] = 0u;
        v.cnt[s] = 0u;
        uint4* q = (uint4*)(v.key + s * JB_VOCAB_SLOT_WORDS);
        q[0] = make_uint4(0u, JB_WC_NOREP, 0u, 0u);
        q[1] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        JbWcHeader h{};
        h.magic = JB_WC_MAGIC;
        h.nslots = nslots;
        h.pool_bytes = pool_bytes;
        *v.hdr = h;
    }
}

}  // namespace

hipError_t run_wc_init(void* d_table, uint64_t nslots, uint64_t pool_bytes, uint32_t ncu, hipStream_t stream) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((nslots + 255u) / 256u, (uint64_t)std::max(1u, ncu) * 8u);
    hipLaunchKernelGGL(k_wc_init, dim3(grid), dim3(256), 0, stream, d_table, nslots, pool_bytes);
    return hipGetLastError();
}

hipError_t run_wc_add(void* d_table, uint64_t ntable, const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start,
                      const uint32_t* d_end, const uint64_t* d_ntok, uint64_t cap, uint32_t bits, bool combine,
                      uint32_t* d_work, uint32_t ncu, hipStream_t stream, KernelTimer* timer) {
    if (cap == 0) return hipSuccess;  // (no token takes part)
    const uint64_t tiles = (cap + T - 1u) / T;
    const uint32_t cus = std::max(1u, ncu);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)cus * kIdsWgPerCu);
    const uint32_t nb = (uint32_t)nbytes;
    JB_TIMED(K_WC_CLAIM, hipLaunchKernelGGL(k_wc_claim, dim3(grid), dim3(256), 0, stream, d_text, nb, d_table, ntable,
                                            d_start, d_end, d_ntok, cap, bits, d_work));
    JB_TIMED(K_WC_STORE, hipLaunchKernelGGL(k_wc_store, dim3(grid), dim3(256), 0, stream, d_text, nb, d_table, ntable,
                                            d_start, d_end, d_ntok, cap, d_work));
    if (combine) {
        const uint32_t g1 = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)cus * 5u);
        JB_TIMED(K_WC_COUNT, hipLaunchKernelGGL(k_wc_count<true>, dim3(g1), dim3(256), 0, stream, d_text, nb, d_table,
                                                ntable, d_start, d_end, d_ntok, cap, bits, d_work));
    } else {
        JB_TIMED(K_WC_COUNT, hipLaunchKernelGGL(k_wc_count<false>, dim3(grid), dim3(256), 0, stream, d_text, nb, d_table,
                                                ntable, d_start, d_end, d_ntok, cap, bits, d_work));
    }
    return hipGetLastError();
}

}  // namespace jb
