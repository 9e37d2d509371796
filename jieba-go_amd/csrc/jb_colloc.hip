// jb_colloc.hip — gfx950 kernels of the collocation calls (jb_colloc_init_device, jb_colloc_add_device,
// jb_colloc_score_device; the rule is jb_colloc_count's and jb_colloc_score's, jb_colloc.cpp; the table and the
// code shared with the host are jb_colloc.h's).
//
// A batch is added by four launches: two small ones that build the boundary bitmap, then two passes with one lane
// per token k < n = min(*ntok, ids_cap) in tiles of kClTile consecutive tokens (jb_wc.hip's shape).  No lane
// waits for another anywhere: there is no spin and no lock, every probe is bounded by nslots steps, and what one
// pass hands to the next travels across the kernel boundary.
//   k_cl_zero    empties the bitmap of ids_cap + 1 bits in d_work.
//   k_cl_bounds  one lane per d <= ndocs sets bit doc_tok[d] of the bitmap (atomicOr; a run of empty documents
//                sets one bit several times), so "is k + 1 the first token of a document" is one bit.
//   k_cl_claim   a lane decides whether (k, k + 1) takes part (jb_cl_pair) and finds the slot of its key from the
//                home slot on: a plain load first, so the keys the table already holds cost reads only; an empty
//                slot is confirmed by a load that bypasses the L1 and then, while fewer than nslots / 2 slots
//                are counted as claimed, claimed by one atomicCAS of the whole key (the count follows the claim).
//                work[k] = the slot, JB_CL_NOSLOT or JB_CL_NOPAIR.
//   k_cl_count   every token of a document with id < nuni adds 1 to uni[id]; every pair adds 1 to its slot's
//                count.  A pair without a slot looks its key up once more (the table no longer changes: a lane
//                that saw the half full while another claimed its key finds it now) and is dropped when it is
//                not there, so a key that is in the table has its exact count.  The totals are summed per
//                workgroup in LDS and added once.
//                Form 0: one global u64 atomic per pair and per unigram.  Form 1 (k_df_combine's shape): a
//                workgroup owns a contiguous share of at least kClShare tiles and two direct-mapped tables in
//                LDS, one keyed by slot and one by id, which it adds to memory at its end; an entry that finds
//                another one's tag goes to memory itself.
// Stale reads cost an atomic and never a result: a slot only goes from empty to its key, and every decision
// that matters is an atomic's return value.  ids, start and end are read only below n, keep only below nkeep,
// uni only below nuni, the bitmap only at bits <= n.
//
// k_cl_score is one lane per slot: jb_cl_score, then a wave ballot, one atomicAdd per wave with a candidate for
// the positions, and the stores below ccap.
#include <hip/hip_runtime.h>

#include "jb_colloc.h"
#include "jb_kernels.h"
#include "jb_kstages.h"

#include <algorithm>

namespace jb {

namespace {

constexpr uint32_t T = kClTile;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// The table of a buffer of ntable bytes, by its own header; mask == 0 when there is none: the kernels then do
// nothing.
__device__ __forceinline__ JbClView cl_table(void* table, uint64_t ntable) {
    const JbClHeader* h = (const JbClHeader*)table;
    const uint64_t nslots = h->nslots;
    const bool ok = h->magic == JB_CL_MAGIC && jb_cl_slots_ok(nslots) && jb_cl_bytes(nslots) <= ntable;
    return jb_cl_view(table, ok ? nslots : 1u);
}

__device__ __forceinline__ uint64_t ld_agent64(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The slot of key, claimed if need be, or JB_CL_NOSLOT.  At most nslots steps.
__device__ __forceinline__ uint32_t cl_claim(const JbClView& v, uint64_t key) {
    const uint64_t limit = ((uint64_t)v.mask + 1u) / 2u;
    uint32_t s = jb_cl_home(key, v.mask);
    for (uint32_t step = 0; step <= v.mask; step++, s = jb_cl_next(s, v.mask)) {
        uint64_t f = v.key[s];
        if (f == JB_CL_EMPTY) f = ld_agent64(&v.key[s]);  // (the L1 may hold the line from before the claim)
        if (f == JB_CL_EMPTY) {
            if (ld_agent64((const uint64_t*)&v.hdr->ctr[JB_CL_DISTINCT]) >= limit) return JB_CL_NOSLOT;  // no new keys
            f = atomicCAS((unsigned long long*)&v.key[s], (unsigned long long)JB_CL_EMPTY, (unsigned long long)key);
            if (f == JB_CL_EMPTY) {
                atomicAdd(&v.hdr->ctr[JB_CL_DISTINCT], 1ull);
                return s;
            }
        }
        if (f == key) return s;
    }
    return JB_CL_NOSLOT;
}

// The bitmap emptied (by a kernel and not a memset, so that a buffer without a table leaves d_work as it is).
__global__ __launch_bounds__(256) void k_cl_zero(const void* table, uint64_t ntable, uint32_t* __restrict__ bits,
                                                 uint64_t nwords) {
    if (cl_table(const_cast<void*>(table), ntable).mask == 0u) return;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nwords; i += stride) bits[i] = 0u;
}

__global__ __launch_bounds__(256) void k_cl_bounds(const void* table, uint64_t ntable, const uint64_t* __restrict__ doc_tok,
                                                   uint32_t ndocs, const uint64_t* __restrict__ ntok, uint64_t cap,
                                                   uint32_t* __restrict__ bits) {
    if (cl_table(const_cast<void*>(table), ntable).mask == 0u) return;
    const uint64_t n = std::min(*ntok, cap);
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t d = (uint64_t)blockIdx.x * 256u + threadIdx.x; d <= ndocs; d += stride) {
        const uint64_t p = doc_tok[d];
        if (p <= n) atomicOr(&bits[p >> 5], 1u << (p & 31u));
    }
}

struct ClBatch {
    const uint32_t* ids;
    const uint64_t* doc_tok;
    const uint64_t* ntok;
    uint64_t cap;
    uint32_t ndocs;
    const uint8_t* keep;
    uint32_t nkeep, flags;
    const uint32_t *start, *end;
    uint32_t nuni;
};

__global__ __launch_bounds__(256) void k_cl_claim(void* table, uint64_t ntable, ClBatch q, const uint32_t* __restrict__ bits,
                                                  uint32_t* __restrict__ work) {
    const JbClView v = cl_table(table, ntable);
    if (v.mask == 0u) return;
    const uint64_t n = std::min(*q.ntok, q.cap);
    uint64_t lo, hi;
    jb_cl_range(q.doc_tok, q.ndocs, n, &lo, &hi);
    const uint64_t step = (uint64_t)gridDim.x * T;
    for (uint64_t k = (uint64_t)blockIdx.x * T + threadIdx.x; k < n; k += step) {
        uint32_t code = JB_CL_NOPAIR;
        if (k >= lo && k + 1u < hi) {
            const uint32_t a = q.ids[k], b = q.ids[k + 1u];
            if (jb_cl_pair(k, hi, jb_cl_bit(bits, k + 1u), a, b, q.nuni, q.keep, q.nkeep, q.flags, q.start, q.end))
                code = cl_claim(v, jb_cl_key(a, b));
        }
        work[k] = code;
    }
}

// One add to a direct-mapped LDS table; false when the entry holds another tag: the caller goes to memory.
__device__ __forceinline__ bool lds_add(uint32_t* tag, uint32_t* cnt, uint32_t what) {
    const uint32_t ls = what & (kClLds - 1u);
    uint32_t t = __hip_atomic_load(&tag[ls], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (t == kNone) {
        t = atomicCAS(&tag[ls], kNone, what);
        if (t == kNone) t = what;
    }
    if (t != what) return false;
    atomicAdd(&cnt[ls], 1u);
    return true;
}

template <bool COMBINE>
__global__ __launch_bounds__(256) void k_cl_count(void* table, uint64_t ntable, ClBatch q, uint64_t* __restrict__ uni,
                                                  const uint32_t* __restrict__ work) {
    __shared__ uint32_t ptag[COMBINE ? kClLds : 1], pcnt[COMBINE ? kClLds : 1];
    __shared__ uint32_t utag[COMBINE ? kClLds : 1], ucnt[COMBINE ? kClLds : 1];
    __shared__ uint32_t s_ctr[3];
    const JbClView v = cl_table(table, ntable);
    if (v.mask == 0u) return;
    const uint64_t n = std::min(*q.ntok, q.cap);
    uint64_t lo, hi;
    jb_cl_range(q.doc_tok, q.ndocs, n, &lo, &hi);
    const uint32_t th = threadIdx.x;
    if (th < 3u) s_ctr[th] = 0u;
    if (COMBINE)
        for (uint32_t i = th; i < kClLds; i += 256u) {
            ptag[i] = kNone;
            pcnt[i] = 0u;
            utag[i] = kNone;
            ucnt[i] = 0u;
        }
    __syncthreads();
    uint32_t c[3] = {0u, 0u, 0u};  // known, pairs, dropped of this lane's tokens
    auto body = [&](uint64_t k) {
        if (k < lo || k >= hi) return;
        const uint32_t a = q.ids[k];
        if (a < q.nuni) {
            c[0]++;
            if (!COMBINE || !lds_add(utag, ucnt, a)) atomicAdd((unsigned long long*)&uni[a], 1ull);
        }
        uint32_t slot = work[k];
        if (slot == JB_CL_NOPAIR) return;
        c[1]++;
        if (slot > v.mask) slot = jb_cl_find(v.key, v.mask, jb_cl_key(a, q.ids[k + 1u]));  // (a pair: k + 1 < hi)
        if (slot == JB_CL_NOSLOT) {
            c[2]++;
            return;
        }
        if (!COMBINE || !lds_add(ptag, pcnt, slot)) atomicAdd((unsigned long long*)&v.cnt[slot], 1ull);
    };
    if (COMBINE) {
        // a contiguous share of whole tiles (under 2^32 tokens, so an LDS count fits 32 bits)
        const uint64_t tiles = (n + T - 1u) / T;
        const uint64_t share = std::max<uint64_t>((tiles + gridDim.x - 1u) / gridDim.x, kClShare);
        const uint64_t first = (uint64_t)blockIdx.x * share * T, last = std::min(n, first + share * T);
        for (uint64_t k = first + th; k < last; k += T) body(k);
    } else {
        const uint64_t step = (uint64_t)gridDim.x * T;
        for (uint64_t k = (uint64_t)blockIdx.x * T + th; k < n; k += step) body(k);
    }
#pragma unroll
    for (uint32_t j = 0; j < 3u; j++)
        if (c[j]) atomicAdd(&s_ctr[j], c[j]);
    __syncthreads();
    if (th < 3u && s_ctr[th]) atomicAdd(&v.hdr->ctr[JB_CL_KNOWN + th], (unsigned long long)s_ctr[th]);
    if (blockIdx.x == 0 && th == 3u && n) atomicAdd(&v.hdr->ctr[JB_CL_TOKENS], (unsigned long long)n);
    if (COMBINE)
        for (uint32_t i = th; i < kClLds; i += 256u) {
            const uint32_t pc = pcnt[i], uc = ucnt[i];
            if (pc) atomicAdd((unsigned long long*)&v.cnt[ptag[i]], (unsigned long long)pc);
            if (uc) atomicAdd((unsigned long long*)&uni[utag[i]], (unsigned long long)uc);
        }
}

__global__ __launch_bounds__(256) void k_cl_init(void* table, uint64_t nslots, uint64_t* __restrict__ uni, uint32_t nuni) {
    const JbClView v = jb_cl_view(table, nslots);
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < nslots; s += stride) {
        v.key[s] = JB_CL_EMPTY;
        v.cnt[s] = 0u;
    }
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nuni; i += stride) uni[i] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        JbClHeader h{};
        h.magic = JB_CL_MAGIC;
        h.nslots = nslots;
        *v.hdr = h;
    }
}

__global__ __launch_bounds__(256) void k_cl_score(const void* table, uint64_t ntable, const uint64_t* __restrict__ uni,
                                                  uint32_t nuni, int scorer, uint64_t min_count, float threshold,
                                                  uint32_t* __restrict__ ca, uint32_t* __restrict__ cb,
                                                  uint64_t* __restrict__ cc, float* __restrict__ cs, uint64_t ccap,
                                                  unsigned long long* __restrict__ ncand) {
    const JbClView v = cl_table(const_cast<void*>(table), ntable);
    if (v.mask == 0u) return;
    const uint64_t N = v.hdr->ctr[JB_CL_KNOWN], nslots = (uint64_t)v.mask + 1u;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    // whole waves step together, so that the ballot sees every lane of the wave
    for (uint64_t s0 = (uint64_t)blockIdx.x * 256u; s0 < nslots; s0 += stride) {
        const uint64_t s = s0 + threadIdx.x;
        uint64_t key = JB_CL_EMPTY, c = 0;
        float score = 0.0f;
        bool cand = false;
        if (s < nslots) {
            key = v.key[s];
            c = v.cnt[s];
            cand = key != JB_CL_EMPTY && jb_cl_score(key, c, uni, nuni, N, min_count, scorer, threshold, &score);
        }
        const uint64_t bal = __ballot(cand);
        if (bal == 0u) continue;
        const uint32_t lane = __lane_id();
        unsigned long long base = 0;
        if (lane == (uint32_t)__ffsll((long long)bal) - 1u) base = atomicAdd(ncand, (unsigned long long)__popcll(bal));
        base = __shfl(base, __ffsll((long long)bal) - 1);
        if (cand) {
            const uint64_t at = base + __popcll(bal & ((1ull << lane) - 1u));
            if (at < ccap) {
                ca[at] = (uint32_t)(key >> 32);
                cb[at] = (uint32_t)key;
                cc[at] = c;
                cs[at] = score;
            }
        }
    }
}

}  // namespace

hipError_t run_colloc_init(void* d_table, uint64_t nslots, uint64_t* d_uni, uint32_t nuni, uint32_t ncu,
                           hipStream_t stream) {
    const uint64_t most = std::max<uint64_t>(nslots, nuni);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((most + 255u) / 256u, (uint64_t)std::max(1u, ncu) * 8u);
    hipLaunchKernelGGL(k_cl_init, dim3(grid), dim3(256), 0, stream, d_table, nslots, d_uni, nuni);
    return hipGetLastError();
}

hipError_t run_colloc_add(void* d_table, uint64_t ntable, uint64_t* d_uni, uint32_t nuni, const uint32_t* d_ids,
                          uint64_t ids_cap, const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint32_t ndocs,
                          const uint8_t* d_keep, uint32_t nkeep, uint32_t flags, const uint32_t* d_start,
                          const uint32_t* d_end, bool combine, void* d_work, uint32_t ncu, hipStream_t stream,
                          KernelTimer* timer) {
    if (ids_cap == 0) return hipSuccess;  // (no token exists)
    uint32_t* work = (uint32_t*)d_work;
    uint32_t* bits = (uint32_t*)((uint8_t*)d_work + jb_cl_work_slots(ids_cap));
    const ClBatch q{d_ids, d_doc_tok, d_ntok, ids_cap, ndocs, d_keep, nkeep, flags, d_start, d_end, nuni};
    const uint64_t tiles = (ids_cap + T - 1u) / T;
    const uint32_t cus = std::max(1u, ncu);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)cus * kIdsWgPerCu);
    const uint32_t gb = (uint32_t)std::min<uint64_t>(((uint64_t)ndocs + 256u) / 256u, (uint64_t)cus * kIdsWgPerCu);
    const uint64_t nwords = jb_cl_work_bitwords(ids_cap);
    const uint32_t gz = (uint32_t)std::min<uint64_t>((nwords + 255u) / 256u, (uint64_t)cus * kIdsWgPerCu);
    JB_TIMED(K_CL_ZERO, hipLaunchKernelGGL(k_cl_zero, dim3(gz), dim3(256), 0, stream, (const void*)d_table, ntable, bits,
                                           nwords));
    JB_TIMED(K_CL_BOUNDS, hipLaunchKernelGGL(k_cl_bounds, dim3(gb), dim3(256), 0, stream, (const void*)d_table, ntable,
                                             d_doc_tok, ndocs, d_ntok, ids_cap, bits));
    JB_TIMED(K_CL_CLAIM, hipLaunchKernelGGL(k_cl_claim, dim3(grid), dim3(256), 0, stream, d_table, ntable, q,
                                            (const uint32_t*)bits, work));
    if (combine) {
        const uint64_t shares = (tiles + kClShare - 1u) / kClShare;
        const uint32_t g1 = (uint32_t)std::min<uint64_t>(shares, (uint64_t)cus * 5u);
        JB_TIMED(K_CL_COUNT, hipLaunchKernelGGL(k_cl_count<true>, dim3(g1), dim3(256), 0, stream, d_table, ntable, q, d_uni,
                                                (const uint32_t*)work));
    } else {
        JB_TIMED(K_CL_COUNT, hipLaunchKernelGGL(k_cl_count<false>, dim3(grid), dim3(256), 0, stream, d_table, ntable, q,
                                                d_uni, (const uint32_t*)work));
    }
    return hipGetLastError();
}

hipError_t run_colloc_score(const void* d_table, uint64_t ntable, uint64_t nslots_hint, const uint64_t* d_uni, uint32_t nuni,
                            int scorer, uint64_t min_count, float threshold, uint32_t* d_cand_a, uint32_t* d_cand_b,
                            uint64_t* d_cand_cnt, float* d_cand_score, uint64_t ccap, uint64_t* d_ncand, uint32_t ncu,
                            hipStream_t stream, KernelTimer* timer) {
    hipError_t e = hipMemsetAsync(d_ncand, 0, 8, stream);
    if (e != hipSuccess) return e;
    const uint32_t grid =
        (uint32_t)std::min<uint64_t>((std::max<uint64_t>(nslots_hint, 1u) + 255u) / 256u, (uint64_t)std::max(1u, ncu) * 8u);
    JB_TIMED(K_CL_SCORE, hipLaunchKernelGGL(k_cl_score, dim3(grid), dim3(256), 0, stream, d_table, ntable, d_uni, nuni, scorer,
                                            min_count, threshold, d_cand_a, d_cand_b, d_cand_cnt, d_cand_score, ccap,
                                            (unsigned long long*)d_ncand));
    return hipGetLastError();
}

}  // namespace jb
