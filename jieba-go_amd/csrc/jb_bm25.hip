// jb_bm25.hip — gfx950 kernels of the BM25 calls (jb_bm25_norms_device, jb_bm25_idf_device,
// jb_bm25_search_device; the rule is jb_bm25_search's, jb_bm25.cpp; the code shared with the host is jb_bm25.h's).
//
//   k_bm25_norms   one lane per document: norm[d] (jb_bm25_norm).
//   k_bm25_idf     one lane per id: weight[t] (jb_bm25_df, jb_bm25_weight).
// The search ranks the documents of an index (the postings of jb_postings*, ascending by document in every
// list) for nq queries given as a CSR of ids.  A document tile is kBm25Tile = 8192 consecutive documents.
// Form 1 (two launches):
//   k_bm25_tile    one workgroup of 512 lanes per pair of query and document tile.  The tile's 8192 u64 scores
//                  live in LDS (64 KiB; the kernel holds 73 KiB, so two workgroups share a CU's 160 KiB).  The
//                  query's entries are taken 512 at a time, one lane each: the lane checks the entry
//                  (jb_bm25_entry) and finds the part of its posting list inside the tile by two binary
//                  searches (jb_bm25_lb).  The parts' lengths are scanned, and the lanes stride over the
//                  postings of all parts together (posting k belongs to the entry found by a search in the
//                  prefixes of the chunk's entries), so a query of one frequent word and a query of 500 rare ones both keep every lane
//                  busy, and no part holds more than 8192 postings.  Each posting adds its contribution
//                  (jb_bm25_contrib) to its document's cell with an LDS atomic.  A tile that no posting reached
//                  writes a zero count and leaves.  Otherwise the workgroup selects the tile's best topk cells.
//   k_bm25_merge   one workgroup per query: the best topk of the tiles' partial records, into the row.
// Form 0 (a memset and three launches): a dense u64 row of ndocs cells per query in the work buffer;
//   k_bm25_scatter the same grid; the workgroups of a query share each entry's whole list, one lane per
//                  posting, and add with a global atomicAdd;
//   k_bm25_select  per pair of query and tile, the row's tile is copied to LDS and selected as in form 1;
//   k_bm25_merge.
// The selection.  Lane l owns the cells l, l + 512, ... of the tile and keeps the best of them in registers
// (score descending, ties by document ascending: jb_bm25_before).  A round takes the best over the workgroup
// (a butterfly in each wave, then the eight waves' leaders through LDS), writes it as the next partial record
// and clears its cell; only the owner looks at its cells again.  It ends after topk rounds or at the first
// round whose best score is 0, so a tile's partial records are its candidates in rank order, and the merge
// takes, topk times, the best record that ranks behind the one before (documents are distinct, so the order
// is strict).  The merge reads ntiles * topk records per round: 90 for the 1 GiB corpus at topk = 10.
// Scores are integers (units of 2^-24) and the order is total, so both forms write the same bytes as the host
// rule, from run to run.  There are no global atomics in form 1, and no lane waits for another workgroup in
// either.  Reads of q_id are below q_cap, of weight below nweights, of post_off at t + 1 <= nids, of post_doc /
// post_tf below npost, of norm below ndocs; LDS cells are indexed by d - tile base only after it is checked
// against the tile (a caller's unsorted list may hold any document inside a part); partial records are written
// below topk per pair and rows below topk per query.
// In k_bm25_tile a lane takes UNR = 4 postings per trip, stage by stage (positions, document and tf loads, norm
// loads, contributions), so that four loads are in flight: the kernel is bound by the latency of a trip, not by
// bandwidth.
// Measured on the 1 GiB corpus's index (profiles/bm25_bench.json; 73,443 documents, 77.3M postings; 1,024 queries
// of 1 to 8 ids drawn by corpus frequency, 141.0M postings under them, topk 10): form 1 0.96 ms (k_bm25_tile
// 0.90 ms, k_bm25_merge 0.03 ms), form 0 1.75 ms (k_bm25_scatter 1.23 ms, k_bm25_select 0.42 ms, k_bm25_merge
// 0.03 ms, the rest the memset); form 1 is the default.
#include <hip/hip_runtime.h>

#include "jb_bm25.h"
#include "jb_kstages.h"

#include <algorithm>

namespace jb {

namespace {

constexpr uint32_t T = kBm25Tile;
constexpr uint32_t NT = 512;         // lanes per workgroup of the tile kernels
constexpr uint32_t NW = NT / 64u;    // waves
constexpr uint32_t OWN = T / NT;     // cells per lane
constexpr uint32_t UNR = 4;          // postings a lane of k_bm25_tile has in flight
static_assert(kBm25Tile == JB_BM25_TILE && kBm25MaxQ == JB_BM25_MAXQ, "the header's constants");
static_assert(JB_BM25_MAXQ % NT == 0, "entries are taken NT at a time");

__global__ __launch_bounds__(256) void k_bm25_norms(const uint32_t* __restrict__ doc_len, uint32_t ndocs, double k1,
                                                    double b, double avgdl, float* __restrict__ norm) {
    const uint64_t d = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (d < ndocs) norm[d] = jb_bm25_norm(doc_len[d], k1, b, avgdl);
}

__global__ __launch_bounds__(256) void k_bm25_idf(const uint64_t* __restrict__ post_off, uint32_t nids,
                                                  uint64_t ndocs_total, float* __restrict__ weight) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t < nids) weight[t] = jb_bm25_weight(jb_bm25_df(post_off, t, ndocs_total), ndocs_total);
}

// Inclusive scan over the 64 lanes of a wave.
__device__ __forceinline__ uint32_t wave_incl(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// The best record of the workgroup (every lane gets it).  sh_s / sh_d hold NW records; the caller alternates
// between two such pairs from round to round, so one barrier per round is enough.
__device__ __forceinline__ void block_best(uint64_t* s, uint32_t* d, uint64_t* sh_s, uint32_t* sh_d) {
    uint64_t bs = *s;
    uint32_t bd = *d;
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) {
        const uint64_t os = (uint64_t)__shfl_xor((unsigned long long)bs, (int)o, 64);
        const uint32_t od = (uint32_t)__shfl_xor((int)bd, (int)o, 64);
        if (jb_bm25_before(os, od, bs, bd)) {
            bs = os;
            bd = od;
        }
    }
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        sh_s[w] = bs;
        sh_d[w] = bd;
    }
    __syncthreads();
    bs = sh_s[0];
    bd = sh_d[0];
#pragma unroll
    for (uint32_t k = 1; k < NW; k++) {
        const uint64_t os = sh_s[k];
        const uint32_t od = sh_d[k];
        if (jb_bm25_before(os, od, bs, bd)) {
            bs = os;
            bd = od;
        }
    }
    *s = bs;
    *d = bd;
}

// The best of lane th's cells of the tile (cell index, not document); score 0 when all are clear.
__device__ __forceinline__ void own_best(const uint64_t* acc, uint32_t th, uint64_t* s, uint32_t* c) {
    uint64_t bs = 0;
    uint32_t bc = th;
#pragma unroll
    for (uint32_t k = 0; k < OWN; k++) {
        const uint32_t cell = th + k * NT;  // (ascending, so the first of equal scores stays)
        const uint64_t v = acc[cell];
        if (v > bs) {
            bs = v;
            bc = cell;
        }
    }
    *s = bs;
    *c = bc;
}

// The tile's best topk cells, in rank order, as the pair's partial records and count.  acc is complete (the
// caller's barrier stands before the call).  Cells are cleared as they are taken.
__device__ __forceinline__ void tile_select(uint64_t* acc, uint64_t d0, uint32_t topk, uint64_t* __restrict__ pscore,
                                            uint32_t* __restrict__ pdoc, uint32_t* __restrict__ pcnt,
                                            uint64_t (*sh_s)[NW], uint32_t (*sh_d)[NW]) {
    const uint32_t th = threadIdx.x;
    uint64_t ms;
    uint32_t mc;
    own_best(acc, th, &ms, &mc);
    uint32_t n = 0;
    for (uint32_t r = 0; r < topk; r++) {
        uint64_t bs = ms;
        uint32_t bc = mc;
        block_best(&bs, &bc, sh_s[r & 1u], sh_d[r & 1u]);
        if (bs == 0) break;  // (the same value in every lane)
        if (th == 0) {
            pscore[r] = bs;
            pdoc[r] = (uint32_t)(d0 + bc);
        }
        n = r + 1u;
        if ((bc & (NT - 1u)) == th) {  // the owner: only its cells changed
            acc[bc] = 0;
            own_best(acc, th, &ms, &mc);
        }
    }
    if (th == 0) *pcnt = n;
}

// What a lane needs of the query entry it holds.
struct Part {
    uint64_t lo;   // the first posting of the list's part
    uint32_t len;  // postings in the part (0: the entry does not take part or has none here)
    float w;
};

// The part of entry j's list with documents in [d0, d1) (form 1), or the whole list (d0 = 0, d1 = 2^32).
__device__ __forceinline__ Part entry_part(const uint32_t* __restrict__ q_id, uint64_t qlo, uint32_t j, uint32_t n,
                                           uint32_t nids, uint32_t nweights, const float* __restrict__ weight,
                                           const uint64_t* __restrict__ post_off, const uint32_t* __restrict__ post_doc,
                                           uint64_t npost, uint64_t d0, uint64_t d1, bool whole) {
    Part p{0, 0, 0.0f};
    if (j >= n) return p;
    const uint32_t t = q_id[qlo + j];
    p.w = jb_bm25_entry(t, nids, nweights, weight);
    if (!(p.w > 0.0f)) return p;
    uint64_t lo, hi;
    jb_bm25_list(post_off, t, npost, &lo, &hi);
    if (!whole) {
        lo = jb_bm25_lb(post_doc, lo, hi, d0);
        hi = jb_bm25_lb(post_doc, lo, hi, d1);
    }
    p.lo = lo;
    // (a sorted list has at most T postings in a tile and 2^32 in all; a caller's unsorted one is cut there)
    p.len = (uint32_t)std::min<uint64_t>(hi - lo, whole ? 0xFFFFFFFFull : (uint64_t)T);
    return p;
}

// Form 1.  grid (ntiles, nq).
__global__ __launch_bounds__(NT, 4) void k_bm25_tile(
    const uint32_t* __restrict__ post_doc, const uint32_t* __restrict__ post_tf, const uint64_t* __restrict__ post_off,
    uint64_t npost, uint32_t nids, const float* __restrict__ norm, uint32_t ndocs, const float* __restrict__ weight,
    uint32_t nweights, double k1p1, const uint32_t* __restrict__ q_id, uint64_t q_cap, const uint64_t* __restrict__ q_off,
    uint32_t topk, uint64_t* __restrict__ pscore, uint32_t* __restrict__ pdoc, uint32_t* __restrict__ pcnt) {
    __shared__ uint64_t acc[T];
    __shared__ uint64_t s_lo[NT];
    __shared__ uint32_t s_pre[NT + 1];  // exclusive prefixes of the parts' lengths
    __shared__ float s_w[NT];
    __shared__ uint32_t s_ws[NW];
    __shared__ uint64_t sh_s[2][NW];
    __shared__ uint32_t sh_d[2][NW];
    const uint32_t th = threadIdx.x, lane = th & 63u, wv = th >> 6;
    const uint32_t tile = blockIdx.x, q = blockIdx.y, ntiles = gridDim.x;
    const uint64_t pair = (uint64_t)q * ntiles + tile;
    const uint64_t d0 = (uint64_t)tile * T, d1 = d0 + T;
#pragma unroll
    for (uint32_t k = 0; k < OWN; k++) acc[th + k * NT] = 0;
    uint64_t qlo;
    const uint32_t n = jb_bm25_query(q_off, q, q_cap, &qlo);
    bool any = false;
    for (uint32_t j0 = 0; j0 < n; j0 += NT) {  // (n is the same in every lane)
        const Part p = entry_part(q_id, qlo, j0 + th, n, nids, nweights, weight, post_off, post_doc, npost, d0, d1, false);
        const uint32_t inc = wave_incl(p.len, lane);
        __syncthreads();  // (the round before has finished with s_lo, s_pre, s_w; acc is zeroed)
        if (lane == 63u) s_ws[wv] = inc;
        __syncthreads();
        uint32_t base = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < NW; k++) {
            const uint32_t x = s_ws[k];
            if (k < wv) base += x;
            total += x;
        }
        s_lo[th] = p.lo;
        s_w[th] = p.w;
        s_pre[th] = base + inc - p.len;
        if (th == 0) s_pre[NT] = total;
        __syncthreads();
        if (total == 0) continue;
        any = true;
        // four postings per lane and trip, stage by stage, so that their loads are in flight together (a lane
        // past the end takes posting 0 of the chunk, which exists, and drops it)
        const uint32_t cnt = std::min<uint32_t>(n - j0, NT);  // the chunk's entries: s_pre[cnt] == total
        for (uint32_t k0 = th; k0 < total; k0 += UNR * NT) {  // (total <= NT * T = 2^22)
            uint64_t i[UNR];
            uint32_t e[UNR], d[UNR], tf[UNR];
            float nr[UNR];
            bool ok[UNR];
#pragma unroll
            for (uint32_t u = 0; u < UNR; u++) {
                ok[u] = k0 + u * NT < total;
                const uint32_t k = ok[u] ? k0 + u * NT : 0u;
                // the entry of posting k: the last e with s_pre[e] <= k (parts of length 0 share a prefix)
                uint32_t lo = 0, hi = cnt;
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_pre[mid] <= k) lo = mid;
                    else hi = mid;
                }
                e[u] = lo;
                i[u] = s_lo[lo] + (k - s_pre[lo]);
            }
#pragma unroll
            for (uint32_t u = 0; u < UNR; u++) {
                d[u] = post_doc[i[u]];
                tf[u] = post_tf[i[u]];
            }
#pragma unroll
            for (uint32_t u = 0; u < UNR; u++) {
                ok[u] = ok[u] && (uint64_t)d[u] >= d0 && (uint64_t)d[u] < d1 && d[u] < ndocs && tf[u] > 0u;
                nr[u] = ok[u] ? norm[d[u]] : -1.0f;
            }
#pragma unroll
            for (uint32_t u = 0; u < UNR; u++) {
                if (ok[u] && nr[u] >= 0.0f) {  // (jb_bm25_posting, its tests in stages)
                    const uint64_t c = jb_bm25_contrib(s_w[e[u]], tf[u], nr[u], k1p1);
                    if (c) atomicAdd((unsigned long long*)&acc[d[u] - (uint32_t)d0], (unsigned long long)c);
                }
            }
        }
    }
    if (!any) {  // (the same in every lane) no posting of the query lies in the tile
        if (th == 0) pcnt[pair] = 0;
        return;
    }
    __syncthreads();
    tile_select(acc, d0, topk, pscore + pair * topk, pdoc + pair * topk, pcnt + pair, sh_s, sh_d);
}

// Form 0: the adds.  grid (ntiles, nq); the ntiles workgroups of a query share every list.
__global__ __launch_bounds__(NT) void k_bm25_scatter(
    const uint32_t* __restrict__ post_doc, const uint32_t* __restrict__ post_tf, const uint64_t* __restrict__ post_off,
    uint64_t npost, uint32_t nids, const float* __restrict__ norm, uint32_t ndocs, const float* __restrict__ weight,
    uint32_t nweights, double k1p1, const uint32_t* __restrict__ q_id, uint64_t q_cap, const uint64_t* __restrict__ q_off,
    uint64_t* __restrict__ dense) {
    const uint32_t q = blockIdx.y;
    uint64_t* row = dense + (uint64_t)q * ndocs;
    uint64_t qlo;
    const uint32_t n = jb_bm25_query(q_off, q, q_cap, &qlo);
    const uint64_t step = (uint64_t)gridDim.x * NT;
    for (uint32_t j = 0; j < n; j++) {
        const Part p = entry_part(q_id, qlo, j, n, nids, nweights, weight, post_off, post_doc, npost, 0, 0, true);
        for (uint64_t k = (uint64_t)blockIdx.x * NT + threadIdx.x; k < p.len; k += step) {
            const uint64_t i = p.lo + k;
            const uint32_t d = post_doc[i], tf = post_tf[i];
            if (jb_bm25_posting(d, tf, ndocs, norm)) {
                const uint64_t c = jb_bm25_contrib(p.w, tf, norm[d], k1p1);
                if (c) atomicAdd((unsigned long long*)&row[d], (unsigned long long)c);
            }
        }
    }
}

// Form 0: the selection of a row's tile.  grid (ntiles, nq).
__global__ __launch_bounds__(NT, 4) void k_bm25_select(const uint64_t* __restrict__ dense, uint32_t ndocs, uint32_t topk,
                                                       uint64_t* __restrict__ pscore, uint32_t* __restrict__ pdoc,
                                                       uint32_t* __restrict__ pcnt) {
    __shared__ uint64_t acc[T];
    __shared__ uint64_t sh_s[2][NW];
    __shared__ uint32_t sh_d[2][NW];
    const uint32_t th = threadIdx.x, tile = blockIdx.x, q = blockIdx.y;
    const uint64_t pair = (uint64_t)q * gridDim.x + tile, d0 = (uint64_t)tile * T;
    const uint64_t* row = dense + (uint64_t)q * ndocs;
#pragma unroll
    for (uint32_t k = 0; k < OWN; k++) {
        const uint64_t d = d0 + th + k * NT;
        acc[th + k * NT] = d < ndocs ? row[d] : 0;
    }
    __syncthreads();
    tile_select(acc, d0, topk, pscore + pair * topk, pdoc + pair * topk, pcnt + pair, sh_s, sh_d);
}

// One workgroup per query: the best topk of the tiles' partial records, then the rest of the row.
__global__ __launch_bounds__(NT) void k_bm25_merge(const uint64_t* __restrict__ pscore, const uint32_t* __restrict__ pdoc,
                                                   const uint32_t* __restrict__ pcnt, uint32_t ntiles, uint32_t nq,
                                                   uint32_t topk, uint32_t* __restrict__ res_doc, uint64_t* __restrict__ res_score,
                                                   uint32_t* __restrict__ res_n) {
    __shared__ uint64_t sh_s[2][NW];
    __shared__ uint32_t sh_d[2][NW];
    const uint32_t th = threadIdx.x;
    const uint64_t nrec = (uint64_t)ntiles * topk;
    for (uint64_t q = blockIdx.x; q < nq; q += gridDim.x) {  // (the same trips in every lane)
        const uint64_t p0 = q * ntiles;
        uint64_t ls = ~0ull;  // the record taken last: every record ranks behind (2^64 - 1, 0)
        uint32_t ld = 0;
        uint32_t n = 0;
        for (uint32_t r = 0; r < topk; r++) {
            uint64_t bs = 0;
            uint32_t bd = JB_ID_UNK;
            for (uint64_t k = th; k < nrec; k += NT) {
                const uint64_t tl = k / topk;
                if ((uint32_t)(k - tl * topk) >= pcnt[p0 + tl]) continue;
                const uint64_t s = pscore[p0 * topk + k];
                const uint32_t d = pdoc[p0 * topk + k];
                if (jb_bm25_before(ls, ld, s, d) && jb_bm25_before(s, d, bs, bd)) {
                    bs = s;
                    bd = d;
                }
            }
            block_best(&bs, &bd, sh_s[r & 1u], sh_d[r & 1u]);
            if (bs == 0) break;  // (the same value in every lane)
            if (th == 0) {
                res_doc[(uint64_t)q * topk + r] = bd;
                res_score[(uint64_t)q * topk + r] = bs;
            }
            ls = bs;
            ld = bd;
            n = r + 1u;
        }
        if (th == 0) res_n[q] = n;
        for (uint32_t r = n + th; r < topk; r += NT) {
            res_doc[(uint64_t)q * topk + r] = JB_ID_UNK;
            res_score[(uint64_t)q * topk + r] = 0;
        }
        __syncthreads();  // (the next query's rounds reuse sh_s / sh_d)
    }
}

}  // namespace

hipError_t run_bm25_norms(const uint32_t* d_doc_len, uint32_t ndocs, double k1, double b, double avgdl, float* d_norm,
                          hipStream_t stream, KernelTimer* timer) {
    if (ndocs == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)(((uint64_t)ndocs + 255u) / 256u);
    JB_TIMED(K_BM25_NORMS,
             hipLaunchKernelGGL(k_bm25_norms, dim3(grid), dim3(256), 0, stream, d_doc_len, ndocs, k1, b, avgdl, d_norm));
    return hipGetLastError();
}

hipError_t run_bm25_idf(const uint64_t* d_post_off, uint32_t nids, uint64_t ndocs_total, float* d_weight,
                        hipStream_t stream, KernelTimer* timer) {
    if (nids == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)(((uint64_t)nids + 255u) / 256u);
    JB_TIMED(K_BM25_IDF,
             hipLaunchKernelGGL(k_bm25_idf, dim3(grid), dim3(256), 0, stream, d_post_off, nids, ndocs_total, d_weight));
    return hipGetLastError();
}

hipError_t run_bm25_search(const uint32_t* d_post_doc, const uint32_t* d_post_tf, const uint64_t* d_post_off,
                           uint64_t npost, uint32_t nids, const float* d_norm, uint32_t ndocs, const float* d_weight,
                           uint32_t nweights, double k1, const uint32_t* d_q_id, uint64_t q_cap, const uint64_t* d_q_off,
                           uint32_t nq, uint32_t topk, uint32_t form, uint32_t* d_res_doc, uint64_t* d_res_score,
                           uint32_t* d_res_n, void* d_work, hipStream_t stream, KernelTimer* timer) {
    if (nq == 0) return hipSuccess;
    const Bm25Work w = bm25_layout(nq, ndocs, topk);
    uint8_t* b = (uint8_t*)d_work;
    uint64_t* pscore = (uint64_t*)(b + w.pscore);
    uint32_t* pdoc = (uint32_t*)(b + w.pdoc);
    uint32_t* pcnt = (uint32_t*)(b + w.pcnt);
    const uint32_t ntiles = (uint32_t)w.ntiles;
    const double k1p1 = k1 + 1.0;
    // (grid.y <= 65535 and a grid of fewer than 2^32 lanes: the queries go in slices)
    const uint32_t slice = std::max<uint32_t>(1u, std::min<uint32_t>(32768u, (1u << 22) / std::max(ntiles, 1u)));
    for (uint32_t q0 = 0; ntiles && q0 < nq; q0 += slice) {
        const uint32_t nqs = std::min<uint32_t>(nq - q0, slice);
        const dim3 grid(ntiles, nqs);
        const uint64_t* qo = d_q_off + q0;
        uint64_t* ps = pscore + (uint64_t)q0 * ntiles * topk;
        uint32_t* pd = pdoc + (uint64_t)q0 * ntiles * topk;
        uint32_t* pc = pcnt + (uint64_t)q0 * ntiles;
        if (form) {
            JB_TIMED(K_BM25_TILE,
                     hipLaunchKernelGGL(k_bm25_tile, grid, dim3(NT), 0, stream, d_post_doc, d_post_tf, d_post_off, npost,
                                        nids, d_norm, ndocs, d_weight, nweights, k1p1, d_q_id, q_cap, qo, topk, ps, pd, pc));
        } else {
            uint64_t* dense = (uint64_t*)(b + w.dense) + (uint64_t)q0 * ndocs;
            hipError_t e = hipMemsetAsync(dense, 0, (size_t)nqs * ndocs * 8u, stream);
            if (e != hipSuccess) return e;
            JB_TIMED(K_BM25_SCATTER,
                     hipLaunchKernelGGL(k_bm25_scatter, grid, dim3(NT), 0, stream, d_post_doc, d_post_tf, d_post_off, npost,
                                        nids, d_norm, ndocs, d_weight, nweights, k1p1, d_q_id, q_cap, qo, dense));
            JB_TIMED(K_BM25_SELECT,
                     hipLaunchKernelGGL(k_bm25_select, grid, dim3(NT), 0, stream, dense, ndocs, topk, ps, pd, pc));
        }
    }
    JB_TIMED(K_BM25_MERGE, hipLaunchKernelGGL(k_bm25_merge, dim3(std::min<uint32_t>(nq, 1u << 20)), dim3(NT), 0, stream, pscore,
                                              pdoc, pcnt, ntiles, nq, topk, d_res_doc, d_res_score, d_res_n));
    return hipGetLastError();
}

}  // namespace jb
