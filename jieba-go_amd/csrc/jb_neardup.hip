// jb_neardup.hip — gfx950 kernels of the near-duplicate call (jb_neardup_device; the rule is jb_neardup's,
// jb_neardup.cpp; the code shared with the host is jb_neardup.h's).
//
// The N = ndocs * B entries (e = d * B + b, key[e]) are sorted by (band, key) with a stable LSD radix sort, 8
// bits per pass: eight passes over the key, low byte first, then one over the band.  A slot carries its key
// (u64) and its entry (u32); the ntl * kNdTile - N padding slots of the last tile carry the key JB_MH_NOKEY and
// the entry 0xFFFFFFFF, whose band digit is 255: no (digit sequence, slot number) is greater, so they end at
// the positions >= N and every sorted position below N holds a real entry.  JB_MH_NOKEY is the greatest key, so
// the entries that are in no bucket end each band.  Every pass is the three launches of jb_postings.hip:
//   k_nd_hist     per tile, the 256 digit counts -> cnt[digit * ntl + tile] (ballot match, one LDS add per group).
//   k_nd_scan     workgroup d scans cnt[d * ntl ..] over the tiles in place (exclusive) and writes tot[d].
//   k_nd_scatter  per tile: rank every slot among the tile's slots of its digit and write key and entry at
//                 (sum of tot[< digit]) + cnt[digit][tile] + rank.  Pass 0 reads the caller's keys.
// The rank is stable for the reason jb_postings.hip gives: wave w owns the tile's slots [w * 1024, (w + 1) *
// 1024) in 16 rounds of 64, the lanes of equal digit are found by the ballot match, the group's lowest lane
// moves the wave's own LDS counter of the digit (a wave's LDS accesses complete in program order: no atomic),
// and after a barrier the four waves' counts become exclusive prefixes in wave order.  Stability keeps the
// entries of equal (band, key) in the order of e, that is, documents ascending: a bucket is a contiguous run
// whose member w + 1 places before position q has a rank w + 1 below q's.  Then five launches:
//   k_nd_mask     a wave takes 64 sorted positions at a time; a lane first tests whether its position has the
//                 bucket of the position before it (if not, its mask and count are 0: most positions).  For
//                 every other position q the wave works together: lane w < W tests position q - 1 - w (same
//                 bucket, then jb_nd_first over the two key rows), the candidates' ballot is counted, and for
//                 each candidate the lanes compare the K slots of the two signature rows, 64 per step, and
//                 count by ballot.  mask[q] (u64, bit w = the pair with position q - 1 - w is kept) and
//                 cnt[e] = its popcount; position q - W - 1 in the same bucket counts into ntrunc.  The three
//                 counters go to part[tile] through LDS.
//   k_nd_tsum     per tile of entries (in the order of e), the sum of cnt -> tbase[tile].
//   k_nd_base     one workgroup: tbase becomes exclusive (u64), the total goes to *npairs and pair_off[ndocs],
//                 the tiles' counters are summed into stat.
//   k_nd_off      per tile: cnt[e] becomes the exclusive prefix inside the tile, and the lane of an entry with
//                 band 0 writes pair_off[d] = tbase[tile] + prefix.
//   k_nd_write    as k_nd_mask over the sorted positions with a mask: for each set bit, highest w first (the
//                 earlier document ascending), agree is counted again and lane 0 stores the pair at tbase[tile
//                 of e] + cnt[e] + (set bits above w) when that is below pcap.
// Measured (profiles/neardup_bench.json): the 1 GiB corpus's 73,443 signatures at B = 32, K = 128, W = 64, 2.35M
// entries, 0.70 ms (the sort 0.55 ms, k_nd_mask 0.13 ms, k_nd_write 0.07 ms); 4,000,000 synthetic signatures, 128M
// entries, 26.9 ms (k_nd_hist 3.5 ms, k_nd_scatter 15.6 ms, k_nd_mask 6.2 ms).  One form: none other was written.
// 3 * 9 + 5 launches whatever the data are (none, three memsets, when ndocs == 0).  No lane waits for another
// workgroup and there are no global atomics; every value is an integer, so the outputs are the same from run
// to run.  Reads of key and sig are at rows below ndocs (an entry read from the work buffer is used only when
// it is below N), reads and writes of the work arrays at positions below ntl * kNdTile, writes to pair_doc /
// pair_agree below pcap, to pair_off at d <= ndocs.
#include <hip/hip_runtime.h>

#include "jb_kstages.h"
#include "jb_neardup.h"

#include <algorithm>

namespace jb {

namespace {

constexpr uint32_t T = kNdTile;
constexpr uint32_t WSLOTS = T / 4u;     // slots per wave
constexpr uint32_t RPW = WSLOTS / 64u;  // rounds per wave
constexpr uint32_t NOENT = 0xFFFFFFFFu;  // the entry of a padding slot
static_assert(kNdTile == JB_ND_TILE && kNdMaxWin == JB_ND_MAXWIN, "the header's constants");
static_assert(RPW * 256u == T, "four waves, RPW rounds of 64 slots each");
static_assert(JB_MH_MAXK <= 256, "a band fits one digit");

// The lanes of the wave whose digit equals this lane's (all 64 lanes take part).
__device__ __forceinline__ uint64_t match8(uint32_t dg) {
    uint64_t m = ~0ull;
#pragma unroll
    for (uint32_t b = 0; b < 8u; b++) {
        const bool bit = (dg >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

__device__ __forceinline__ uint32_t popc64(uint64_t v) { return (uint32_t)__popcll((unsigned long long)v); }
__device__ __forceinline__ uint32_t low64(uint64_t v) { return (uint32_t)__ffsll((unsigned long long)v) - 1u; }

// Inclusive scan over the 64 lanes of a wave.
template <class V>
__device__ __forceinline__ V wave_incl(V v, uint32_t lane) {
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const V u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// The exclusive scan of one value per thread over the NW waves of the workgroup; *total is the sum.
template <uint32_t NW, class V>
__device__ __forceinline__ V block_excl(V v, V* sh /* NW */, V* total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const V inc = wave_incl(v, lane);
    __syncthreads();  // (sh may still be read from an earlier call)
    if (lane == 63u) sh[w] = inc;
    __syncthreads();
    V before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < NW; k++) {
        const V x = sh[k];
        if (k < w) before += x;
        all += x;
    }
    *total = all;
    return before + inc - v;
}

// Slot i of a pass: pass 0 from the caller's keys, later passes from what the pass before wrote.
__device__ __forceinline__ void slot_get(bool first, const uint64_t* __restrict__ ksrc, const uint32_t* __restrict__ psrc,
                                         uint64_t i, uint32_t N, uint64_t* k, uint32_t* p) {
    if (first) {
        *k = i < N ? ksrc[i] : JB_MH_NOKEY;
        *p = i < N ? (uint32_t)i : NOENT;
    } else {
        *k = ksrc[i];
        *p = psrc[i];
    }
}

// The digit of a slot in pass `pass`: a key byte, then the band.
__device__ __forceinline__ uint32_t digit_of(uint64_t k, uint32_t p, uint32_t pass, uint32_t B) {
    if (pass < 8u) return (uint32_t)(k >> (8u * pass)) & 255u;
    return p == NOENT ? 255u : jb_nd_band(p, B);
}

__global__ __launch_bounds__(256) void k_nd_hist(const uint64_t* __restrict__ ksrc, const uint32_t* __restrict__ psrc,
                                                 uint32_t pass, uint32_t N, uint32_t B, uint32_t ntl,
                                                 uint32_t* __restrict__ cnt) {
    __shared__ uint32_t s_h[256];
    const uint32_t th = threadIdx.x, lane = th & 63u, w = th >> 6;
    s_h[th] = 0;
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * T + w * WSLOTS + lane;
    // (the ballots stand outside every divergent branch: all 64 lanes take part)
#pragma unroll 4
    for (uint32_t r = 0; r < RPW; r++) {
        uint64_t k;
        uint32_t p;
        slot_get(pass == 0, ksrc, psrc, t0 + r * 64u, N, &k, &p);
        const uint32_t dg = digit_of(k, p, pass, B);
        const uint64_t m = match8(dg);
        if (lane == low64(m)) atomicAdd(&s_h[dg], popc64(m));
    }
    __syncthreads();
    cnt[(uint64_t)th * ntl + blockIdx.x] = s_h[th];
}

__global__ __launch_bounds__(1024) void k_nd_scan(uint32_t* __restrict__ cnt, uint32_t ntl, uint32_t* __restrict__ tot) {
    __shared__ uint32_t sh[16];
    uint32_t* c = cnt + (uint64_t)blockIdx.x * ntl;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < ntl; c0 += 1024u) {
        const uint32_t i = c0 + threadIdx.x;
        const uint32_t v = i < ntl ? c[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl<16>(v, sh, &total);
        if (i < ntl) c[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256, 4) void k_nd_scatter(const uint64_t* __restrict__ ksrc, const uint32_t* __restrict__ psrc,
                                                       uint32_t pass, uint32_t N, uint32_t B, uint32_t ntl,
                                                       const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ tot,
                                                       uint64_t* __restrict__ key_out, uint32_t* __restrict__ pay_out) {
    __shared__ uint32_t s_c[4][256];  // per wave: the digit's count so far, then the wave's base for the digit
    __shared__ uint32_t s_sc[4];
    const uint32_t th = threadIdx.x, lane = th & 63u, w = th >> 6;
    const uint64_t nslots = (uint64_t)ntl * T, tb = (uint64_t)blockIdx.x * T;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) s_c[k][th] = 0;
    __syncthreads();
    uint64_t key[RPW];
    uint32_t pay[RPW], rank[RPW];
    const uint64_t t0 = tb + w * WSLOTS + lane;
#pragma unroll
    for (uint32_t r = 0; r < RPW; r++) slot_get(pass == 0, ksrc, psrc, t0 + r * 64u, N, &key[r], &pay[r]);
    // the ranks inside the wave, round by round (the header comment: why this is the slot order)
    volatile uint32_t* cw = s_c[w];
#pragma unroll
    for (uint32_t r = 0; r < RPW; r++) {
        const uint32_t dg = digit_of(key[r], pay[r], pass, B);
        const uint64_t m = match8(dg);
        const uint32_t lead = low64(m);
        uint32_t old = 0;
        if (lane == lead) {
            old = cw[dg];
            cw[dg] = old + popc64(m);
        }
        rank[r] = (uint32_t)__shfl((int)old, (int)lead, 64) + popc64(m & ((1ull << lane) - 1ull));
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // thread d: the digit's global base, and the waves' counts as exclusive prefixes in wave order
    uint32_t total;
    const uint32_t c0 = s_c[0][th], c1 = s_c[1][th], c2 = s_c[2][th];
    const uint32_t g = block_excl<4>(tot[th], s_sc, &total) + cnt[(uint64_t)th * ntl + blockIdx.x];
    s_c[0][th] = g;
    s_c[1][th] = g + c0;
    s_c[2][th] = g + c0 + c1;
    s_c[3][th] = g + c0 + c1 + c2;
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < RPW; r++) {
        const uint64_t pos = (uint64_t)s_c[w][digit_of(key[r], pay[r], pass, B)] + rank[r];
        if (pos >= nslots) continue;  // (never: the counters are this pass's own)
        key_out[pos] = key[r];
        pay_out[pos] = pay[r];
    }
}

// agree(i, j) by the whole wave: 64 slots per step, counted by ballot (all 64 lanes take part).
__device__ __forceinline__ uint32_t wave_agree(const uint32_t* __restrict__ sig, uint32_t i, uint32_t j, uint32_t K,
                                               uint32_t lane) {
    uint32_t agree = 0;
    for (uint32_t s0 = 0; s0 < K; s0 += 64u) agree += popc64(__ballot(jb_nd_eq(sig, i, j, K, s0 + lane) != 0u));
    return agree;
}

__global__ __launch_bounds__(256) void k_nd_mask(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ spay,
                                                 const uint64_t* __restrict__ key, const uint32_t* __restrict__ sig,
                                                 uint32_t N, uint32_t B, uint32_t K, uint32_t W, uint32_t min_agree,
                                                 uint64_t* __restrict__ mask, uint32_t* __restrict__ cnt,
                                                 uint32_t* __restrict__ part) {
    __shared__ uint32_t s_p[4][3];
    const uint32_t th = threadIdx.x, lane = th & 63u, w = th >> 6;
    uint32_t nent = 0, ncand = 0, ntrunc = 0;  // the wave's, the same in every lane
    const uint64_t q0w = (uint64_t)blockIdx.x * T + w * WSLOTS;
    for (uint32_t r = 0; r < RPW; r++) {
        const uint64_t q0 = q0w + r * 64u, q = q0 + lane;
        if (q0 >= N) break;  // (the same for the whole wave)
        uint64_t k = JB_MH_NOKEY;
        uint32_t e = NOENT;
        if (q < N) {
            k = skey[q];
            e = spay[q];
        }
        const bool member = e < N && k != JB_MH_NOKEY;
        // the position before mine holds my bucket: only then can a pair end here
        const bool has = member && q > 0 && jb_nd_same(spay[q - 1u], skey[q - 1u], e, k, B);
        nent += popc64(__ballot(member));
        uint64_t todo = __ballot(has), mine = 0;
        while (todo) {  // (the same in every lane)
            const uint32_t l = low64(todo);
            todo &= todo - 1u;
            const uint64_t qq = q0 + l, kk = (uint64_t)__shfl((unsigned long long)k, (int)l, 64);
            const uint32_t ee = (uint32_t)__shfl((int)e, (int)l, 64), j = jb_nd_doc(ee, B), b = jb_nd_band(ee, B);
            bool cand = false;
            uint32_t i = 0;
            if (lane < W && qq >= 1u + lane) {
                const uint64_t p = qq - 1u - lane;
                const uint32_t e1 = spay[p];
                if (e1 < N && jb_nd_same(e1, skey[p], ee, kk, B)) {
                    i = jb_nd_doc(e1, B);
                    cand = jb_nd_first(key, i, j, B, b);
                }
            }
            if (qq >= (uint64_t)W + 1u) {  // the member W + 1 places below: this one's rank is above W
                const uint64_t p = qq - W - 1u;
                const uint32_t e1 = spay[p];
                ntrunc += e1 < N && jb_nd_same(e1, skey[p], ee, kk, B) ? 1u : 0u;
            }
            uint64_t cm = __ballot(cand), keep = 0;
            ncand += popc64(cm);
            while (cm) {
                const uint32_t c = low64(cm);
                cm &= cm - 1u;
                const uint32_t ii = (uint32_t)__shfl((int)i, (int)c, 64);
                if (wave_agree(sig, ii, j, K, lane) >= min_agree) keep |= 1ull << c;
            }
            if (lane == l) mine = keep;
        }
        if (q < N) {
            mask[q] = mine;
            if (e < N) cnt[e] = popc64(mine);
        }
    }
    if (lane == 0) {
        s_p[w][0] = nent;
        s_p[w][1] = ncand;
        s_p[w][2] = ntrunc;
    }
    __syncthreads();
    if (th < 3u) part[(uint64_t)blockIdx.x * 3u + th] = s_p[0][th] + s_p[1][th] + s_p[2][th] + s_p[3][th];
}

__global__ __launch_bounds__(256) void k_nd_tsum(const uint32_t* __restrict__ cnt, uint32_t N, uint64_t* __restrict__ tbase) {
    __shared__ uint32_t sh[4];
    const uint64_t tb = (uint64_t)blockIdx.x * T;
    uint32_t v = 0;
#pragma unroll 4
    for (uint32_t k = 0; k < T / 256u; k++) {
        const uint64_t e = tb + k * 256u + threadIdx.x;
        if (e < N) v += cnt[e];
    }
    uint32_t total;
    (void)block_excl<4>(v, sh, &total);
    if (threadIdx.x == 0) tbase[blockIdx.x] = total;  // (at most kNdTile * 64)
}

__global__ __launch_bounds__(1024) void k_nd_base(uint64_t* __restrict__ tbase, const uint32_t* __restrict__ part,
                                                  uint32_t ntl, uint32_t ndocs, uint64_t* __restrict__ pair_off,
                                                  uint64_t* __restrict__ npairs, uint64_t* __restrict__ stat) {
    __shared__ uint64_t sh[16];
    __shared__ unsigned long long s_st[3];
    if (threadIdx.x < 3u) s_st[threadIdx.x] = 0;
    uint64_t carry = 0;
    for (uint32_t c0 = 0; c0 < ntl; c0 += 1024u) {
        const uint32_t i = c0 + threadIdx.x;
        const uint64_t v = i < ntl ? tbase[i] : 0u;
        uint64_t total;
        const uint64_t ex = block_excl<16>(v, sh, &total);
        if (i < ntl) tbase[i] = carry + ex;
        carry += total;
    }
    uint64_t a[3] = {0, 0, 0};
    for (uint32_t i = threadIdx.x; i < ntl; i += 1024u)
        for (uint32_t c = 0; c < 3u; c++) a[c] += part[(uint64_t)i * 3u + c];
    for (uint32_t c = 0; c < 3u; c++)
        if (a[c]) atomicAdd(&s_st[c], (unsigned long long)a[c]);  // (LDS: integer sums, any order)
    __syncthreads();
    if (threadIdx.x < 3u) stat[threadIdx.x] = s_st[threadIdx.x];
    if (threadIdx.x == 0) {
        *npairs = carry;
        pair_off[ndocs] = carry;
    }
}

__global__ __launch_bounds__(256) void k_nd_off(uint32_t* __restrict__ cnt, const uint64_t* __restrict__ tbase, uint32_t N,
                                                uint32_t B, uint64_t* __restrict__ pair_off) {
    __shared__ uint32_t sh[4];
    constexpr uint32_t PER = T / 256u;  // consecutive entries per thread
    const uint64_t e0 = (uint64_t)blockIdx.x * T + threadIdx.x * PER;
    uint32_t v[PER], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
        v[k] = e0 + k < N ? cnt[e0 + k] : 0u;
        sum += v[k];
    }
    uint32_t total;
    uint32_t ex = block_excl<4>(sum, sh, &total);
    const uint64_t base = tbase[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
        const uint64_t e = e0 + k;
        if (e < N) {
            cnt[e] = ex;
            if (jb_nd_band((uint32_t)e, B) == 0u) pair_off[jb_nd_doc((uint32_t)e, B)] = base + ex;
        }
        ex += v[k];
    }
}

__global__ __launch_bounds__(256) void k_nd_write(const uint32_t* __restrict__ spay, const uint64_t* __restrict__ mask,
                                                  const uint32_t* __restrict__ loc, const uint64_t* __restrict__ tbase,
                                                  const uint32_t* __restrict__ sig, uint32_t N, uint32_t B, uint32_t K,
                                                  uint32_t* __restrict__ pair_doc, uint32_t* __restrict__ pair_agree,
                                                  uint64_t pcap) {
    const uint32_t th = threadIdx.x, lane = th & 63u, w = th >> 6;
    const uint64_t q0w = (uint64_t)blockIdx.x * T + w * WSLOTS;
    for (uint32_t r = 0; r < RPW; r++) {
        const uint64_t q0 = q0w + r * 64u, q = q0 + lane;
        if (q0 >= N) break;  // (the same for the whole wave)
        uint64_t m = 0;
        uint32_t e = NOENT;
        if (q < N) {
            m = mask[q];
            e = spay[q];
        }
        uint64_t todo = __ballot(m != 0 && e < N);
        while (todo) {  // (the same in every lane)
            const uint32_t l = low64(todo);
            todo &= todo - 1u;
            const uint64_t qq = q0 + l;
            uint64_t mm = (uint64_t)__shfl((unsigned long long)m, (int)l, 64);
            const uint32_t ee = (uint32_t)__shfl((int)e, (int)l, 64), j = jb_nd_doc(ee, B);
            uint64_t pos = tbase[ee / T] + loc[ee];
            while (mm) {  // highest w first: the earlier document ascends
                const uint32_t c = 63u - (uint32_t)__clzll((long long)mm);
                mm &= ~(1ull << c);
                const uint32_t e1 = qq >= 1u + c ? spay[qq - 1u - c] : NOENT;
                if (e1 < N) {  // (always, for a mask of k_nd_mask)
                    const uint32_t i = jb_nd_doc(e1, B), agree = wave_agree(sig, i, j, K, lane);
                    if (lane == 0 && pos < pcap) {
                        pair_doc[pos] = i;
                        pair_agree[pos] = agree;
                    }
                }
                pos++;
            }
        }
    }
}

}  // namespace

hipError_t run_neardup(const uint64_t* d_key, const uint32_t* d_sig, uint32_t ndocs, uint32_t B, uint32_t K, uint32_t W,
                       uint32_t min_agree, uint32_t* d_pair_doc, uint32_t* d_pair_agree, uint64_t pcap,
                       uint64_t* d_pair_off, uint64_t* d_npairs, uint64_t* d_stat, void* d_work, hipStream_t stream,
                       KernelTimer* timer) {
    if (ndocs == 0) {  // no entry: the zero outputs, no launch
        hipError_t e = hipMemsetAsync(d_pair_off, 0, 8, stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_npairs, 0, 8, stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_stat, 0, JB_ND_NSTAT * 8u, stream);
        return e;
    }
    const uint32_t N = ndocs * B;
    const NeardupWork w = neardup_layout(N);
    uint8_t* b = (uint8_t*)d_work;
    uint64_t* key[2] = {(uint64_t*)(b + w.key[0]), (uint64_t*)(b + w.key[1])};
    uint32_t* pay[2] = {(uint32_t*)(b + w.pay[0]), (uint32_t*)(b + w.pay[1])};
    uint32_t* cnt = (uint32_t*)(b + w.cnt);
    uint32_t* tot = (uint32_t*)(b + w.tot);
    uint32_t* part = (uint32_t*)(b + w.part);
    uint64_t* tbase = (uint64_t*)(b + w.tbase);
    const uint32_t ntl = (uint32_t)w.ntl;
    constexpr uint32_t P = 9;  // eight key bytes, then the band: the last pass writes arrays 0
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t* ks = p == 0 ? d_key : key[(p - 1u) & 1u];
        const uint32_t* ps = p == 0 ? nullptr : pay[(p - 1u) & 1u];
        JB_TIMED(K_ND_HIST, hipLaunchKernelGGL(k_nd_hist, dim3(ntl), dim3(256), 0, stream, ks, ps, p, N, B, ntl, cnt));
        JB_TIMED(K_ND_SCAN, hipLaunchKernelGGL(k_nd_scan, dim3(256), dim3(1024), 0, stream, cnt, ntl, tot));
        JB_TIMED(K_ND_SCATTER, hipLaunchKernelGGL(k_nd_scatter, dim3(ntl), dim3(256), 0, stream, ks, ps, p, N, B, ntl, cnt,
                                                  tot, key[p & 1u], pay[p & 1u]));
    }
    const uint64_t* skey = key[(P - 1u) & 1u];
    const uint32_t* spay = pay[(P - 1u) & 1u];
    uint64_t* mask = key[P & 1u];   // (free after the last pass)
    uint32_t* pcnt = pay[P & 1u];
    JB_TIMED(K_ND_MASK, hipLaunchKernelGGL(k_nd_mask, dim3(ntl), dim3(256), 0, stream, skey, spay, d_key, d_sig, N, B, K, W,
                                           min_agree, mask, pcnt, part));
    JB_TIMED(K_ND_TSUM, hipLaunchKernelGGL(k_nd_tsum, dim3(ntl), dim3(256), 0, stream, pcnt, N, tbase));
    JB_TIMED(K_ND_BASE, hipLaunchKernelGGL(k_nd_base, dim3(1), dim3(1024), 0, stream, tbase, part, ntl, ndocs, d_pair_off,
                                           d_npairs, d_stat));
    JB_TIMED(K_ND_OFF, hipLaunchKernelGGL(k_nd_off, dim3(ntl), dim3(256), 0, stream, pcnt, tbase, N, B, d_pair_off));
    JB_TIMED(K_ND_WRITE, hipLaunchKernelGGL(k_nd_write, dim3(ntl), dim3(256), 0, stream, spay, mask, pcnt, tbase, d_sig, N,
                                            B, K, d_pair_doc, d_pair_agree, pcap));
    return hipGetLastError();
}

}  // namespace jb
