// jb_hostbatch.cpp — batches in host memory: the packed-span decoder, the mask helpers, the
// three-stream piece pipeline of one device's range (RangePipeline) and the sharding of a batch
// over the devices (cut_sharded).
#include <immintrin.h>
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <thread>

#include "jb_host.h"
#include "jb_plan.h"

// memcpy whose destination lines are written without being read first (non-temporal
// 16-byte stores; plain stores read every destination line before writing it): staging
// a batch into pinned memory, which the copy engine then reads.  Fenced at the end.
static void nt_copy(void* dst, const void* src, size_t n) {
    typedef long long v2i __attribute__((vector_size(16)));
    char* d = static_cast<char*>(dst);
    const char* s = static_cast<const char*>(src);
    const size_t head = std::min(n, (size_t)((16u - ((uintptr_t)d & 15u)) & 15u));
    memcpy(d, s, head);
    d += head;
    s += head;
    n -= head;
    for (; n >= 64; n -= 64, d += 64, s += 64) {
        v2i a, b, c, e;
        memcpy(&a, s, 16);
        memcpy(&b, s + 16, 16);
        memcpy(&c, s + 32, 16);
        memcpy(&e, s + 48, 16);
        __builtin_nontemporal_store(a, reinterpret_cast<v2i*>(d));
        __builtin_nontemporal_store(b, reinterpret_cast<v2i*>(d + 16));
        __builtin_nontemporal_store(c, reinterpret_cast<v2i*>(d + 32));
        __builtin_nontemporal_store(e, reinterpret_cast<v2i*>(d + 48));
    }
    memcpy(d, s, n);
    __builtin_ia32_sfence();
}

// fn(0..n-1) on n threads (the caller's thread runs fn(0))
constexpr unsigned kCopyThreads = 8;
template <class F>
void run_threads(unsigned n, F& fn) {
    std::vector<std::thread> th;
    for (unsigned t = 1; t < n; t++) th.emplace_back([&fn, t] { fn(t); });
    fn(0);
    for (auto& x : th) x.join();
}

// Words [lo, hi) of a range's masks (range word j = caller word rw + j, nw words in all)
// into the caller's arrays.  The range's first and last words may be shared with the
// neighbouring ranges of other devices: those are ORed (atomically) into words the
// caller zeroed first; the rest belong to this range alone and are stored.
static void put_mask_words(const MaskDst* m, uint64_t rw, uint64_t nw, uint64_t lo, uint64_t hi, const uint64_t* ms,
                           const uint64_t* me) {
    auto one = [&](uint64_t j) {
        if (j == 0 || j + 1 == nw) {
            __atomic_fetch_or(m->s + rw + j, ms[j], __ATOMIC_RELAXED);
            __atomic_fetch_or(m->e + rw + j, me[j], __ATOMIC_RELAXED);
        } else {
            m->s[rw + j] = ms[j];
            m->e[rw + j] = me[j];
        }
    };
    if (lo < hi && lo == 0) one(lo++);
    if (lo < hi && hi == nw) one(--hi);
    if (lo >= hi) return;
    const uint64_t n = hi - lo;
    const unsigned nth = n >= (1u << 18) ? kCopyThreads : 1u;
    auto work = [&](unsigned t) {
        const uint64_t a = lo + n * t / nth, b = lo + n * (t + 1) / nth;
        memcpy(m->s + rw + a, ms + a, (b - a) * 8);
        memcpy(m->e + rw + a, me + a, (b - a) * 8);
    };
    run_threads(nth, work);
}

// One token of a packed piece: start = previous end + gap, end = start + length, or an
// escaped token's span from the sorted side list.  e: the previous token's end (batch offset).
static inline void unpack_one(uint32_t x, uint32_t i, const uint4* side, uint32_t nside, uint64_t base, uint64_t& s,
                              uint64_t& e) {
    if (x != 0xFFFFu) {
        s = e + (x & kPackGapEsc);
        e = s + (x >> kPackGapBits);
    } else {
        const uint4* q = std::lower_bound(side, side + nside, i, [](const uint4& a, uint32_t v) { return a.x < v; });
        s = base + q->y;
        e = base + q->z;
    }
}

// Tokens [i0, i1) of one block, eight at a time with AVX-512: the ends are a running sum
// of gap + length (an in-register scan: three shifted adds), the starts the ends minus
// the lengths; a group of eight with an escaped token goes through unpack_one.  T is the
// output word (u64 batch offsets, or u32 for jb_cut_batch_into32: base is then relative to
// the caller's first byte).  Stores are streaming where both outputs are aligned alike to
// the vector width (after a scalar head), plain otherwise.
template <class T>
__attribute__((target("avx512f"))) static void unpack_block_avx512(const uint16_t* pk, uint32_t i0, uint32_t i1,
                                                                  uint64_t e, const uint4* side, uint32_t nside,
                                                                  uint64_t base, T* os, T* oe) {
    constexpr uintptr_t kVec = 8u * sizeof(T) - 1u;  // (eight outputs: 64 or 32 bytes)
    uint32_t i = i0;
    const bool al = (((uintptr_t)(os + i) ^ (uintptr_t)(oe + i)) & kVec) == 0u;
    if (al)
        for (; i < i1 && ((uintptr_t)(os + i) & kVec); i++) {
            uint64_t s;
            unpack_one(pk[i], i, side, nside, base, s, e);
            __builtin_nontemporal_store((T)s, os + i);
            __builtin_nontemporal_store((T)e, oe + i);
        }
    const __m512i m6 = _mm512_set1_epi64(kPackGapEsc), z = _mm512_setzero_si512(), last = _mm512_set1_epi64(7);
    __m512i cv = _mm512_set1_epi64((long long)e);  // the previous token's end in every lane
    for (; i + 8u <= i1; i += 8u) {
        const __m128i raw = _mm_loadu_si128(reinterpret_cast<const __m128i*>(pk + i));
        if (_mm_movemask_epi8(_mm_cmpeq_epi16(raw, _mm_set1_epi16(-1)))) {  // an escaped token: one at a time
            e = (uint64_t)_mm_cvtsi128_si64(_mm512_castsi512_si128(cv));
            for (uint32_t k = i; k < i + 8u; k++) {
                uint64_t s;
                unpack_one(pk[k], k, side, nside, base, s, e);
                os[k] = (T)s;
                oe[k] = (T)e;
            }
            cv = _mm512_set1_epi64((long long)e);
            continue;
        }
        const __m512i x = _mm512_cvtepu16_epi64(raw);
        const __m512i l = _mm512_srli_epi64(x, kPackGapBits);
        __m512i t = _mm512_add_epi64(_mm512_and_si512(x, m6), l);  // gap + length
        t = _mm512_add_epi64(t, _mm512_alignr_epi64(t, z, 7));     // inclusive scan over 8 lanes
        t = _mm512_add_epi64(t, _mm512_alignr_epi64(t, z, 6));
        t = _mm512_add_epi64(t, _mm512_alignr_epi64(t, z, 4));
        const __m512i ev = _mm512_add_epi64(cv, t);
        const __m512i sv = _mm512_sub_epi64(ev, l);
        if constexpr (sizeof(T) == 8) {
            if (al) {
                _mm512_stream_si512(reinterpret_cast<__m512i*>(os + i), sv);
                _mm512_stream_si512(reinterpret_cast<__m512i*>(oe + i), ev);
            } else {
                _mm512_storeu_si512(os + i, sv);
                _mm512_storeu_si512(oe + i, ev);
            }
        } else {
            const __m256i s32 = _mm512_cvtepi64_epi32(sv), e32 = _mm512_cvtepi64_epi32(ev);
            if (al) {
                _mm256_stream_si256(reinterpret_cast<__m256i*>(os + i), s32);
                _mm256_stream_si256(reinterpret_cast<__m256i*>(oe + i), e32);
            } else {
                _mm256_storeu_si256(reinterpret_cast<__m256i*>(os + i), s32);
                _mm256_storeu_si256(reinterpret_cast<__m256i*>(oe + i), e32);
            }
        }
        cv = _mm512_permutexvar_epi64(last, ev);
    }
    e = (uint64_t)_mm_cvtsi128_si64(_mm512_castsi512_si128(cv));
    for (; i < i1; i++) {
        uint64_t s;
        unpack_one(pk[i], i, side, nside, base, s, e);
        os[i] = (T)s;
        oe[i] = (T)e;
    }
}

// k_span_pack's packed spans of one piece back to batch offsets (base = the piece's first
// byte in the batch, or relative to the caller's first byte for u32 outputs): blocks of
// kPackBlock tokens decode independently from their header, on kCopyThreads threads
// (eight tokens at a time with AVX-512 where the CPU has it); an escaped token (0xFFFF)
// takes its span from the side list, sorted by token index first (on ordinary text it is
// empty or nearly so).  The outputs are written without reading the caller's lines first
// (streaming stores), fenced before each thread ends.
template <class T>
static void unpack_spans(const uint16_t* pk, const uint32_t* hdr, uint4* side, uint32_t nside, uint32_t nt,
                         uint64_t base, T* os, T* oe) {
    if (nside > 1) std::sort(side, side + nside, [](const uint4& a, const uint4& b) { return a.x < b.x; });
    const uint32_t nb = (nt + kPackBlock - 1u) / kPackBlock;
    static const unsigned kDecodeThreads = (unsigned)std::min(32, std::max(1, env_int("JB_DECODE_THREADS", 8)));
    static const bool avx512 = __builtin_cpu_supports("avx512f") && env_int("JB_DECODE_AVX512", 1) != 0;
    const unsigned nth = nt >= (1u << 18) ? kDecodeThreads : 1u;
    auto work = [&](unsigned t) {
        const uint32_t b0 = (uint32_t)((uint64_t)nb * t / nth), b1 = (uint32_t)((uint64_t)nb * (t + 1) / nth);
        for (uint32_t b = b0; b < b1; b++) {
            const uint32_t i0 = b * kPackBlock, i1 = std::min(nt, i0 + kPackBlock);
            uint64_t e = base + hdr[b];
            if (avx512) {
                unpack_block_avx512<T>(pk, i0, i1, e, side, nside, base, os, oe);
                continue;
            }
            for (uint32_t i = i0; i < i1; i++) {
                uint64_t s;
                unpack_one(pk[i], i, side, nside, base, s, e);
                __builtin_nontemporal_store((T)s, os + i);
                __builtin_nontemporal_store((T)e, oe + i);
            }
        }
        __builtin_ia32_sfence();  // (the streaming stores are visible before the thread is joined)
    };
    run_threads(nth, work);
}

// Text already in pinned memory (jb_host_alloc): the pieces are copied to the device
// straight from it, without staging.
struct HostAlloc { uintptr_t a; size_t n; };
static std::mutex g_host_mu;
static std::vector<HostAlloc> g_host;  // jb_host_alloc allocations
static bool host_pinned(const void* p, uint64_t n) {
    const uintptr_t x = (uintptr_t)p;
    std::lock_guard<std::mutex> g(g_host_mu);
    for (const HostAlloc& h : g_host)
        if (x >= h.a && x + n <= h.a + h.n) return true;
    return false;
}
void host_register(const void* p, size_t n) {
    std::lock_guard<std::mutex> g(g_host_mu);
    g_host.push_back(HostAlloc{(uintptr_t)p, n});
}
void host_unregister(const void* p) {
    std::lock_guard<std::mutex> g(g_host_mu);
    for (size_t i = 0; i < g_host.size(); i++)
        if (g_host[i].a == (uintptr_t)p) {
            g_host.erase(g_host.begin() + (long)i);
            break;
        }
}

namespace {

using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

// os[i] = base + hs[i], oe[i] = base + hs[nt + i]: a piece's unpacked u32 spans (starts, then
// ends) into the caller's arrays, a few threads when large
template <class T>
void widen_spans(const uint32_t* hs, uint32_t nt, T base, T* os, T* oe) {
    const unsigned nth = nt >= (1u << 20) ? kCopyThreads : 1u;
    auto work = [&](unsigned t) {
        const uint64_t a = (uint64_t)nt * t / nth, b = (uint64_t)nt * (t + 1) / nth;
        for (uint64_t i = a; i < b; i++) os[i] = base + hs[i];
        for (uint64_t i = a; i < b; i++) oe[i] = base + hs[nt + i];
    };
    run_threads(nth, work);
}

// Mask geometry of the range [r0, r0 + rbytes): range word j = caller word rw + j (nw words), the
// range's first bit is bit rsh of word 0.
struct MaskGeo { uint64_t rw, rsh, nw; };
MaskGeo mask_geo(const MaskDst* mask, uint64_t r0, uint64_t rbytes) {
    const uint64_t rrel = mask ? r0 - mask->batch0 : 0, rsh = rrel & 63u;
    return MaskGeo{rrel >> 6, rsh, mask ? (rsh + rbytes + 63u) >> 6 : 0};
}

// One device's range of a host batch, cut in pieces of whole documents (plan_pieces) as a
// three-stage pipeline over three streams and three threads: the stager stages piece after piece
// into pinned memory and copies it up on cstream (every piece has its own pinned and device text
// region); the launcher queues piece k's kernels on `stream` once its copy is queued (and, for
// spans, once the output set it reuses has been copied back); the calling thread (run) queues the
// copies back on dstream and hands results to the caller in order.  Each publishes its progress
// under pm_.  The caller holds d->mu.
// Search and full mode: the spans come back unpacked (they overlap, and k_span_pack's gap coding
// wants ascending disjoint spans).  A full-mode piece may give more spans than its output set
// holds: it is then run once more with a set of the size it reported, so a piece's kernels start
// only when the piece before has been collected.
class RangePipeline {
  public:
    RangePipeline(Device* d, const uint8_t* text, const uint64_t* doc_off, uint32_t d0, uint32_t d1, bool hmm,
                  SpanBuf* out, const MaskDst* mask, CutMode mode)
        : d_(d), text_(text), doc_off_(doc_off), hmm_(hmm), out_(out), mask_(mask), mode_(mode),
          search_(mode != kModePlain), full_(mode == kModeFull), r0_(doc_off[d0]), rbytes_(doc_off[d1] - r0_),
          mg_(mask_geo(mask, r0_, rbytes_)), pl_(plan_pieces(doc_off, d0, d1, d->piece_bytes)), np_(pl_.pcs.size()),
          ntok_(np_, 0), words_(np_) {}
    int prepare();  // the buffers and events the pieces need
    int run();

  private:
    static constexpr size_t kAhead = 3;  // pieces staged beyond the last collected one, at most
    static constexpr size_t kSets = Device::kSets;
    int stage(size_t k);
    int compute(size_t k);
    int collect(size_t k);  // piece k's kernels are done: queue its results' copy back
    int finish(size_t k);   // piece k's results have landed: into the caller's arrays
    template <class T>
    void put_spans(size_t k, uint64_t base, T* os, T* oe);
    void stager();
    void launcher();
    void publish(size_t* ctr, size_t v, int r) {
        std::lock_guard<std::mutex> l(pm_);
        if (r && prc_ == JB_OK) {  // (the first error's message, from the thread that met it)
            prc_ = r;
            perr_ = g_err;
        }
        if (!r) *ctr = v;
        pcv_.notify_all();
    }
    bool wait_for(const size_t* ctr, size_t v) {  // false: an error or stop
        std::unique_lock<std::mutex> l(pm_);
        pcv_.wait(l, [&] { return *ctr >= v || prc_ != JB_OK || stop_; });
        return *ctr >= v;
    }
    void stop_threads() {
        {
            std::lock_guard<std::mutex> l(pm_);
            stop_ = true;
        }
        pcv_.notify_all();
        stager_th_.join();
        launcher_th_.join();
    }
    void drain() {  // an error with work in flight: let the streams finish first
        (void)hipStreamSynchronize(d_->cstream);
        (void)hipStreamSynchronize(d_->stream);
        (void)hipStreamSynchronize(d_->dstream);
    }
    int bail(int code, const std::string& msg) {  // stop the other threads, drain, keep the message
        stop_threads();
        drain();
        g_err = msg;
        return code;
    }
    void tmark(size_t i, hipStream_t st) {
        if (i < tev_.size()) (void)hipEventRecord(tev_[i], st);
    }
    void report_pieces();

    Device* const d_;
    const uint8_t* const text_;
    const uint64_t* const doc_off_;
    const bool hmm_;
    SpanBuf* const out_;
    const MaskDst* const mask_;
    const CutMode mode_;
    const bool search_, full_;  // (search: a pass follows the pipeline)
    const uint64_t r0_, rbytes_;
    const MaskGeo mg_;
    const PiecePlan pl_;
    const size_t np_;
    bool pinned_in_ = false, pack_ = false, nt_stage_ = true;
    uint32_t side_cap_ = 0;
    std::vector<uint32_t> ntok_;  // spans each piece returns (search and full mode: the pass's count)
    std::vector<std::pair<uint64_t, uint64_t>> words_;  // mask words each piece copies back
    uint64_t mask_done_ = 0;
    jb_stats acc_{};
    std::vector<hipEvent_t> tev_;  // JB_DEBUG=2: t0, then per piece H2D done, kernels done, results back
    std::mutex pm_;  // the progress counters, the first error and stop_
    std::condition_variable pcv_;
    size_t staged_ = 0, launched_ = 0, collected_ = 0;
    int prc_ = JB_OK;
    std::string perr_;
    bool stop_ = false;
    std::thread stager_th_, launcher_th_;
    double t_stage_ = 0, t_launch_ = 0;
};

int RangePipeline::prepare() {
    Device* const d = d_;
    const uint64_t maxb = pl_.maxb, nw = mg_.nw;
    int rc;
    pinned_in_ = host_pinned(text_ + r0_, rbytes_);
    if ((rc = grow_dev(&d->text, &d->text_cap, pl_.dev_bytes)) || (rc = grow_dev(&d->doc_off, &d->doc_cap, pl_.slots)) ||
        (rc = grow_pinned(&d->h_misc, &d->h_misc_cap, pl_.slots)) ||
        (rc = grow_mapped(&d->h_pcnt, &d->d_pcnt, &d->h_pcnt_cap, (uint64_t)np_ * kSnapWords)) ||
        (!pinned_in_ && (rc = grow_pinned(&d->h_text, &d->h_text_cap, pl_.dev_bytes))) ||
        (rc = ensure_work(d, maxb, pl_.maxd)) || (rc = ensure_mode(d, mode_)))
        return rc;
    for (auto* v : {&d->ev_h2d, &d->ev_comp, &d->ev_d2h})
        while (v->size() < np_) {
            hipEvent_t e;
            HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            v->push_back(e);
        }
    pack_ = !mask_ && !search_ && d->span_pack;
    side_cap_ = pack_side_cap(maxb);
    if (!mask_) {
        for (auto& o : d->outs) {
            if ((rc = grow_dev_pair(&o.ts, &o.te, &o.cap_tok, maxb + 4)) ||
                (rc = grow_dev(&o.dt, &o.cap_docs, (uint64_t)pl_.maxd + 2)))
                return rc;
            if (pack_ && ((rc = grow_dev(&o.pk, &o.cap_pk, maxb + 4)) ||
                          (rc = grow_dev(&o.phdr, &o.cap_phdr, (maxb + 4) / kPackBlock + 2)) ||
                          (rc = grow_dev(&o.pside, &o.cap_pside, side_cap_))))
                return rc;
        }
    } else {
        if ((rc = grow_dev(&d->d_mask, &d->mask_cap, 2 * nw)) || (rc = grow_pinned(&d->h_mask, &d->mask_cap_h, 2 * nw)))
            return rc;
        HIPCHK(run_zero(d->d_mask, 2 * nw * 8, d->stream));
    }
    std::lock_guard<std::mutex> g(d->stats_mu);
    d->last_small = false;
    return JB_OK;
}

int RangePipeline::stage(size_t k) {
    Device* const d = d_;
    const uint8_t* const text = text_;
    const Piece& p = pl_.pcs[k];
    const uint64_t pb = doc_off_[p.d0], len = doc_off_[p.d1] - pb;
    for (uint32_t j = 0; j <= p.d1 - p.d0; j++) d->h_misc[p.slot + j] = doc_off_[p.d0 + j] - pb;
    HIPCHK(hipMemcpyAsync(d->doc_off + p.slot, d->h_misc + p.slot, (uint64_t)(p.d1 - p.d0 + 1) * 8,
                          hipMemcpyHostToDevice, d->cstream));
    if (pinned_in_) {
        // (the 64 zero bytes after the piece come from pinned zeros: a memset would be a
        // kernel, queued behind the persistent k_zh for CUs, and the copies behind it)
        if (len) HIPCHK(hipMemcpyAsync(d->text + p.off, text + pb, len, hipMemcpyHostToDevice, d->cstream));
        HIPCHK(hipMemcpyAsync(d->text + p.off + len, d->h_zero, 64, hipMemcpyHostToDevice, d->cstream));
    } else {
        // kCopyThreads threads stage their share in 4 MiB sub-pieces and queue each one's copy at once
        const uint64_t total = len + 64, kSub = 4ull << 20;
        memset(d->h_text + p.off + len, 0, 64);
        const unsigned nth = total >= (16ull << 20) ? kCopyThreads : 1u;
        const uint64_t share = ((total + nth - 1) / nth + 4095) & ~4095ull;
        const bool nt_stage = nt_stage_;
        std::atomic<int> err{0};
        auto work = [&](unsigned t) {
            if (hipSetDevice(d->ordinal) != hipSuccess) err = 1;
            const uint64_t lo = std::min(total, t * share), hi = std::min(total, lo + share);
            for (uint64_t o = lo; o < hi; o += kSub) {
                const uint64_t l = std::min(kSub, hi - o);
                if (o < len) {
                    if (nt_stage) nt_copy(d->h_text + p.off + o, text + pb + o, std::min(l, len - o));
                    else memcpy(d->h_text + p.off + o, text + pb + o, std::min(l, len - o));
                }
                if (hipMemcpyAsync(d->text + p.off + o, d->h_text + p.off + o, l, hipMemcpyHostToDevice,
                                   d->cstream) != hipSuccess)
                    err = 1;
            }
        };
        run_threads(nth, work);
        if (err) return fail(JB_EDEVICE, "H2D copy failed");
    }
    HIPCHK(hipEventRecord(d->ev_h2d[k], d->cstream));
    tmark(1 + 3 * k, d->cstream);
    return JB_OK;
}

int RangePipeline::compute(size_t k) {
    Device* const d = d_;
    const Piece& p = pl_.pcs[k];
    const uint64_t pb = doc_off_[p.d0], len = doc_off_[p.d1] - pb;
    HIPCHK(hipStreamWaitEvent(d->stream, d->ev_h2d[k], 0));
    const Device::OutSet& o = d->outs[k % kSets];
    MaskOut mo{nullptr, nullptr, 0};
    if (mask_) mo = MaskOut{d->d_mask, d->d_mask + mg_.nw, mg_.rsh + (pb - r0_)};
    else if (k >= kSets) HIPCHK(hipStreamWaitEvent(d->stream, d->ev_d2h[k - kSets], 0));
    // (search and full mode: the plain spans stay in the workspace, the mode's list goes to the output set)
    const SpanDst dst{o.ts, o.te, o.cap_tok, o.dt, nullptr};
    const SpanTarget t = span_target(d, mode_, mask_ ? nullptr : &dst, d->w.cap_bytes);
    int r;
    if ((r = launch(d, t.w, d->text + p.off, len, d->doc_off + p.slot, p.d1 - p.d0, hmm_, d->stream,
                    mask_ ? &mo : nullptr, t.post())))
        return r;
    d->last_nbytes = len;
    if (pack_) {  // the spans packed for the trip back: 4 B per token (k_span_pack)
        const hipError_t ep = run_span_pack(o.ts, o.te, d->w.counters, o.pk, o.phdr, o.pside, side_cap_, len + 1,
                                            d->stream);
        if (ep != hipSuccess) return fail(JB_EDEVICE, "k_span_pack: %s", hipGetErrorString(ep));
    }
    // counters and block counts by a kernel into mapped memory: a copy-engine transfer here
    // would queue behind the bulk copies of later pieces and hold up this stream
    const hipError_t es = run_snap(d->w, len, d->d_pcnt + k * kSnapWords, d->stream);
    if (es != hipSuccess) return fail(JB_EDEVICE, "k_snap: %s", hipGetErrorString(es));
    HIPCHK(hipEventRecord(d->ev_comp[k], d->stream));
    tmark(2 + 3 * k, d->stream);
    return JB_OK;
}

int RangePipeline::collect(size_t k) {
    Device* const d = d_;
    const Piece& p = pl_.pcs[k];
    Device::OutSet& o = d->outs[k % kSets];
    const volatile uint32_t* c = d->h_pcnt + k * kSnapWords;
    int r;
    for (int tries = 0;; tries++) {  // (full mode: at most two)
        HIPCHK(hipEventSynchronize(d->ev_comp[k]));
        if (c[CNT_ERR] & 2u) return fail(JB_EDEVICE, "k_long: a phase wait gave up (no progress for JB_LONG_WAIT_US)");
        if (c[CNT_ERR] & 4u) return fail(JB_EDEVICE, "internal: k_span_pack's side list overflowed");
        if (c[CNT_ERR] & ~8u) return fail(JB_EPANIC, "a Han block has no DAG path (the reference panics in cutDAG)");
        if (c[CNT_NTOK] != c[CNT_NTOKE])
            return fail(JB_EDEVICE, "internal: %u token starts vs %u ends", c[CNT_NTOK], c[CNT_NTOKE]);
        if (!full_) break;
        // (bit 3 of CNT_ERR: the list is longer than the output set)
        const uint64_t nfull = (uint64_t)c[CNT_NSRCH] | (uint64_t)c[CNT_NSRCH + 1] << 32;
        if (nfull >= (1ull << 32))
            return fail(JB_ELIMIT, "a piece of the batch gives %llu full-mode spans (limit 2^32 - 1)",
                        (unsigned long long)nfull);
        if (nfull <= o.cap_tok) break;
        if (tries) return fail(JB_EDEVICE, "internal: %llu full-mode spans after a run that counted fewer",
                               (unsigned long long)nfull);
        // the launcher waits for this piece's collection, so the stream is idle and the set unused:
        // once more, with a set of the size the piece reported
        if ((r = grow_dev_pair(&o.ts, &o.te, &o.cap_tok, nfull + 4)) || (r = compute(k))) return r;
    }
    const uint32_t nt = ntok_[k] = search_ ? c[CNT_NSRCH] : c[CNT_NTOK];
    HIPCHK(hipStreamWaitEvent(d->dstream, d->ev_comp[k], 0));
    if (!mask_) {
        if ((!pack_ && (r = grow_pinned(&o.hs, &o.hcap_tok, 2ull * nt + 2))) ||
            (r = grow_pinned(&o.hdt, &o.hcap_docs, (uint64_t)(p.d1 - p.d0) + 2)))
            return r;
        if (pack_) {
            const uint32_t nside = c[CNT_SIDE], nb = (nt + kPackBlock - 1u) / kPackBlock;
            if ((r = grow_pinned(&o.hpk, &o.hcap_pk, (uint64_t)nt + 1)) ||
                (r = grow_pinned(&o.hhdr, &o.hcap_hdr, (uint64_t)nb + 1)) ||
                (r = grow_pinned(&o.hside, &o.hcap_side, (uint64_t)nside + 1)))
                return r;
            if (nt) {
                HIPCHK(hipMemcpyAsync(o.hpk, o.pk, (uint64_t)nt * 2, hipMemcpyDeviceToHost, d->dstream));
                HIPCHK(hipMemcpyAsync(o.hhdr, o.phdr, (uint64_t)nb * 4, hipMemcpyDeviceToHost, d->dstream));
            }
            if (nside)
                HIPCHK(hipMemcpyAsync(o.hside, o.pside, (uint64_t)nside * 16, hipMemcpyDeviceToHost, d->dstream));
        } else if (nt) {
            HIPCHK(hipMemcpyAsync(o.hs, o.ts, (uint64_t)nt * 4, hipMemcpyDeviceToHost, d->dstream));
            HIPCHK(hipMemcpyAsync(o.hs + nt, o.te, (uint64_t)nt * 4, hipMemcpyDeviceToHost, d->dstream));
        }
        HIPCHK(hipMemcpyAsync(o.hdt, o.dt, (uint64_t)(p.d1 - p.d0 + 1) * 8, hipMemcpyDeviceToHost, d->dstream));
    } else {
        // final words: those before the word that holds the next piece's first bit
        const uint64_t nw = mg_.nw;
        const uint64_t hi = k + 1 < np_ ? (mg_.rsh + (doc_off_[pl_.pcs[k + 1].d0] - r0_)) >> 6 : nw;
        const uint64_t lo = mask_done_;
        if (hi > lo) {
            HIPCHK(hipMemcpyAsync(d->h_mask + lo, d->d_mask + lo, (hi - lo) * 8, hipMemcpyDeviceToHost, d->dstream));
            HIPCHK(hipMemcpyAsync(d->h_mask + nw + lo, d->d_mask + nw + lo, (hi - lo) * 8, hipMemcpyDeviceToHost,
                                  d->dstream));
            mask_done_ = hi;
        }
        words_[k] = {lo, std::max(lo, hi)};
    }
    HIPCHK(hipEventRecord(d->ev_d2h[k], d->dstream));
    tmark(3 + 3 * k, d->dstream);
    return JB_OK;
}

// Piece k's spans from its output set's pinned copy to os / oe (T: u64 batch offsets, or u32
// offsets from the caller's first byte).
template <class T>
void RangePipeline::put_spans(size_t k, uint64_t base, T* os, T* oe) {
    const Device::OutSet& o = d_->outs[k % kSets];
    if (pack_) unpack_spans(o.hpk, o.hhdr, o.hside, d_->h_pcnt[k * kSnapWords + CNT_SIDE], ntok_[k], base, os, oe);
    else widen_spans(o.hs, ntok_[k], (T)base, os, oe);
}

int RangePipeline::finish(size_t k) {
    Device* const d = d_;
    SpanBuf* const out = out_;
    const Piece& p = pl_.pcs[k];
    HIPCHK(hipEventSynchronize(d->ev_d2h[k]));
    const uint32_t nt = ntok_[k];
    {
        const volatile uint32_t* c = d->h_pcnt + k * kSnapWords;
        acc_.tokens += c[CNT_NTOK];  // (the Cut tokens, in search mode too)
        acc_.long_blocks += c[CNT_NLONG];
        acc_.viterbi_ties += c[CNT_TIES];
        acc_.blocks += (uint64_t)c[CNT_CLEAR] | (uint64_t)c[CNT_CLEAR + 1] << 32;
        acc_.zh_blocks += (uint64_t)c[CNT_CLEAR + 2] | (uint64_t)c[CNT_CLEAR + 3] << 32;
    }
    if (mask_) {
        put_mask_words(mask_, mg_.rw, mg_.nw, words_[k].first, words_[k].second, d->h_mask, d->h_mask + mg_.nw);
        out->n += nt;
        return JB_OK;
    }
    const bool write = out->reserve(out->n + nt);
    if (!write && !out->external) return fail(JB_ENOMEM, "out of host memory for %u tokens", nt);
    if (write && out->s32) {
        put_spans(k, doc_off_[p.d0] - out->b32, out->s32 + out->n, out->e32 + out->n);
    } else if (write) {
        put_spans(k, doc_off_[p.d0], out->s + out->n, out->e + out->n);
    } else {  // caller arrays too small: count the rest, write nothing more
        out->cap = 0;
    }
    out->n += nt;
    const uint64_t* const hdt = d->outs[k % kSets].hdt;
    for (uint32_t j = 0; j < p.d1 - p.d0; j++) out->per_doc.push_back(hdt[j + 1] - hdt[j]);
    return JB_OK;
}

void RangePipeline::stager() {
    const auto a = Clock::now();
    if (hipSetDevice(d_->ordinal) != hipSuccess) {
        publish(&staged_, 0, fail(JB_EDEVICE, "hipSetDevice(%d) failed", d_->ordinal));
        return;
    }
    for (size_t k = 0; k < np_; k++) {
        {
            std::lock_guard<std::mutex> l(pm_);
            if (stop_ || prc_) break;
        }
        // at most kAhead pieces' copies queued beyond the last piece whose kernels are done: a
        // deeper queue of bulk copies (pinned input queues all of them at once) delayed the
        // first pieces' kernels by 13 ms, everything on the device waiting behind the copies
        if (k >= kAhead && !wait_for(&collected_, k - kAhead + 1)) break;
        const int r = stage(k);
        publish(&staged_, k + 1, r);
        if (r) break;
    }
    t_stage_ = ms_between(a, Clock::now());
}

void RangePipeline::launcher() {
    const auto a = Clock::now();
    if (hipSetDevice(d_->ordinal) != hipSuccess) {
        publish(&launched_, 0, fail(JB_EDEVICE, "hipSetDevice(%d) failed", d_->ordinal));
        return;
    }
    for (size_t k = 0; k < np_; k++) {
        if (!wait_for(&staged_, k + 1)) break;
        if (!mask_ && k >= kSets && !wait_for(&collected_, k - kSets + 1)) break;
        if (full_ && !wait_for(&collected_, k)) break;  // (collect may run piece k - 1 once more)
        const int r = compute(k);
        publish(&launched_, k + 1, r);
        if (r) break;
    }
    t_launch_ = ms_between(a, Clock::now());
}

void RangePipeline::report_pieces() {  // JB_DEBUG=2
    (void)hipDeviceSynchronize();
    fprintf(stderr, "[jb] piece: H2D done / kernels done / results back (ms from the start)\n");
    for (size_t k = 0; k < np_; k++) {
        float a = 0, b = 0, c = 0;
        (void)hipEventElapsedTime(&a, tev_[0], tev_[1 + 3 * k]);
        (void)hipEventElapsedTime(&b, tev_[0], tev_[2 + 3 * k]);
        (void)hipEventElapsedTime(&c, tev_[0], tev_[3 + 3 * k]);
        fprintf(stderr, "[jb]   %2zu: %7.2f %7.2f %7.2f\n", k, a, b, c);
    }
    for (auto& e : tev_) (void)hipEventDestroy(e);
}

int RangePipeline::run() {
    Device* const d = d_;
    static const bool tdbg2 = env_int("JB_DEBUG", 0) >= 2;  // per-piece event clocks
    if (tdbg2) {
        tev_.resize(1 + 3 * np_);
        for (auto& e : tev_) (void)hipEventCreate(&e);
        (void)hipEventRecord(tev_[0], d->stream);
    }
    static const bool nt_stage = env_int("JB_NT_STAGE", 1) != 0;  // (A/B switch)
    nt_stage_ = nt_stage;
    static const bool tdbg = getenv("JB_DEBUG") != nullptr;
    const auto c0 = Clock::now();
    stager_th_ = std::thread([this] { stager(); });
    launcher_th_ = std::thread([this] { launcher(); });
    double t_wait = 0, t_collect = 0, t_finish = 0;
    int rc;
    for (size_t k = 0; k < np_; k++) {
        auto a = Clock::now();
        const bool ok = wait_for(&launched_, k + 1);
        t_wait += ms_between(a, Clock::now());
        if (!ok) {
            int code;
            std::string msg;
            {
                std::lock_guard<std::mutex> l(pm_);
                code = prc_ ? prc_ : JB_EDEVICE;
                msg = prc_ ? perr_ : "host pipeline stopped";
            }
            return bail(code, msg);
        }
        a = Clock::now();
        rc = collect(k);
        t_collect += ms_between(a, Clock::now());
        if (rc) return bail(rc, g_err);
        publish(&collected_, k + 1, JB_OK);
        if (k == 0) continue;
        a = Clock::now();
        rc = finish(k - 1);
        t_finish += ms_between(a, Clock::now());
        if (rc) return bail(rc, g_err);
    }
    stop_threads();
    if ((rc = finish(np_ - 1))) {
        drain();
        return rc;
    }
    d->acc = acc_;
    d->acc_valid = true;
    if (tdbg2) report_pieces();
    if (tdbg)
        fprintf(stderr, "[jb] host range %.1f MiB (%s%s) in %zu pieces: %.2f ms (stager %.2f, launcher %.2f; here: "
                        "waits for launches %.2f, kernels %.2f, results %.2f)\n", rbytes_ / 1048576.0,
                mask_ ? "masks" : "spans", pinned_in_ ? ", pinned input" : "", np_, ms_between(c0, Clock::now()),
                t_stage_, t_launch_, t_wait, t_collect, t_finish);
    return JB_OK;
}

// Cut documents [d0, d1) of a host batch on one device: appends spans to `out`, or
// with `mask` writes the range's boundary bits into the caller's masks (out->n counts
// the tokens).  A plain range that fits k_small is one launch (cut_small); any other,
// and every search- or full-mode range, takes the piece pipeline.
int cut_range(Device* d, const uint8_t* text, const uint64_t* doc_off, uint32_t d0, uint32_t d1, bool hmm,
              SpanBuf* out, const MaskDst* mask, CutMode mode) {
    if (d0 >= d1) return JB_OK;
    const uint64_t r0 = doc_off[d0], rbytes = doc_off[d1] - r0;
    const uint32_t ndr = d1 - d0;
    int rc;
    // (small batches: k_small on its own stream and buffers, coalesced across callers, without
    // the device lock that the pipeline below holds)
    if (mode == kModePlain && d->lc.small_max && rbytes <= d->lc.small_max && ndr <= kSmallDocs) {
        if (!mask) return cut_small(d, text, doc_off + d0, ndr, hmm, out);
        const MaskGeo mg = mask_geo(mask, r0, rbytes);
        SpanBuf tmp;
        if ((rc = cut_small(d, text, doc_off + d0, ndr, hmm, &tmp))) {
            tmp.release();
            return rc;
        }
        std::vector<uint64_t> ws(2 * mg.nw, 0ull);
        for (size_t k = 0; k < tmp.n; k++) {
            const uint64_t a = tmp.s[k] - r0 + mg.rsh, b = tmp.e[k] - 1 - r0 + mg.rsh;
            ws[a >> 6] |= 1ull << (a & 63u);
            ws[mg.nw + (b >> 6)] |= 1ull << (b & 63u);
        }
        put_mask_words(mask, mg.rw, mg.nw, 0, mg.nw, ws.data(), ws.data() + mg.nw);
        out->n += tmp.n;
        tmp.release();
        return JB_OK;
    }
    std::lock_guard<std::mutex> g(d->mu);
    HIPCHK(hipSetDevice(d->ordinal));
    for (uint32_t k = d0; k < d1; k++)
        if (doc_off[k + 1] - doc_off[k] >= (1ull << 31))
            return fail(JB_ELIMIT, "document %u is %llu bytes (limit 2 GiB)", k,
                        (unsigned long long)(doc_off[k + 1] - doc_off[k]));
    RangePipeline rp(d, text, doc_off, d0, d1, hmm, out, mask, mode);
    if ((rc = rp.prepare())) return rc;
    return rp.run();
}

}  // namespace

int cut_sharded(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                std::vector<SpanBuf>* sbp, const MaskDst* mask, std::vector<uint32_t>* unit_doc, CutMode mode) {
    if (ndocs && !text && doc_off[ndocs] > doc_off[0]) return fail(JB_EINVAL, "null text");
    for (uint32_t k = 0; k < ndocs; k++)
        if (doc_off[k + 1] < doc_off[k]) return fail(JB_EINVAL, "doc_off not monotonic at %u", k);
    std::vector<SpanBuf>& sb = *sbp;
    const size_t nd = ctx->devs.size();
    std::vector<uint64_t> piece_bytes(nd > 1 ? nd : 0);  // (one device: no allocation on a small call's path)
    for (size_t k = 0; k < piece_bytes.size(); k++) piece_bytes[k] = ctx->devs[k]->piece_bytes;
    const uint64_t* const pbs = nd > 1 ? piece_bytes.data() : &ctx->devs[0]->piece_bytes;
    Units un;
    std::vector<uint64_t> cutb;
    bool split;
    int rc0 = plan_units(text, doc_off, ndocs, pbs, nd, &un, &cutb, &split);
    if (rc0) return rc0;
    const uint64_t* uoff = split ? un.off.data() : doc_off;
    if (unit_doc) {
        unit_doc->clear();
        if (split) *unit_doc = un.doc;
    }
    for (auto& d : ctx->devs) {  // jb_last_stats: only the devices this batch reaches
        std::lock_guard<std::mutex> g(d->stats_mu);
        d->has_stats = false;
    }
    if (mask)  // the words a device range shares with its neighbours are ORed into: clear them first
        for (size_t k = 0; k < nd; k++)
            if (cutb[k] < cutb[k + 1]) {
                mask->s[(cutb[k] - mask->batch0) >> 6] = 0;
                mask->e[(cutb[k] - mask->batch0) >> 6] = 0;
                mask->s[(cutb[k + 1] - 1 - mask->batch0) >> 6] = 0;
                mask->e[(cutb[k + 1] - 1 - mask->batch0) >> 6] = 0;
            }
    std::vector<int> rcs(nd, JB_OK);
    std::vector<std::string> errs(nd);
    auto work = [&](size_t k) {
        const uint32_t u0 = split ? un.dev[k] : (k == 0 ? 0u : ndocs), u1 = split ? un.dev[k + 1] : ndocs;
        if (u0 < u1) {
            rcs[k] = cut_range(ctx->devs[k].get(), text, uoff, u0, u1, hmm != 0, &sb[k], mask, mode);
            if (rcs[k]) errs[k] = g_err;
        }
    };
    if (nd == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (size_t k = 0; k < nd; k++) th.emplace_back(work, k);
        for (auto& t : th) t.join();
    }
    for (size_t k = 0; k < nd; k++)
        if (rcs[k]) return fail(rcs[k], "%s", errs[k].c_str());
    return JB_OK;
}

// doc_tok from the tokens per unit (in unit order over the devices' buffers)
void fill_doc_tok(const std::vector<SpanBuf>& sb, uint32_t ndocs, uint64_t* doc_tok,
                         const std::vector<uint32_t>& unit_doc) {
    for (uint32_t d = 0; d <= ndocs; d++) doc_tok[d] = 0;
    size_t u = 0;
    for (const auto& b : sb)
        for (uint64_t c : b.per_doc) {
            const uint32_t d = unit_doc.empty() ? (uint32_t)u : unit_doc[u];
            doc_tok[d + 1] += c;
            u++;
        }
    for (uint32_t d = 0; d < ndocs; d++) doc_tok[d + 1] += doc_tok[d];
}
