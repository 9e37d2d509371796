// jb_small.cpp — small host batches: one k_small launch, shared by concurrent callers.
#include <string.h>

#include <chrono>
#include <thread>

#include "jb_host.h"

// A batch of at most lc.small_max bytes and kSmallDocs documents (a single Cut
// call, BASELINE config 1) is one k_small launch that reads the text and offsets
// from mapped pinned host memory (or its kernel arguments) and writes the spans
// there.  Concurrent calls on a device are coalesced (the reference runs Cut calls
// side by side under RLock, tokenizer.go:151-153): each call queues a SmallReq.  A
// caller that finds a slot free (one of JB_SMALL_SLOTS pinned input/output buffer pairs,
// each with its own stream on its own CU) launches the queue's head requests (same hmm,
// up to the k_small limits together) as ONE k_small batch on it, their documents back to
// back, waits for that batch's completion word and hands each caller its own spans by its
// documents' doc_tok ranges.  The slot then goes straight to the caller of the next
// queued request, with the next batch: callers wait on their own request's state word,
// so a finished batch wakes the callers it served and the one it hands the slot to, not
// every waiting caller.  One caller alone: a batch of one.
struct SmallReq {
    const uint8_t* text;
    const uint64_t* doc_off;  // doc_off[0..nd] absolute in text
    uint32_t nd;
    bool hmm;
    SpanBuf* out;
    int rc = JB_OK;
    std::string err;
    // kQueued, then kDone; or kLaunch first: this caller launches `batch` (its own request at
    // the head) on slot `sl`, which the caller that finished that slot's last batch handed over
    std::atomic<uint32_t> state{0};
    Device::SmallSlot* sl = nullptr;
    std::vector<SmallReq*> batch;
};
enum : uint32_t { kQueued = 0, kLaunch = 1, kDone = 2 };

// Every request of a batch fails with rc and the thread's message.
static void small_fail(SmallReq* const* rq, uint32_t n, int rc) {
    for (uint32_t i = 0; i < n; i++) {
        rq[i]->rc = rc;
        rq[i]->err = g_err;
    }
}

// One k_small launch over requests rq[0..n) (together within the limits) on the slot's
// next output buffer: stage, launch, wait for the completion word.  Returns the output
// (header, spans, doc_tok), or nullptr with each request's rc / err set.
static const uint32_t* small_launch(Device* d, Device::SmallSlot* sl, SmallReq* const* rq, uint32_t n) {
    auto fail_all = [&](int rc) { small_fail(rq, n, rc); };
    auto chk = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        fail_all(fail(e == hipErrorOutOfMemory ? JB_ENOMEM : JB_EDEVICE, "%s: %s", what, hipGetErrorString(e)));
        return false;
    };
    if (!chk(hipSetDevice(d->ordinal), "hipSetDevice")) return nullptr;
    if (!sl->h_sin || !sl->h_sout[0] || !sl->h_sout[1]) {
        // all three buffers or none: a failure part way frees what was allocated, so the
        // next call on the slot allocates again instead of using a null buffer
        auto drop = [&]() {
            for (void** p : {(void**)&sl->h_sin, (void**)&sl->h_sout[0], (void**)&sl->h_sout[1]})
                if (*p) {
                    (void)hipHostFree(*p);
                    *p = nullptr;
                }
            sl->d_sin = nullptr;
            sl->d_sout[0] = sl->d_sout[1] = nullptr;
        };
        drop();
        const unsigned fl = hipHostMallocMapped | hipHostMallocCoherent;
        if (!chk(hipHostMalloc(&sl->h_sin, kSmallBytes + 128 + 8 * (kSmallDocs + 1), fl), "hipHostMalloc") ||
            !chk(hipHostGetDevicePointer((void**)&sl->d_sin, sl->h_sin, 0), "hipHostGetDevicePointer")) {
            drop();
            return nullptr;
        }
        for (int k = 0; k < 2; k++) {
            if (!chk(hipHostMalloc(&sl->h_sout[k], kSmallOutBytes, fl), "hipHostMalloc") ||
                !chk(hipHostGetDevicePointer((void**)&sl->d_sout[k], sl->h_sout[k], 0), "hipHostGetDevicePointer")) {
                drop();
                return nullptr;
            }
            sl->h_sout[k][SM_DONE] = 0;  // (recycled pinned memory may hold any value; seq starts at 1)
        }
    }
    // the other buffer: the last batch's callers may still be taking their spans from this one
    sl->ob ^= 1u;
    while (sl->reading[sl->ob].load(std::memory_order_acquire)) __builtin_ia32_pause();
    const bool hmm = rq[0]->hmm;
    uint64_t nbytes = 0;
    uint32_t nd = 0;
    for (uint32_t i = 0; i < n; i++) {
        nbytes += rq[i]->doc_off[rq[i]->nd] - rq[i]->doc_off[0];
        nd += rq[i]->nd;
    }
    const auto c0 = std::chrono::steady_clock::now();
    // a batch that fits the kernel arguments (96 bytes, 7 documents) travels in them (the kernel reads them from
    // the kernarg segment instead of host memory over PCIe); others go through h_sin
    const bool inl = nbytes <= kSmallInline && nd <= kSmallInlineDocs;
    SmallInline in;
    memset(&in, 0, sizeof in);
    uint8_t* const tx = inl ? in.txt : sl->h_sin;
    uint64_t* const hoff = reinterpret_cast<uint64_t*>(sl->h_sin + kSmallBytes + 128);
    uint64_t at = 0;
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; i++) {
        const SmallReq& r = *rq[i];
        const uint64_t base = r.doc_off[0], len = r.doc_off[r.nd] - base;
        if (len) memcpy(tx + at, r.text + base, len);
        for (uint32_t j = 0; j < r.nd; j++, k++) {
            if (inl) in.doff[k] = (uint16_t)(at + r.doc_off[j] - base);
            else hoff[k] = at + r.doc_off[j] - base;
        }
        at += len;
    }
    if (inl) in.doff[nd] = (uint16_t)nbytes;
    else {
        hoff[nd] = nbytes;
        memset(sl->h_sin + nbytes, 0, 16);
    }
    // the kernel writes the call's sequence number after everything else (system-scope
    // release); spinning on it returns as soon as the results are in host memory
    const uint32_t seq = ++sl->seq;
    volatile uint32_t* done = sl->h_sout[sl->ob] + SM_DONE;
    if (!chk(run_small(d->dim, inl ? nullptr : sl->d_sin, (uint32_t)nbytes,
                       inl ? nullptr : reinterpret_cast<const uint64_t*>(sl->d_sin + kSmallBytes + 128), nd, hmm,
                       sl->d_sout[sl->ob], seq, in, sl->st),
             "k_small launch"))
        return nullptr;
    const auto c1 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0; *done != seq; spin++) {
        if ((spin & 1023u) != 1023u) continue;
        const hipError_t q = hipStreamQuery(sl->st);
        if (q == hipErrorNotReady) continue;
        if (!chk(q, "k_small")) return nullptr;
        if (*done != seq) {
            fail_all(fail(JB_EDEVICE, "k_small finished without its completion word"));
            return nullptr;
        }
        break;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    const auto c2 = std::chrono::steady_clock::now();
    static const bool trace = getenv("JB_SMALL_TRACE") != nullptr;
    if (trace) {
        auto us = [](std::chrono::steady_clock::time_point t) {
            return std::chrono::duration<double, std::micro>(t.time_since_epoch()).count();
        };
        std::lock_guard<std::mutex> g(d->stats_mu);
        d->small_trace.push_back({(double)(sl - d->slots), (double)n, us(c0), us(c1), us(c2),
                                  us(std::chrono::steady_clock::now())});
    }
    const uint32_t* h = sl->h_sout[sl->ob];
    {
        std::lock_guard<std::mutex> g(d->stats_mu);  // (jb_last_stats reads these; not d->mu: see Device)
        memcpy(d->small_hdr, h, sizeof d->small_hdr);
        d->last_small = true;
        d->has_stats = true;
    }
    static const bool dbg = getenv("JB_DEBUG") != nullptr;
    if (dbg) {  // k_small's phase clocks (10 ns ticks from its start)
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double, std::micro>(b - a).count();
        };
        fprintf(stderr, "[jb] k_small %llu bytes, %u calls: stage+launch %.2f us, sync %.2f us; phases (us):",
                (unsigned long long)nbytes, n, us(c0, c1), us(c1, c2));
        for (int q = 0; q < 15; q++) fprintf(stderr, " %.2f", h[SM_CLK + q] * 0.01);
        fprintf(stderr, "; %u clocks (walk end %u, viterbi fwd %u, traceback %u; dp %u %u %u)", h[SM_CLK + 15],
                h[SM_CLK + 16], h[SM_CLK + 17], h[SM_CLK + 18], h[SM_CLK + 19], h[SM_CLK + 20], h[SM_CLK + 21]);
        fprintf(stderr, "\n");
    }
    return h;
}

// After a batch: its errors.  0 = spans to split; 1 = each request's rc / err set (a
// panic on one request of several: they were rerun one by one on the slot).
static void small_batch(Device* d, Device::SmallSlot* sl, SmallReq* const* rq, uint32_t n);
static int small_check(Device* d, Device::SmallSlot* sl, const uint32_t* h, SmallReq* const* rq, uint32_t n) {
    auto fail_all = [&](int rc) { small_fail(rq, n, rc); };
    if (h[SM_ERR]) {  // the reference panics on some document: find whose (each call alone)
        if (n > 1) {
            for (uint32_t i = 0; i < n; i++) small_batch(d, sl, rq + i, 1);
            return 1;
        }
        fail_all(fail(JB_EPANIC, "a Han block has no DAG path (the reference panics in cutDAG)"));
        return 1;
    }
    if (h[SM_NTOK] != h[SM_NTOKE]) {
        fail_all(fail(JB_EDEVICE, "internal: %u token starts vs %u ends", h[SM_NTOK], h[SM_NTOKE]));
        return 1;
    }
    return 0;
}

// Each request's spans out of a batch's output h (batch offsets -> the call's own text).
static void small_split(const uint32_t* h, SmallReq* const* rq, uint32_t n) {
    uint64_t at = 0;
    uint32_t k = 0;
    const uint32_t* hs = h + kSmallHdr;
    const uint32_t* he = hs + kSmallBytes;
    const uint64_t* dt = reinterpret_cast<const uint64_t*>(he + kSmallBytes);
    for (uint32_t i = 0; i < n; i++) {
        SmallReq& r = *rq[i];
        SpanBuf* out = r.out;
        const uint64_t base = r.doc_off[0];
        const uint64_t t0 = dt[k], t1 = dt[k + r.nd], nt = t1 - t0;
        const bool write = out->reserve(out->n + nt);
        if (!write && !out->external) {
            r.rc = fail(JB_ENOMEM, "out of host memory for %llu tokens", (unsigned long long)nt);
            r.err = g_err;
        } else {
            if (write && out->s32) {
                for (uint64_t t = 0; t < nt; t++) {  // (batch offsets -> this call's text, less b32)
                    out->s32[out->n + t] = (uint32_t)(base - out->b32 + hs[t0 + t] - at);
                    out->e32[out->n + t] = (uint32_t)(base - out->b32 + he[t0 + t] - at);
                }
            } else if (write) {
                for (uint64_t t = 0; t < nt; t++) {  // (batch offsets -> this call's text)
                    out->s[out->n + t] = base + hs[t0 + t] - at;
                    out->e[out->n + t] = base + he[t0 + t] - at;
                }
            } else {  // caller arrays too small: count the rest, write nothing more
                out->cap = 0;
            }
            out->n += nt;
            for (uint32_t j = 0; j < r.nd; j++) out->per_doc.push_back(dt[k + j + 1] - dt[k + j]);
        }
        at += r.doc_off[r.nd] - base;
        k += r.nd;
    }
}

// One whole batch, its callers' spans split before it returns (a lone rerun).
static void small_batch(Device* d, Device::SmallSlot* sl, SmallReq* const* rq, uint32_t n) {
    const uint32_t* h = small_launch(d, sl, rq, n);
    if (h && !small_check(d, sl, h, rq, n)) small_split(h, rq, n);
}

// The queue's head requests (same hmm as the head, together within the k_small limits),
// taken off the queue.  Under small_mu.
static std::vector<SmallReq*> take_batch(Device* d) {
    std::vector<SmallReq*> b;
    uint64_t bytes = 0;
    uint32_t docs = 0;
    const bool h = d->small_q.front()->hmm;
    for (auto it = d->small_q.begin(); it != d->small_q.end();) {
        SmallReq* q = *it;
        const uint64_t len = q->doc_off[q->nd] - q->doc_off[0];
        if (q->hmm != h || bytes + len > d->lc.small_max || docs + q->nd > kSmallDocs) {
            ++it;
            continue;
        }
        bytes += len;
        docs += q->nd;
        b.push_back(q);
        it = d->small_q.erase(it);
    }
    return b;
}

// Runs batch b on slot sl, completes its requests, and passes the slot on: the next batch
// from the queue goes to its head request's caller (which is waiting on its own state word,
// so a finished batch wakes one caller, not every waiting one), else the slot goes free.
static void small_run(Device* d, Device::SmallSlot* sl, std::vector<SmallReq*> b) {
    const uint32_t n = (uint32_t)b.size();
    const uint32_t* h = small_launch(d, sl, b.data(), n);
    const bool split = h && !small_check(d, sl, h, b.data(), n);
    const uint32_t ob = sl->ob;
    if (split) sl->reading[ob].store(true, std::memory_order_relaxed);  // (the slot is still ours)
    std::unique_lock<std::mutex> lk(d->small_mu);
    if (!d->small_q.empty()) {
        std::vector<SmallReq*> nb = take_batch(d);
        SmallReq* const next = nb[0];
        next->sl = sl;
        next->batch = std::move(nb);
        next->state.store(kLaunch, std::memory_order_release);
    } else {
        sl->busy = false;
    }
    const bool asleep = d->small_sleepers > 0;
    lk.unlock();
    if (asleep) d->small_cv.notify_all();  // (the caller handed the slot may be asleep)
    if (split) {  // (the slot's next batch writes the other buffer meanwhile)
        small_split(h, b.data(), n);
        sl->reading[ob].store(false, std::memory_order_release);
    }
    for (SmallReq* q : b) q->state.store(kDone, std::memory_order_release);  // (q may be gone after this)
    lk.lock();  // (a caller asleep on small_cv checked its state under small_mu)
    const bool wake = d->small_sleepers > 0;
    lk.unlock();
    if (wake) d->small_cv.notify_all();
}

int cut_small(Device* d, const uint8_t* text, const uint64_t* doc_off, uint32_t nd, bool hmm,
                     SpanBuf* out) {
    SmallReq r{text, doc_off, nd, hmm, out};
    {
        std::unique_lock<std::mutex> lk(d->small_mu);
        d->small_q.push_back(&r);
        Device::SmallSlot* sl = nullptr;
        for (uint32_t k = 0; k < d->small_slots && !sl; k++)
            if (!d->slots[k].busy) sl = &d->slots[k];
        if (sl) {  // a free slot: launch the queue's head requests on it now
            sl->busy = true;
            std::vector<SmallReq*> b = take_batch(d);
            lk.unlock();
            small_run(d, sl, std::move(b));
        }
    }
    // wait on this request's own word: done by another caller's batch, or handed a slot to
    // launch on.  Spin up to ~100 us first (a batch takes 20-40 us; a sleeping caller's
    // wake-up costs about as much again), then yield the CPU between looks up to ~2 ms
    // (queued behind other batches), then sleep on small_cv.
    for (;;) {
        uint32_t st = r.state.load(std::memory_order_acquire);
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t i = 1; st == kQueued; i++) {
            if ((i & 63u) == 0) {
                const auto w = std::chrono::steady_clock::now() - t0;
                if (w > std::chrono::microseconds(2000)) break;
                if (w > std::chrono::microseconds(100)) std::this_thread::yield();
            }
            __builtin_ia32_pause();
            st = r.state.load(std::memory_order_acquire);
        }
        if (st == kQueued) {
            std::unique_lock<std::mutex> lk(d->small_mu);
            d->small_sleepers++;
            d->small_cv.wait(lk, [&] { return r.state.load(std::memory_order_acquire) != kQueued; });
            d->small_sleepers--;
            st = r.state.load(std::memory_order_acquire);
        }
        if (st == kDone) break;
        // kLaunch: this caller runs the batch it was handed (its own request among them)
        r.state.store(kQueued, std::memory_order_relaxed);
        small_run(d, r.sl, std::move(r.batch));
    }
    if (r.rc) g_err = r.err;
    return r.rc;
}
