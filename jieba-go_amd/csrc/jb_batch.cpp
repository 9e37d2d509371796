// jb_batch.cpp — the host-text analytics calls of the C ABI (include/jiebahip.h): a batch in host memory in, one
// result out, through the public *_device entry points of jb_capi.cpp on a stream of the first device and in the
// ctx's grow-only buffers (jb_batch.h).
//
// Every call but jb_neardup_sig, which takes signatures and no text, starts with batch_args, batch_device and
// batch_front; the calls differ in the front as follows:
//
//   call                                     mode      vocabulary  ctx batch filter        other
//   jb_cut_batch_join                        caller's  no          yes
//   jb_wc_batch                              caller's  no          yes
//   jb_minhash_batch                         caller's  no          yes
//   jb_cut_batch_charspans                   caller's  no          no                      the caller's capacity
//   jb_cut_batch_filter                      caller's  no          no: the caller's rule   the rule's stop set
//   jb_colloc_batch                          plain     yes         yes
//   batch_chain: jb_keywords_batch,          plain     yes         no                      extra bytes of kArText
//     jb_df_batch, jb_textrank_batch,
//     jb_postings_batch, jb_search_batch
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "jb_device.h"  // (first: the HIP runtime, which the feature headers' host/device helpers need)

#include "jb_bm25.h"
#include "jb_charspans.h"
#include "jb_colloc.h"
#include "jb_filter.h"
#include "jb_join.h"
#include "jb_minhash.h"
#include "jb_neardup.h"
#include "jb_postings.h"
#include "jb_textrank.h"
#include "jb_wc.h"

int kw_arena(jb_ctx* ctx, KwBuf which, size_t need, Arena* a) {
    if (ctx->kw_cap[which] < need) {
        dfree(ctx->kw_buf[which]);
        ctx->kw_buf[which] = nullptr;
        ctx->kw_cap[which] = 0;
        HIPCHK(hipMalloc(&ctx->kw_buf[which], need));
        ctx->kw_cap[which] = need;
    }
    *a = Arena{};
    a->p = (uint8_t*)ctx->kw_buf[which];
    return JB_OK;
}

int batch_args(const char* who, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, uint64_t* nb) {
    for (uint32_t k = 0; k < ndocs; k++)
        if (doc_off[k] > doc_off[k + 1]) return fail(JB_EINVAL, "%s: doc_off decreases at %u", who, k);
    *nb = doc_off[ndocs] - doc_off[0];
    if (*nb && !text) return fail(JB_EINVAL, "%s: null text", who);
    if (*nb >= (1ull << 31)) return fail(JB_ELIMIT, "batch of %llu bytes (limit 2 GiB)", (unsigned long long)*nb);
    return JB_OK;
}

int batch_device(jb_ctx* ctx, const char* who, bool need_vocab, const jb_filter_rule* rule, int* ordinal) {
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    if (need_vocab && !ctx->vocab) return fail(JB_EINVAL, "%s: no vocabulary attached (jb_vocab_set)", who);
    *ordinal = ctx->devs[0]->ordinal;
    if (rule && (rule->flags & JB_FILTER_STOP) && !ctx->stopw)
        return fail(JB_EINVAL, "%s: JB_FILTER_STOP without a stop set (jb_stopwords_set)", who);
    return JB_OK;
}

int batch_filter_step(jb_ctx* ctx, const char* who, const jb_filter_rule& rule, Front* f) {
    const uint64_t tcap = std::max<uint64_t>(std::min(f->ntok, f->cap), 1);  // (kept tokens never exceed the cut's)
    if (const int r = filter_args(who, f->nb, tcap, &rule, true)) return r;  // (the stop set is jb_filter_device's check)
    const size_t nwork = jb_filter_work_bytes(tcap, f->ndocs), ndoc8 = ((size_t)f->ndocs + 1) * 8;
    Arena a;
    if (const int r = kw_arena(ctx, kArFilter, r256(nwork) + r256(2 * tcap * 4) + r256(ndoc8) + r256(64), &a)) return r;
    void* work = a.take(nwork);
    uint32_t* ose = (uint32_t*)a.take(2 * tcap * 4);
    uint64_t* otok = (uint64_t*)a.take(ndoc8);
    uint64_t* ocnt = (uint64_t*)a.take(64);  // (the count, a spare word as the cut's has, the statistics)
    if (const int r = jb_filter_device(ctx, f->dt, f->nb, f->dse, f->dse + f->cap, f->dtok, f->dcnt, tcap, f->ndocs, &rule,
                                       f->st, ose, ose + tcap, nullptr, tcap, otok, ocnt, ocnt + 2, work, nwork))
        return r;
    f->dse = ose;
    f->cap = tcap;
    f->dtok = otok;
    f->dcnt = ocnt;
    return JB_OK;
}

template <class Next>
int batch_front(jb_ctx* ctx, const char* who, int ordinal, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs,
                uint64_t nb, const FrontOpts& o, Next next) {
    HIPCHK(hipSetDevice(ordinal));
    std::vector<uint64_t> rel;
    try {
        rel.resize((size_t)ndocs + 1);
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "out of host memory for %u document offsets", ndocs);
    }
    for (uint32_t k = 0; k <= ndocs; k++) rel[k] = doc_off[k] - doc_off[0];
    std::lock_guard<std::mutex> kg(ctx->kw_mu);
    hipStream_t st = nullptr;
    auto run = [&]() -> int {
        int rc;
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        Front f;
        f.st = st;
        f.nb = nb;
        f.ndocs = ndocs;
        f.cap = std::max<uint64_t>(nb, 1);  // (plain and search mode: a batch of n bytes has at most n spans)
        const BatchLayout l = batch_layout(nb, ndocs, f.cap, o.extra);
        if ((rc = kw_arena(ctx, kArText, l.total, &f.a))) return rc;
        uint8_t* dt = f.dt = f.a.p + l.text;
        f.doff = (uint64_t*)(f.a.p + l.doff);
        f.dtok = (uint64_t*)(f.a.p + l.dtok);
        f.dcnt = (uint64_t*)(f.a.p + l.dcnt);
        f.dse = (uint32_t*)(f.a.p + l.dse);  // (starts, ends)
        f.a.off = l.extra;
        HIPCHK(hipMemsetAsync(dt + nb, 0, 64, st));
        if (nb) HIPCHK(hipMemcpyAsync(dt, text + doc_off[0], nb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(f.doff, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, st));
        f.ntok = 0;
        for (int pass = 0;; pass++) {
            if (o.mode == JB_MODE_CUT)
                rc = jb_cut_device_into(ctx, dt, nb, f.doff, ndocs, o.hmm, st, f.dse, f.dse + f.cap, f.cap, f.dtok, f.dcnt);
            else if (o.mode == JB_MODE_SEARCH)
                rc = jb_cut_device_search_into(ctx, dt, nb, f.doff, ndocs, o.hmm, st, f.dse, f.dse + f.cap, f.cap, f.dtok,
                                               f.dcnt);
            else
                rc = jb_cut_device_full_into(ctx, dt, nb, f.doff, ndocs, st, f.dse, f.dse + f.cap, f.cap, f.dtok, f.dcnt);
            if (rc) return rc;
            rc = jb_device_status(ctx, st);  // (waits; the cut's errors, JB_EPANIC included)
            HIPCHK(hipMemcpy(&f.ntok, f.dcnt, 8, hipMemcpyDeviceToHost));
            // full mode's list is longer than the arrays
            const bool longer = rc == JB_ELIMIT && o.mode == JB_MODE_FULL && f.ntok > f.cap;
            if (o.ntokens && (rc == JB_OK || longer) && f.ntok > o.out_cap) {
                // the caller's arrays are too small: say so before a regrow and a second cut
                *o.ntokens = f.ntok;
                return fail(JB_ELIMIT, "%llu tokens do not fit the %llu-token output arrays", (unsigned long long)f.ntok,
                            (unsigned long long)o.out_cap);
            }
            if (longer && pass == 0) {
                // larger arrays in the buffer sized by tokens, once more
                f.cap = f.ntok;
                Arena b;
                if ((rc = kw_arena(ctx, kArTokens, r256(2 * f.cap * 4), &b))) return rc;
                f.dse = (uint32_t*)b.take(2 * f.cap * 4);
                continue;
            }
            if (rc) return rc;
            break;
        }
        const jb_filter_rule* rule = o.rule ? o.rule : (o.ctx_filter && ctx->bfilter_on) ? &ctx->bfilter : nullptr;
        if (rule && (rc = batch_filter_step(ctx, who, *rule, &f))) return rc;
        f.tcap = std::max<uint64_t>(std::min(f.ntok, f.cap), 1);
        if ((rc = next(f))) return rc;
        HIPCHK(hipStreamSynchronize(st));
        return JB_OK;
    };
    const int rc = run();
    if (st) {
        (void)hipStreamSynchronize(st);  // (copies from and to the caller's memory may be in flight)
        (void)hipStreamDestroy(st);
    }
    return rc;
}

template <class Last>
int batch_chain(jb_ctx* ctx, const char* who, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                size_t extra0, Last last) {
    uint64_t nb;
    int ordinal;
    if (const int rc = batch_args(who, text, doc_off, ndocs, &nb)) return rc;
    if (const int rc = batch_device(ctx, who, true, nullptr, &ordinal)) return rc;
    if (ndocs == 0) return JB_OK;
    const FrontOpts o{JB_MODE_CUT, hmm, false, nullptr, batch_chain_extra(ndocs, extra0)};
    return batch_front(ctx, who, ordinal, text, doc_off, ndocs, nb, o, [&](Front& f) -> int {
        int rc;
        uint64_t* dtoff = (uint64_t*)f.a.take(((size_t)ndocs + 1) * 8);
        // the token count sizes the rest: 28 bytes per token instead of per byte of text (plain mode never
        // regrows, so kArTokens is the chain's alone in this call)
        const uint64_t tcap = f.tcap;
        const size_t nwork = terms_work_bytes(tcap, ndocs);
        Arena b;
        if ((rc = kw_arena(ctx, kArTokens, r256(tcap * 4) + r256(2 * tcap * 4) + r256(nwork), &b))) return rc;
        uint32_t* did = (uint32_t*)b.take(tcap * 4);
        uint32_t* dterm = (uint32_t*)b.take(2 * tcap * 4);  // (term ids, term counts)
        void* dwork = b.take(nwork);
        if ((rc = jb_ids_device(ctx, f.dt, nb, f.dse, f.dse + f.cap, f.dcnt, tcap, f.st, did))) return rc;
        if ((rc = jb_terms_device(ctx, did, tcap, f.dtok, f.dcnt, ndocs, f.st, dterm, dterm + tcap, tcap, dtoff, f.dcnt + 1,
                                  dwork, nwork)))
            return rc;
        return last(BatchCsr{f.st, dterm, dterm + tcap, dtoff, f.dcnt + 1, tcap, did, f.dtok, f.dcnt}, &f.a);
    });
}

namespace {
int batch_mode(const char* who, int mode) {
    if (mode != JB_MODE_CUT && mode != JB_MODE_SEARCH && mode != JB_MODE_FULL)
        return fail(JB_EINVAL, "%s: mode %d (JB_MODE_CUT, JB_MODE_SEARCH or JB_MODE_FULL)", who, mode);
    return JB_OK;
}
}  // namespace

extern "C" int jb_batch_filter_set(jb_ctx* ctx, const jb_filter_rule* rule) {
    const char* who = "jb_batch_filter_set";
    if (!ctx) return fail(JB_EINVAL, "%s: null ctx", who);
    if (rule)  // (a stop set is asked for when a batch call runs the rule)
        if (const int rc = filter_args(who, 0, 0, rule, true)) return rc;
    std::lock_guard<std::mutex> kg(ctx->kw_mu);
    ctx->bfilter_on = rule != nullptr;
    ctx->bfilter = rule ? *rule : jb_filter_rule{0, 0, 0, 0};
    return JB_OK;
}

// Host text in, keywords out: batch_chain, then jb_keywords_device and the records' way back.
extern "C" int jb_keywords_batch(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                                 const float* weights, uint32_t nweights, uint32_t topk, uint32_t* kw_id,
                                 float* kw_score, uint32_t* kw_cnt, uint32_t* kw_n) {
    // (the limits of topk come first: they need no ctx)
    if (topk == 0) return fail(JB_EINVAL, "jb_keywords_batch: topk is 0");
    if (topk > kKwMaxK) return fail(JB_ELIMIT, "jb_keywords_batch: topk %u (limit JB_KW_MAXK = %u)", topk, kKwMaxK);
    if (!ctx || !doc_off || (nweights && !weights) || (ndocs && (!kw_id || !kw_score || !kw_cnt || !kw_n)))
        return fail(JB_EINVAL, "jb_keywords_batch: null argument");
    const size_t nrec = (size_t)ndocs * topk;
    const size_t extra = r256((3 * nrec + ndocs) * 4) + r256(std::max<size_t>(nweights, 1) * 4);
    return batch_chain(ctx, "jb_keywords_batch", text, doc_off, ndocs, hmm, extra, [&](const BatchCsr& c, Arena* a) -> int {
        uint32_t* dkw = (uint32_t*)a->take((3 * nrec + ndocs) * 4);  // (ids, scores, counts, kw_n)
        float* dw = (float*)a->take(std::max<size_t>(nweights, 1) * 4);
        if (nweights) HIPCHK(hipMemcpyAsync(dw, weights, (size_t)nweights * 4, hipMemcpyHostToDevice, c.st));
        if (const int rc = jb_keywords_device(ctx, c.term_id, c.term_cnt, c.term_off, ndocs, c.tcap, dw, nweights, topk,
                                              c.st, dkw, (float*)(dkw + nrec), dkw + 2 * nrec, dkw + 3 * nrec))
            return rc;
        HIPCHK(hipMemcpyAsync(kw_id, dkw, nrec * 4, hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipMemcpyAsync(kw_score, dkw + nrec, nrec * 4, hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipMemcpyAsync(kw_cnt, dkw + 2 * nrec, nrec * 4, hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipMemcpyAsync(kw_n, dkw + 3 * nrec, (size_t)ndocs * 4, hipMemcpyDeviceToHost, c.st));
        return JB_OK;
    });
}

// Host text in, the batch's document frequencies added to df: batch_chain, then jb_df_device into kArDf and ndf
// counters back.
extern "C" int jb_df_batch(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                           uint32_t* df, uint32_t ndf) {
    if (!ctx) return fail(JB_EINVAL, "jb_df_batch: null ctx");
    if (!doc_off) return fail(JB_EINVAL, "jb_df_batch: null doc_off");
    if (ndf && !df) return fail(JB_EINVAL, "jb_df_batch: null df");
    std::vector<uint32_t> got;
    try {
        got.resize(ndf);
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "out of host memory for %u counters", ndf);
    }
    bool ran = false;
    const int rc = batch_chain(ctx, "jb_df_batch", text, doc_off, ndocs, hmm, 0, [&](const BatchCsr& c, Arena*) -> int {
        if (ndf == 0) return JB_OK;
        Arena b;
        if (const int r = kw_arena(ctx, kArDf, (size_t)ndf * 4, &b)) return r;
        uint32_t* ddf = (uint32_t*)b.p;
        HIPCHK(hipMemsetAsync(ddf, 0, (size_t)ndf * 4, c.st));
        if (const int r = jb_df_device(ctx, c.term_id, c.nterms, c.tcap, ddf, ndf, c.st)) return r;
        HIPCHK(hipMemcpyAsync(got.data(), ddf, (size_t)ndf * 4, hipMemcpyDeviceToHost, c.st));
        ran = true;
        return JB_OK;
    });
    if (rc == JB_OK && ran)
        for (uint32_t k = 0; k < ndf; k++) df[k] += got[k];
    return rc;
}

// Host text in, TextRank keywords out: batch_chain, then jb_textrank_device with the keep mask, the records and
// the work buffer in kArTextrank, and the records' way back.
extern "C" int jb_textrank_batch(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                                 const uint8_t* keep, uint32_t nkeep, uint32_t span, uint32_t iters, uint32_t topk,
                                 uint32_t* kw_id, float* kw_score, uint32_t* kw_n) {
    if (const int rc = textrank_args("jb_textrank_batch", 0, 0, span, iters, topk)) return rc;
    if (!ctx || !doc_off || (nkeep && !keep) || (ndocs && (!kw_id || !kw_score || !kw_n)))
        return fail(JB_EINVAL, "jb_textrank_batch: null argument");
    const size_t nrec = (size_t)ndocs * topk;
    return batch_chain(ctx, "jb_textrank_batch", text, doc_off, ndocs, hmm, 0, [&](const BatchCsr& c, Arena*) -> int {
        const size_t nwork = textrank_work_bytes(c.tcap, c.tcap, ndocs);
        Arena b;
        if (const int r = kw_arena(ctx, kArTextrank,
                                   r256(std::max<size_t>(nkeep, 1)) + r256((2 * nrec + ndocs) * 4) + r256(nwork), &b))
            return r;
        uint8_t* dkeep = (uint8_t*)b.take(std::max<size_t>(nkeep, 1));
        uint32_t* dkw = (uint32_t*)b.take((2 * nrec + ndocs) * 4);  // (ids, scores, kw_n)
        void* dwork = b.take(nwork);
        if (nkeep) HIPCHK(hipMemcpyAsync(dkeep, keep, nkeep, hipMemcpyHostToDevice, c.st));
        if (const int r = jb_textrank_device(ctx, c.ids, c.tcap, c.doc_tok, c.ntok, ndocs, c.term_id, c.term_off, c.tcap,
                                             dkeep, nkeep, span, iters, topk, c.st, dkw, (float*)(dkw + nrec),
                                             dkw + 2 * nrec, dwork, nwork))
            return r;
        HIPCHK(hipMemcpyAsync(kw_id, dkw, nrec * 4, hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipMemcpyAsync(kw_score, dkw + nrec, nrec * 4, hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipMemcpyAsync(kw_n, dkw + 2 * nrec, (size_t)ndocs * 4, hipMemcpyDeviceToHost, c.st));
        return JB_OK;
    });
}

// jb_joined::text is page-locked, so that the copy back runs at the link's rate and touches no fresh page.
// Pinning a gigabyte costs far more than the whole call, so jb_joined_free keeps the largest block it was
// handed (one per process) and the next jb_cut_batch_join takes it; jb_close lets it go.  A block starts
// with a header that holds its capacity.
namespace {
constexpr size_t kJoinedHdr = 64;
std::mutex g_joined_mu;
uint8_t* g_joined_block = nullptr;  // (under g_joined_mu)
size_t g_joined_cap = 0;

int joined_alloc(uint64_t nbytes, uint8_t** text) {
    uint8_t* b = nullptr;
    {
        std::lock_guard<std::mutex> g(g_joined_mu);
        if (g_joined_block && g_joined_cap >= nbytes) {
            b = g_joined_block;
            g_joined_block = nullptr;
        }
    }
    if (!b) {
        HIPCHK(hipHostMalloc(&b, kJoinedHdr + std::max<uint64_t>(nbytes, 1), hipHostMallocDefault));
        *(uint64_t*)b = nbytes;
    }
    *text = b + kJoinedHdr;
    return JB_OK;
}

void joined_release(uint8_t* text) {
    if (!text) return;
    uint8_t* b = text - kJoinedHdr;
    {
        std::lock_guard<std::mutex> g(g_joined_mu);
        if (!g_joined_block || g_joined_cap < *(uint64_t*)b) {
            std::swap(b, g_joined_block);
            g_joined_cap = *(uint64_t*)g_joined_block;
        }
    }
    hfree(b);  // (the smaller of the two, or nothing)
}
}  // namespace

void joined_drop_cache() {
    uint8_t* b;
    {
        std::lock_guard<std::mutex> g(g_joined_mu);
        b = g_joined_block;
        g_joined_block = nullptr;
        g_joined_cap = 0;
    }
    hfree(b);
}

extern "C" void jb_joined_free(jb_joined* j) {
    if (!j) return;
    joined_release(j->text);
    free(j->doc_off);
    memset(j, 0, sizeof *j);
}

// Host text in, joined text out: the front, jb_join_device into kArJoinOut with its work buffer and offsets in
// kArJoinWork, and nout, the offsets and the nout bytes back.  The join runs again when its output was larger
// than kArJoinOut had room for.
extern "C" int jb_cut_batch_join(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                                 int mode, const uint8_t* sep, uint32_t seplen, const uint8_t* term, uint32_t termlen,
                                 jb_joined* out) {
    const char* who = "jb_cut_batch_join";
    if (!ctx || !doc_off || !out) return fail(JB_EINVAL, "%s: null argument", who);
    memset(out, 0, sizeof *out);
    if (const int rc = batch_mode(who, mode)) return rc;
    uint64_t nb;
    int ordinal;
    if (const int rc = batch_args(who, text, doc_off, ndocs, &nb)) return rc;
    if (const int rc = join_args(who, nb, 0, sep, seplen, term, termlen)) return rc;
    if (const int rc = batch_device(ctx, who, false, nullptr, &ordinal)) return rc;
    out->doc_off = (uint64_t*)calloc((size_t)ndocs + 1, 8);
    if (!out->doc_off) return fail(JB_ENOMEM, "out of host memory for %u document offsets", ndocs);
    out->ndocs = ndocs;
    if (ndocs == 0) return JB_OK;
    const int rc = batch_front(ctx, who, ordinal, text, doc_off, ndocs, nb, {mode, hmm, true}, [&](Front& f) -> int {
        int rc;
        if (const int r = join_args(who, nb, f.cap, sep, seplen, term, termlen)) return r;
        const size_t nwork = join_work_bytes(f.cap, ndocs), ndoc8 = ((size_t)ndocs + 1) * 8;
        Arena w;
        if ((rc = kw_arena(ctx, kArJoinWork, r256(nwork) + r256(ndoc8), &w))) return rc;
        void* dwork = w.take(nwork);
        uint64_t* dooff = (uint64_t*)w.take(ndoc8);
        // a first guess at the output's size: the text (plain mode without replaced bytes gives less), a
        // separator per token and a terminator per document
        uint64_t ocap = std::max<uint64_t>(ctx->kw_cap[kArJoinOut],
                                           nb + std::min(f.ntok, f.cap) * seplen + (uint64_t)ndocs * termlen + 256);
        uint64_t nout = 0;
        for (int pass = 0; pass < 2; pass++) {
            Arena a;
            if ((rc = kw_arena(ctx, kArJoinOut, ocap, &a))) return rc;
            if ((rc = jb_join_device(ctx, f.dt, nb, f.dse, f.dse + f.cap, f.dtok, f.dcnt, f.cap, ndocs, sep, seplen, term,
                                     termlen, f.st, a.p, ocap, dooff, f.dcnt + 1, dwork, nwork)))
                return rc;
            HIPCHK(hipMemcpyAsync(&nout, f.dcnt + 1, 8, hipMemcpyDeviceToHost, f.st));
            HIPCHK(hipStreamSynchronize(f.st));
            if (nout <= ocap) break;
            ocap = nout;  // (replaced bytes or overlapping spans: the complete size is known now)
        }
        if ((rc = joined_alloc(nout, &out->text))) return rc;
        out->nbytes = nout;
        if (nout) HIPCHK(hipMemcpyAsync(out->text, ctx->kw_buf[kArJoinOut], nout, hipMemcpyDeviceToHost, f.st));
        HIPCHK(hipMemcpyAsync(out->doc_off, dooff, ndoc8, hipMemcpyDeviceToHost, f.st));
        return JB_OK;
    });
    if (rc) jb_joined_free(out);
    return rc;
}

// Host text in, character spans out: the front, jb_charspans_device in place on the span arrays with its work
// buffer and doc_units in kArCharspans, and the count, the converted spans, doc_tok and doc_units back.
extern "C" int jb_cut_batch_charspans(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                                      int mode, int unit, uint32_t* cstart, uint32_t* cend, uint64_t cap,
                                      uint64_t* doc_tok, uint64_t* ntokens, uint32_t* doc_units) {
    const char* who = "jb_cut_batch_charspans";
    if (!ctx || !doc_off || !doc_tok || !ntokens || (cap && (!cstart || !cend)) || (ndocs && !doc_units))
        return fail(JB_EINVAL, "%s: null argument", who);
    *ntokens = 0;
    if (const int rc = batch_mode(who, mode)) return rc;
    uint64_t nb;
    int ordinal;
    if (const int rc = batch_args(who, text, doc_off, ndocs, &nb)) return rc;
    if (const int rc = charspans_args(who, nb, 0, unit)) return rc;
    if (ndocs == 0) {
        doc_tok[0] = 0;
        return JB_OK;
    }
    if (const int rc = batch_device(ctx, who, false, nullptr, &ordinal)) return rc;
    const FrontOpts o{mode, hmm, false, nullptr, 0, ntokens, cap};
    return batch_front(ctx, who, ordinal, text, doc_off, ndocs, nb, o, [&](Front& f) -> int {
        *ntokens = f.ntok;
        if (const int r = charspans_args(who, nb, f.cap, unit)) return r;
        const size_t nwork = charspans_work_bytes(nb, ndocs);
        Arena w;
        if (const int r = kw_arena(ctx, kArCharspans, r256(nwork) + r256((size_t)ndocs * 4), &w)) return r;
        void* dwork = w.take(nwork);
        uint32_t* dunits = (uint32_t*)w.take((size_t)ndocs * 4);
        if (const int r = jb_charspans_device(ctx, f.dt, nb, f.doff, ndocs, f.dse, f.dse + f.cap, f.dtok, f.dcnt, f.cap, unit,
                                              f.st, f.dse, f.dse + f.cap, dunits, dwork, nwork))
            return r;
        if (f.ntok) {
            HIPCHK(hipMemcpyAsync(cstart, f.dse, f.ntok * 4, hipMemcpyDeviceToHost, f.st));
            HIPCHK(hipMemcpyAsync(cend, f.dse + f.cap, f.ntok * 4, hipMemcpyDeviceToHost, f.st));
        }
        HIPCHK(hipMemcpyAsync(doc_tok, f.dtok, ((size_t)ndocs + 1) * 8, hipMemcpyDeviceToHost, f.st));
        HIPCHK(hipMemcpyAsync(doc_units, dunits, (size_t)ndocs * 4, hipMemcpyDeviceToHost, f.st));
        return JB_OK;
    });
}

// Host text in, the batch's tokens into the table: the front, then jb_wc_add_device with its work buffer in kArWc.
extern "C" int jb_wc_batch(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm, int mode,
                           void* d_table, size_t ntable) {
    const char* who = "jb_wc_batch";
    if (!ctx || !doc_off) return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = batch_mode(who, mode)) return rc;
    if (const int rc = wc_table_args(who, d_table, ntable)) return rc;
    uint64_t nb;
    int ordinal;
    if (const int rc = batch_args(who, text, doc_off, ndocs, &nb)) return rc;
    if (const int rc = batch_device(ctx, who, false, nullptr, &ordinal)) return rc;
    if (ndocs == 0) return JB_OK;
    return batch_front(ctx, who, ordinal, text, doc_off, ndocs, nb, {mode, hmm, true}, [&](Front& f) -> int {
        const size_t nwork = jb_wc_work_bytes(f.tcap);
        Arena w;
        if (const int r = kw_arena(ctx, kArWc, nwork, &w)) return r;
        return jb_wc_add_device(ctx, d_table, ntable, f.dt, nb, f.dse, f.dse + f.cap, f.dcnt, f.tcap, f.st, w.p, nwork);
    });
}

// Host text in, signatures out: the front, then jb_minhash_device with its work buffer, sig and doc_n in
// kArMinhash; only sig and doc_n come back.
extern "C" int jb_minhash_batch(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                                int mode, uint32_t n, uint32_t K, uint64_t seed, uint32_t* sig, uint32_t* doc_n) {
    const char* who = "jb_minhash_batch";
    if (!ctx || !doc_off || (ndocs && (!sig || !doc_n))) return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = batch_mode(who, mode)) return rc;
    if (const int rc = minhash_args(who, 0, 0, n, K)) return rc;
    uint64_t nb;
    int ordinal;
    if (const int rc = batch_args(who, text, doc_off, ndocs, &nb)) return rc;
    if (const int rc = batch_device(ctx, who, false, nullptr, &ordinal)) return rc;
    if (ndocs == 0) return JB_OK;
    return batch_front(ctx, who, ordinal, text, doc_off, ndocs, nb, {mode, hmm, true}, [&](Front& f) -> int {
        if (const int r = minhash_args(who, nb, f.tcap, n, K)) return r;
        const size_t nwork = jb_minhash_work_bytes(f.tcap, ndocs), nsig = (size_t)ndocs * K * 4, ndn = (size_t)ndocs * 4;
        Arena w;
        if (const int r = kw_arena(ctx, kArMinhash, r256(nwork) + r256(nsig) + r256(ndn), &w)) return r;
        void* dwork = w.take(nwork);
        uint32_t* dsig = (uint32_t*)w.take(nsig);
        uint32_t* ddn = (uint32_t*)w.take(ndn);
        if (const int r = jb_minhash_device(ctx, f.dt, nb, f.dse, f.dse + f.cap, f.dtok, f.dcnt, f.tcap, ndocs, n, K, seed, f.st,
                                            dsig, ddn, dwork, nwork))
            return r;
        HIPCHK(hipMemcpyAsync(sig, dsig, nsig, hipMemcpyDeviceToHost, f.st));
        HIPCHK(hipMemcpyAsync(doc_n, ddn, ndn, hipMemcpyDeviceToHost, f.st));
        return JB_OK;
    });
}

// Host text in, the filtered spans out: the front with the caller's rule, and the count, the statistics and, when
// the count fits the caller's arrays, the spans and doc_tok back.
extern "C" int jb_cut_batch_filter(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                                   int mode, const jb_filter_rule* rule, uint32_t* start, uint32_t* end, uint64_t cap,
                                   uint64_t* doc_tok, uint64_t* ntokens, uint64_t* stats) {
    const char* who = "jb_cut_batch_filter";
    if (!ctx || !doc_off || !doc_tok || !ntokens || (cap && (!start || !end))) return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = batch_mode(who, mode)) return rc;
    if (const int rc = filter_args(who, 0, 0, rule, true)) return rc;
    uint64_t nb;
    int ordinal;
    if (const int rc = batch_args(who, text, doc_off, ndocs, &nb)) return rc;
    if (const int rc = batch_device(ctx, who, false, rule, &ordinal)) return rc;
    *ntokens = 0;
    if (stats) memset(stats, 0, 40);
    if (ndocs == 0) {
        doc_tok[0] = 0;
        return JB_OK;
    }
    return batch_front(ctx, who, ordinal, text, doc_off, ndocs, nb, {mode, hmm, false, rule}, [&](Front& f) -> int {
        uint64_t head[7];  // (the count, a spare word, the statistics)
        HIPCHK(hipMemcpyAsync(head, f.dcnt, sizeof head, hipMemcpyDeviceToHost, f.st));
        HIPCHK(hipStreamSynchronize(f.st));
        *ntokens = head[0];
        if (stats) memcpy(stats, head + 2, 40);
        if (head[0] > cap)
            return fail(JB_ELIMIT, "%s: %llu tokens, the arrays hold %llu", who, (unsigned long long)head[0],
                        (unsigned long long)cap);
        if (head[0]) {
            HIPCHK(hipMemcpyAsync(start, f.dse, head[0] * 4, hipMemcpyDeviceToHost, f.st));
            HIPCHK(hipMemcpyAsync(end, f.dse + f.cap, head[0] * 4, hipMemcpyDeviceToHost, f.st));
        }
        HIPCHK(hipMemcpyAsync(doc_tok, f.dtok, ((size_t)ndocs + 1) * 8, hipMemcpyDeviceToHost, f.st));
        return JB_OK;
    });
}

// Host text in, the batch's postings out: batch_chain, then jb_postings_device with its work buffer and its
// outputs in kArPostings; post_off and the count come back first, the lists when they fit pcap.
extern "C" int jb_postings_batch(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                                 uint32_t doc_base, uint64_t pcap, uint64_t* post_off, uint32_t nids,
                                 uint32_t* post_doc, uint32_t* post_tf, uint64_t* nposts, uint32_t* doc_len) {
    const char* who = "jb_postings_batch";
    if (!ctx || !doc_off || !post_off || !nposts || (pcap && (!post_doc || !post_tf)))
        return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = postings_args(who, 0, ndocs, doc_base)) return rc;
    bool ran = false;
    const int rc = batch_chain(ctx, who, text, doc_off, ndocs, hmm, 0, [&](const BatchCsr& c, Arena*) -> int {
        const size_t nwork = jb_postings_work_bytes(c.tcap, nids, ndocs), noff = ((size_t)nids + 1) * 8;
        Arena b;
        if (const int r = kw_arena(ctx, kArPostings, r256(nwork) + r256(2 * c.tcap * 4) + r256(noff) + r256(8), &b)) return r;
        void* work = b.take(nwork);
        uint32_t* dpost = (uint32_t*)b.take(2 * c.tcap * 4);  // (documents, term frequencies)
        uint64_t* dpoff = (uint64_t*)b.take(noff);
        uint64_t* dn = (uint64_t*)b.take(8);
        if (const int r = jb_postings_device(ctx, c.term_id, c.term_cnt, c.term_off, c.nterms, c.tcap, ndocs, nids,
                                             doc_base, c.st, dpost, dpost + c.tcap, c.tcap, dpoff, dn, work, nwork))
            return r;
        std::vector<uint64_t> dtok;
        if (doc_len) {
            try {
                dtok.resize((size_t)ndocs + 1);
            } catch (const std::bad_alloc&) {
                return fail(JB_ENOMEM, "out of host memory for %u document offsets", ndocs);
            }
            HIPCHK(hipMemcpyAsync(dtok.data(), c.doc_tok, dtok.size() * 8, hipMemcpyDeviceToHost, c.st));
        }
        HIPCHK(hipMemcpyAsync(post_off, dpoff, noff, hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipMemcpyAsync(nposts, dn, 8, hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipStreamSynchronize(c.st));
        ran = true;
        if (*nposts > pcap)
            return fail(JB_ELIMIT, "%s: %llu postings, the arrays hold %llu", who, (unsigned long long)*nposts,
                        (unsigned long long)pcap);
        if (doc_len)
            for (uint32_t k = 0; k < ndocs; k++) doc_len[k] = (uint32_t)(dtok[k + 1] - dtok[k]);
        if (*nposts) {
            HIPCHK(hipMemcpyAsync(post_doc, dpost, *nposts * 4, hipMemcpyDeviceToHost, c.st));
            HIPCHK(hipMemcpyAsync(post_tf, dpost + c.tcap, *nposts * 4, hipMemcpyDeviceToHost, c.st));
        }
        return JB_OK;
    });
    if (rc == JB_OK && !ran) {  // (no document: the empty index)
        for (uint64_t t = 0; t <= nids; t++) post_off[t] = 0;
        *nposts = 0;
    }
    return rc;
}

// Host text in, the batch's pairs and unigrams into the table and d_uni: the front in plain mode, then
// jb_ids_device and jb_colloc_add_device with the ids, the keep mask and the work buffer in kArColloc.
extern "C" int jb_colloc_batch(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                               const uint8_t* keep, uint32_t nkeep, uint32_t flags, void* d_table, size_t ntable,
                               uint64_t* d_uni, uint32_t nuni) {
    const char* who = "jb_colloc_batch";
    if (!ctx || !doc_off || (nkeep && !keep)) return fail(JB_EINVAL, "%s: null argument", who);
    if (flags & ~JB_COLLOC_CONTIG) return fail(JB_EINVAL, "%s: flags %#x (JB_COLLOC_CONTIG)", who, flags);
    if (const int rc = colloc_table_args(who, d_table, ntable, d_uni, nuni)) return rc;
    uint64_t nb;
    int ordinal;
    if (const int rc = batch_args(who, text, doc_off, ndocs, &nb)) return rc;
    if (const int rc = batch_device(ctx, who, true, nullptr, &ordinal)) return rc;
    if (ndocs == 0) return JB_OK;
    return batch_front(ctx, who, ordinal, text, doc_off, ndocs, nb, {JB_MODE_CUT, hmm, true}, [&](Front& f) -> int {
        const size_t nwork = jb_colloc_work_bytes(f.tcap, ndocs);
        Arena b;
        if (const int r = kw_arena(ctx, kArColloc, r256(f.tcap * 4) + r256(std::max<size_t>(nkeep, 1)) + r256(nwork), &b))
            return r;
        uint32_t* did = (uint32_t*)b.take(f.tcap * 4);
        uint8_t* dkeep = (uint8_t*)b.take(std::max<size_t>(nkeep, 1));
        void* dwork = b.take(nwork);
        if (nkeep) HIPCHK(hipMemcpyAsync(dkeep, keep, nkeep, hipMemcpyHostToDevice, f.st));
        if (const int r = jb_ids_device(ctx, f.dt, nb, f.dse, f.dse + f.cap, f.dcnt, f.tcap, f.st, did)) return r;
        return jb_colloc_add_device(ctx, d_table, ntable, d_uni, nuni, did, f.tcap, f.dtok, f.dcnt, ndocs, dkeep, nkeep, flags,
                                    f.dse, f.dse + f.cap, f.st, dwork, nwork);
    });
}

// Host signatures in, the pairs out: the upload, jb_minhash_bands_device and jb_neardup_device with every device
// array in kArNeardup; pair_off, the count and the counters come back first, the pairs when they fit pcap.
extern "C" int jb_neardup_sig(jb_ctx* ctx, const uint32_t* sig, const uint32_t* doc_n, uint32_t ndocs, uint32_t K,
                              uint32_t B, uint32_t R, uint32_t W, uint32_t min_agree, uint32_t* pair_doc,
                              uint32_t* pair_agree, uint64_t pcap, uint64_t* pair_off, uint64_t* npairs, uint64_t* stat) {
    const char* who = "jb_neardup_sig";
    if (const int rc = minhash_band_args(who, K, B, R)) return rc;
    if (const int rc = neardup_args(who, ndocs, B, K, W, min_agree)) return rc;
    if (!ctx || !pair_off || !npairs || !stat || (ndocs && (!sig || !doc_n)) || (pcap && (!pair_doc || !pair_agree)))
        return fail(JB_EINVAL, "%s: null argument", who);
    if (ndocs == 0) {
        pair_off[0] = 0;
        *npairs = 0;
        for (uint32_t k = 0; k < JB_ND_NSTAT; k++) stat[k] = 0;
        return JB_OK;
    }
    int ordinal;
    {
        std::shared_lock<std::shared_mutex> rl(ctx->lock);
        ordinal = ctx->devs[0]->ordinal;
    }
    HIPCHK(hipSetDevice(ordinal));
    std::lock_guard<std::mutex> kg(ctx->kw_mu);
    hipStream_t st = nullptr;
    auto run = [&]() -> int {
        int rc;
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        const size_t nsig = (size_t)ndocs * K * 4, ndn = (size_t)ndocs * 4, nkey = (size_t)ndocs * B * 8,
                     nwork = jb_neardup_work_bytes(ndocs, B), noff = ((size_t)ndocs + 1) * 8;
        Arena a;
        if ((rc = kw_arena(ctx, kArNeardup, r256(nsig) + r256(ndn) + r256(nkey) + r256(nwork) + 2 * r256(pcap * 4) +
                                                r256(noff) + r256(8) + r256(JB_ND_NSTAT * 8), &a)))
            return rc;
        uint32_t* dsig = (uint32_t*)a.take(nsig);
        uint32_t* ddn = (uint32_t*)a.take(ndn);
        uint64_t* dkey = (uint64_t*)a.take(nkey);
        void* work = a.take(nwork);
        uint32_t* dpd = (uint32_t*)a.take(pcap * 4);
        uint32_t* dpa = (uint32_t*)a.take(pcap * 4);
        uint64_t* dpoff = (uint64_t*)a.take(noff);
        uint64_t* dn = (uint64_t*)a.take(8);
        uint64_t* dstat = (uint64_t*)a.take(JB_ND_NSTAT * 8);
        HIPCHK(hipMemcpyAsync(dsig, sig, nsig, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ddn, doc_n, ndn, hipMemcpyHostToDevice, st));
        if ((rc = jb_minhash_bands_device(ctx, dsig, ddn, ndocs, K, B, R, st, dkey))) return rc;
        if ((rc = jb_neardup_device(ctx, dkey, dsig, ndocs, B, K, W, min_agree, pcap ? dpd : nullptr, pcap ? dpa : nullptr,
                                    pcap, dpoff, dn, dstat, work, nwork, st)))
            return rc;
        HIPCHK(hipMemcpyAsync(pair_off, dpoff, noff, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(npairs, dn, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(stat, dstat, JB_ND_NSTAT * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (*npairs > pcap)
            return fail(JB_ELIMIT, "%s: %llu pairs, the arrays hold %llu", who, (unsigned long long)*npairs,
                        (unsigned long long)pcap);
        if (*npairs) {
            HIPCHK(hipMemcpyAsync(pair_doc, dpd, *npairs * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(pair_agree, dpa, *npairs * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        return JB_OK;
    };
    const int rc = run();
    if (st) {
        (void)hipStreamSynchronize(st);  // (a copy from or to the caller's memory may be in flight)
        (void)hipStreamDestroy(st);
    }
    return rc;
}

// Host query text in, the best documents out: batch_chain (its token ids in token order and its token offsets
// are the queries' CSR), then the search with its work buffer and its records in kArSearch.
extern "C" int jb_search_batch(jb_ctx* ctx, const uint8_t* qtext, const uint64_t* q_off, uint32_t nq, int hmm,
                               uint32_t topk, uint32_t* res_doc, uint64_t* res_score, uint32_t* res_n) {
    const char* who = "jb_search_batch";
    if (const int rc = bm25_topk(who, topk)) return rc;
    if (!ctx || !q_off || (nq && (!res_doc || !res_score || !res_n))) return fail(JB_EINVAL, "%s: null argument", who);
    {
        std::shared_lock<std::shared_mutex> rl(ctx->lock);
        if (!ctx->vocab) return fail(JB_EINVAL, "%s: no vocabulary attached (jb_vocab_set)", who);
        if (!ctx->index.base) return fail(JB_EINVAL, "%s: no index attached (jb_index_set)", who);
        if (ctx->index.nids != ctx->vocab->nkeys)
            return fail(JB_EINVAL, "%s: the index has %u ids, the vocabulary %u keys", who, ctx->index.nids,
                        (uint32_t)ctx->vocab->nkeys);
    }
    const size_t nrec = (size_t)nq * topk;
    return batch_chain(ctx, who, qtext, q_off, nq, hmm, 0, [&](const BatchCsr& c, Arena*) -> int {
        // (the lock keeps the index while the search is queued; a jb_index_set that follows waits for the device)
        std::shared_lock<std::shared_mutex> rl(ctx->lock);
        const jb_ctx::Index& ix = ctx->index;
        if (!ix.base || !ctx->vocab || ix.nids != ctx->vocab->nkeys)
            return fail(JB_EINVAL, "%s: the index was replaced during the call", who);
        const Bm25Work w = bm25_layout(nq, ix.ndocs, topk);
        const size_t nwork = ctx->devs[0]->lc.bm25_form ? w.bytes1 : w.bytes;
        if (nwork == SIZE_MAX) return fail(JB_ELIMIT, "%s: %u queries over %u documents", who, nq, ix.ndocs);
        Arena b;
        if (const int r = kw_arena(ctx, kArSearch, r256(nwork) + r256(nrec * 8) + r256(nrec * 4) + r256((size_t)nq * 4), &b))
            return r;
        void* work = b.take(nwork);
        uint64_t* dscore = (uint64_t*)b.take(nrec * 8);
        uint32_t* ddoc = (uint32_t*)b.take(nrec * 4);
        uint32_t* dn = (uint32_t*)b.take((size_t)nq * 4);
        if (const int r = bm25_queue(ctx, ix.post_doc, ix.post_tf, ix.post_off, ix.npost, ix.nids, ix.norm, ix.ndocs,
                                     ix.weight, ix.nids, ix.k1, c.ids, c.tcap, c.doc_tok, nq, topk, c.st, ddoc, dscore, dn,
                                     work))
            return r;
        HIPCHK(hipMemcpyAsync(res_doc, ddoc, nrec * 4, hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipMemcpyAsync(res_score, dscore, nrec * 8, hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipMemcpyAsync(res_n, dn, (size_t)nq * 4, hipMemcpyDeviceToHost, c.st));
        return JB_OK;
    });
}
