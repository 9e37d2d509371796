// jb_batch.h — the host-text analytics calls (jb_batch.cpp): the ctx's grow-only device buffers, the layout of
// the one every call starts in, and the front they share.  Library-internal.  The first part needs no HIP and
// no ctx (tests/host/batch_layout_check.cpp takes it alone, with JB_BATCH_LAYOUT_ONLY defined).
#pragma once
#include <stddef.h>
#include <stdint.h>

#pragma GCC visibility push(hidden)

// A part of one device allocation, cut into 256-byte aligned pieces.
struct Arena {
    uint8_t* p = nullptr;
    size_t off = 0;
    void* take(size_t nbytes) {
        void* r = p + off;
        off += (nbytes + 255u) & ~(size_t)255u;
        return r;
    }
};
inline size_t r256(size_t x) { return (x + 255u) & ~(size_t)255u; }

// jb_ctx::kw_buf: the host-text calls' device buffers on the first device, kept for the next call.  They only
// grow, and a call cuts them up anew (kw_arena); calls take kw_mu in turn.
enum KwBuf {
    kArText,       // batch_front: the text, the document offsets, doc_tok, the counts and the span arrays, then the
                   // caller's extra bytes (batch_chain's term offsets, jb_keywords_batch's records and weights)
    kArTokens,     // sized by the token count: batch_front's span arrays when full mode's list is longer than the
                   // text has bytes, or batch_chain's ids, terms and work buffer.  The chain cuts in plain mode only,
                   // where the list never outgrows the text, so the two uses never meet in one call.
    kArDf,         // jb_df_batch's ndf counters
    kArTextrank,   // jb_textrank_batch's keep mask, records and work buffer
    kArJoinOut,    // jb_cut_batch_join's output
    kArJoinWork,   // its work buffer and output offsets
    kArCharspans,  // jb_cut_batch_charspans' work buffer and doc_units
    kArWc,         // jb_wc_batch's work buffer
    kArMinhash,    // jb_minhash_batch's work buffer, signatures and shingle counts
    kArFilter,     // batch_filter_step's work buffer and filtered span list
    kArPostings,   // jb_postings_batch's work buffer and postings
    kArSearch,     // jb_search_batch's work buffer and records
    kArNeardup,    // jb_neardup_sig's signatures, keys, work buffer and pairs
    kArColloc,     // jb_colloc_batch's ids, keep mask and work buffer
    kArCount
};

// batch_front's part of kArText, as offsets from the buffer's start: the text (nb bytes and 64 of padding), the
// document offsets and doc_tok (ndocs + 1 u64 each), the counts (2 u64) and the span arrays (cap starts, cap
// ends), every piece on a 256-byte boundary; the caller's `extra` bytes start at `extra`, and `total` is the
// size the buffer is grown to.
struct BatchLayout {
    size_t text, doff, dtok, dcnt, dse, extra, total;
};
inline BatchLayout batch_layout(uint64_t nb, uint32_t ndocs, uint64_t cap, size_t extra) {
    const size_t ndoc8 = ((size_t)ndocs + 1) * 8;
    BatchLayout l;
    l.text = 0;
    l.doff = l.text + r256(nb + 64);
    l.dtok = l.doff + r256(ndoc8);
    l.dcnt = l.dtok + r256(ndoc8);
    l.dse = l.dcnt + r256(16);
    l.extra = l.dse + r256(2 * cap * 4);
    l.total = l.extra + extra;
    return l;
}
// batch_chain's extra bytes: its term offsets (ndocs + 1 u64), then its caller's.
inline size_t batch_chain_extra(uint32_t ndocs, size_t extra0) { return r256(((size_t)ndocs + 1) * 8) + extra0; }

#ifndef JB_BATCH_LAYOUT_ONLY
#include <hip/hip_runtime_api.h>

#include "../../include/jiebahip.h"

// ctx->kw_buf[which], grown to `need` bytes (under kw_mu).
int kw_arena(jb_ctx* ctx, KwBuf which, size_t need, Arena* a);

// What every host-text call checks of its batch: doc_off does not decrease, a text is there, under 2 GiB.
// *nb is the batch's size in bytes.
int batch_args(const char* who, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, uint64_t* nb);
// The first device's ordinal, read under the ctx's shared lock; under the same lock, JB_EINVAL when the call
// needs a vocabulary and none is attached, or `rule` (may be null) asks for a stop set and none is attached.
int batch_device(jb_ctx* ctx, const char* who, bool need_vocab, const jb_filter_rule* rule, int* ordinal);

// How the calls' fronts differ.
struct FrontOpts {
    int mode = JB_MODE_CUT;  // (checked by the caller)
    int hmm = 0;
    bool ctx_filter = false;               // the ctx's batch filter (jb_batch_filter_set) runs after the cut when one is set
    const jb_filter_rule* rule = nullptr;  // the caller's own rule runs after the cut (jb_cut_batch_filter)
    size_t extra = 0;                      // the caller's bytes of kArText
    // jb_cut_batch_charspans: a count over out_cap is JB_ELIMIT with *ntokens set, before a regrow and a second cut
    uint64_t* ntokens = nullptr;
    uint64_t out_cap = 0;
};

// What the front leaves on the device for the call's own step.
struct Front {
    hipStream_t st;
    uint8_t* dt;  // the text, 64 zero bytes behind it
    uint64_t nb;
    uint64_t* doff;  // ndocs + 1, from 0
    uint32_t ndocs;
    uint32_t* dse;   // starts at dse, ends at dse + cap: the cut's list, or the filtered one
    uint64_t cap;
    uint64_t* dtok;  // ndocs + 1
    uint64_t* dcnt;  // [0] the list's count, [1] spare; behind a filter [2 .. 6] are its statistics
    uint64_t ntok;   // the cut's count, before any filter
    uint64_t tcap;   // min(ntok, cap), at least 1: the entries the call's own step sizes its buffers for
    Arena a;         // kArText, at the caller's extra bytes
};

// The front of every host-text call with at least one document, after batch_args and batch_device: one
// non-blocking stream on the device, the batch uploaded into kArText, the cut of o.mode through the public entry
// points (each takes the ctx's lock for itself) with its errors collected (jb_device_status, which waits), full
// mode's regrow into kArTokens, and the filter step that `o` asks for.  `next(Front&)` queues the call's own step
// and its copies back; the stream is synchronised after it and destroyed, on error paths too.  kw_mu is held from
// before the stream's creation to after that.  `who` names the entry point in the messages.
template <class Next>
int batch_front(jb_ctx* ctx, const char* who, int ordinal, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs,
                uint64_t nb, const FrontOpts& o, Next next);

// The filter's step between the front's cut and the call's own step (under kw_mu): jb_filter_device over f's span
// list, with its work buffer and the filtered list in kArFilter.  On return f's names for the span list (dse,
// cap, dtok, dcnt) are the filtered list's; f->ntok stays the cut's count.
int batch_filter_step(jb_ctx* ctx, const char* who, const jb_filter_rule& rule, Front* f);

// What the chain leaves on the device for the call's last step.
struct BatchCsr {
    hipStream_t st;
    const uint32_t *term_id, *term_cnt;  // tcap entries each
    const uint64_t* term_off;            // ndocs + 1
    const uint64_t* nterms;
    uint64_t tcap;
    const uint32_t* ids;      // tcap entries, in token order
    const uint64_t* doc_tok;  // ndocs + 1
    const uint64_t* ntok;
};

// batch_args, batch_device (a vocabulary is needed, also for no document) and batch_front in plain mode, then
// ids -> terms in kArTokens (sized by the token count) and `last(csr, arena)`, which queues the call's last step
// and its copies back; the arena is kArText at the `extra0` bytes the caller asked for.
template <class Last>
int batch_chain(jb_ctx* ctx, const char* who, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                size_t extra0, Last last);

// The page-locked block jb_joined_free keeps for the next jb_cut_batch_join, let go (jb_close).
void joined_drop_cache();

// jb_bm25_search_device's launch (jb_capi.cpp), which jb_search_batch queues under its own hold of the ctx's
// lock: the caller holds it (shared or exclusive) and has checked the arguments.
int bm25_queue(jb_ctx* ctx, const uint32_t* d_post_doc, const uint32_t* d_post_tf, const uint64_t* d_post_off,
               uint64_t npost, uint32_t nids, const float* d_norm, uint32_t ndocs, const float* d_weight,
               uint32_t nweights, double k1, const uint32_t* d_q_id, uint64_t q_cap, const uint64_t* d_q_off, uint32_t nq,
               uint32_t topk, hipStream_t s, uint32_t* d_res_doc, uint64_t* d_res_score, uint32_t* d_res_n, void* d_work);
#endif  // JB_BATCH_LAYOUT_ONLY

#pragma GCC visibility pop
