// jb_pipeline.cpp — run_pipeline: the gfx950 kernels of the jieba-go Cut path, in launch order.
// (Host code only: every kernel is enqueued by its own unit through jb_kstages.h.)
//
// Pipeline for one batch of documents (all in HBM, one stream):
//   k_docbits     document starts -> 1 bit per byte
//   k_mark_walk   per 4 KiB tile: UTF-8 decode at lead bytes (Go rules), \p{Han}
//                 runs -> block-start masks + counts (zh regex + splitText,
//                 tokenizer.go:21,154-155,165-210); then the trie walk (DAG
//                 edges) of every Han rune of the tile, one walk per lane at a
//                 time from an LDS entry list (buildDag, :462-497)
//   k_zh          per 6 KiB group (1 KiB in small batches): its Han blocks from the
//                 block-start masks, dealt to lanes by length; backward max-prob DP
//                 over the edges + forward path + BMES Viterbi on singleton runs
//                                               (cutZh/cutDAG/buildDag/calcDagProba/
//                                                findDagPath/maxIndexProba/viterbi/cutHMM,
//                                                tokenizer.go:221-285,462-578,668-756)
//   k_long_*      Han blocks of 8 KiB or more (one serial DP chain each)
//   k_nonzh       the non-Han blocks with an alnum byte, from the alnum16 bits and
//                 the masks: alnum runs, single runes, spaces dropped (cutNonZh,
//                 tokenizer.go:289-310; blocks without alnum have no tokens)
//   k_tok<0>/k_tok<1>  token start/end bitmaps -> counts (+ 256-tile sums, k_sup)
//                 -> (start, end) spans
//   k_doc_tok     per document first token (Cut per document)
//
// Output format on the device: two bitmaps, 1 bit per input byte each (token
// first byte, token last byte), compacted to u32 spans.  All float64
// arithmetic is IEEE add/compare in the reference's order; the library is
// built with -ffp-contract=off and without fast-math (±Inf must propagate).
#include "jb_kstages.h"

#include <algorithm>

namespace jb {

const char* const kKernelNames[K_NUM] = {"k_docbits", "k_mark_walk", "k_zh", "k_nonzh", "k_tok_count", "k_scan_tok",
                                         "k_tok_write", "k_doc_tok", "k_long_spec", "k_long_dp", "k_long_seg", "k_long_path",
                                         "k_long_tail", "k_mask_merge", "k_long_pbits", "k_long", "k_tok1", "k_srch_count",
                                         "k_srch_scan", "k_srch_write", "k_srch_doc", "k_full_count", "k_full_scan",
                                         "k_full_write", "k_full_doc", "k_ids", "k_terms_sort", "k_terms_merge",
                                         "k_terms_count", "k_terms_scan", "k_terms_write", "k_keywords", "k_df",
                                         "k_idf", "k_tr_init", "k_tr_setup", "k_tr_count", "k_tr_step", "k_tr_push",
                                         "k_tr_final", "k_join_count", "k_join_scan", "k_join_doc", "k_join_write",
                                         "k_cs_class", "k_cs_scan", "k_cs_lookup", "k_wc_claim", "k_wc_store",
                                         "k_wc_count", "k_mh_init", "k_mh_hash", "k_mh_sig", "k_mh_bands",
                                         "k_filt_mark", "k_filt_scan", "k_filt_write",
                                         "k_post_hist", "k_post_scan", "k_post_scatter", "k_post_off",
                                         "k_bm25_norms", "k_bm25_idf", "k_bm25_tile", "k_bm25_scatter", "k_bm25_select",
                                         "k_bm25_merge",
                                         "k_nd_hist", "k_nd_scan", "k_nd_scatter", "k_nd_mask", "k_nd_tsum",
                                         "k_nd_base", "k_nd_off", "k_nd_write",
                                         "k_cl_zero", "k_cl_bounds", "k_cl_claim", "k_cl_count", "k_cl_score"};

hipError_t run_pipeline(const DevImage& im, const Work& w, const uint8_t* d_text, uint64_t nbytes,
                        const uint64_t* d_doc_off, uint32_t ndocs, bool hmm, const LaunchCfg& lc,
                        hipStream_t stream, KernelTimer* timer, const MaskOut* mask) {
    const uint32_t diag = lc.diag;
    const uint64_t nwords = (nbytes + 31) / 32;
    const uint32_t ntiles = (uint32_t)((nbytes + kTileBytes - 1) / kTileBytes);
    // k_zh work unit: a small batch gets small groups, so that enough waves share it
    const uint32_t grp = lc.zh_group ? lc.zh_group : zh_group_for(nbytes);
    const uint32_t nttiles = (uint32_t)((nwords + kTokTileWords - 1) / kTokTileWords);
    // k_zh: a persistent grid, but no more 4-wave workgroups than the batch has groups
    // the last zh_tail bytes (at most) in groups of zh_tail_group (tail_groups)
    uint32_t g1, sgrp;
    const uint64_t ngroups = zh_tail_groups(nbytes, grp, lc, &g1, &sgrp);
    // the wide form (16 waves per workgroup, weights in LDS) for batches in 6 KiB groups whose
    // weight table fits; JB_ZH_WIDE (lc.zh_wide) forces either form
    const bool wide = im.nw1 <= kZhWtabWide && (lc.zh_wide > 0 || (lc.zh_wide < 0 && grp == kZhGroupBytes));
    const uint32_t nw = wide ? kZhWgWide : 4u;
    const uint32_t grid_zh = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>((wide ? lc.zh_waves_wide : lc.zh_waves) / nw, (ngroups + nw - 1) / nw));
    // No clearing pass: the document bitmap is all zeros between runs (k_nonzh clears
    // what k_docbits set; a fresh or dirty workspace is cleared by the caller), k_docbits
    // clears the counters and k_mark_walk the token bitmaps, tile by tile.
    if (nbytes == 0)  // (kernels, not hipMemsetAsync: see k_zero)
        return run_zero(w.doc_tok, (ndocs + 1) * sizeof(uint64_t), stream, w.counters, CNT_CLEAR * sizeof(uint32_t));
    JB_TIMED(K_DOCBITS, enq_docbits(w, d_doc_off, ndocs, nbytes, nttiles, stream));
    // a batch with fewer tiles than CUs: two workgroups per tile (k_mark_walk's split)
    const uint32_t mws = lc.mw_split >= 0 ? (uint32_t)lc.mw_split : (ntiles <= lc.ncu ? 1u : 0u);
    JB_TIMED(K_MARK_WALK, enq_mark_walk(im, w, d_text, nbytes, ntiles, mws, diag, stream));
    JB_TIMED(K_ZH, enq_zh(im, w, d_text, nbytes, hmm, wide, grid_zh, grp, g1, sgrp, diag, stream));
    bool nz_done = false;  // (k_nonzh's work ran inside k_long)
    {
        // long blocks: the chain, then one lane per 64-rune segment (at most
        // nbytes / 192 + nbytes / kZhLongMin segments), one wave per block
        const uint64_t segs = nbytes / (3u * kSeg) + nbytes / kZhLongMin + 2u;
        const uint32_t gseg = (uint32_t)std::min<uint64_t>(1024u, (segs + 255u) / 256u);
        const uint32_t spec = lc.long_spec;
        if (lc.long_fused) {
            // one workgroup per 64 segments (k_long_spec's lanes), at most one per CU; a batch of at most
            // JB_NZ_FUSE_MIB MiB (default 4) runs k_nonzh's work in it too (one launch less)
            uint32_t gl = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(lc.ncu, (segs + 63u) / 64u));
            const bool nzf = nbytes <= ((uint64_t)lc.nz_fuse_mib << 20);
            if (nzf) gl = std::max(gl, (uint32_t)((nbytes + 1023u) / 1024u + 255u) / 256u);
            JB_TIMED(K_LONG, enq_long(im, w, d_text, nbytes, ntiles, d_doc_off, ndocs, hmm, nzf, gl, spec,
                                      lc.long_wait_ticks, stream));
            nz_done = nzf;
        } else {
            if (spec) JB_TIMED(K_LONG_SPEC, enq_long_spec(im, w, d_text, spec, stream));
            if (spec && lc.long_spec != 3u) {  // the path of the decided choices (the path chain's blocks, lflag 3)
                JB_TIMED(K_LONG_PATH, enq_long_path(w, 3u, 3u, stream));
                JB_TIMED(K_LONG_PBITS, enq_long_pbits(w, gseg, stream));
            }
            JB_TIMED(K_LONG_DP, enq_long_dp(im, w, d_text, hmm, spec, stream));
            JB_TIMED(K_LONG_SEG, enq_long_seg(im, w, d_text, gseg, stream));
            JB_TIMED(K_LONG_PATH, enq_long_path(w, 2u, 1u, stream));
            JB_TIMED(K_LONG_TAIL, enq_long_tail(im, w, d_text, hmm, gseg, stream));
        }
    }
    if (!nz_done) JB_TIMED(K_NONZH, enq_nonzh(w, d_text, nbytes, ntiles, d_doc_off, ndocs, stream));
    if (mask) {  // boundary masks instead of spans
        JB_TIMED(K_MASK_MERGE, enq_mask_merge(w, nbytes, *mask, stream));
        return hipGetLastError();
    }
    // the span kernels in one pass for batches of at most 256 token tiles (4 MiB): at 1 GiB
    // (65K tiles) the look-back chains cost more than the passes it saves (0.33 -> 0.84 ms)
    if (lc.tok1 && nttiles <= 256u) {
        JB_TIMED(K_TOK1, enq_tok1(w, nwords, nttiles, d_doc_off, ndocs, stream));
        return hipGetLastError();
    }
    JB_TIMED(K_TOK_COUNT, enq_tok_count(w, nwords, nttiles, stream));
    if (nttiles > 256u)  // (k_tok's write pass reads the sums of whole groups of 256 tiles only)
        JB_TIMED(K_SCAN_TOK, enq_sup(w.ttile_cnt, nttiles, w.supt, stream));
    JB_TIMED(K_TOK_WRITE, enq_tok_write(w, nwords, nttiles, stream));
    JB_TIMED(K_DOC_TOK, enq_doc_tok(w, d_doc_off, ndocs, stream));
    return hipGetLastError();
}

}  // namespace jb
