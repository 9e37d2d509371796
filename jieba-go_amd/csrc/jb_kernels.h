// jb_kernels.h — host-side launch interface of the gfx950 segmentation kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "jb_common.h"
#include "jb_vocab.h"
#include "jiebahip.h"

namespace jb {

// Device copy of the image (jb_common.h), passed by value to kernels.
struct DevImage {
    const uint16_t* pagemap;
    const double* emit;
    const uint32_t* code;   // dense rune code per row (0: in no key)
    const uint64_t* cells;  // double-array trie over codes; level-1 nodes at their codes
    const double* wtab;
    // wtab shifted by one: wtab1[0] = -Inf, wtab1[i + 1] = wtab[i].  DAG records hold
    // weight index + 1 per slot, so an unused slot gathers -Inf (k_mark_walk, k_zh)
    const double* wtab1;
    // per row: the rune's level-1 cell cells[code] with its check field
    // replaced by the code (bits 0-16) and bit 21 = "that check was the root",
    // so k_mark_walk gets code and level-1 cell in one load (jb_l1row_make)
    const uint64_t* l1row;
    // hot level-1 rows (jb_common.h JB_HOT_SLOTS): u64 l1row values, then u16 tags
    const uint64_t* hot;
    uint32_t nrows;
    uint32_t nw1;  // entries in wtab1 (distinct weights + 1)
    // 1: every weight is finite or -Inf (a dictionary whose size is > 0).  k_zh's
    // record fold relies on it; otherwise k_mark_walk writes only overflow records
    // and k_zh folds every rune with maxIndexProba's literal rule.
    uint32_t plainw;
};

// Device counters (u32 slots unless noted)
enum {
    CNT_NSRCH = 0,  // u64 at u32 slots 0-1: spans of the search-mode expansion (run_search) or of the full-mode
                    // list (run_full); 0 after a plain run
    CNT_NTOK = 2,   // token starts
    CNT_NTOKE = 3,  // token ends (== CNT_NTOK when consistent)
    CNT_ERR = 4,    // bit 0: a zh block reached a tail index -1 (the reference panics); bit 1: a k_long
                    // phase wait gave up (no progress for LaunchCfg::long_wait_ticks); bit 2: k_span_pack's
                    // side list overflowed (internal); bit 3: run_full's list is longer than the output
                    // arrays (FullOut::cap): the spans past them were counted and not written
    CNT_WORK = 5,   // k_zh work counter: next group (kZhGroupBytes of text)
    CNT_SIDE = 6,   // k_span_pack: tokens in the side list
    CNT_TOKT = 30,  // k_tok1's tile tickets
    CNT_PHASE = 32, // k_long's phases: claimed items at 32 + 2 p, finished items at 33 + 2 p
    CNT_ALL = 64,   // (u32 slots of the counters buffer; k_docbits clears them all)
    CNT_TIES = 7,   // exact Viterbi route ties (Q12)
    CNT_NWORDS = 8, // u64 token count lives at u32 slots 8-9 (byte offset 32)
    CNT_NLONG = 10, // long zh blocks k_zh left to k_long_* (u64 with CNT_NLSEG: one atomic)
    CNT_NLSEG = 11, // their 64-rune segments
    CNT_CLEAR = 12  // u32 slots cleared per batch
};

constexpr int kTileBytes = 4096;       // k_blocks: 256 threads x 16 bytes
constexpr int kTokTileWords = 512;     // k_tok: 256 threads x 2 words (16 KiB of text)
#ifndef JB_ZH_GROUP
#define JB_ZH_GROUP 6144
#endif
constexpr uint32_t kErecPad = 8;  // erec slots before slot 0 (k_zh reads a few slots past a block's start)
// k_zh work unit: the zh blocks that start in one group of text bytes (a
// multiple of 32): kZhGroupBytes, or kZhGroupSmall for batches under
// kZhSmallBatch bytes so that a small batch still spreads over enough waves
constexpr uint32_t kZhGroupBytes = JB_ZH_GROUP;
constexpr uint32_t kZhGroupSmall = 1024;
constexpr uint64_t kZhSmallBatch = 16ull << 20;
constexpr uint32_t kZhLongMin = 8192;  // zh blocks of at least this many bytes go to k_long_*
constexpr uint32_t kSeg = 64;          // runes per segment of a long block (k_long_seg/path/tail)
inline uint32_t zh_group_for(uint64_t nbytes) { return nbytes < kZhSmallBatch ? kZhGroupSmall : kZhGroupBytes; }
// k_zh's wide form: 16-wave workgroups, one per CU, sharing one LDS copy of the weight
// table (up to kZhWtab entries of wtab1) for the DP's weight reads
constexpr uint32_t kZhWgWide = 16;
constexpr uint32_t kZhWtab = 5120;
// ... of which k_zh's wide form holds up to kZhWtabWide (its LDS also holds the per-wave slots
// and block tables, which larger groups make larger)
#ifndef JB_ZH_WTAB
#define JB_ZH_WTAB 5120
#endif
constexpr uint32_t kZhWtabWide = JB_ZH_WTAB;

// Per-call device workspace, sized for `nbytes` of text.
struct Work {
    uint32_t* docbits;     // 1 bit per byte: a document starts here
    uint32_t* sbits;       // 1 bit per byte: a token starts here
    uint32_t* ebits;       // 1 bit per byte: a token ends here (last byte)
    uint64_t bits_stride;  // words between docbits, sbits and ebits (one allocation)
    uint2* supt;           // per 256 token tiles: (starts, ends) (k_sup)
    uint2* tile_cnt;       // per k_mark_walk tile: (blocks, zh blocks) starting in it
    uint2* ttile_cnt;      // per token tile (starts, ends); k_tok1: its look-back status word
    uint64_t* alnum16;     // 1 bit per 16 bytes of text: some [0-9A-Za-z] byte there
    uint64_t* erec;        // per Han rune (slot = byte / 3): packed DAG edges (k_mark_walk -> k_zh)
    uint32_t* lanemask;    // per 16 bytes: block starts | Han block starts << 16 (k_zh and k_nonzh read
                           // their blocks from these bits: a block ends at the next start)
    uint2* longblk;        // (start, end) of each long zh block (k_zh -> k_long_*)
    uint32_t* lsegb;       // per long block: its first segment (ascending with the block index)
    uint8_t* lmap;         // per 64-segment chunk of a long block: its path-state map (k_long_seg -> k_long_path)
    uint8_t* lcx;          // per chunk: the path state at its start (k_long_path -> k_long_tail)
    uint64_t* lpath;       // per segment: the runes where a piece of the decided path starts (k_long_pbits -> k_long_dp)
    uint32_t* tile4;       // per tile: a 4-byte Han rune starts in it
    uint8_t* gbl;          // per Han rune: chosen piece length, then Viterbi back-pointers / labels
                           // (+512 bytes: k_zh_long reads 256-slot windows)
    uint32_t* lflag;       // per long block: 3 decided by k_long_spec (the path chain's), then k_long_dp's
                           // verdict: 0 cut by its one-lane path, 2 DP done, 1 entries found (or path verified)
    uint8_t* lbp;          // long blocks, per slot: path exit codes (k_long_seg -> k_long_path, k_long_tail)
    double* gbest;         // per Han rune: best proba, kept only for blocks with an edge > 8 runes
    uint32_t* tok_start;
    uint32_t* tok_end;
    uint64_t* doc_tok;
    uint32_t* counters;    // CNT_* (+ u64 ntok at counters + 8)
    uint64_t* dbg = nullptr;       // diagnostic per-wave clocks of k_zh (JB_ABLATE bit 8), 8 u64 per wave
    uint64_t* dbg_walk = nullptr;  // the same for k_mark_walk
    uint64_t cap_bytes = 0;
    uint32_t cap_docs = 0;
};

// Kernel ids for per-launch timing.
enum KernelId {
    K_DOCBITS = 0, K_MARK_WALK, K_ZH, K_NONZH,
    K_TOK_COUNT, K_SCAN_TOK, K_TOK_WRITE, K_DOC_TOK, K_LONG_SPEC, K_LONG_DP, K_LONG_SEG, K_LONG_PATH, K_LONG_TAIL, K_MASK_MERGE,
    K_LONG_PBITS, K_LONG, K_TOK1, K_SRCH_COUNT, K_SRCH_SCAN, K_SRCH_WRITE, K_SRCH_DOC,
    K_FULL_COUNT, K_FULL_SCAN, K_FULL_WRITE, K_FULL_DOC, K_IDS,
    K_TERMS_SORT, K_TERMS_MERGE, K_TERMS_COUNT, K_TERMS_SCAN, K_TERMS_WRITE, K_KEYWORDS,
    K_DF, K_IDF,
    K_TR_INIT, K_TR_SETUP, K_TR_COUNT, K_TR_STEP, K_TR_PUSH, K_TR_FINAL,
    K_JOIN_COUNT, K_JOIN_SCAN, K_JOIN_DOC, K_JOIN_WRITE,
    K_CS_CLASS, K_CS_SCAN, K_CS_LOOKUP,
    K_WC_CLAIM, K_WC_STORE, K_WC_COUNT,
    K_MH_INIT, K_MH_HASH, K_MH_SIG, K_MH_BANDS,
    K_FILT_MARK, K_FILT_SCAN, K_FILT_WRITE,
    K_POST_HIST, K_POST_SCAN, K_POST_SCATTER, K_POST_OFF,
    K_BM25_NORMS, K_BM25_IDF, K_BM25_TILE, K_BM25_SCATTER, K_BM25_SELECT, K_BM25_MERGE,
    K_ND_HIST, K_ND_SCAN, K_ND_SCATTER, K_ND_MASK, K_ND_TSUM, K_ND_BASE, K_ND_OFF, K_ND_WRITE,
    K_CL_ZERO, K_CL_BOUNDS, K_CL_CLAIM, K_CL_COUNT, K_CL_SCORE,
    K_NUM
};
extern const char* const kKernelNames[K_NUM];

// Optional per-launch timer (HIP events recorded on the launch stream).
struct KernelTimer {
    virtual void begin(int kernel_id, hipStream_t s) = 0;
    virtual void end(int kernel_id, hipStream_t s) = 0;
    virtual ~KernelTimer() {}
};

// Launch shape of one pipeline run (fixed per device at jb_open).
struct LaunchCfg {
    uint32_t zh_waves;       // persistent grid of k_zh, in waves (4-wave workgroups)
    uint32_t zh_waves_wide;  // ... of its wide form (kZhWgWide-wave workgroups)
    int32_t zh_wide;         // k_zh's wide form: -1 by batch size, 0 never, 1 whenever the weights fit
    uint32_t zh_group;  // k_zh group bytes (0: zh_group_for(nbytes))
    uint32_t diag;      // diagnostic clocks (STAMPS builds only; 0 otherwise)
    uint32_t small_max; // host batches up to this many bytes take k_small (0: never)
    uint32_t zh_tail;        // k_zh: about this many bytes at the batch end go in smaller groups (0: none)
    uint32_t zh_tail_group;  // ... of this many bytes (a multiple of 32, at most the group size)
    uint32_t long_spec;      // long blocks: speculative choices, then (JB_LONG_SPEC) 1 the path chain (default),
                             // 3 the decided chain (round 4), 0 neither (the exact chain); 2 testing: as 1 with
                             // some choices wrong on purpose, so that the exact chain redoes the block
    uint32_t long_fused;     // the long-block kernels as one launch, k_long (JB_LONG_FUSED: 1 default, 0 separate)
    uint32_t ncu;            // the device's CUs (k_long's grid: at most one workgroup per CU)
    uint32_t tok1;           // the span kernels as one pass, k_tok1, for batches of <= 256 token tiles
                             // (JB_TOK1: 1 default, 0 the count/write passes always)
    uint32_t nz_fuse_mib;    // k_nonzh's work inside k_long (fused) for batches of at most this many MiB
                             // (JB_NZ_FUSE_MIB: 4 default, 0 never)
    uint32_t long_wait_ticks;  // k_long: a phase wait gives up after this many 100 MHz ticks without progress
                               // (JB_LONG_WAIT_US x 100; default 20 s)
    int32_t mw_split;        // k_mark_walk: 2^s workgroups per tile, each walking its share of the entries
                             // (JB_MW_SPLIT: -1 = 1 when the batch has at most one tile per CU, else 0; 0-3 fixed)
    uint32_t df_combine;     // jb_df_device: 1 k_df_combine, 0 k_df (JB_DF_COMBINE; results do not depend on it)
    uint32_t tr_window;      // jb_textrank_device's push: 1 k_tr_push_win, 0 k_tr_push (JB_TR_WINDOW; results do not
                             // depend on it)
    uint32_t join_stage;     // jb_join_device's write: 0 the plain form (default), 1 the staged form (JB_JOIN_STAGE; results do
                             // not depend on it)
    uint32_t wc_combine;     // jb_wc_add_device's count pass: 0 one global atomic per token, 1 combined in LDS
                             // (JB_WC_COMBINE; results do not depend on it)
    uint32_t wc_bits;        // the fingerprint keeps this many low bits of the hash (JB_WC_HASHBITS: 64; fewer
                             // only to test the collision path)
    uint32_t mh_form;        // jb_minhash_device's signature pass: 0 the plain form, 1 the staged form (JB_MH_FORM;
                             // results do not depend on it)
    uint32_t post_form;      // jb_postings_device's scatter: 0 from the lanes (default: 3.26 ms against 3.37 ms on the
                             // 1 GiB corpus, profiles/postings_bench.json), 1 through LDS in runs (JB_POSTINGS_FORM;
                             // results do not depend on it)
    uint32_t bm25_form;      // jb_bm25_search_device: 0 a dense row per query and global atomics, 1 a document tile's
                             // scores in LDS (default: 0.96 ms against 1.75 ms on the 1 GiB corpus's index,
                             // profiles/bm25_bench.json) (JB_BM25_FORM; results do not depend on it)
    uint32_t colloc_combine; // jb_colloc_add_device's count pass: 0 one global atomic per pair and per unigram, 1
                             // combined in LDS (default: 16.29 ms against 132.74 ms on the 1 GiB corpus,
                             // profiles/colloc_bench.json) (JB_COLLOC_COMBINE; results do not depend on it)
};

// k_zh's group split: g1 groups of grp bytes, then groups of *sgrp bytes to the end.
// Returns the number of groups.
inline uint64_t zh_tail_groups(uint64_t nbytes, uint32_t grp, const LaunchCfg& lc, uint32_t* g1, uint32_t* sgrp) {
    *sgrp = grp;
    *g1 = (uint32_t)((nbytes + grp - 1) / grp);
    if (lc.zh_tail && lc.zh_tail_group && lc.zh_tail_group < grp && nbytes > lc.zh_tail) {
        *g1 = (uint32_t)((nbytes - lc.zh_tail) / grp);
        *sgrp = lc.zh_tail_group;
    }
    const uint64_t tail0 = (uint64_t)*g1 * grp;
    return *g1 + (tail0 < nbytes ? (nbytes - tail0 + *sgrp - 1) / *sgrp : 0);
}

// Boundary-mask output of one pipeline run (jb_cut_batch_mask): the batch's token
// start / end bits go into the u64 bitmaps s / e at bit offset rel (k_mask_merge)
// instead of becoming spans; the counters still receive the token count.
struct MaskOut {
    uint64_t* s;
    uint64_t* e;
    uint64_t rel;
};

// Enqueue the whole Cut pipeline on `stream`.  Returns hipSuccess or the first
// launch error.  d_text must be readable 64 bytes past nbytes.  mask != nullptr:
// boundary masks instead of spans (tok_start / tok_end / doc_tok are not written).
hipError_t run_pipeline(const DevImage& im, const Work& w, const uint8_t* d_text, uint64_t nbytes,
                        const uint64_t* d_doc_off, uint32_t ndocs, bool hmm, const LaunchCfg& lc,
                        hipStream_t stream, KernelTimer* timer, const MaskOut* mask = nullptr);

// Search mode (jb_cut_*_search): the spans of a finished run_pipeline, expanded.  Every Han token
// of three or more runes is preceded by the dictionary words of two runes inside it, then (four
// or more runes) those of three runes, each in text order; every other token stays as it is.
// Token tile = kSrchTile consecutive tokens, one workgroup each.
constexpr uint32_t kSrchPer = 16;                  // tokens per thread
constexpr uint32_t kSrchTile = 256u * kSrchPer;    // tokens per workgroup
inline uint64_t srch_tiles(uint64_t nbytes) { return std::max<uint64_t>(1u, (nbytes + kSrchTile - 1u) / kSrchTile); }
struct SearchOut {
    uint32_t* start;    // expanded spans (at least nbytes entries: a token gives at most as many spans as it has bytes)
    uint32_t* end;
    uint64_t* doc_tok;  // ndocs + 1: document d's spans are [doc_tok[d], doc_tok[d+1])
    uint64_t* ntok;     // the expanded count (also left in the counters, CNT_NSRCH)
    // workspace
    uint32_t* off;      // per plain token: its span count (k_srch_count), then its first span (k_srch_write)
    uint2* tile;        // per token tile: (spans, 0); srch_tiles(nbytes) entries
    uint2* sup;         // per 256 token tiles: their sum (k_sup)
};
// Enqueue the search pass on `stream`, after run_pipeline's kernels for the same batch (w.tok_start /
// w.tok_end / w.doc_tok hold its plain spans, w.erec its DAG records).
hipError_t run_search(const DevImage& im, const Work& w, const SearchOut& so, const uint8_t* d_text, uint64_t nbytes,
                      uint32_t ndocs, hipStream_t stream, KernelTimer* timer);

// Full mode (jb_cut_*_full, jieba's cut_all): the spans of a finished run_pipeline with hmm = 0 replaced,
// inside every Han block, by each dictionary word of two or more runes (by start, then by length) and by the
// single runes that no such word accounts for; non-Han tokens are copied.  The list can be longer than
// the text, so the counts are 64 bits wide and the output arrays have a capacity of their own.
struct FullOut {
    uint32_t* start;    // the spans, cap entries: a span whose index is >= cap is not written
    uint32_t* end;
    uint64_t cap;
    uint64_t* doc_tok;  // ndocs + 1, of the complete list
    uint64_t* ntok;     // the count of the complete list (also left in the counters, CNT_NSRCH)
    // workspace (SearchOut's, which both modes may share, and tbase)
    uint32_t* off;      // per plain token: its span count (k_full_count), then its first span within its tile
    uint64_t* tile;     // per token tile: its spans; srch_tiles(nbytes) entries
    uint64_t* sup;      // per 256 token tiles: their sum (k_sup64)
    uint64_t* tbase;    // per token tile: the spans before it (k_full_write)
    uint32_t maxlen;    // the image's longest key, runes
};
// Enqueue the full-mode pass on `stream`, after run_pipeline's kernels (hmm = false) for the same batch.
hipError_t run_full(const DevImage& im, const Work& w, const FullOut& fo, const uint8_t* d_text, uint64_t nbytes,
                    uint32_t ndocs, hipStream_t stream, KernelTimer* timer);

// Token ids (jb_ids_device, jb_spans_ids): every span of a device span list looked up in the ctx's
// vocabulary (jb_vocab.h), one lane per span.  The device copy of the table, passed by value:
using DevVocab = JbVocabView;
constexpr uint32_t kIdsTile = 256;     // spans per workgroup and trip: thread t owns spans j * 256 + t
constexpr uint32_t kIdsWgPerCu = 8;    // the fixed grid: 8 workgroups of 4 waves fill a CU's 32 wave slots
// Enqueue k_ids on `stream`: ids[k] for k < min(*d_ntok, cap), read on the device; nothing else is
// written and no text byte outside [0, nbytes) + 64 is read, whatever the spans hold.  d_text is
// 4-byte aligned.  A grid of at most ncu * kIdsWgPerCu workgroups loops over the tiles.
hipError_t run_ids(const DevVocab& v, const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start,
                   const uint32_t* d_end, const uint64_t* d_ntok, uint64_t cap, uint32_t* d_ids, uint32_t ncu,
                   hipStream_t stream, KernelTimer* timer);

// Term counts and keywords (jb_terms_device, jb_keywords_device; jb_terms.hip).  Sort tile = kTermsTile
// consecutive tokens, one workgroup each: 4096 x 8 bytes of keys are 32 KiB of LDS.
constexpr uint32_t kTermsTile = 4096;
constexpr uint32_t kKwMaxK = 64;  // JB_KW_MAXK: k_keywords keeps one key per lane of a wave
// Bytes of the work buffer run_terms needs for an id list of up to max_tokens entries.  Host only.
size_t terms_work_bytes(uint64_t max_tokens, uint32_t ndocs);
// Enqueue the term-count kernels on `stream`: the CSR of the tokens k < min(*d_ntok, ids_cap) whose id is
// not JB_VOCAB_UNK.  term_id / term_cnt entries with index >= cap are not written; term_off (ndocs + 1) and
// *d_nterms describe the complete list.  d_work holds terms_work_bytes(ids_cap, ndocs) bytes, 8-byte aligned.
// (K_TERMS_MERGE times k_terms_merge and k_terms_copy together.)
hipError_t run_terms(const uint32_t* d_ids, uint64_t ids_cap, const uint64_t* d_doc_tok, const uint64_t* d_ntok,
                     uint32_t ndocs, uint32_t* d_term_id, uint32_t* d_term_cnt, uint64_t cap, uint64_t* d_term_off,
                     uint64_t* d_nterms, void* d_work, hipStream_t stream, KernelTimer* timer);
// Enqueue k_keywords on `stream`: per document the topk (1 .. kKwMaxK) candidates by score, then id.
hipError_t run_keywords(const uint32_t* d_term_id, const uint32_t* d_term_cnt, const uint64_t* d_term_off,
                        uint32_t ndocs, uint64_t cap, const float* d_weight, uint32_t nweights, uint32_t topk,
                        uint32_t* d_kw_id, float* d_kw_score, uint32_t* d_kw_cnt, uint32_t* d_kw_n,
                        hipStream_t stream, KernelTimer* timer);
// Document frequencies and IDF weights (jb_df_device, jb_idf_device; jb_terms.hip).
// Enqueue k_df (combine: k_df_combine, the same sums through a table in LDS) on `stream`: d_df[id] += 1
// for every entry i < min(*d_nterms, cap) of d_term_id whose id is < ndf (ndf > 0); nothing else is
// written and nothing at or past cap is read.  A grid of a few workgroups per CU, sized by cap.
hipError_t run_df(const uint32_t* d_term_id, const uint64_t* d_nterms, uint64_t cap, uint32_t* d_df, uint32_t ndf,
                  bool combine, uint32_t ncu, hipStream_t stream, KernelTimer* timer);
// Enqueue k_idf on `stream`: d_weight[id] for every id < ndf (ndf > 0) by jb_idf's rule, bit for bit.
hipError_t run_idf(const uint32_t* d_df, uint32_t ndf, uint64_t ndocs_total, uint32_t min_df, uint32_t max_df,
                   const uint8_t* d_keep, float* d_weight, hipStream_t stream, KernelTimer* timer);

// TextRank keywords (jb_textrank_device; jb_textrank.hip).  Chunk = kTrChunk consecutive tokens, one
// workgroup each in the setup and in the windowed push, with a halo of span - 1 tokens on each side.
constexpr uint32_t kTrChunk = 1024;
constexpr uint32_t kTrMaxSpan = 32;   // JB_TR_MAXSPAN: the halo fits one byte of reach per side
constexpr uint32_t kTrMaxIter = 100;  // JB_TR_MAXITER
// Bytes of the work buffer run_textrank needs: 6 per token, 28 per term, 4 per document.  Host only.
size_t textrank_work_bytes(uint64_t max_tokens, uint64_t max_terms, uint32_t ndocs);
// Enqueue the TextRank kernels on `stream` (ndocs > 0, 2 <= span <= kTrMaxSpan, iters <= kTrMaxIter,
// 1 <= topk <= kKwMaxK): 4 launches and 2 per iteration (only 2 when ids_cap or cap is 0).  `window`
// chooses the push kernel.  d_work holds textrank_work_bytes(ids_cap, cap, ndocs) bytes, 8-byte aligned.
// (K_TR_PUSH times whichever push kernel runs.)
hipError_t run_textrank(const uint32_t* d_ids, uint64_t ids_cap, const uint64_t* d_doc_tok, const uint64_t* d_ntok,
                        uint32_t ndocs, const uint32_t* d_term_id, const uint64_t* d_term_off, uint64_t cap,
                        const uint8_t* d_keep, uint32_t nkeep, uint32_t span, uint32_t iters, uint32_t topk,
                        bool window, uint32_t* d_kw_id, float* d_kw_score, uint32_t* d_kw_n, void* d_work,
                        hipStream_t stream, KernelTimer* timer);

// Joined text (jb_join_device; jb_join.hip).  Tile = kJoinTile consecutive tokens, one workgroup each.
constexpr uint32_t kJoinTile = 2048;    // JB_JOIN_TILE: 256 threads x 8 tokens
constexpr uint32_t kJoinLong = 256;     // JB_JOIN_LONG: keys from here on are copied by the whole workgroup
constexpr uint32_t kJoinStage = 24576;  // bytes of a tile's output staged in LDS at a time
constexpr uint32_t kJoinMaxSep = 8;     // JB_JOIN_MAXSEP: separator and terminator travel as one u64 each
// Bytes of the work buffer run_join needs: 16 per tile, 16 per document and 16 per 256 documents.  Host only.
size_t join_work_bytes(uint64_t max_tokens, uint32_t ndocs);
// Enqueue the four join kernels on `stream`: the keys of the tokens k < min(*d_ntok, cap), the separators
// between a document's tokens and a terminator per document, into d_out below out_cap; d_out_doc_off
// (ndocs + 1) and *d_nout describe the complete output.  sep / term are host pointers (seplen, termlen <=
// kJoinMaxSep).  `staged` chooses the write kernel's form.  d_work holds join_work_bytes(cap, ndocs) bytes,
// 8-byte aligned.  (K_JOIN_WRITE times whichever form runs.)
hipError_t run_join(const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start, const uint32_t* d_end,
                    const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint64_t cap, uint32_t ndocs, const uint8_t* sep,
                    uint32_t seplen, const uint8_t* term, uint32_t termlen, bool staged, uint8_t* d_out,
                    uint64_t out_cap, uint64_t* d_out_doc_off, uint64_t* d_nout, void* d_work, hipStream_t stream,
                    KernelTimer* timer);

// Character offsets (jb_charspans_device; jb_charspans.hip).  Tile = kCsTile text bytes, one workgroup each; a
// bitmap word covers 64 text bytes.
constexpr uint32_t kCsTile = 4096;      // JB_CHARSPANS_TILE: 256 lanes x 16 bytes, 64 bitmap words
constexpr uint32_t kCsTokTile = 1024;   // tokens per workgroup of the lookup: 256 lanes x 4 tokens
// Bytes of the work buffer run_charspans needs: per 64 text bytes two u64 bitmap words and a u32 prefix,
// per tile a u32 sum and a u32 base.  It does not depend on ndocs today.  Host only.
size_t charspans_work_bytes(uint64_t nbytes, uint32_t ndocs);
// Enqueue the three kernels on `stream`: cstart / cend of the tokens k < min(*d_ntok, cap) (they may be
// d_start / d_end) and doc_units (ndocs), in runes (utf16 false) or UTF-16 code units.  d_work holds
// charspans_work_bytes(nbytes, ndocs) bytes, 8-byte aligned.
hipError_t run_charspans(const uint8_t* d_text, uint64_t nbytes, const uint64_t* d_doc_off, uint32_t ndocs,
                         const uint32_t* d_start, const uint32_t* d_end, const uint64_t* d_doc_tok,
                         const uint64_t* d_ntok, uint64_t cap, bool utf16, uint32_t* d_cstart, uint32_t* d_cend,
                         uint32_t* d_doc_units, void* d_work, hipStream_t stream, KernelTimer* timer);

// Word counts (jb_wc_init_device, jb_wc_add_device; jb_wc.hip, the table is jb_wc.h's).  Tile = kWcTile
// consecutive tokens per workgroup and trip, under k_ids' fixed grid.
constexpr uint32_t kWcTile = 256;
// Enqueue k_wc_init on `stream`: an empty table of nslots slots (valid by wc_sizes) and pool_bytes of pool.
hipError_t run_wc_init(void* d_table, uint64_t nslots, uint64_t pool_bytes, uint32_t ncu, hipStream_t stream);
// Enqueue the three passes on `stream` (none when cap is 0): the tokens k < min(*d_ntok, cap) added to the
// table at d_table (ntable bytes; a buffer that holds no table is left alone).  d_text is 4-byte aligned and
// no byte at or past nbytes + 64 is read; d_work holds 4 bytes per token of cap.  `bits` is the
// fingerprint's width, `combine` chooses the count pass's form.
hipError_t run_wc_add(void* d_table, uint64_t ntable, const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start,
                      const uint32_t* d_end, const uint64_t* d_ntok, uint64_t cap, uint32_t bits, bool combine,
                      uint32_t* d_work, uint32_t ncu, hipStream_t stream, KernelTimer* timer);

// MinHash signatures (jb_minhash_device, jb_minhash_bands_device; jb_minhash.hip, the rule's shared code is
// jb_minhash.h's).  Tile = kMhTile consecutive tokens, one workgroup each in the staged form.
constexpr uint32_t kMhTile = 1024;  // JB_MH_TILE
constexpr uint32_t kMhMaxN = 8;     // JB_MH_MAXN: the halo of a tile is at most 7 tokens
constexpr uint32_t kMhMaxK = 256;   // JB_MH_MAXK: one lane of a workgroup per hash function
// Enqueue k_mh_init, k_mh_hash and k_mh_sig on `stream` (k_mh_init alone when cap or ndocs is 0): sig (ndocs x
// K) and doc_n (ndocs) of the tokens k < min(*d_ntok, cap) under shingles of n tokens (1 .. kMhMaxN) and K
// (1 .. kMhMaxK) hash functions of `seed`.  d_text is 4-byte aligned and no byte at or past nbytes + 64 is
// read; d_work holds 8 bytes per token of cap.  `staged` chooses the signature kernel's form.
hipError_t run_minhash(const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start, const uint32_t* d_end,
                       const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint64_t cap, uint32_t ndocs, uint32_t n,
                       uint32_t K, uint64_t seed, bool staged, uint32_t* d_sig, uint32_t* d_doc_n, uint64_t* d_work,
                       uint32_t ncu, hipStream_t stream, KernelTimer* timer);
// Enqueue k_mh_bands on `stream`: keys (ndocs x B) from sig and doc_n, one lane per (document, band).
hipError_t run_minhash_bands(const uint32_t* d_sig, const uint32_t* d_doc_n, uint32_t ndocs, uint32_t K, uint32_t B,
                             uint32_t R, uint64_t* d_keys, uint32_t ncu, hipStream_t stream, KernelTimer* timer);

// The token filter (jb_filter_device; jb_filter.hip, the rule's shared code is jb_filter.h's).  Tile = kFiltTile
// consecutive tokens, one workgroup each.
constexpr uint32_t kFiltTile = 2048;  // JB_FILTER_TILE
// Enqueue k_filt_mark, k_filt_scan and k_filt_write on `stream` (three memsets and no launch when cap is 0):
// the tokens k < min(*d_ntok, cap) that `rule` keeps, in order, into d_out_start / d_out_end / d_out_src (may
// be null) at ranks below out_cap, d_out_doc_tok (ndocs + 1), *d_out_ntok and d_stats (5).  `stop` is the
// device copy of the stop set (read only with JB_FILTER_STOP).  d_text is 4-byte aligned and no byte at or
// past nbytes + 64 is read; d_work holds jb_filter_work_bytes(cap, ndocs) bytes, 8-byte aligned.
hipError_t run_filter(const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start, const uint32_t* d_end,
                      const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint64_t cap, uint32_t ndocs,
                      const jb_filter_rule& rule, const DevVocab& stop, uint32_t* d_out_start, uint32_t* d_out_end,
                      uint32_t* d_out_src, uint64_t out_cap, uint64_t* d_out_doc_tok, uint64_t* d_out_ntok,
                      uint64_t* d_stats, void* d_work, hipStream_t stream, KernelTimer* timer);

// Postings (jb_postings_device; jb_postings.hip, the rule's shared code is jb_postings.h's).  Tile = kPostTile
// consecutive entries, one workgroup each.
constexpr uint32_t kPostTile = 4096;  // JB_POSTINGS_TILE
// Enqueue 3 * jb_postings_passes(nids) + 1 launches on `stream` (two memsets and no launch when cap or nids is
// 0): the entries i < min(*d_nterms, cap, d_term_off[ndocs]) of the CSR whose id is below nids, stably sorted
// by id, as d_post_doc (doc_base + row) / d_post_tf at positions below pcap, d_post_off (nids + 1) and
// *d_nposts.  d_work holds jb_postings_work_bytes(cap, nids, ndocs) bytes, 8-byte aligned.  `form` chooses
// the scatter kernel's form.
hipError_t run_postings(const uint32_t* d_term_id, const uint32_t* d_term_cnt, const uint64_t* d_term_off,
                        const uint64_t* d_nterms, uint64_t cap, uint32_t ndocs, uint32_t nids, uint32_t doc_base,
                        uint32_t form, uint32_t* d_post_doc, uint32_t* d_post_tf, uint64_t pcap, uint64_t* d_post_off,
                        uint64_t* d_nposts, void* d_work, hipStream_t stream, KernelTimer* timer);

// Near-duplicate pairs (jb_neardup_device; jb_neardup.hip, the rule's shared code is jb_neardup.h's).  Tile =
// kNdTile entries, one workgroup.
constexpr uint32_t kNdTile = 4096;  // JB_ND_TILE
constexpr uint32_t kNdMaxWin = 64;  // JB_ND_MAXWIN: one bit of a u64 keep mask per place of the window
// Enqueue 32 launches on `stream` (three memsets and no launch when ndocs is 0): the entries (d, b) of d_key
// (ndocs x B) sorted by (band, key), the candidates of the window W verified against d_sig (ndocs x K), the
// kept pairs as a CSR by the later document in d_pair_doc / d_pair_agree at positions below pcap, d_pair_off
// (ndocs + 1), *d_npairs and d_stat (JB_ND_NSTAT).  d_work holds jb_neardup_work_bytes(ndocs, B) bytes, 8-byte
// aligned.
hipError_t run_neardup(const uint64_t* d_key, const uint32_t* d_sig, uint32_t ndocs, uint32_t B, uint32_t K, uint32_t W,
                       uint32_t min_agree, uint32_t* d_pair_doc, uint32_t* d_pair_agree, uint64_t pcap,
                       uint64_t* d_pair_off, uint64_t* d_npairs, uint64_t* d_stat, void* d_work, hipStream_t stream,
                       KernelTimer* timer);

// Collocations (jb_colloc_*_device; jb_colloc.hip, the table and the rule's shared code are jb_colloc.h's).
constexpr uint32_t kClTile = 256;   // JB_COLLOC_TILE
constexpr uint32_t kClLds = 2048;   // JB_COLLOC_LDS: entries of each of form 1's two tables, 32 KiB of LDS in all
constexpr uint32_t kClShare = 64;   // JB_COLLOC_SHARE: form 1's least share of a workgroup, in tiles
// Enqueue the kernel that empties a table of nslots slots and zeroes d_uni.
hipError_t run_colloc_init(void* d_table, uint64_t nslots, uint64_t* d_uni, uint32_t nuni, uint32_t ncu,
                           hipStream_t stream);
// Enqueue the four launches (none when ids_cap is 0) that add the tokens k < min(*d_ntok, ids_cap) of an id list to
// the table of d_table and to d_uni.  d_work holds jb_colloc_work_bytes(ids_cap, ndocs) bytes, 4-byte aligned.
hipError_t run_colloc_add(void* d_table, uint64_t ntable, uint64_t* d_uni, uint32_t nuni, const uint32_t* d_ids,
                          uint64_t ids_cap, const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint32_t ndocs,
                          const uint8_t* d_keep, uint32_t nkeep, uint32_t flags, const uint32_t* d_start,
                          const uint32_t* d_end, bool combine, void* d_work, uint32_t ncu, hipStream_t stream,
                          KernelTimer* timer);
// Enqueue a memset of *d_ncand and the score pass over the table's slots (nslots_hint sizes the grid only).
hipError_t run_colloc_score(const void* d_table, uint64_t ntable, uint64_t nslots_hint, const uint64_t* d_uni, uint32_t nuni,
                            int scorer, uint64_t min_count, float threshold, uint32_t* d_cand_a, uint32_t* d_cand_b,
                            uint64_t* d_cand_cnt, float* d_cand_score, uint64_t ccap, uint64_t* d_ncand, uint32_t ncu,
                            hipStream_t stream, KernelTimer* timer);

// BM25 (jb_bm25_*_device; jb_bm25.hip, the rule's shared code is jb_bm25.h's).  A document tile is kBm25Tile
// consecutive documents, one workgroup per pair of query and tile.
constexpr uint32_t kBm25Tile = 8192;  // JB_BM25_TILE
constexpr uint32_t kBm25MaxQ = 1024;  // JB_BM25_MAXQ
// One launch each (none for no document / no id): norm[d] for d < ndocs; weight[t] for t < nids.
hipError_t run_bm25_norms(const uint32_t* d_doc_len, uint32_t ndocs, double k1, double b, double avgdl, float* d_norm,
                          hipStream_t stream, KernelTimer* timer);
hipError_t run_bm25_idf(const uint64_t* d_post_off, uint32_t nids, uint64_t ndocs_total, float* d_weight,
                        hipStream_t stream, KernelTimer* timer);
// Enqueue the search on `stream`: per slice of up to 32,768 queries (fewer past 128 tiles) k_bm25_tile (form 1) or a memset, k_bm25_scatter
// and k_bm25_select (form 0), none when ndocs is 0, then k_bm25_merge; nothing at all when nq is 0.  d_work holds
// jb_bm25_work_bytes(nq, ndocs, topk) bytes (form 1 uses the first bm25_layout().bytes1 of them), 8-byte aligned.
hipError_t run_bm25_search(const uint32_t* d_post_doc, const uint32_t* d_post_tf, const uint64_t* d_post_off,
                           uint64_t npost, uint32_t nids, const float* d_norm, uint32_t ndocs, const float* d_weight,
                           uint32_t nweights, double k1, const uint32_t* d_q_id, uint64_t q_cap, const uint64_t* d_q_off,
                           uint32_t nq, uint32_t topk, uint32_t form, uint32_t* d_res_doc, uint64_t* d_res_score,
                           uint32_t* d_res_n, void* d_work, hipStream_t stream, KernelTimer* timer);

// One-workgroup path for small batches (k_small): the text and document offsets
// are read from `text`/`doc_off` (device or mapped pinned host memory; text
// readable 16 bytes past nbytes), the results written to `out`:
//   u32 header[kSmallHdr] (SM_*), u32 tok_start[kSmallBytes], u32 tok_end[kSmallBytes],
//   u64 doc_tok[ndocs + 1]
constexpr uint32_t kSmallBytes = 4096;  // 1024 threads x 4 bytes
constexpr uint32_t kSmallDocs = 4096;
constexpr uint32_t kSmallHdr = 32;
constexpr uint64_t kSmallOutBytes = 4ull * (kSmallHdr + 2ull * kSmallBytes) + 8ull * (kSmallDocs + 1ull);
enum { SM_NTOK = 0, SM_NTOKE, SM_ERR, SM_TIES, SM_BLOCKS, SM_ZHBLOCKS, SM_DONE, SM_CLK = 8 };  // SM_CLK..+10: phase clocks (10 ns ticks)
// A batch small enough to travel in the kernel arguments (text == nullptr): the
// kernel then reads it from the kernarg segment instead of host memory over PCIe.
constexpr uint32_t kSmallInline = 96;  // text bytes (zero-padded)
constexpr uint32_t kSmallInlineDocs = 7;
struct alignas(16) SmallInline {
    uint8_t txt[kSmallInline];
    uint16_t doff[kSmallInlineDocs + 1];  // document offsets, doff[ndocs] = nbytes
    uint32_t pad[4];
};
// out[SM_DONE] = seq is the kernel's last write (after a system-scope release).
hipError_t run_small(const DevImage& im, const uint8_t* text, uint32_t nbytes, const uint64_t* doc_off,
                     uint32_t ndocs, bool hmm, uint32_t* out, uint32_t seq, const SmallInline& in,
                     hipStream_t stream);

// After a pipeline run on `stream`: its counters (u32[CNT_CLEAR]) and the summed
// (blocks, zh blocks) of its tiles (two u64 after them) into `out`, mapped pinned
// host memory of kSnapWords u32, by a one-workgroup kernel.
constexpr uint32_t kSnapWords = CNT_CLEAR + 4;
// Zero `bytes` (a multiple of 4) at p with a kernel on `stream`.
// (and, in the same launch, bytes2 <= 1024 at p2)
hipError_t run_zero(void* p, uint64_t bytes, hipStream_t stream, void* p2 = nullptr, uint32_t bytes2 = 0);
hipError_t run_snap(const Work& w, uint64_t nbytes, uint32_t* out, hipStream_t stream);
// The spans of a pipeline run (ts/te, its counters' token count) packed for the host:
// pk[i] = gap from token i-1's end | length << kPackGapBits (u16), or 0xFFFF with
// (i, start, end) in the side list (counters[CNT_SIDE] entries, at most side_cap);
// hdr[b] = token b x kPackBlock - 1's end (0 for b = 0).  max_tokens bounds the count (the grid).
constexpr uint32_t kPackBlock = 4096;
constexpr uint32_t kPackGapBits = 6;
constexpr uint32_t kPackGapEsc = (1u << kPackGapBits) - 1u;         // gaps from here on are escaped
constexpr uint32_t kPackLenEsc = (1u << (16u - kPackGapBits)) - 1u;  // lengths from here on are escaped
// (an escaped gap covers >= 63 bytes, an escaped token >= 1,023: at most nbytes / 63 + nbytes / 1023 + 2)
inline uint32_t pack_side_cap(uint64_t nbytes) { return (uint32_t)(nbytes / kPackGapEsc + nbytes / kPackLenEsc + 4u); }
hipError_t run_span_pack(const uint32_t* ts, const uint32_t* te, uint32_t* counters, uint16_t* pk, uint32_t* hdr,
                         uint4* side, uint32_t side_cap, uint64_t max_tokens, hipStream_t stream);

// Resident k_zh waves per CU (occupancy API), 4-wave or wide workgroups.
uint32_t zh_waves_per_cu(bool hmm, bool wide);

}  // namespace jb
