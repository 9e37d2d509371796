// jb_device.cpp — device bring-up, the image's device copy, workspaces, the launch shape, the
// pipeline launch with its graph cache, and close (jb_device.h).
#include "jb_device.h"

#include <stdio.h>
#include <string.h>

#include <cmath>

void dfree(void* p) {
    if (p) (void)hipFree(p);
}
void hfree(void* p) {
    if (p) (void)hipHostFree(p);
}

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

// ---------------------------------------------------------------------------
// devices
// ---------------------------------------------------------------------------
template <class T>
static int upload(T** dst, const std::vector<T>& src) {
    *dst = nullptr;
    HIPCHK(hipMalloc(dst, std::max<size_t>(src.size(), 1) * sizeof(T)));
    if (!src.empty()) HIPCHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return JB_OK;
}

void free_image_bufs(ImageBufs* b) {
    dfree(b->pagemap); dfree(b->emit); dfree(b->cells); dfree(b->code); dfree(b->wtab); dfree(b->l1row);
    dfree(b->hot);
    *b = ImageBufs{};
}

// Copy an image into fresh buffers on `ordinal` (nothing of the device's current image
// changes; on failure nothing is left allocated).
int stage_image(int ordinal, const Image& img, ImageBufs* b) {
    *b = ImageBufs{};
    HIPCHK(hipSetDevice(ordinal));
    // row-indexed level-1 table: code and level-1 cell of a rune in one 8-byte load
    std::vector<uint64_t> l1(img.code.size());
    for (size_t r = 0; r < l1.size(); r++) {
        const uint32_t cd = img.code[r];
        l1[r] = jb_l1row_make(cd, cd < img.cells.size() ? img.cells[cd] : 0ull);
    }
    // the weights behind one leading -Inf (DevImage::wtab1: record slots hold index + 1)
    std::vector<double> wt1(img.wtab.size() + 1);
    wt1[0] = -HUGE_VAL;
    std::copy(img.wtab.begin(), img.wtab.end(), wt1.begin() + 1);
    // hot level-1 rows (k_mark_walk keeps them in LDS)
    std::vector<uint64_t> hot(JB_HOT_SLOTS + JB_HOT_SLOTS / 4u, 0ull);
    build_hot_rows(img, hot.data(), reinterpret_cast<uint16_t*>(hot.data() + JB_HOT_SLOTS));
    int rc;
    if ((rc = upload(&b->pagemap, img.pagemap)) || (rc = upload(&b->emit, img.emit)) ||
        (rc = upload(&b->cells, img.cells)) || (rc = upload(&b->code, img.code)) ||
        (rc = upload(&b->wtab, wt1)) || (rc = upload(&b->l1row, l1)) || (rc = upload(&b->hot, hot))) {
        free_image_bufs(b);
        return rc;
    }
    return JB_OK;
}

// Make staged buffers the device's image (the old ones are freed).  The caller holds
// d->mu and nothing is queued on the device that reads the old image.
int install_image(Device* d, ImageBufs* b, const Image& img) {
    free_image_bufs(&d->ib);
    d->ib = *b;
    *b = ImageBufs{};
    d->dim.l1row = d->ib.l1row;
    d->dim.hot = d->ib.hot;
    d->dim.pagemap = d->ib.pagemap;
    d->dim.emit = d->ib.emit;
    d->dim.cells = d->ib.cells;
    d->dim.code = d->ib.code;
    d->dim.wtab1 = d->ib.wtab;
    d->dim.wtab = d->ib.wtab + 1;
    d->dim.nrows = img.nrows;
    d->dim.nw1 = (uint32_t)std::min<size_t>(img.wtab.size() + 1, 0xFFFFFFFFu);
    d->dim.plainw = 1u;
    for (double w : img.wtab)
        if (std::isnan(w) || w == HUGE_VAL) d->dim.plainw = 0u;  // (a dictionary size <= 0)
    d->maxlen = std::max<uint32_t>(img.maxlen, 1u);
    // a captured pipeline holds the old image pointers in its kernel arguments
    d->drop_graphs();
    return JB_OK;
}

static void free_work(Work* w) {
    dfree(w->docbits); dfree(w->tile_cnt);
    dfree(w->ttile_cnt); dfree(w->supt); dfree(w->alnum16); dfree(w->erec); dfree(w->lanemask);
    dfree(w->gbl); dfree(w->lsegb); dfree(w->lmap); dfree(w->lcx); dfree(w->lpath); dfree(w->lflag); dfree(w->lbp); dfree(w->gbest); dfree(w->tile4); dfree(w->longblk);
    dfree(w->tok_start); dfree(w->tok_end); dfree(w->doc_tok); dfree(w->counters); dfree(w->dbg); dfree(w->dbg_walk);
    *w = Work{};
}

// Grow-only workspace for nbytes of text and ndocs documents.
int ensure_work(Device* d, uint64_t nbytes, uint32_t ndocs) {
    Work& w = d->w;
    if (nbytes <= w.cap_bytes && ndocs <= w.cap_docs && w.counters) return JB_OK;
    const uint64_t nb = std::max<uint64_t>(std::max(nbytes, w.cap_bytes), 4096);
    const uint32_t ndc = std::max(std::max(ndocs, w.cap_docs), 1024u);
    free_work(&w);
    d->drop_graphs();
    d->work_gen++;
    const uint64_t nwords = (nb + 31) / 32 + 8;
    const uint64_t ntiles = (nb + kTileBytes - 1) / kTileBytes + 1;
    const uint64_t nttiles = (nwords + kTokTileWords - 1) / kTokTileWords + 1;
    // docbits, sbits, ebits back to back so one memset clears all three
    HIPCHK(hipMalloc(&w.docbits, 3 * nwords * 4));
    w.sbits = w.docbits + nwords;
    w.ebits = w.docbits + 2 * nwords;
    w.bits_stride = nwords;
    HIPCHK(hipMalloc(&w.tile_cnt, ntiles * sizeof(uint2)));
    HIPCHK(hipMalloc(&w.ttile_cnt, nttiles * sizeof(uint2)));
    HIPCHK(hipMalloc(&w.alnum16, (nb / 1024 + 8) * 8));
    HIPCHK(hipMalloc(&w.erec, (nb / 3 + 8 + kErecPad) * 8));
    HIPCHK(hipMalloc(&w.lanemask, ntiles * 256 * 4));
    HIPCHK(hipMalloc(&w.gbl, nb / 3 + 8 + 512));
    HIPCHK(hipMalloc(&w.lflag, (nb / kZhLongMin + 2) * 4));
    HIPCHK(hipMalloc(&w.lsegb, (nb / kZhLongMin + 2) * 4));
    {
        const uint64_t nchunk = (nb / (3 * kSeg) + nb / kZhLongMin + 4) / kSeg + 2;  // 64-segment chunks
        HIPCHK(hipMalloc(&w.lmap, nchunk * 256));
        HIPCHK(hipMalloc(&w.lcx, nchunk));
        HIPCHK(hipMalloc(&w.lpath, nchunk * kSeg * sizeof(uint64_t)));  // per segment
    }
    HIPCHK(hipMalloc(&w.lbp, nb / 3 + 256));
    HIPCHK(hipMalloc(&w.tile4, ntiles * 4));
    HIPCHK(hipMalloc(&w.longblk, (nb / kZhLongMin + 2) * sizeof(uint2)));
    HIPCHK(hipMalloc(&w.gbest, (nb / 3 + 8) * sizeof(double)));

    HIPCHK(hipMalloc(&w.tok_start, (nb + 4) * 4));
    HIPCHK(hipMalloc(&w.tok_end, (nb + 4) * 4));
    HIPCHK(hipMalloc(&w.doc_tok, ((uint64_t)ndc + 2) * 8));
    HIPCHK(hipMalloc(&w.counters, 64 * 4));
    HIPCHK(hipMalloc(&w.supt, (nttiles / 256 + 2) * sizeof(uint2)));
    if (d->lc.diag & 0x100u) {
        HIPCHK(hipMalloc(&w.dbg, 65536 * 16 * 8));
        HIPCHK(hipMalloc(&w.dbg_walk, ntiles * 4 * 8 * 8));
        HIPCHK(hipMemset(w.dbg_walk, 0, ntiles * 4 * 8 * 8));
    }
    w.cap_bytes = nb;
    w.cap_docs = ndc;
    d->docbits_dirty = true;
    return JB_OK;
}

static void free_search(Device* d) {
    SearchOut& so = d->srch;
    dfree(so.start); dfree(so.end); dfree(so.doc_tok); dfree(so.off); dfree(so.tile); dfree(so.sup);
    so = SearchOut{};
    dfree(d->full_tbase);
    d->full_tbase = nullptr;
}

// The search pass's buffers, sized like the workspace's spans (after ensure_work).  A context
// that never cuts in search mode never gets here.
static int ensure_search(Device* d) {
    SearchOut& so = d->srch;
    if (so.off && d->srch_gen == d->work_gen) return JB_OK;
    free_search(d);
    const uint64_t nb = d->w.cap_bytes, ntt = srch_tiles(nb);
    HIPCHK(hipMalloc(&so.start, (nb + 4) * 4));
    HIPCHK(hipMalloc(&so.end, (nb + 4) * 4));
    HIPCHK(hipMalloc(&so.doc_tok, ((uint64_t)d->w.cap_docs + 2) * 8));
    HIPCHK(hipMalloc(&so.off, (nb + 4) * 4));
    HIPCHK(hipMalloc(&so.tile, (ntt + 1) * sizeof(uint2)));
    HIPCHK(hipMalloc(&so.sup, (ntt / 256 + 2) * sizeof(uint2)));
    so.ntok = reinterpret_cast<uint64_t*>(d->w.counters + CNT_NSRCH);
    d->srch_gen = d->work_gen;
    return JB_OK;
}

// Full mode's buffers: search mode's (the ctx-owned spans, nbytes entries, and the workspace: an
// 8-byte tile sum either way), and the per-tile bases.
static int ensure_full(Device* d) {
    int rc;
    if ((rc = ensure_search(d))) return rc;
    if (d->full_tbase && d->full_gen == d->work_gen) return JB_OK;
    dfree(d->full_tbase);
    d->full_tbase = nullptr;
    HIPCHK(hipMalloc(&d->full_tbase, (srch_tiles(d->w.cap_bytes) + 1) * 8));
    d->full_gen = d->work_gen;
    return JB_OK;
}
static_assert(sizeof(uint2) == sizeof(uint64_t), "full mode keeps 64-bit sums in search mode's tile arrays");
// The pass's arguments with the ctx-owned outputs (cap = the workspace's bytes).
static FullOut full_out(const Device* d) {
    const SearchOut& so = d->srch;
    return FullOut{so.start, so.end, d->w.cap_bytes, so.doc_tok, so.ntok, so.off,
                   reinterpret_cast<uint64_t*>(so.tile), reinterpret_cast<uint64_t*>(so.sup), d->full_tbase, d->maxlen};
}

int ensure_mode(Device* d, CutMode mode) {
    return mode == kModeFull ? ensure_full(d) : mode == kModeSearch ? ensure_search(d) : JB_OK;
}

SpanTarget span_target(const Device* d, CutMode mode, const SpanDst* dst, uint64_t own_cap) {
    const SearchOut& own = d->srch;  // (search and full mode: the plain spans stay in the workspace)
    SpanTarget t{d->w, PostOut{mode, own, mode == kModeFull ? full_out(d) : FullOut{}},
                 mode == kModePlain ? SpanDst{d->w.tok_start, d->w.tok_end, 0, d->w.doc_tok,
                                              reinterpret_cast<uint64_t*>(d->w.counters + CNT_NWORDS)}
                                    : SpanDst{own.start, own.end, own_cap, own.doc_tok, own.ntok}};
    SpanDst& at = t.at;
    if (dst) {  // (a plain run's count stays in the workspace)
        uint64_t* const ntok = dst->ntok && mode != kModePlain ? dst->ntok : at.ntok;
        at = SpanDst{dst->start, dst->end, dst->cap, dst->doc_tok, ntok};
    }
    if (mode == kModePlain) {
        t.w.tok_start = at.start, t.w.tok_end = at.end, t.w.doc_tok = at.doc_tok;
    } else if (mode == kModeSearch) {
        SearchOut& so = t.po.so;
        so.start = at.start, so.end = at.end, so.doc_tok = at.doc_tok, so.ntok = at.ntok;
    } else {
        FullOut& fo = t.po.fo;
        fo.start = at.start, fo.end = at.end, fo.cap = at.cap, fo.doc_tok = at.doc_tok, fo.ntok = at.ntok;
    }
    return t;
}

static void free_outs(Device* d) {
    for (auto& o : d->outs) {
        dfree(o.ts); dfree(o.te); dfree(o.dt); hfree(o.hs); hfree(o.hdt);
        dfree(o.pk); dfree(o.phdr); dfree(o.pside); hfree(o.hpk); hfree(o.hhdr); hfree(o.hside);
        o = Device::OutSet{};
    }
}

static const uint64_t kMaxPiece = 1ull << 30;  // (a piece of several documents; device offsets are u32)

// The launch shape of a device, fixed at jb_open.  Tuning knobs come from the
// environment once, here (results do not depend on them):
//   JB_GRID_ZH   k_zh workgroups (default: resident workgroups per CU x CUs)
//   JB_ZH_GROUP  k_zh group bytes, a multiple of 32 in [kZhGroupSmall, kZhGroupBytes]
//                (default: by batch size, zh_group_for)
//   JB_PIECE_KIB host batches are cut in pieces of whole documents of at most this many KiB
//                (default 65536), pipelined over three streams (cut_range)
//   JB_SMALL     host batches up to this many bytes take k_small (0: never)
//   JB_STAMPS    (STAMPS=1 builds only) per-wave phase clocks to stderr
//   JB_DF_COMBINE jb_df_device's kernel: 1 k_df_combine (default), 0 k_df
//   JB_TR_WINDOW jb_textrank_device's push kernel: 1 k_tr_push_win (default), 0 k_tr_push
//   JB_JOIN_STAGE jb_join_device's write kernel: 0 the plain form (default), 1 the staged form
//   JB_WC_COMBINE jb_wc_add_device's count pass: 0 one global atomic per token, 1 combined in LDS (default)
//   JB_WC_HASHBITS the word-count fingerprint's width, 1 .. 64 (default 64; fewer to test collisions)
//   JB_MH_FORM   jb_minhash_device's signature kernel: 0 the plain form, 1 the staged form (default)
//   JB_POSTINGS_FORM jb_postings_device's scatter kernel: 0 from the lanes (default), 1 through LDS in runs
//   JB_BM25_FORM jb_bm25_search_device: 0 a dense row per query and global atomics, 1 a tile's scores in LDS (default)
//   JB_COLLOC_COMBINE jb_colloc_add_device's count pass: 0 one global atomic per pair and per unigram, 1 combined in
//                 LDS (default)
static int init_launch_cfg(Device* d) {
    LaunchCfg& lc = d->lc;
    lc.zh_waves = d->ncu * std::max(zh_waves_per_cu(true, false), zh_waves_per_cu(false, false));
    lc.zh_waves_wide = d->ncu * std::max(zh_waves_per_cu(true, true), zh_waves_per_cu(false, true));
    const int gz = env_int("JB_GRID_ZH", 0);  // (in 4-wave workgroups)
    if (gz > 0) lc.zh_waves = lc.zh_waves_wide = 4u * (uint32_t)gz;
    const int wide = env_int("JB_ZH_WIDE", -1);
    if (wide < -1 || wide > 1) return fail(JB_EINVAL, "JB_ZH_WIDE=%d: want -1 (by batch size), 0 or 1", wide);
    lc.zh_wide = wide;
    const int mws = env_int("JB_MW_SPLIT", -1);
    if (mws < -1 || mws > 3) return fail(JB_EINVAL, "JB_MW_SPLIT=%d: want -1 (by tile count) or 0-3", mws);
    lc.mw_split = mws;
    const int grp = env_int("JB_ZH_GROUP", 0);
    if (grp != 0) {
        if (grp < 256 || grp > (int)kZhGroupBytes || grp % 32 != 0)
            return fail(JB_EINVAL, "JB_ZH_GROUP=%d: want a multiple of 32 in [256, %u]", grp, kZhGroupBytes);
        lc.zh_group = (uint32_t)grp;
    }
    const int zt = env_int("JB_ZH_TAIL_KIB", 0), ztg = env_int("JB_ZH_TAIL_GROUP", 1024);
    if (zt < 0 || zt > (1 << 20) || ztg < (int)kZhGroupSmall || ztg > (int)kZhGroupBytes || ztg % 32 != 0)
        return fail(JB_EINVAL, "JB_ZH_TAIL_KIB=%d / JB_ZH_TAIL_GROUP=%d: want 0 .. 1048576 KiB, a multiple of 32 "
                    "in [%u, %u] bytes", zt, ztg, kZhGroupSmall, kZhGroupBytes);
    lc.zh_tail = (uint32_t)zt << 10;
    lc.zh_tail_group = (uint32_t)ztg;
#if JB_STAMPS
    lc.diag = (uint32_t)env_int("JB_STAMPS", 0) ? 0x100u : 0u;
#endif
    const int pk = env_int("JB_PIECE_KIB", 64 << 10);  // host-batch pipeline piece (KiB of whole documents)
    if (pk < 1 || (uint64_t)pk > kMaxPiece / 1024)
        return fail(JB_EINVAL, "JB_PIECE_KIB=%d: want 1 .. %llu", pk, (unsigned long long)(kMaxPiece / 1024));
    d->piece_bytes = (uint64_t)pk << 10;
    const int sm = env_int("JB_SMALL", (int)kSmallBytes);
    if (sm < 0 || sm > (int)kSmallBytes)
        return fail(JB_EINVAL, "JB_SMALL=%d: want 0 (off) .. %u bytes", sm, kSmallBytes);
    lc.small_max = (uint32_t)sm;
    const int ls = env_int("JB_LONG_SPEC", 1);
    if (ls < 0 || ls > 3) return fail(JB_EINVAL, "JB_LONG_SPEC=%d: want 0, 1, 3 (or 2: testing)", ls);
    lc.long_spec = (uint32_t)ls;
    const int lf = env_int("JB_LONG_FUSED", 1);
    if (lf < 0 || lf > 1) return fail(JB_EINVAL, "JB_LONG_FUSED=%d: want 0 or 1", lf);
    lc.long_fused = (uint32_t)lf;
    lc.ncu = std::max(1u, d->ncu);
    const int t1 = env_int("JB_TOK1", 1);
    if (t1 < 0 || t1 > 1) return fail(JB_EINVAL, "JB_TOK1=%d: want 0 or 1", t1);
    lc.tok1 = (uint32_t)t1;
    const int nzm = env_int("JB_NZ_FUSE_MIB", 4);
    if (nzm < 0 || nzm > 1024) return fail(JB_EINVAL, "JB_NZ_FUSE_MIB=%d: want 0 .. 1024", nzm);
    lc.nz_fuse_mib = (uint32_t)nzm;
    const int sp = env_int("JB_SPAN_PACK", 1);
    if (sp < 0 || sp > 1) return fail(JB_EINVAL, "JB_SPAN_PACK=%d: want 0 or 1", sp);
    d->span_pack = sp != 0;
    // k_long's phase waits give up after this long without progress (100 MHz ticks)
    const int lw = env_int("JB_LONG_WAIT_US", 20000000);
    if (lw < 1 || lw > 40000000) return fail(JB_EINVAL, "JB_LONG_WAIT_US=%d: want 1 .. 40000000", lw);
    lc.long_wait_ticks = (uint32_t)lw * 100u;
    const int ss = env_int("JB_SMALL_SLOTS", 4);
    if (ss < 1 || ss > 8) return fail(JB_EINVAL, "JB_SMALL_SLOTS=%d: want 1 .. 8", ss);
    d->small_slots = (uint32_t)ss;
    const int dc = env_int("JB_DF_COMBINE", 1);
    if (dc < 0 || dc > 1) return fail(JB_EINVAL, "JB_DF_COMBINE=%d: want 0 or 1", dc);
    lc.df_combine = (uint32_t)dc;
    const int tw = env_int("JB_TR_WINDOW", 1);
    if (tw < 0 || tw > 1) return fail(JB_EINVAL, "JB_TR_WINDOW=%d: want 0 or 1", tw);
    lc.tr_window = (uint32_t)tw;
    const int js = env_int("JB_JOIN_STAGE", 0);
    if (js < 0 || js > 1) return fail(JB_EINVAL, "JB_JOIN_STAGE=%d: want 0 or 1", js);
    lc.join_stage = (uint32_t)js;
    const int wcc = env_int("JB_WC_COMBINE", 1);
    if (wcc < 0 || wcc > 1) return fail(JB_EINVAL, "JB_WC_COMBINE=%d: want 0 or 1", wcc);
    lc.wc_combine = (uint32_t)wcc;
    const int wcb = env_int("JB_WC_HASHBITS", 64);
    if (wcb < 1 || wcb > 64) return fail(JB_EINVAL, "JB_WC_HASHBITS=%d: want 1 .. 64", wcb);
    lc.wc_bits = (uint32_t)wcb;
    const int mhf = env_int("JB_MH_FORM", 1);
    if (mhf < 0 || mhf > 1) return fail(JB_EINVAL, "JB_MH_FORM=%d: want 0 or 1", mhf);
    lc.mh_form = (uint32_t)mhf;
    const int pf = env_int("JB_POSTINGS_FORM", 0);
    if (pf < 0 || pf > 1) return fail(JB_EINVAL, "JB_POSTINGS_FORM=%d: want 0 or 1", pf);
    lc.post_form = (uint32_t)pf;
    const int bf = env_int("JB_BM25_FORM", 1);
    if (bf < 0 || bf > 1) return fail(JB_EINVAL, "JB_BM25_FORM=%d: want 0 or 1", bf);
    lc.bm25_form = (uint32_t)bf;
    const int clc = env_int("JB_COLLOC_COMBINE", 1);
    if (clc < 0 || clc > 1) return fail(JB_EINVAL, "JB_COLLOC_COMBINE=%d: want 0 or 1", clc);
    lc.colloc_combine = (uint32_t)clc;
    return JB_OK;
}

// Diagnostic (STAMPS builds, JB_STAMPS=1): the per-wave clocks the last pipeline's kernels left in the
// workspace, summed and printed to stderr.
static int dump_stamps(Device* d, uint64_t nbytes, hipStream_t s) {
    const LaunchCfg& lc = d->lc;
    const uint32_t nwv = std::min<uint32_t>(std::max(lc.zh_waves, lc.zh_waves_wide), 16384u);
    std::vector<uint64_t> st((size_t)nwv * 16);
    HIPCHK(hipMemcpyAsync(st.data(), d->w.dbg, st.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double a[16] = {0};
    double n = 0;
    for (uint32_t i = 0; i < nwv; i++)
        if (st[i * 16 + 3]) {
            for (int k = 0; k < 16; k++) a[k] += (double)st[i * 16 + k];
            n++;
        }
    if (n == 0) n = 1;
    {  // the grid's tail: every wave starts with the kernel, so the spread of their totals is idle time
        std::vector<uint64_t> tot;
        for (uint32_t i = 0; i < nwv; i++)
            if (st[i * 16 + 3]) tot.push_back(st[i * 16 + 6]);
        if (!tot.empty()) {
            std::sort(tot.begin(), tot.end());
            fprintf(stderr, "[jb] k_zh wave totals: min %llu p10 %llu median %llu max %llu (waves %zu)\n",
                    (unsigned long long)tot.front(), (unsigned long long)tot[tot.size() / 10],
                    (unsigned long long)tot[tot.size() / 2], (unsigned long long)tot.back(), tot.size());
        }
    }
    fprintf(stderr, "[jb] k_zh clocks/wave: setup %.0f dp %.0f fwd walk %.0f viterbi fwd %.0f back+flush+rest %.0f "
                    "total %.0f; chunks/wave %.1f; lane DP steps %.0f vs 64*max %.0f (DP lane use %.2f); blocks past "
                    "the window per chunk %.3f; Viterbi lane use %.2f (longest lane %.1f runes per chunk)\n",
            a[0] / n, a[1] / n, a[8] / n, a[9] / n, a[2] / n, a[6] / n, a[3] / n, a[4] / n, 64.0 * a[5] / n,
            a[4] / (64.0 * a[5] + 1e-9), a[7] / (a[3] + 1e-9), a[10] / (64.0 * a[11] + 1e-9), a[11] / (a[3] + 1e-9));
    fprintf(stderr, "[jb] k_zh Viterbi forward half per chunk: longest lane %.2f runes, longest single run %.2f, "
                    "the wave's runes split evenly %.2f\n",
            a[11] / (a[3] + 1e-9), a[12] / (a[3] + 1e-9), a[13] / (a[3] + 1e-9));
    fprintf(stderr, "[jb] k_zh DP per chunk: longest lane %.2f runes, longest single block %.2f, the wave's runes "
                    "split evenly %.2f\n",
            a[5] / (a[3] + 1e-9), a[14] / (a[3] + 1e-9), a[4] / (64.0 * (a[3] + 1e-9)));
    HIPCHK(hipMemsetAsync(d->w.dbg, 0, (size_t)nwv * 128, s));
    const uint64_t nww = (nbytes + kTileBytes - 1) / kTileBytes * 4;
    std::vector<uint64_t> sw(nww * 8);
    HIPCHK(hipMemcpyAsync(sw.data(), d->w.dbg_walk, sw.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double b[8] = {0, 0, 0, 0, 0, 0, 0, 0}, m = 0;
    for (uint64_t i = 0; i < nww; i++)
        if (sw[i * 8 + 5] == 1) {
            for (int k = 0; k < 8; k++) b[k] += (double)sw[i * 8 + k];
            m++;
        }
    if (m == 0) m = 1;
    fprintf(stderr, "[jb] k_mark_walk clocks/wave: mark %.0f (staging %.0f) entries %.0f (loads %.0f) walk %.0f "
                    "tail %.0f; trips/wave %.2f\n",
            b[0] / m, b[6] / m, b[1] / m, b[7] / m, b[2] / m, b[3] / m, b[4] / m);
    std::vector<uint64_t> sl(64 * 32);
    HIPCHK(hipMemcpyAsync(sl.data(), d->w.dbg + 65536 * 4, sl.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < 64; i++) {  // per wave: run, barrier, windows, slow
        const uint64_t* o = sl.data() + i * 16;
        if (o[2])
            fprintf(stderr, "[jb] k_long_dp wg %d: chain run %llu bar %llu windows %llu slow %llu | "
                            "wave 1 run %llu bar %llu | wave 2 run %llu bar %llu (%llu) | wave 3 run %llu bar %llu\n", i,
                    (unsigned long long)o[0], (unsigned long long)o[1], (unsigned long long)o[2],
                    (unsigned long long)o[3], (unsigned long long)o[4], (unsigned long long)o[5],
                    (unsigned long long)o[8], (unsigned long long)o[9], (unsigned long long)o[11],
                    (unsigned long long)o[12], (unsigned long long)o[13]);
        const uint64_t* p = sl.data() + 64 * 16 + i * 16;
        if (o[2])
            fprintf(stderr, "[jb] k_long_dp wg %d sub-phases: w0 %llu %llu %llu %llu | w1 %llu %llu %llu %llu | "
                            "w2 %llu %llu %llu %llu | w3 %llu %llu %llu %llu\n", i,
                    (unsigned long long)p[0], (unsigned long long)p[1], (unsigned long long)p[2],
                    (unsigned long long)p[3], (unsigned long long)p[4], (unsigned long long)p[5],
                    (unsigned long long)p[6], (unsigned long long)p[7], (unsigned long long)p[8],
                    (unsigned long long)p[9], (unsigned long long)p[10], (unsigned long long)p[11],
                    (unsigned long long)p[12], (unsigned long long)p[13], (unsigned long long)p[14],
                    (unsigned long long)p[15]);
    }
    HIPCHK(hipMemsetAsync(d->w.dbg + 65536 * 4, 0, sl.size() * 8, s));
    if (const char* wo = getenv("JB_LDW_OUT")) {  // k_long_dp per-window records of block 0
        std::vector<uint64_t> wr(65536 * 2 * 4);
        HIPCHK(hipMemcpyAsync(wr.data(), d->w.dbg + 65536 * 8, wr.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (FILE* f = fopen(wo, "wb")) {
            fwrite(wr.data(), 8, wr.size(), f);
            fclose(f);
        }
        HIPCHK(hipMemsetAsync(d->w.dbg + 65536 * 8, 0, wr.size() * 8, s));
    }
    return JB_OK;
}

static int launch_pipeline_(Device* d, const Work& w, const uint8_t* d_text, uint64_t nbytes,
                            const uint64_t* d_doc_off, uint32_t ndocs, bool hmm, hipStream_t s, const MaskOut* mask,
                            const PostOut* po);
static int launch_pipeline(Device* d, const Work& w, const uint8_t* d_text, uint64_t nbytes,
                           const uint64_t* d_doc_off, uint32_t ndocs, bool hmm, hipStream_t s, const MaskOut* mask,
                           const PostOut* po) {
    if (d->docbits_dirty) {  // the whole bitmap, once (see Device::docbits_dirty)
        HIPCHK(run_zero(w.docbits, w.bits_stride * 4, s));
        d->docbits_dirty = false;
    }
    const int rc = launch_pipeline_(d, w, d_text, nbytes, d_doc_off, ndocs, hmm, s, mask, po);
    if (rc) d->docbits_dirty = true;
    return rc;
}
// po != nullptr: search or full mode, the mode's pass (run_search, run_full) follows the pipeline's kernels
static int launch_pipeline_(Device* d, const Work& w, const uint8_t* d_text, uint64_t nbytes,
                            const uint64_t* d_doc_off, uint32_t ndocs, bool hmm, hipStream_t s, const MaskOut* mask,
                            const PostOut* po) {
    const SearchOut* const so = po && po->mode == kModeSearch ? &po->so : nullptr;
    const FullOut* const fo = po && po->mode == kModeFull ? &po->fo : nullptr;
    static const bool dbg = getenv("JB_DEBUG") != nullptr;
    const LaunchCfg& lc = d->lc;
    d->last_nbytes = nbytes;
    {
        std::lock_guard<std::mutex> g(d->stats_mu);
        d->last_small = false;
    }
    if (dbg)
        fprintf(stderr, "[jb] nbytes=%llu ndocs=%u zh_waves=%u/%u wide=%d zh_group=%u\n", (unsigned long long)nbytes,
                ndocs, lc.zh_waves, lc.zh_waves_wide, lc.zh_wide, lc.zh_group ? lc.zh_group : zh_group_for(nbytes));
    static const bool use_graph = env_int("JB_GRAPH", 1) != 0;
    auto run = [&](KernelTimer* tm) {  // the pipeline's kernels, then search or full mode's
        hipError_t e = run_pipeline(d->dim, w, d_text, nbytes, d_doc_off, ndocs, hmm, lc, s, tm, mask);
        if (e == hipSuccess && so) e = run_search(d->dim, w, *so, d_text, nbytes, ndocs, s, tm);
        if (e == hipSuccess && fo) e = run_full(d->dim, w, *fo, d_text, nbytes, ndocs, s, tm);
        return e;
    };
    if (use_graph && !d->profile && lc.diag == 0 && s != nullptr && !mask) {
        const Device::GraphKey key{d_text, nbytes, d_doc_off, ndocs, hmm, d->work_gen, s, w.tok_start, w.tok_end,
                                   w.doc_tok, po ? (int)po->mode : (int)kModePlain,
                                   so ? so->start : (fo ? fo->start : nullptr), so ? so->end : (fo ? fo->end : nullptr),
                                   so ? (const void*)so->doc_tok : (fo ? (const void*)fo->doc_tok : nullptr),
                                   so ? (const void*)so->ntok : (fo ? (const void*)fo->ntok : nullptr),
                                   fo ? fo->cap : 0ull};
        Device::GraphSlot& slot = d->graphs[key.mode];  // (each mode has its own)
        hipGraphExec_t& gexec = slot.exec;
        const bool repeat = slot.gen != 0 && key == slot.key;
        if (!repeat) {  // first call with this key: run directly, capture if it comes again
            if (gexec) (void)hipGraphExecDestroy(gexec);
            gexec = nullptr;
            slot.key = key;
            slot.gen = 1;
            const hipError_t e = run(nullptr);
            if (e != hipSuccess) return fail(JB_EDEVICE, "pipeline launch: %s", hipGetErrorString(e));
            return JB_OK;
        }
        if (!gexec) {
            hipGraph_t g = nullptr;
            HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            const hipError_t ec = run(nullptr);
            const hipError_t ee = hipStreamEndCapture(s, &g);
            if (ec != hipSuccess) return fail(JB_EDEVICE, "pipeline capture: %s", hipGetErrorString(ec));
            if (ee != hipSuccess) return fail(JB_EDEVICE, "pipeline capture end: %s", hipGetErrorString(ee));
            const hipError_t ei = hipGraphInstantiate(&gexec, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ei != hipSuccess) {
                gexec = nullptr;
                return fail(JB_EDEVICE, "pipeline graph instantiate: %s", hipGetErrorString(ei));
            }
        }
        const hipError_t el = hipGraphLaunch(gexec, s);
        if (el != hipSuccess) return fail(JB_EDEVICE, "pipeline graph launch: %s", hipGetErrorString(el));
        return JB_OK;
    }
    const hipError_t e = run(d->profile ? &d->timer : nullptr);
    if (e != hipSuccess) return fail(JB_EDEVICE, "pipeline launch: %s", hipGetErrorString(e));
    if ((lc.diag & 0x100u) && d->w.dbg) return dump_stamps(d, nbytes, s);
    return JB_OK;
}

// Queue the pipeline on stream s.  The workspace is one per device: a pipeline waits
// for the previous one (on whatever stream it ran) before it starts.  `w` is the
// device's workspace, or a copy with caller-owned outputs (jb_cut_device_into).
int launch(Device* d, const Work& w, const uint8_t* d_text, uint64_t nbytes, const uint64_t* d_doc_off,
           uint32_t ndocs, bool hmm, hipStream_t s, const MaskOut* mask, const PostOut* po) {
    if (!d->ws_done) HIPCHK(hipEventCreateWithFlags(&d->ws_done, hipEventDisableTiming));
    else HIPCHK(hipStreamWaitEvent(s, d->ws_done, 0));  // (free on the stream that recorded it)
    int rc = launch_pipeline(d, w, d_text, nbytes, d_doc_off, ndocs, hmm, s, mask, po);
    if (rc) return rc;
    HIPCHK(hipEventRecord(d->ws_done, s));
    {
        std::lock_guard<std::mutex> g(d->stats_mu);
        d->has_stats = true;
    }
    d->acc_valid = false;
    return JB_OK;
}

// Streams, image and launch shape of one device of a new ctx.
int open_device(Device* d, int ordinal, const Image& img) {
    d->ordinal = ordinal;
    int rc;
    HIPCHK(hipSetDevice(d->ordinal));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, d->ordinal));
    d->ncu = (uint32_t)prop.multiProcessorCount;
    HIPCHK(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&d->cstream, hipStreamNonBlocking));
    HIPCHK(hipHostMalloc(&d->h_zero, 64, hipHostMallocDefault));
    memset(d->h_zero, 0, 64);
    HIPCHK(hipStreamCreateWithFlags(&d->dstream, hipStreamNonBlocking));
    ImageBufs b;
    if ((rc = stage_image(d->ordinal, img, &b))) return rc;
    if ((rc = install_image(d, &b, img))) return rc;
    if ((rc = init_launch_cfg(d))) return rc;  // (sets small_slots)
    {
        // k_small runs one workgroup per batch, one stream per slot.  With JB_SMALL_CUMASK=1
        // (round 4's default) each slot's stream is masked to one CU (JB_SMALL_CU + slot x
        // JB_SMALL_CU_STRIDE), so that its batch finds the trie's hot lines in that XCD's L2;
        // round 5 measured plain streams faster (the sentence 21.8-22.2 -> 20.0-21.0 us per
        // call; concurrent calls the same at 4 slots and better at 8), so they are the default
        const int cu = env_int("JB_SMALL_CU", 0), cs = env_int("JB_SMALL_CU_STRIDE", 1);
        const int last = cu + ((int)d->small_slots - 1) * cs;  // (only the slots in use get a stream)
        if (cu < 0 || cs < 0 || last >= (int)d->ncu)
            return fail(JB_EINVAL,
                        "JB_SMALL_CU=%d, JB_SMALL_CU_STRIDE=%d, JB_SMALL_SLOTS=%u: slot k runs on CU "
                        "JB_SMALL_CU + k x JB_SMALL_CU_STRIDE, and the last one (%d) is past the device's %u CUs",
                        cu, cs, d->small_slots, last, d->ncu);
        const bool masked = env_int("JB_SMALL_CUMASK", 0) != 0;
        for (int k = 0; k < (int)d->small_slots; k++) {
            std::vector<uint32_t> mask((d->ncu + 31) / 32, 0u);
            const int c = cu + k * cs;
            mask[c / 32] = 1u << (c % 32);
            if (masked) HIPCHK(hipExtStreamCreateWithCUMask(&d->slots[k].st, (uint32_t)mask.size(), mask.data()));
            else HIPCHK(hipStreamCreateWithFlags(&d->slots[k].st, hipStreamNonBlocking));
        }
    }
    return JB_OK;
}

void close_device(Device* d) {
        if (const char* tp = getenv("JB_SMALL_TRACE"); tp && !d->small_trace.empty())
            if (FILE* f = fopen(tp, "a")) {
                for (const auto& r : d->small_trace)
                    fprintf(f, "%g %g %.3f %.3f %.3f %.3f\n", r[0], r[1], r[2], r[3], r[4], r[5]);
                fclose(f);
            }
        (void)hipSetDevice(d->ordinal);
        (void)hipStreamSynchronize(d->stream);
        for (auto& sl : d->slots)
            if (sl.st) (void)hipStreamSynchronize(sl.st);
        d->timer.reset();
        // a jb_cut_device pipeline queued on a caller's stream may still use the workspace:
        // wait for its completion event before freeing anything (the caller's stream may be
        // gone by now, the event is ours)
        if (d->ws_done) (void)hipEventSynchronize(d->ws_done);
        d->drop_graphs();
        free_work(&d->w);
        free_search(d);
        dfree(d->text); dfree(d->doc_off);
        free_image_bufs(&d->ib);
        if (d->ws_done) (void)hipEventDestroy(d->ws_done);
        hfree(d->h_text); hfree(d->h_misc);
        for (auto& sl : d->slots) {
            hfree(sl.h_sin);
            hfree(sl.h_sout[0]);
            hfree(sl.h_sout[1]);
        }
        free_outs(d);
        hfree(d->h_pcnt); dfree(d->d_mask); hfree(d->h_mask); hfree(d->h_zero);
        for (auto* v : {&d->ev_h2d, &d->ev_comp, &d->ev_d2h})
            for (hipEvent_t e : *v) (void)hipEventDestroy(e);
        if (d->cstream) (void)hipStreamDestroy(d->cstream);
        if (d->dstream) (void)hipStreamDestroy(d->dstream);
        (void)hipStreamDestroy(d->stream);
        for (auto& sl : d->slots)
            if (sl.st) (void)hipStreamDestroy(sl.st);
}
