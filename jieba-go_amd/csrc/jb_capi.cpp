// jb_capi.cpp — the C ABI of libjiebahip.so (include/jiebahip.h): the entry points.
//
// Argument checks, the context's lock, and one call into the layers below: the image builder
// (jb_image.cpp), the devices (jb_device.cpp), host batches (jb_small.cpp, jb_hostbatch.cpp) and
// the kernels' launch interface (jb_kernels.h).  The planners' entry points are in jb_plan.cpp,
// jb_last_error in jb_err.cpp, the host-text analytics calls (jb_*_batch, jb_cut_batch_join and its
// like) in jb_batch.cpp.  No segmentation happens on the CPU: without a usable HIP device
// every cut returns JB_EDEVICE.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <iterator>
#include <type_traits>

#include "jb_charspans.h"
#include "jb_host.h"
#include "jb_join.h"
#include "jb_textrank.h"
#include "jb_filter.h"
#include "jb_minhash.h"
#include "jb_neardup.h"
#include "jb_postings.h"
#include "jb_bm25.h"
#include "jb_colloc.h"
#include "jb_wc.h"

// ---------------------------------------------------------------------------
// image
// ---------------------------------------------------------------------------
static int read_file(const char* path, std::string* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return fail(JB_EIO, "open %s: %s", path, strerror(errno));
    std::string s;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    const bool err = ferror(f);
    fclose(f);
    if (err) return fail(JB_EIO, "read %s failed", path);
    *out = std::move(s);
    return JB_OK;
}

extern "C" int jb_image_build(const jb_config* cfg, jb_image** out) {
    if (!cfg || !out) return fail(JB_EINVAL, "jb_image_build: null argument");
    const int kind = cfg->dict_kind;
    if (kind != JB_DICT_TXT && kind != JB_DICT_PREFIX && kind != JB_DICT_GOB && kind != JB_DICT_IMAGE)
        return fail(JB_EINVAL, "unknown dict_kind %d", kind);
    std::string dbuf, ebuf;
    const char* d = cfg->dict_buf;
    size_t dl = cfg->dict_len;
    const char* e = cfg->emit_buf;
    size_t el = cfg->emit_len;
    int rc;
    if (cfg->dict_path) {
        if ((rc = read_file(cfg->dict_path, &dbuf))) return rc;
        d = dbuf.data();
        dl = dbuf.size();
    }
    if (!d && dl) return fail(JB_EINVAL, "no dictionary given");
    if (cfg->nlog && (!cfg->log_keys || !cfg->log_vals)) return fail(JB_EINVAL, "nlog > 0 without log_keys/log_vals");
    auto im = std::make_unique<jb_image>();
    im->dict_kind = kind;
    for (size_t i = 0; i < cfg->nlog; i++) im->dict.log_of[cfg->log_keys[i]] = cfg->log_vals[i];
    std::string err;
    if (kind == JB_DICT_IMAGE) {
        if ((rc = load_image(d ? d : "", dl, &im->dict, &im->emit, &im->img, &err))) return fail(rc, "%s", err.c_str());
        for (size_t i = 0; i < cfg->nlog; i++) im->dict.log_of[cfg->log_keys[i]] = cfg->log_vals[i];
        if ((cfg->size_override > 0 && cfg->size_override != im->dict.size) || cfg->nlog) {  // reweigh
            if (cfg->size_override > 0) im->dict.size = cfg->size_override;
            if (!reweigh_image(im->dict, &im->img) && (rc = build_image(im->dict, im->emit, &im->img, &err)))
                return fail(rc, "%s", err.c_str());
        }
        *out = im.release();
        return JB_OK;
    }
    if (cfg->emit_path) {
        if ((rc = read_file(cfg->emit_path, &ebuf))) return rc;
        e = ebuf.data();
        el = ebuf.size();
    }
    if (!e) return fail(JB_EINVAL, "no emission table given (prob_emit.json)");
    if (kind == JB_DICT_GOB) {
        // newJiebaPrefixDictionary (tokenizer.go:439-458): the gob map as stored, size hard-coded
        if ((rc = parse_gob_dictionary(d ? d : "", dl, &im->dict, &err))) return fail(rc, "%s", err.c_str());
        im->dict.size = JB_JIEBA_SIZE;
    } else if ((rc = parse_dictionary(d ? d : "", dl, kind, &im->dict, &err))) {
        return fail(rc, "%s", err.c_str());
    }
    if (cfg->size_override > 0) im->dict.size = cfg->size_override;
    if ((rc = parse_emission(e, el, &im->emit, &err))) return fail(rc, "%s", err.c_str());
    if ((rc = build_image(im->dict, im->emit, &im->img, &err))) return fail(rc, "%s", err.c_str());
    if (im->img.maxlen > 255) return fail(JB_ELIMIT, "dictionary word of %u runes (max 255)", im->img.maxlen);
    *out = im.release();
    return JB_OK;
}

static int write_file(const char* path, const std::string& data) {
    // write to a temporary name and rename, so a reader never sees half an image
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(JB_EIO, "create %s: %s", tmp.c_str(), strerror(errno));
    const bool ok = fwrite(data.data(), 1, data.size(), f) == data.size();
    if (fclose(f) != 0 || !ok) {
        remove(tmp.c_str());
        return fail(JB_EIO, "write %s failed", tmp.c_str());
    }
    if (rename(tmp.c_str(), path) != 0) {
        remove(tmp.c_str());
        return fail(JB_EIO, "rename to %s: %s", path, strerror(errno));
    }
    return JB_OK;
}

extern "C" int jb_image_save(const jb_image* img, const char* path) {
    if (!img || !path) return fail(JB_EINVAL, "jb_image_save: null argument");
    std::string data;
    save_image(img->dict, img->emit, img->img, &data);
    return write_file(path, data);
}

extern "C" int jb_image_dict_info(const jb_image* img, uint64_t* nentries, int64_t* size) {
    if (!img) return fail(JB_EINVAL, "jb_image_dict_info: null argument");
    if (nentries) *nentries = img->dict.term_freq.size();
    if (size) *size = img->dict.size;
    return JB_OK;
}

extern "C" void jb_image_free(jb_image* img) { delete img; }

extern "C" int jb_image_lookup(const jb_image* img, const char* word, size_t len, int64_t* freq, double* w) {
    if (!img || (!word && len)) return fail(JB_EINVAL, "jb_image_lookup: null argument");
    std::vector<uint32_t> runes;
    size_t i = 0;
    while (i < len) {
        uint32_t x = 0;
        for (size_t k = 0; k < 4 && i + k < len; k++) x |= (uint32_t)(uint8_t)word[i + k] << (8 * k);
        uint32_t r;
        const uint32_t wd = jb_decode(x, (uint32_t)std::min<size_t>(4, len - i), &r);
        runes.push_back(r);
        i += wd;
    }
    const Lookup lk = image_lookup(img->img, runes.data(), runes.size());
    if (!lk.found) return 0;
    if (freq) {
        auto it = img->dict.term_freq.find(std::string(word, len));
        *freq = it != img->dict.term_freq.end() ? it->second : (lk.fc == JB_FC_ZERO ? 0 : -1);
    }
    if (w) *w = img->img.wtab[lk.widx];
    return 1;
}

extern "C" int jb_image_stats(const jb_image* img, uint64_t* nodes, uint64_t* cap, uint32_t* npages,
                              uint32_t* maxlen, int64_t* size, double* w_absent) {
    if (!img) return fail(JB_EINVAL, "null image");
    if (nodes) *nodes = img->img.nnodes;
    if (cap) *cap = img->img.cells.size();
    if (npages) *npages = img->img.npages;
    if (maxlen) *maxlen = img->img.maxlen;
    if (size) *size = img->img.size;
    if (w_absent) *w_absent = img->img.w_absent;
    return JB_OK;
}

extern "C" double jb_image_emit(const jb_image* img, int state, uint32_t rune) {
    if (!img || state < 0 || state > 3 || rune >= 0x110000u) return JB_MIN_FLOAT;
    const Image& m = img->img;
    return m.emit[(size_t)jb_row(m.pagemap.data(), rune) * 4 + state];
}

extern "C" int jb_image_log_keys(const jb_image* img, int64_t* keys, size_t cap, size_t* n) {
    if (!img || !n || (cap && !keys)) return fail(JB_EINVAL, "jb_image_log_keys: null argument");
    const std::vector<int64_t> k = weight_log_keys(img->dict);
    *n = k.size();
    if (k.size() > cap) return cap ? fail(JB_ELIMIT, "%zu log keys do not fit %zu", k.size(), cap) : JB_ELIMIT;
    std::copy(k.begin(), k.end(), keys);
    return JB_OK;
}

extern "C" double jb_go_log(double x) { return go_log(x); }

// ---------------------------------------------------------------------------
// contexts
// ---------------------------------------------------------------------------
extern "C" int jb_open_image(jb_image* img, const jb_config* cfg, jb_ctx** out) {
    std::unique_ptr<jb_image> own(img);  // consumed on every path
    if (!img || !cfg || !out) return fail(JB_EINVAL, "jb_open_image: null argument");
    *out = nullptr;
    if (cfg->nlog && (!cfg->log_keys || !cfg->log_vals)) return fail(JB_EINVAL, "nlog > 0 without log_keys/log_vals");
    if (cfg->nlog) {  // the caller's logarithms: new weights, same trie
        for (size_t i = 0; i < cfg->nlog; i++) img->dict.log_of[cfg->log_keys[i]] = cfg->log_vals[i];
        if (!reweigh_image(img->dict, &img->img)) {
            std::string err;
            const int rc = build_image(img->dict, img->emit, &img->img, &err);
            if (rc) return fail(rc, "%s", err.c_str());
        }
    }
    auto ctx = std::make_unique<jb_ctx>();
    ctx->im = std::move(own);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(JB_EDEVICE, "no HIP device available");
    const int nuse = cfg->ndevices > 0 ? cfg->ndevices : 1;
    // JB_DEVICE_WRAP=1 (tests): device ordinals wrap around the devices present, so the
    // multi-device host path (one thread, stream and workspace per device) runs on one GPU
    const bool wrap = env_int("JB_DEVICE_WRAP", 0) != 0;
    if (cfg->device < 0 || (!wrap && cfg->device + nuse > ndev) || (wrap && cfg->device >= ndev))
        return fail(JB_EINVAL, "devices %d..%d requested, %d present", cfg->device, cfg->device + nuse - 1, ndev);
    int rc = JB_OK;
    for (int k = 0; k < nuse && rc == JB_OK; k++) {
        ctx->devs.push_back(std::make_unique<Device>());  // (jb_close releases a partial one)
        rc = open_device(ctx->devs.back().get(), (cfg->device + k) % ndev, ctx->im->img);
    }
    if (rc) {
        jb_close(ctx.release());
        return rc;
    }
    *out = ctx.release();
    return JB_OK;
}

extern "C" int jb_open(const jb_config* cfg, jb_ctx** out) {
    if (!cfg || !out) return fail(JB_EINVAL, "jb_open: null argument");
    *out = nullptr;
    jb_image* img = nullptr;
    int rc = jb_image_build(cfg, &img);
    if (rc) return rc;
    jb_config c = *cfg;
    c.nlog = 0;  // (jb_image_build applied the log table)
    return jb_open_image(img, &c, out);
}

extern "C" void jb_close(jb_ctx* ctx) {
    if (!ctx) return;
    joined_drop_cache();
    if (ctx->vocab && !ctx->devs.empty()) {  // (k_ids may still be queued on a caller's stream)
        (void)hipSetDevice(ctx->devs[0]->ordinal);
        (void)hipDeviceSynchronize();
        dfree(ctx->d_vslots);
        dfree(ctx->d_vpool);
    }
    if (ctx->stopw && !ctx->devs.empty()) {  // (k_filt_mark may still be queued on a caller's stream)
        (void)hipSetDevice(ctx->devs[0]->ordinal);
        (void)hipDeviceSynchronize();
        dfree(ctx->d_sslots);
        dfree(ctx->d_spool);
    }
    if (ctx->index.base && !ctx->devs.empty()) {  // (a search may still be queued on a caller's stream)
        (void)hipSetDevice(ctx->devs[0]->ordinal);
        (void)hipDeviceSynchronize();
        dfree(ctx->index.base);
    }
    if (std::any_of(std::begin(ctx->kw_buf), std::end(ctx->kw_buf), [](void* p) { return p != nullptr; }) &&
        !ctx->devs.empty()) {
        (void)hipSetDevice(ctx->devs[0]->ordinal);
        for (void* p : ctx->kw_buf) dfree(p);
    }
    for (auto& d : ctx->devs) close_device(d.get());
    delete ctx;
}

// ---------------------------------------------------------------------------
// cutting
// ---------------------------------------------------------------------------
// The devices' span buffers of one batch, released at the end of the call.
struct Shards {
    std::vector<SpanBuf> sb;
    explicit Shards(size_t nd) : sb(nd) {}
    ~Shards() {
        for (auto& b : sb) b.release();
    }
    uint64_t ntokens() const {
        uint64_t nt = 0;
        for (const auto& b : sb) nt += b.n;
        return nt;
    }
};

// jb_cut_batch with ctx->lock already held by the caller.
static int cut_batch_locked(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                            jb_spans* out, CutMode mode = kModePlain) {
    const size_t nd = ctx->devs.size();
    Shards sh(nd);
    std::vector<SpanBuf>& sb = sh.sb;
    std::vector<uint32_t> unit_doc;
    int rc = cut_sharded(ctx, text, doc_off, ndocs, hmm, &sb, nullptr, &unit_doc, mode);
    if (rc) return rc;
    const uint64_t nt = sh.ntokens();
    out->ntokens = nt;
    out->ndocs = ndocs;
    out->doc_tok = (uint64_t*)malloc(((uint64_t)ndocs + 1) * 8);
    if (nd == 1 || nt == sb[0].n) {  // one device's buffers are the result
        out->start = sb[0].s ? sb[0].s : (uint64_t*)malloc(8);
        out->end = sb[0].e ? sb[0].e : (uint64_t*)malloc(8);
        sb[0].s = sb[0].e = nullptr;
    } else {
        out->start = (uint64_t*)malloc(std::max<uint64_t>(nt, 1) * 8);
        out->end = (uint64_t*)malloc(std::max<uint64_t>(nt, 1) * 8);
        if (out->start && out->end) {
            uint64_t w = 0;
            for (size_t k = 0; k < nd; k++) {
                if (sb[k].n) {
                    memcpy(out->start + w, sb[k].s, sb[k].n * 8);
                    memcpy(out->end + w, sb[k].e, sb[k].n * 8);
                }
                w += sb[k].n;
            }
        }
    }
    if (!out->start || !out->end || !out->doc_tok) {
        jb_spans_free(out);
        return fail(JB_ENOMEM, "out of host memory for %llu tokens", (unsigned long long)nt);
    }
    fill_doc_tok(sb, ndocs, out->doc_tok, unit_doc);
    return JB_OK;
}

// The jb_cut_batch trio (`who` names the entry point in its error text).
static int cut_batch_entry(const char* who, jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs,
                           int hmm, jb_spans* out, CutMode mode) {
    if (!ctx || !out || (!doc_off && ndocs)) return fail(JB_EINVAL, "%s: null argument", who);
    memset(out, 0, sizeof *out);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    return cut_batch_locked(ctx, text, doc_off, ndocs, hmm, out, mode);
}

extern "C" int jb_cut_batch(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                            jb_spans* out) {
    return cut_batch_entry("jb_cut_batch", ctx, text, doc_off, ndocs, hmm, out, kModePlain);
}

extern "C" int jb_cut_batch_search(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                                   jb_spans* out) {
    return cut_batch_entry("jb_cut_batch_search", ctx, text, doc_off, ndocs, hmm, out, kModeSearch);
}

extern "C" int jb_cut_batch_full(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs,
                                 jb_spans* out) {
    return cut_batch_entry("jb_cut_batch_full", ctx, text, doc_off, ndocs, 0, out, kModeFull);
}

// One text as a batch of one document (jb_cut, jb_cut_search, jb_cut_full).
static int cut_one_entry(const char* who, jb_ctx* ctx, const uint8_t* text, size_t len, int hmm, jb_spans* out,
                         CutMode mode) {
    const uint64_t off[2] = {0, (uint64_t)len};
    static const uint8_t empty[1] = {0};
    return cut_batch_entry(who, ctx, text ? text : empty, off, 1, hmm, out, mode);
}

extern "C" int jb_cut(jb_ctx* ctx, const uint8_t* text, size_t len, int hmm, jb_spans* out) {
    return cut_one_entry("jb_cut_batch", ctx, text, len, hmm, out, kModePlain);
}

extern "C" int jb_cut_search(jb_ctx* ctx, const uint8_t* text, size_t len, int hmm, jb_spans* out) {
    return cut_one_entry("jb_cut_batch_search", ctx, text, len, hmm, out, kModeSearch);
}

extern "C" int jb_cut_full(jb_ctx* ctx, const uint8_t* text, size_t len, jb_spans* out) {
    return cut_one_entry("jb_cut_batch_full", ctx, text, len, 0, out, kModeFull);
}

// jb_cut_batch_into (T = u64: batch offsets) and jb_cut_batch_into32 (T = u32: offsets from b0,
// the batch's first byte) after their argument checks.  One device decodes its pieces' spans
// straight into the caller's arrays; several devices' u64 spans are merged into them here.
template <class T>
static int cut_batch_into(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm, T* start,
                          T* end, uint64_t cap, uint64_t* doc_tok, uint64_t* ntokens, uint64_t b0) {
    constexpr bool k32 = std::is_same<T, uint32_t>::value;
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    const size_t nd = ctx->devs.size();
    Shards sh(nd);
    std::vector<SpanBuf>& sb = sh.sb;
    if (nd == 1) {
        if constexpr (k32) {
            sb[0].s32 = start;
            sb[0].e32 = end;
            sb[0].b32 = b0;
        } else {
            sb[0].s = start;
            sb[0].e = end;
        }
        sb[0].cap = cap;
        sb[0].external = true;
    }
    std::vector<uint32_t> unit_doc;
    int rc = cut_sharded(ctx, text, doc_off, ndocs, hmm, &sb, nullptr, &unit_doc);
    if (rc) return rc;
    const uint64_t nt = *ntokens = sh.ntokens();
    if (nt > cap)
        return fail(JB_ELIMIT, "%llu tokens do not fit the %llu-token output arrays", (unsigned long long)nt,
                    (unsigned long long)cap);
    if (nd > 1) {
        uint64_t w = 0;
        for (size_t k = 0; k < nd; k++) {
            if constexpr (k32) {  // (narrowed here)
                for (uint64_t i = 0; i < sb[k].n; i++) {
                    start[w + i] = (uint32_t)(sb[k].s[i] - b0);
                    end[w + i] = (uint32_t)(sb[k].e[i] - b0);
                }
            } else if (sb[k].n) {
                memcpy(start + w, sb[k].s, sb[k].n * 8);
                memcpy(end + w, sb[k].e, sb[k].n * 8);
            }
            w += sb[k].n;
        }
    }
    fill_doc_tok(sb, ndocs, doc_tok, unit_doc);
    return JB_OK;
}

extern "C" int jb_cut_batch_into(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs,
                                 int hmm, uint64_t* start, uint64_t* end, uint64_t cap, uint64_t* doc_tok,
                                 uint64_t* ntokens) {
    if (!ctx || !ntokens || !doc_tok || (!doc_off && ndocs) || (cap && (!start || !end)))
        return fail(JB_EINVAL, "jb_cut_batch_into: null argument");
    *ntokens = 0;
    return cut_batch_into(ctx, text, doc_off, ndocs, hmm, start, end, cap, doc_tok, ntokens, 0);
}

extern "C" int jb_cut_batch_into32(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs,
                                   int hmm, uint32_t* start, uint32_t* end, uint64_t cap, uint64_t* doc_tok,
                                   uint64_t* ntokens) {
    if (!ctx || !ntokens || !doc_tok || (!doc_off && ndocs) || (cap && (!start || !end)))
        return fail(JB_EINVAL, "jb_cut_batch_into32: null argument");
    *ntokens = 0;
    const uint64_t b0 = ndocs ? doc_off[0] : 0;
    if (ndocs && doc_off[ndocs] - b0 > 0xFFFFFFFFull)
        return fail(JB_ELIMIT, "jb_cut_batch_into32: a batch of %llu bytes (u32 offsets: under 4 GiB)",
                    (unsigned long long)(doc_off[ndocs] - b0));
    return cut_batch_into(ctx, text, doc_off, ndocs, hmm, start, end, cap, doc_tok, ntokens, b0);
}

extern "C" int jb_cut_batch_mask(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs,
                                 int hmm, uint64_t* starts, uint64_t* ends, uint64_t nwords, uint64_t* ntokens) {
    if (!ctx || !ntokens || (!doc_off && ndocs)) return fail(JB_EINVAL, "jb_cut_batch_mask: null argument");
    *ntokens = 0;
    const uint64_t nbytes = ndocs ? doc_off[ndocs] - doc_off[0] : 0;
    const uint64_t need = (nbytes + 63) / 64;
    if (nwords < need) return fail(JB_EINVAL, "jb_cut_batch_mask: %llu words for %llu bytes (want %llu)",
                                   (unsigned long long)nwords, (unsigned long long)nbytes, (unsigned long long)need);
    if (need && (!starts || !ends)) return fail(JB_EINVAL, "jb_cut_batch_mask: null mask");
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Shards sh(ctx->devs.size());
    const MaskDst m{starts, ends, ndocs ? doc_off[0] : 0};
    int rc = cut_sharded(ctx, text, doc_off, ndocs, hmm, &sh.sb, &m);
    if (rc) return rc;
    if (nwords > need) {  // the header promises every word: clear the caller's tail past the batch
        memset(starts + need, 0, (nwords - need) * 8);
        memset(ends + need, 0, (nwords - need) * 8);
    }
    *ntokens = sh.ntokens();
    return JB_OK;
}

extern "C" int jb_host_alloc(size_t n, void** p) {
    if (!p) return fail(JB_EINVAL, "jb_host_alloc: null argument");
    *p = nullptr;
    const hipError_t e = hipHostMalloc(p, std::max<size_t>(n, 1), hipHostMallocPortable);
    if (e != hipSuccess) {
        *p = nullptr;
        return fail(e == hipErrorOutOfMemory ? JB_ENOMEM : JB_EDEVICE, "hipHostMalloc(%zu): %s", n,
                    hipGetErrorString(e));
    }
    host_register(*p, n);
    return JB_OK;
}

extern "C" void jb_host_free(void* p) {
    if (!p) return;
    host_unregister(p);
    (void)hipHostFree(p);
}

extern "C" void jb_spans_free(jb_spans* s) {
    if (!s) return;
    free(s->start);
    free(s->end);
    free(s->doc_tok);
    memset(s, 0, sizeof *s);
}

// The jb_cut_device* sextet after their own checks: one pipeline on the first device, queued on the
// caller's stream.  o_*: caller-owned outputs (the *_into calls), else d_* report where the spans are.
static int cut_device(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint64_t* d_doc_off,
                      uint32_t ndocs, int hmm, void* stream, uint32_t* o_start, uint32_t* o_end, uint64_t* o_doc_tok,
                      uint64_t* o_ntok, uint32_t** d_start, uint32_t** d_end, uint64_t** d_doc_tok, uint64_t** d_ntok,
                      CutMode mode = kModePlain, uint64_t cap = 0) {
    if (!ctx || (!d_text && nbytes) || !d_doc_off) return fail(JB_EINVAL, "jb_cut_device: null argument");
    if (nbytes >= (1ull << 31)) return fail(JB_ELIMIT, "device batch of %llu bytes (limit 2 GiB)",
                                            (unsigned long long)nbytes);
    if (((uintptr_t)d_text & 15u) != 0) return fail(JB_EINVAL, "d_text must be 16-byte aligned");
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    for (size_t k = 1; k < ctx->devs.size(); k++) {
        std::lock_guard<std::mutex> g(ctx->devs[k]->stats_mu);
        ctx->devs[k]->has_stats = false;
    }
    Device* d = ctx->devs[0].get();
    std::lock_guard<std::mutex> g(d->mu);
    HIPCHK(hipSetDevice(d->ordinal));
    int rc;
    if ((rc = ensure_work(d, nbytes, ndocs)) || (rc = ensure_mode(d, mode))) return rc;
    const hipStream_t s = (hipStream_t)stream;
    // (full mode's ctx-owned arrays: nbytes entries, whatever the workspace has grown to)
    const SpanDst dst{o_start, o_end, cap, o_doc_tok, o_ntok};
    const SpanTarget t = span_target(d, mode, o_start ? &dst : nullptr, nbytes);
    if ((rc = launch(d, t.w, d_text, nbytes, d_doc_off, ndocs, hmm != 0, s, nullptr, t.post()))) return rc;
    if (mode == kModePlain && o_start) {  // (search and full mode's pass writes its count to o_ntok itself)
        HIPCHK(hipMemcpyAsync(o_ntok, t.at.ntok, 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipEventRecord(d->ws_done, s));  // (the counters are workspace too)
    }
    if (d_start) *d_start = t.at.start;
    if (d_end) *d_end = t.at.end;
    if (d_doc_tok) *d_doc_tok = t.at.doc_tok;
    if (d_ntok) *d_ntok = t.at.ntok;
    return JB_OK;
}

extern "C" int jb_cut_device(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint64_t* d_doc_off,
                             uint32_t ndocs, int hmm, void* stream, uint32_t** d_start, uint32_t** d_end,
                             uint64_t** d_doc_tok, uint64_t** d_ntok) {
    return cut_device(ctx, d_text, nbytes, d_doc_off, ndocs, hmm, stream, nullptr, nullptr, nullptr, nullptr, d_start,
                      d_end, d_doc_tok, d_ntok);
}

extern "C" int jb_cut_device_into(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint64_t* d_doc_off,
                                  uint32_t ndocs, int hmm, void* stream, uint32_t* d_start, uint32_t* d_end,
                                  uint64_t cap, uint64_t* d_doc_tok, uint64_t* d_ntok) {
    if (!d_start || !d_end || !d_doc_tok || !d_ntok) return fail(JB_EINVAL, "jb_cut_device_into: null output");
    if (cap < nbytes) return fail(JB_EINVAL, "jb_cut_device_into: cap %llu < nbytes %llu (a batch of n bytes "
                                  "has up to n tokens)", (unsigned long long)cap, (unsigned long long)nbytes);
    return cut_device(ctx, d_text, nbytes, d_doc_off, ndocs, hmm, stream, d_start, d_end, d_doc_tok, d_ntok, nullptr,
                      nullptr, nullptr, nullptr);
}

extern "C" int jb_cut_device_search(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint64_t* d_doc_off,
                                    uint32_t ndocs, int hmm, void* stream, uint32_t** d_start, uint32_t** d_end,
                                    uint64_t** d_doc_tok, uint64_t** d_ntok) {
    return cut_device(ctx, d_text, nbytes, d_doc_off, ndocs, hmm, stream, nullptr, nullptr, nullptr, nullptr, d_start,
                      d_end, d_doc_tok, d_ntok, kModeSearch);
}

extern "C" int jb_cut_device_search_into(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes,
                                         const uint64_t* d_doc_off, uint32_t ndocs, int hmm, void* stream,
                                         uint32_t* d_start, uint32_t* d_end, uint64_t cap, uint64_t* d_doc_tok,
                                         uint64_t* d_ntok) {
    if (!d_start || !d_end || !d_doc_tok || !d_ntok) return fail(JB_EINVAL, "jb_cut_device_search_into: null output");
    if (cap < nbytes) return fail(JB_EINVAL, "jb_cut_device_search_into: cap %llu < nbytes %llu (a batch of n bytes "
                                  "has up to n search-mode spans)", (unsigned long long)cap, (unsigned long long)nbytes);
    return cut_device(ctx, d_text, nbytes, d_doc_off, ndocs, hmm, stream, d_start, d_end, d_doc_tok, d_ntok, nullptr,
                      nullptr, nullptr, nullptr, kModeSearch);
}

extern "C" int jb_cut_device_full(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint64_t* d_doc_off,
                                  uint32_t ndocs, void* stream, uint32_t** d_start, uint32_t** d_end,
                                  uint64_t** d_doc_tok, uint64_t** d_ntok) {
    return cut_device(ctx, d_text, nbytes, d_doc_off, ndocs, 0, stream, nullptr, nullptr, nullptr, nullptr, d_start,
                      d_end, d_doc_tok, d_ntok, kModeFull);
}

extern "C" int jb_cut_device_full_into(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint64_t* d_doc_off,
                                       uint32_t ndocs, void* stream, uint32_t* d_start, uint32_t* d_end, uint64_t cap,
                                       uint64_t* d_doc_tok, uint64_t* d_ntok) {
    if (!d_start || !d_end || !d_doc_tok || !d_ntok) return fail(JB_EINVAL, "jb_cut_device_full_into: null output");
    return cut_device(ctx, d_text, nbytes, d_doc_off, ndocs, 0, stream, d_start, d_end, d_doc_tok, d_ntok, nullptr,
                      nullptr, nullptr, nullptr, kModeFull, cap);
}

// ---------------------------------------------------------------------------
// dictionary mutation / introspection
// ---------------------------------------------------------------------------
extern "C" int jb_dict_get(jb_ctx* ctx, const char* word, size_t len, int64_t* freq) {
    if (!ctx || (!word && len)) return fail(JB_EINVAL, "jb_dict_get: null argument");
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    auto it = ctx->im->dict.term_freq.find(std::string(word ? word : "", len));
    if (it == ctx->im->dict.term_freq.end()) return 0;
    if (freq) *freq = it->second;
    return 1;
}

extern "C" int64_t jb_dict_size(jb_ctx* ctx) {
    if (!ctx) return 0;
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    return ctx->im->dict.size;
}

// suggestFreq (tokenizer.go:589-614); the caller holds ctx->lock
static int suggest_freq(jb_ctx* ctx, const char* word, size_t len, int64_t* out) {
    const Dictionary& dict = ctx->im->dict;
    double dsize = (double)dict.size;
    if (dsize < 1.0) dsize = 1.0;
    double freq = 1.0;
    jb_spans sp;
    memset(&sp, 0, sizeof sp);
    static const uint8_t empty[1] = {0};
    const uint64_t off[2] = {0, (uint64_t)len};
    int rc = cut_batch_locked(ctx, word ? (const uint8_t*)word : empty, off, 1, 0, &sp);
    if (rc) return rc;
    for (uint64_t k = 0; k < sp.ntokens; k++) {
        std::string piece;
        if (sp.end[k] - sp.start[k] == 1 && (uint8_t)word[sp.start[k]] >= 0x80) piece = "\xEF\xBF\xBD";
        else piece.assign(word + sp.start[k], sp.end[k] - sp.start[k]);
        auto it = dict.term_freq.find(piece);
        const int64_t pf = it != dict.term_freq.end() ? it->second : 1;
        freq *= (double)pf / dsize;
    }
    jb_spans_free(&sp);
    const int64_t a = (int64_t)(freq * dsize) + 1;
    int64_t b = 1;
    auto it = dict.term_freq.find(std::string(word, len));
    if (it != dict.term_freq.end()) b = it->second;
    *out = a > b ? a : b;
    return JB_OK;
}

extern "C" int jb_suggest_freq(jb_ctx* ctx, const char* word, size_t len, int64_t* freq) {
    if (!ctx || !freq || (!word && len)) return fail(JB_EINVAL, "jb_suggest_freq: null argument");
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    return suggest_freq(ctx, word ? word : "", len, freq);
}

extern "C" int jb_add_log(jb_ctx* ctx, const int64_t* keys, const double* vals, size_t n) {
    if (!ctx || (n && (!keys || !vals))) return fail(JB_EINVAL, "jb_add_log: null argument");
    std::unique_lock<std::shared_mutex> wl(ctx->lock);
    for (size_t i = 0; i < n; i++) ctx->im->dict.log_of[keys[i]] = vals[i];
    return JB_OK;
}

extern "C" int jb_add_word(jb_ctx* ctx, const char* word, size_t len, int64_t freq) {
    if (!ctx || (!word && len)) return fail(JB_EINVAL, "jb_add_word: null argument");
    int rc;
    std::unique_lock<std::shared_mutex> wl(ctx->lock);  // (the reference deadlocks here: :376 + :581)
    if (freq < 1 && (rc = suggest_freq(ctx, word, len, &freq))) return rc;
    // addTerm (tokenizer.go:580-585): no prefix entries are added.  The new dictionary and
    // image are built aside and staged on every device; ctx changes only once all of that
    // worked, so a failure (JB_ELIMIT, JB_EDEVICE, JB_ENOMEM) leaves it as it was.
    try {
        Dictionary nd = ctx->im->dict;
        nd.term_freq[std::string(word, len)] = freq;
        nd.size += freq;
        Image ni;
        std::string err;
        if ((rc = build_image(nd, ctx->im->emit, &ni, &err))) return fail(rc, "%s", err.c_str());
        if (ni.maxlen > 255) return fail(JB_ELIMIT, "dictionary word of %u runes (max 255)", ni.maxlen);
        std::vector<ImageBufs> staged(ctx->devs.size());
        for (size_t k = 0; k < ctx->devs.size() && rc == JB_OK; k++)
            rc = stage_image(ctx->devs[k]->ordinal, ni, &staged[k]);
        if (rc) {
            for (auto& b : staged) {
                (void)hipSetDevice(ctx->devs[&b - staged.data()]->ordinal);
                free_image_bufs(&b);
            }
            return rc;
        }
        for (size_t k = 0; k < ctx->devs.size(); k++) {  // commit
            Device* d = ctx->devs[k].get();
            std::lock_guard<std::mutex> g(d->mu);
            (void)hipSetDevice(d->ordinal);
            (void)hipStreamSynchronize(d->stream);
            if (d->ws_done) (void)hipEventSynchronize(d->ws_done);  // (a jb_cut_device pipeline)
            (void)install_image(d, &staged[k], ni);
        }
        ctx->im->dict = std::move(nd);
        ctx->im->img = std::move(ni);
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "out of host memory rebuilding the dictionary");
    }
    return JB_OK;
}

extern "C" int jb_save(jb_ctx* ctx, const char* path) {
    if (!ctx || !path) return fail(JB_EINVAL, "jb_save: null argument");
    std::string data;
    {
        std::shared_lock<std::shared_mutex> rl(ctx->lock);
        save_image(ctx->im->dict, ctx->im->emit, ctx->im->img, &data);
    }
    return write_file(path, data);
}

extern "C" int jb_last_stats(jb_ctx* ctx, jb_stats* out) {
    if (!ctx || !out) return fail(JB_EINVAL, "jb_last_stats: null argument");
    memset(out, 0, sizeof *out);
    uint32_t err = 0;  // CNT_ERR of a device pipeline (jb_cut_device*)
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    for (auto& d : ctx->devs) {
        {
            std::lock_guard<std::mutex> sg(d->stats_mu);
            if (!d->has_stats) continue;  // not reached by the last batch (its counters are older)
            if (d->last_small) {  // k_small's counters came back with its spans (no device lock needed)
                out->tokens += d->small_hdr[SM_NTOK];
                out->blocks += d->small_hdr[SM_BLOCKS];
                out->zh_blocks += d->small_hdr[SM_ZHBLOCKS];
                out->viterbi_ties += d->small_hdr[SM_TIES];
                continue;
            }
        }
        std::lock_guard<std::mutex> g(d->mu);
        if (d->acc_valid) {  // a host range cut in pieces: summed as they came back
            out->tokens += d->acc.tokens;
            out->blocks += d->acc.blocks;
            out->zh_blocks += d->acc.zh_blocks;
            out->long_blocks += d->acc.long_blocks;
            out->viterbi_ties += d->acc.viterbi_ties;
            continue;
        }
        if (!d->w.counters) continue;
        HIPCHK(hipSetDevice(d->ordinal));
        HIPCHK(hipDeviceSynchronize());  // (jb_cut_device may have queued on a caller's stream)
        uint32_t c[CNT_CLEAR];
        HIPCHK(hipMemcpy(c, d->w.counters, sizeof c, hipMemcpyDeviceToHost));
        uint64_t ntok;
        memcpy(&ntok, c + CNT_NWORDS, 8);
        out->tokens += ntok;
        // blocks: the per-tile counts k_mark_walk left in the workspace
        const uint64_t ntiles = (d->last_nbytes + kTileBytes - 1) / kTileBytes;
        if (ntiles) {
            std::vector<uint2> tc(ntiles);
            HIPCHK(hipMemcpy(tc.data(), d->w.tile_cnt, ntiles * sizeof(uint2), hipMemcpyDeviceToHost));
            for (const uint2& t : tc) {
                out->blocks += t.x;
                out->zh_blocks += t.y;
            }
        }
        out->long_blocks += c[CNT_NLONG];
        out->viterbi_ties += c[CNT_TIES];
        err |= c[CNT_ERR];
    }
    // (a host batch already returned these from its own call; a device pipeline reports them here)
    if (err & 2u) return fail(JB_EDEVICE, "k_long: a phase wait gave up (no progress for JB_LONG_WAIT_US)");
    // (bit 3, a full-mode list longer than its arrays, is jb_device_status's to report: the plain counts stand)
    if (err & ~8u) return fail(JB_EPANIC, "a Han block has no DAG path (the reference panics in cutDAG)");
    return JB_OK;
}

extern "C" int jb_device_status(jb_ctx* ctx, void* stream) {
    if (!ctx) return fail(JB_EINVAL, "jb_device_status: null ctx");
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    std::lock_guard<std::mutex> g(d->mu);
    if (!d->w.counters) return JB_OK;  // no device pipeline has run
    HIPCHK(hipSetDevice(d->ordinal));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (d->ws_done) HIPCHK(hipEventSynchronize(d->ws_done));
    uint32_t e = 0;
    HIPCHK(hipMemcpy(&e, d->w.counters + CNT_ERR, sizeof e, hipMemcpyDeviceToHost));
    if (e & 2u) return fail(JB_EDEVICE, "k_long: a phase wait gave up (no progress for JB_LONG_WAIT_US)");
    if (e & ~8u) return fail(JB_EPANIC, "a Han block has no DAG path (the reference panics in cutDAG)");
    if (e & 8u) {
        uint64_t n = 0;
        HIPCHK(hipMemcpy(&n, d->w.counters + CNT_NSRCH, sizeof n, hipMemcpyDeviceToHost));
        return fail(JB_ELIMIT, "the full-mode list has %llu spans, more than the output arrays hold: the spans "
                               "past their capacity were not written", (unsigned long long)n);
    }
    return JB_OK;
}

// ---------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------
extern "C" int jb_profile_enable(jb_ctx* ctx, int on) {
    if (!ctx) return fail(JB_EINVAL, "null ctx");
    for (auto& d : ctx->devs) d->profile = on != 0;
    return JB_OK;
}

extern "C" int jb_profile_reset(jb_ctx* ctx) {
    if (!ctx) return fail(JB_EINVAL, "null ctx");
    for (auto& d : ctx->devs) {
        (void)hipSetDevice(d->ordinal);
        d->timer.reset();
    }
    return JB_OK;
}

extern "C" int jb_profile_read(jb_ctx* ctx, const char** names, double* ms, uint64_t* launches, int cap) {
    if (!ctx) return fail(JB_EINVAL, "null ctx");
    double tot_ms[K_NUM] = {0};
    uint64_t tot_n[K_NUM] = {0};
    for (auto& d : ctx->devs) {
        (void)hipSetDevice(d->ordinal);
        d->timer.harvest();
        for (int k = 0; k < K_NUM; k++) {
            tot_ms[k] += d->timer.ms[k];
            tot_n[k] += d->timer.launches[k];
        }
    }
    int n = 0;
    for (int k = 0; k < K_NUM && n < cap; k++, n++) {
        if (names) names[n] = kKernelNames[k];
        if (ms) ms[n] = tot_ms[k];
        if (launches) launches[n] = tot_n[k];
    }
    return n;
}

// ---------------------------------------------------------------------------
// token ids: a caller's vocabulary (jb_vocab.h) and the lookup of span lists in it
// ---------------------------------------------------------------------------
extern "C" int jb_vocab_build(const uint8_t* keys, const uint64_t* key_off, uint32_t nkeys, jb_vocab** out) {
    if (!out) return fail(JB_EINVAL, "jb_vocab_build: null argument");
    *out = nullptr;
    try {
        auto v = std::make_unique<jb_vocab>();
        std::string err;
        const int rc = vocab_build(keys, key_off, nkeys, &v->v, &err);
        if (rc) return fail(rc, "%s", err.c_str());
        *out = v.release();
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "out of host memory building the vocabulary");
    }
    return JB_OK;
}

extern "C" void jb_vocab_free(jb_vocab* v) { delete v; }

extern "C" int jb_vocab_lookup(const jb_vocab* v, const uint8_t* tok, size_t len, uint32_t* id) {
    if (!v || (!tok && len)) return fail(JB_EINVAL, "jb_vocab_lookup: null argument");
    const uint32_t r = vocab_lookup(v->v, tok, len);
    if (id) *id = r;
    return r != JB_VOCAB_UNK;
}

extern "C" int jb_vocab_info(const jb_vocab* v, uint32_t* nkeys, uint32_t* maxlen, uint64_t* nslots) {
    if (!v) return fail(JB_EINVAL, "jb_vocab_info: null vocabulary");
    if (nkeys) *nkeys = v->v.nkeys;
    if (maxlen) *maxlen = v->v.maxlen;
    if (nslots) *nslots = v->v.nslots;
    return JB_OK;
}

static_assert(JB_ID_UNK == JB_VOCAB_UNK, "the header's unknown id is the table's");

namespace {
// jb_vocab_set and jb_stopwords_set: the caller's list built aside, uploaded to the first device and swapped in
// under the exclusive lock, after the device's queued work (which may read the old table) has finished.
int table_set(jb_ctx* ctx, const char* who, const uint8_t* keys, const uint64_t* key_off, uint32_t nkeys,
              std::unique_ptr<Vocab> jb_ctx::*tab, uint32_t* jb_ctx::*dslots, uint8_t* jb_ctx::*dpool,
              DevVocab jb_ctx::*dview) {
    if (!ctx) return fail(JB_EINVAL, "%s: null ctx", who);
    const bool remove = !keys && nkeys == 0;
    std::unique_ptr<Vocab> nv;
    if (!remove) {  // built aside: on any error the old table stays attached
        try {
            nv = std::make_unique<Vocab>();
            std::string err;
            const int rc = vocab_build(keys, key_off, nkeys, nv.get(), &err);
            if (rc) return fail(rc, "%s", err.c_str());
        } catch (const std::bad_alloc&) {
            return fail(JB_ENOMEM, "out of host memory building the vocabulary");
        }
    }
    std::unique_lock<std::shared_mutex> wl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    uint32_t* ns = nullptr;
    uint8_t* np = nullptr;
    if (nv) {
        hipError_t e = hipMalloc(&ns, nv->slots.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&np, nv->pool.size());
        if (e == hipSuccess) e = hipMemcpy(ns, nv->slots.data(), nv->slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(np, nv->pool.data(), nv->pool.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            dfree(ns);
            dfree(np);
            return fail(JB_EDEVICE, "%s: uploading the table: %s", who, hipGetErrorString(e));
        }
    }
    // the old table may be in use by kernels queued earlier, on any stream of the device
    if (ctx->*tab) (void)hipDeviceSynchronize();
    dfree(ctx->*dslots);
    dfree(ctx->*dpool);
    ctx->*dslots = ns;
    ctx->*dpool = np;
    ctx->*tab = std::move(nv);
    ctx->*dview = ctx->*tab ? DevVocab{ns, np, (uint32_t)((ctx->*tab)->nslots - 1u), (ctx->*tab)->maxlen} : DevVocab{};
    return JB_OK;
}
}  // namespace

extern "C" int jb_vocab_set(jb_ctx* ctx, const uint8_t* keys, const uint64_t* key_off, uint32_t nkeys) {
    return table_set(ctx, "jb_vocab_set", keys, key_off, nkeys, &jb_ctx::vocab, &jb_ctx::d_vslots, &jb_ctx::d_vpool,
                     &jb_ctx::dvocab);
}

extern "C" int jb_stopwords_set(jb_ctx* ctx, const uint8_t* keys, const uint64_t* key_off, uint32_t nkeys) {
    return table_set(ctx, "jb_stopwords_set", keys, key_off, nkeys, &jb_ctx::stopw, &jb_ctx::d_sslots, &jb_ctx::d_spool,
                     &jb_ctx::dstop);
}

extern "C" int64_t jb_stopwords_size(jb_ctx* ctx) {
    if (!ctx) return -1;
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    return ctx->stopw ? (int64_t)ctx->stopw->nkeys : -1;
}

extern "C" int64_t jb_vocab_size(jb_ctx* ctx) {
    if (!ctx) return -1;
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    return ctx->vocab ? (int64_t)ctx->vocab->nkeys : -1;
}

extern "C" int jb_ids_device(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start,
                             const uint32_t* d_end, const uint64_t* d_ntok, uint64_t cap, void* stream,
                             uint32_t* d_ids) {
    if (!ctx || (!d_text && nbytes) || !d_ntok || (cap && (!d_start || !d_end || !d_ids)))
        return fail(JB_EINVAL, "jb_ids_device: null argument");
    if (nbytes >= (1ull << 31)) return fail(JB_ELIMIT, "device batch of %llu bytes (limit 2 GiB)",
                                            (unsigned long long)nbytes);
    if (((uintptr_t)d_text & 3u) != 0) return fail(JB_EINVAL, "d_text must be 4-byte aligned");
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    if (!ctx->vocab) return fail(JB_EINVAL, "jb_ids_device: no vocabulary attached (jb_vocab_set)");
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_ids(ctx->dvocab, d_text, nbytes, d_start, d_end, d_ntok, cap, d_ids, d->ncu, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_ids(ctx->dvocab, d_text, nbytes, d_start, d_end, d_ntok, cap, d_ids, d->ncu, s, nullptr));
    return JB_OK;
}

extern "C" int jb_spans_ids(jb_ctx* ctx, const uint8_t* text, const jb_spans* spans, uint32_t* ids) {
    if (!ctx || !spans || (spans->ntokens && (!text || !spans->start || !spans->end || !ids)))
        return fail(JB_EINVAL, "jb_spans_ids: null argument");
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    if (!ctx->vocab) return fail(JB_EINVAL, "jb_spans_ids: no vocabulary attached (jb_vocab_set)");
    const uint64_t n = spans->ntokens;
    if (n == 0) return JB_OK;
    // the byte range the spans cover (empty and reversed spans cover nothing: they are unknown)
    uint64_t lo = UINT64_MAX, hi = 0;
    for (uint64_t k = 0; k < n; k++)
        if (spans->start[k] < spans->end[k]) {
            lo = std::min(lo, spans->start[k]);
            hi = std::max(hi, spans->end[k]);
        }
    if (lo > hi) lo = hi = 0;
    const uint64_t nb = hi - lo;
    if (nb >= (1ull << 31))
        return fail(JB_ELIMIT, "the spans cover %llu bytes (limit 2 GiB)", (unsigned long long)nb);
    std::vector<uint32_t> se;
    try {
        se.resize(2 * n);
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "out of host memory for %llu spans", (unsigned long long)n);
    }
    for (uint64_t k = 0; k < n; k++) {
        const bool ok = spans->start[k] < spans->end[k];
        se[k] = ok ? (uint32_t)(spans->start[k] - lo) : 0u;
        se[n + k] = ok ? (uint32_t)(spans->end[k] - lo) : 0u;
    }
    Device* d = ctx->devs[0].get();
    std::lock_guard<std::mutex> g(d->mu);  // (d->stream and the timer)
    HIPCHK(hipSetDevice(d->ordinal));
    uint8_t* dt = nullptr;
    uint32_t *dse = nullptr, *did = nullptr;
    uint64_t* dn = nullptr;
    auto run = [&]() -> int {
        HIPCHK(hipMalloc(&dt, nb + 64));
        HIPCHK(hipMalloc(&dse, 2 * n * sizeof(uint32_t)));
        HIPCHK(hipMalloc(&did, n * sizeof(uint32_t)));
        HIPCHK(hipMalloc(&dn, sizeof(uint64_t)));
        HIPCHK(hipMemsetAsync(dt + nb, 0, 64, d->stream));
        if (nb) HIPCHK(hipMemcpyAsync(dt, text + lo, nb, hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipMemcpyAsync(dse, se.data(), 2 * n * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipMemcpyAsync(dn, &n, sizeof n, hipMemcpyHostToDevice, d->stream));
        HIPCHK(run_ids(ctx->dvocab, dt, nb, dse, dse + n, dn, n, did, d->ncu, d->stream,
                       d->profile ? &d->timer : nullptr));
        HIPCHK(hipMemcpyAsync(ids, did, n * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        return JB_OK;
    };
    const int rc = run();
    if (rc) (void)hipStreamSynchronize(d->stream);  // (copies from `se` may be in flight)
    dfree(dt);
    dfree(dse);
    dfree(did);
    dfree(dn);
    return rc;
}

// ---------------------------------------------------------------------------
// term counts and keywords (jb_terms.hip)
// ---------------------------------------------------------------------------
static_assert(JB_KW_MAXK == kKwMaxK && JB_TERMS_TILE == kTermsTile, "the header's constants are the kernels'");

extern "C" size_t jb_terms_work_bytes(uint64_t max_tokens, uint32_t ndocs) { return terms_work_bytes(max_tokens, ndocs); }

extern "C" int jb_terms_device(jb_ctx* ctx, const uint32_t* d_ids, uint64_t ids_cap, const uint64_t* d_doc_tok,
                               const uint64_t* d_ntok, uint32_t ndocs, void* stream, uint32_t* d_term_id,
                               uint32_t* d_term_cnt, uint64_t cap, uint64_t* d_term_off, uint64_t* d_nterms,
                               void* d_work, size_t nwork) {
    if (!ctx || !d_doc_tok || !d_ntok || !d_term_off || !d_nterms || !d_work || (ids_cap && !d_ids) ||
        (cap && (!d_term_id || !d_term_cnt)))
        return fail(JB_EINVAL, "jb_terms_device: null argument");
    if (ids_cap >= (1ull << 32) - kTermsTile)
        return fail(JB_ELIMIT, "jb_terms_device: an id list of %llu entries (limit 2^32 - %u)",
                    (unsigned long long)ids_cap, kTermsTile);
    if (((uintptr_t)d_work & 7u) != 0) return fail(JB_EINVAL, "jb_terms_device: d_work must be 8-byte aligned");
    const size_t need = terms_work_bytes(ids_cap, ndocs);
    if (nwork < need)
        return fail(JB_EINVAL, "jb_terms_device: a work buffer of %llu bytes, jb_terms_work_bytes asks for %llu",
                    (unsigned long long)nwork, (unsigned long long)need);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_terms(d_ids, ids_cap, d_doc_tok, d_ntok, ndocs, d_term_id, d_term_cnt, cap, d_term_off, d_nterms,
                         d_work, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_terms(d_ids, ids_cap, d_doc_tok, d_ntok, ndocs, d_term_id, d_term_cnt, cap, d_term_off, d_nterms, d_work,
                     s, nullptr));
    return JB_OK;
}

extern "C" int jb_keywords_device(jb_ctx* ctx, const uint32_t* d_term_id, const uint32_t* d_term_cnt,
                                  const uint64_t* d_term_off, uint32_t ndocs, uint64_t cap, const float* d_weight,
                                  uint32_t nweights, uint32_t topk, void* stream, uint32_t* d_kw_id, float* d_kw_score,
                                  uint32_t* d_kw_cnt, uint32_t* d_kw_n) {
    // (the limits of topk come first: they need no ctx)
    if (topk == 0) return fail(JB_EINVAL, "jb_keywords_device: topk is 0");
    if (topk > kKwMaxK) return fail(JB_ELIMIT, "jb_keywords_device: topk %u (limit JB_KW_MAXK = %u)", topk, kKwMaxK);
    if (!ctx || !d_term_off || (cap && (!d_term_id || !d_term_cnt)) || (nweights && !d_weight) ||
        (ndocs && (!d_kw_id || !d_kw_score || !d_kw_cnt || !d_kw_n)))
        return fail(JB_EINVAL, "jb_keywords_device: null argument");
    if (ndocs == 0) return JB_OK;
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    if (d->profile) {
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_keywords(d_term_id, d_term_cnt, d_term_off, ndocs, cap, d_weight, nweights, topk, d_kw_id,
                            d_kw_score, d_kw_cnt, d_kw_n, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_keywords(d_term_id, d_term_cnt, d_term_off, ndocs, cap, d_weight, nweights, topk, d_kw_id, d_kw_score,
                        d_kw_cnt, d_kw_n, s, nullptr));
    return JB_OK;
}

// ---------------------------------------------------------------------------
// document frequencies and IDF weights (jb_terms.hip)
// ---------------------------------------------------------------------------
extern "C" int jb_df_device(jb_ctx* ctx, const uint32_t* d_term_id, const uint64_t* d_nterms, uint64_t cap,
                            uint32_t* d_df, uint32_t ndf, void* stream) {
    if (!ctx) return fail(JB_EINVAL, "jb_df_device: null ctx");
    if (!d_nterms) return fail(JB_EINVAL, "jb_df_device: null d_nterms");
    if (cap && !d_term_id) return fail(JB_EINVAL, "jb_df_device: null d_term_id");
    if (ndf && !d_df) return fail(JB_EINVAL, "jb_df_device: null d_df");
    if (ndf == 0 || cap == 0) return JB_OK;  // (nothing to add)
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    const bool combine = d->lc.df_combine != 0;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_df(d_term_id, d_nterms, cap, d_df, ndf, combine, d->ncu, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_df(d_term_id, d_nterms, cap, d_df, ndf, combine, d->ncu, s, nullptr));
    return JB_OK;
}

static int idf_args(const char* who, const void* df, uint32_t ndf, uint64_t ndocs_total, const void* weight) {
    if (ndf && !df) return fail(JB_EINVAL, "%s: null df", who);
    if (ndf && !weight) return fail(JB_EINVAL, "%s: null weight", who);
    if (ndocs_total >= (1ull << 53))
        return fail(JB_ELIMIT, "%s: ndocs_total %llu (limit 2^53 - 1)", who, (unsigned long long)ndocs_total);
    return JB_OK;
}

extern "C" int jb_idf(const uint32_t* df, uint32_t ndf, uint64_t ndocs_total, uint32_t min_df, uint32_t max_df,
                      const uint8_t* keep, float* weight) {
    if (const int rc = idf_args("jb_idf", df, ndf, ndocs_total, weight)) return rc;
    const double num = (double)(ndocs_total + 1u);
    for (uint32_t id = 0; id < ndf; id++) {
        const uint32_t f = df[id];
        float w = 0.0f;
        if (f != 0 && f >= min_df && f <= max_df && (keep == nullptr || keep[id] != 0))
            w = (float)(go_log(num / (double)((uint64_t)f + 1u)) + 1.0);
        weight[id] = w;
    }
    return JB_OK;
}

extern "C" int jb_idf_device(jb_ctx* ctx, const uint32_t* d_df, uint32_t ndf, uint64_t ndocs_total, uint32_t min_df,
                             uint32_t max_df, const uint8_t* d_keep, void* stream, float* d_weight) {
    if (!ctx) return fail(JB_EINVAL, "jb_idf_device: null ctx");
    if (const int rc = idf_args("jb_idf_device", d_df, ndf, ndocs_total, d_weight)) return rc;
    if (ndf == 0) return JB_OK;
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    if (d->profile) {
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_idf(d_df, ndf, ndocs_total, min_df, max_df, d_keep, d_weight, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_idf(d_df, ndf, ndocs_total, min_df, max_df, d_keep, d_weight, s, nullptr));
    return JB_OK;
}

// ---------------------------------------------------------------------------
// TextRank keywords (jb_textrank.hip; the host rule, jb_textrank, is jb_textrank.cpp)
// ---------------------------------------------------------------------------
static_assert(JB_TR_MAXSPAN == kTrMaxSpan && JB_TR_MAXITER == kTrMaxIter, "the header's constants are the kernels'");

extern "C" size_t jb_textrank_work_bytes(uint64_t max_tokens, uint64_t max_terms, uint32_t ndocs) {
    return textrank_work_bytes(max_tokens, max_terms, ndocs);
}

extern "C" int jb_textrank_device(jb_ctx* ctx, const uint32_t* d_ids, uint64_t ids_cap, const uint64_t* d_doc_tok,
                                  const uint64_t* d_ntok, uint32_t ndocs, const uint32_t* d_term_id,
                                  const uint64_t* d_term_off, uint64_t cap, const uint8_t* d_keep, uint32_t nkeep,
                                  uint32_t span, uint32_t iters, uint32_t topk, void* stream, uint32_t* d_kw_id,
                                  float* d_kw_score, uint32_t* d_kw_n, void* d_work, size_t nwork) {
    // (the limits come first: they need no ctx)
    if (const int rc = textrank_args("jb_textrank_device", ids_cap, cap, span, iters, topk)) return rc;
    if (!ctx || !d_doc_tok || !d_ntok || !d_term_off || !d_work || (ids_cap && !d_ids) || (cap && !d_term_id) ||
        (nkeep && !d_keep) || (ndocs && (!d_kw_id || !d_kw_score || !d_kw_n)))
        return fail(JB_EINVAL, "jb_textrank_device: null argument");
    if (((uintptr_t)d_work & 7u) != 0) return fail(JB_EINVAL, "jb_textrank_device: d_work must be 8-byte aligned");
    const size_t need = textrank_work_bytes(ids_cap, cap, ndocs);
    if (nwork < need)
        return fail(JB_EINVAL, "jb_textrank_device: a work buffer of %llu bytes, jb_textrank_work_bytes asks for %llu",
                    (unsigned long long)nwork, (unsigned long long)need);
    if (ndocs == 0) return JB_OK;
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    const bool window = d->lc.tr_window != 0;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_textrank(d_ids, ids_cap, d_doc_tok, d_ntok, ndocs, d_term_id, d_term_off, cap, d_keep, nkeep, span,
                            iters, topk, window, d_kw_id, d_kw_score, d_kw_n, d_work, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_textrank(d_ids, ids_cap, d_doc_tok, d_ntok, ndocs, d_term_id, d_term_off, cap, d_keep, nkeep, span, iters,
                        topk, window, d_kw_id, d_kw_score, d_kw_n, d_work, s, nullptr));
    return JB_OK;
}

// ---------------------------------------------------------------------------
// joined text (jb_join.hip; the host rule, jb_join, is jb_join.cpp)
// ---------------------------------------------------------------------------
static_assert(JB_JOIN_TILE == kJoinTile && JB_JOIN_LONG == kJoinLong && JB_JOIN_MAXSEP == kJoinMaxSep,
              "the header's constants are the kernels'");

extern "C" size_t jb_join_work_bytes(uint64_t max_tokens, uint32_t ndocs) { return join_work_bytes(max_tokens, ndocs); }

extern "C" int jb_join_device(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start,
                              const uint32_t* d_end, const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint64_t cap,
                              uint32_t ndocs, const uint8_t* sep, uint32_t seplen, const uint8_t* term, uint32_t termlen,
                              void* stream, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_doc_off, uint64_t* d_nout,
                              void* d_work, size_t nwork) {
    // (the limits come first: they need no ctx)
    if (const int rc = join_args("jb_join_device", nbytes, cap, sep, seplen, term, termlen)) return rc;
    if (!ctx || !d_text || !d_doc_tok || !d_ntok || !d_out_doc_off || !d_nout || !d_work || (cap && (!d_start || !d_end)) ||
        (out_cap && !d_out))
        return fail(JB_EINVAL, "jb_join_device: null argument");
    if (((uintptr_t)d_work & 7u) != 0) return fail(JB_EINVAL, "jb_join_device: d_work must be 8-byte aligned");
    const size_t need = join_work_bytes(cap, ndocs);
    if (nwork < need)
        return fail(JB_EINVAL, "jb_join_device: a work buffer of %llu bytes, jb_join_work_bytes asks for %llu",
                    (unsigned long long)nwork, (unsigned long long)need);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    const bool staged = d->lc.join_stage != 0;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_join(d_text, nbytes, d_start, d_end, d_doc_tok, d_ntok, cap, ndocs, sep, seplen, term, termlen, staged,
                        d_out, out_cap, d_out_doc_off, d_nout, d_work, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_join(d_text, nbytes, d_start, d_end, d_doc_tok, d_ntok, cap, ndocs, sep, seplen, term, termlen, staged, d_out,
                    out_cap, d_out_doc_off, d_nout, d_work, s, nullptr));
    return JB_OK;
}

// ---------------------------------------------------------------------------
// character offsets (jb_charspans.hip; the host rule, jb_charspans, is jb_charspans.cpp)
// ---------------------------------------------------------------------------
static_assert(JB_CHARSPANS_TILE == kCsTile, "the header's constant is the kernels'");

extern "C" size_t jb_charspans_work_bytes(uint64_t nbytes, uint32_t ndocs) { return charspans_work_bytes(nbytes, ndocs); }

extern "C" int jb_charspans_device(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint64_t* d_doc_off,
                                   uint32_t ndocs, const uint32_t* d_start, const uint32_t* d_end,
                                   const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint64_t cap, int unit, void* stream,
                                   uint32_t* d_cstart, uint32_t* d_cend, uint32_t* d_doc_units, void* d_work,
                                   size_t nwork) {
    // (the limits come first: they need no ctx)
    if (const int rc = charspans_args("jb_charspans_device", nbytes, cap, unit)) return rc;
    if (!ctx || !d_text || !d_doc_off || !d_doc_tok || !d_ntok || !d_work ||
        (cap && (!d_start || !d_end || !d_cstart || !d_cend)) || (ndocs && !d_doc_units))
        return fail(JB_EINVAL, "jb_charspans_device: null argument");
    if (((uintptr_t)d_work & 7u) != 0) return fail(JB_EINVAL, "jb_charspans_device: d_work must be 8-byte aligned");
    const size_t need = charspans_work_bytes(nbytes, ndocs);
    if (nwork < need)
        return fail(JB_EINVAL, "jb_charspans_device: a work buffer of %llu bytes, jb_charspans_work_bytes asks for %llu",
                    (unsigned long long)nwork, (unsigned long long)need);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    const bool utf16 = unit == JB_UNIT_UTF16;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_charspans(d_text, nbytes, d_doc_off, ndocs, d_start, d_end, d_doc_tok, d_ntok, cap, utf16, d_cstart,
                             d_cend, d_doc_units, d_work, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_charspans(d_text, nbytes, d_doc_off, ndocs, d_start, d_end, d_doc_tok, d_ntok, cap, utf16, d_cstart, d_cend,
                         d_doc_units, d_work, s, nullptr));
    return JB_OK;
}

// ---------------------------------------------------------------------------
// word counts (jb_wc.hip; the host rule, jb_wc_count, the reader and the size helpers are jb_wc.cpp)
// ---------------------------------------------------------------------------
extern "C" int jb_device_alloc(jb_ctx* ctx, size_t n, void** p) {
    if (!ctx || !p) return fail(JB_EINVAL, "jb_device_alloc: null argument");
    *p = nullptr;
    int ordinal;
    {
        std::shared_lock<std::shared_mutex> rl(ctx->lock);
        ordinal = ctx->devs[0]->ordinal;
    }
    HIPCHK(hipSetDevice(ordinal));
    if (hipMalloc(p, n ? n : 1) != hipSuccess) {
        *p = nullptr;
        return fail(JB_ENOMEM, "jb_device_alloc: no device memory for %llu bytes", (unsigned long long)n);
    }
    return JB_OK;
}

extern "C" void jb_device_free(jb_ctx* ctx, void* p) {
    if (!ctx || !p) return;
    int ordinal;
    {
        std::shared_lock<std::shared_mutex> rl(ctx->lock);
        ordinal = ctx->devs[0]->ordinal;
    }
    if (hipSetDevice(ordinal) == hipSuccess) (void)hipFree(p);  // (hipFree waits for the work that uses p)
}

extern "C" int jb_wc_init_device(jb_ctx* ctx, void* d_table, size_t ntable, uint64_t nslots, uint64_t pool_bytes,
                                 void* stream) {
    if (!ctx) return fail(JB_EINVAL, "jb_wc_init_device: null ctx");
    if (const int rc = wc_sizes("jb_wc_init_device", nslots, pool_bytes)) return rc;
    if (const int rc = wc_table_args("jb_wc_init_device", d_table, ntable)) return rc;
    if (ntable < jb_wc_bytes(nslots, pool_bytes))
        return fail(JB_EINVAL, "jb_wc_init_device: a table buffer of %llu bytes, jb_wc_table_bytes asks for %llu",
                    (unsigned long long)ntable, (unsigned long long)jb_wc_bytes(nslots, pool_bytes));
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    HIPCHK(run_wc_init(d_table, nslots, pool_bytes, d->ncu, (hipStream_t)stream));
    return JB_OK;
}

extern "C" int jb_wc_add_device(jb_ctx* ctx, void* d_table, size_t ntable, const uint8_t* d_text, uint64_t nbytes,
                                const uint32_t* d_start, const uint32_t* d_end, const uint64_t* d_ntok, uint64_t cap,
                                void* stream, void* d_work, size_t nwork) {
    if (!ctx || (!d_text && nbytes) || !d_ntok || (cap && (!d_start || !d_end || !d_work)))
        return fail(JB_EINVAL, "jb_wc_add_device: null argument");
    if (nbytes >= (1ull << 31))
        return fail(JB_ELIMIT, "device batch of %llu bytes (limit 2 GiB)", (unsigned long long)nbytes);
    if (cap >= (1ull << 32) - kWcTile)
        return fail(JB_ELIMIT, "jb_wc_add_device: a span list of %llu entries (limit 2^32 - %u)", (unsigned long long)cap,
                    kWcTile);
    if (const int rc = wc_table_args("jb_wc_add_device", d_table, ntable)) return rc;
    if (((uintptr_t)d_text & 3u) != 0) return fail(JB_EINVAL, "d_text must be 4-byte aligned");
    if (((uintptr_t)d_work & 3u) != 0) return fail(JB_EINVAL, "jb_wc_add_device: d_work must be 4-byte aligned");
    const size_t need = jb_wc_work_bytes(cap);
    if (cap && nwork < need)
        return fail(JB_EINVAL, "jb_wc_add_device: a work buffer of %llu bytes, jb_wc_work_bytes asks for %llu",
                    (unsigned long long)nwork, (unsigned long long)need);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    const bool combine = d->lc.wc_combine != 0;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_wc_add(d_table, ntable, d_text, nbytes, d_start, d_end, d_ntok, cap, d->lc.wc_bits, combine,
                          (uint32_t*)d_work, d->ncu, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_wc_add(d_table, ntable, d_text, nbytes, d_start, d_end, d_ntok, cap, d->lc.wc_bits, combine,
                      (uint32_t*)d_work, d->ncu, s, nullptr));
    return JB_OK;
}

extern "C" int jb_wc_read(jb_ctx* ctx, const void* d_table, size_t ntable, void* stream, uint64_t min_count,
                          uint64_t max_keys, jb_wc_result* out) {
    if (!ctx || !out) return fail(JB_EINVAL, "jb_wc_read: null argument");
    memset(out, 0, sizeof *out);
    if (const int rc = wc_table_args("jb_wc_read", d_table, ntable)) return rc;
    int ordinal;
    {
        std::shared_lock<std::shared_mutex> rl(ctx->lock);
        ordinal = ctx->devs[0]->ordinal;
    }
    HIPCHK(hipSetDevice(ordinal));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    // the header says how much of the buffer the table takes
    JbWcHeader h;
    HIPCHK(hipMemcpy(&h, d_table, sizeof h, hipMemcpyDeviceToHost));
    if (h.magic != JB_WC_MAGIC || wc_sizes("jb_wc_read", h.nslots, h.pool_bytes) != JB_OK ||
        jb_wc_bytes(h.nslots, h.pool_bytes) > ntable)
        return fail(JB_EINVAL, "jb_wc_read: the buffer holds no table (jb_wc_init_device)");
    const size_t nb = (size_t)jb_wc_bytes(h.nslots, h.pool_bytes);
    void* host = malloc(nb);
    if (!host) return fail(JB_ENOMEM, "jb_wc_read: out of host memory for a table of %llu bytes", (unsigned long long)nb);
    const hipError_t e = hipMemcpy(host, d_table, nb, hipMemcpyDeviceToHost);
    int rc = e == hipSuccess ? wc_read_host(host, nb, min_count, max_keys, out)
                             : fail(JB_EDEVICE, "jb_wc_read: %s", hipGetErrorString(e));
    free(host);
    if (rc) jb_wc_result_free(out);
    return rc;
}

// ---------------------------------------------------------------------------
// MinHash signatures (jb_minhash.hip; the host rule, jb_minhash, jb_minhash_params, jb_minhash_bands and the
// size helper are jb_minhash.cpp)
// ---------------------------------------------------------------------------
static_assert(JB_MH_TILE == kMhTile && JB_MH_MAXN == kMhMaxN && JB_MH_MAXK == kMhMaxK,
              "the header's constants are the kernels'");

extern "C" int jb_minhash_device(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start,
                                 const uint32_t* d_end, const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint64_t cap,
                                 uint32_t ndocs, uint32_t n, uint32_t K, uint64_t seed, void* stream, uint32_t* d_sig,
                                 uint32_t* d_doc_n, void* d_work, size_t nwork) {
    const char* who = "jb_minhash_device";
    // (the limits come first: they need no ctx)
    if (const int rc = minhash_args(who, nbytes, cap, n, K)) return rc;
    if (!ctx || (!d_text && nbytes) || !d_doc_tok || !d_ntok || !d_work || (cap && (!d_start || !d_end)) ||
        (ndocs && (!d_sig || !d_doc_n)))
        return fail(JB_EINVAL, "%s: null argument", who);
    if (((uintptr_t)d_text & 3u) != 0) return fail(JB_EINVAL, "d_text must be 4-byte aligned");
    if (((uintptr_t)d_work & 7u) != 0) return fail(JB_EINVAL, "%s: d_work must be 8-byte aligned", who);
    const size_t need = jb_minhash_work_bytes(cap, ndocs);
    if (nwork < need)
        return fail(JB_EINVAL, "%s: a work buffer of %llu bytes, jb_minhash_work_bytes asks for %llu", who,
                    (unsigned long long)nwork, (unsigned long long)need);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    const bool staged = d->lc.mh_form != 0;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_minhash(d_text, nbytes, d_start, d_end, d_doc_tok, d_ntok, cap, ndocs, n, K, seed, staged, d_sig,
                           d_doc_n, (uint64_t*)d_work, d->ncu, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_minhash(d_text, nbytes, d_start, d_end, d_doc_tok, d_ntok, cap, ndocs, n, K, seed, staged, d_sig, d_doc_n,
                       (uint64_t*)d_work, d->ncu, s, nullptr));
    return JB_OK;
}

extern "C" int jb_minhash_bands_device(jb_ctx* ctx, const uint32_t* d_sig, const uint32_t* d_doc_n, uint32_t ndocs,
                                       uint32_t K, uint32_t B, uint32_t R, void* stream, uint64_t* d_keys) {
    const char* who = "jb_minhash_bands_device";
    if (const int rc = minhash_band_args(who, K, B, R)) return rc;
    if (!ctx || (ndocs && (!d_sig || !d_doc_n || !d_keys))) return fail(JB_EINVAL, "%s: null argument", who);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_minhash_bands(d_sig, d_doc_n, ndocs, K, B, R, d_keys, d->ncu, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_minhash_bands(d_sig, d_doc_n, ndocs, K, B, R, d_keys, d->ncu, s, nullptr));
    return JB_OK;
}

// ---------------------------------------------------------------------------
// The token filter (jb_filter.hip; the host rule, jb_filter, the argument checks and the size helper are
// jb_filter.cpp; the stop set, jb_stopwords_set, is with jb_vocab_set above)
// ---------------------------------------------------------------------------
static_assert(JB_FILTER_TILE == kFiltTile, "the header's constant is the kernels'");

extern "C" int jb_filter_device(jb_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint32_t* d_start,
                                const uint32_t* d_end, const uint64_t* d_doc_tok, const uint64_t* d_ntok, uint64_t cap,
                                uint32_t ndocs, const jb_filter_rule* rule, void* stream, uint32_t* d_out_start,
                                uint32_t* d_out_end, uint32_t* d_out_src, uint64_t out_cap, uint64_t* d_out_doc_tok,
                                uint64_t* d_out_ntok, uint64_t* d_stats, void* d_work, size_t nwork) {
    const char* who = "jb_filter_device";
    // (the limits come first: they need no ctx; the stop set is looked at under the lock)
    if (const int rc = filter_args(who, nbytes, cap, rule, true)) return rc;
    if (!ctx || (!d_text && nbytes) || !d_doc_tok || !d_ntok || !d_out_doc_tok || !d_out_ntok || !d_stats || !d_work ||
        (cap && (!d_start || !d_end)) || (out_cap && (!d_out_start || !d_out_end)))
        return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = filter_alias(who, d_start, d_end, d_doc_tok, d_out_start, d_out_end, d_out_src, d_out_doc_tok))
        return rc;
    if (((uintptr_t)d_text & 3u) != 0) return fail(JB_EINVAL, "d_text must be 4-byte aligned");
    if (((uintptr_t)d_work & 7u) != 0) return fail(JB_EINVAL, "%s: d_work must be 8-byte aligned", who);
    const size_t need = jb_filter_work_bytes(cap, ndocs);
    if (nwork < need)
        return fail(JB_EINVAL, "%s: a work buffer of %llu bytes, jb_filter_work_bytes asks for %llu", who,
                    (unsigned long long)nwork, (unsigned long long)need);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    if ((rule->flags & JB_FILTER_STOP) && !ctx->stopw)
        return fail(JB_EINVAL, "%s: JB_FILTER_STOP without a stop set (jb_stopwords_set)", who);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_filter(d_text, nbytes, d_start, d_end, d_doc_tok, d_ntok, cap, ndocs, *rule, ctx->dstop, d_out_start,
                          d_out_end, d_out_src, out_cap, d_out_doc_tok, d_out_ntok, d_stats, d_work, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_filter(d_text, nbytes, d_start, d_end, d_doc_tok, d_ntok, cap, ndocs, *rule, ctx->dstop, d_out_start,
                      d_out_end, d_out_src, out_cap, d_out_doc_tok, d_out_ntok, d_stats, d_work, s, nullptr));
    return JB_OK;
}

// ---------------------------------------------------------------------------
// Postings (jb_postings.hip; the host rule, jb_postings, the argument checks, the work buffer's layout and the
// size helper are jb_postings.cpp)
// ---------------------------------------------------------------------------
static_assert(JB_POSTINGS_TILE == kPostTile, "the header's constant is the kernels'");

extern "C" int jb_postings_device(jb_ctx* ctx, const uint32_t* d_term_id, const uint32_t* d_term_cnt,
                                  const uint64_t* d_term_off, const uint64_t* d_nterms, uint64_t cap, uint32_t ndocs,
                                  uint32_t nids, uint32_t doc_base, void* stream, uint32_t* d_post_doc,
                                  uint32_t* d_post_tf, uint64_t pcap, uint64_t* d_post_off, uint64_t* d_nposts,
                                  void* d_work, size_t nwork) {
    const char* who = "jb_postings_device";
    // (the limits come first: they need no ctx)
    if (const int rc = postings_args(who, cap, ndocs, doc_base)) return rc;
    if (!ctx || !d_term_off || !d_nterms || !d_post_off || !d_nposts || !d_work || (cap && (!d_term_id || !d_term_cnt)) ||
        (pcap && (!d_post_doc || !d_post_tf)))
        return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = postings_alias(who, d_term_id, d_term_cnt, d_term_off, d_nterms, d_post_doc, d_post_tf, d_post_off,
                                      d_nposts, d_work))
        return rc;
    if (((uintptr_t)d_work & 7u) != 0) return fail(JB_EINVAL, "%s: d_work must be 8-byte aligned", who);
    const size_t need = jb_postings_work_bytes(cap, nids, ndocs);
    if (nwork < need)
        return fail(JB_EINVAL, "%s: a work buffer of %llu bytes, jb_postings_work_bytes asks for %llu", who,
                    (unsigned long long)nwork, (unsigned long long)need);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t form = d->lc.post_form;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_postings(d_term_id, d_term_cnt, d_term_off, d_nterms, cap, ndocs, nids, doc_base, form, d_post_doc,
                            d_post_tf, pcap, d_post_off, d_nposts, d_work, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_postings(d_term_id, d_term_cnt, d_term_off, d_nterms, cap, ndocs, nids, doc_base, form, d_post_doc,
                        d_post_tf, pcap, d_post_off, d_nposts, d_work, s, nullptr));
    return JB_OK;
}

// ---------------------------------------------------------------------------
// Collocations (jb_colloc.hip; the host rules, jb_colloc_count and jb_colloc_score, the argument checks, the
// sort of a result and the size helpers are jb_colloc.cpp)
// ---------------------------------------------------------------------------
static_assert(JB_COLLOC_TILE == kClTile && JB_COLLOC_LDS == kClLds && JB_COLLOC_SHARE == kClShare,
              "the header's constants are the kernels'");

namespace {

// The slots a buffer of ntable bytes has room for: the score pass's grid (the kernel reads the header itself).
uint64_t colloc_room(size_t ntable) { return (ntable - JB_CL_HDR_BYTES) / JB_CL_SLOT_BYTES; }

}  // namespace

extern "C" int jb_colloc_init_device(jb_ctx* ctx, void* d_table, size_t ntable, uint64_t nslots, uint64_t* d_uni,
                                     uint32_t nuni, void* stream) {
    const char* who = "jb_colloc_init_device";
    if (!ctx) return fail(JB_EINVAL, "%s: null ctx", who);
    if (const int rc = colloc_slots(who, nslots)) return rc;
    if (const int rc = colloc_table_args(who, d_table, ntable, d_uni, nuni)) return rc;
    if (ntable < jb_cl_bytes(nslots))
        return fail(JB_EINVAL, "%s: a table buffer of %llu bytes, jb_colloc_table_bytes asks for %llu", who,
                    (unsigned long long)ntable, (unsigned long long)jb_cl_bytes(nslots));
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    HIPCHK(run_colloc_init(d_table, nslots, d_uni, nuni, d->ncu, (hipStream_t)stream));
    return JB_OK;
}

extern "C" int jb_colloc_add_device(jb_ctx* ctx, void* d_table, size_t ntable, uint64_t* d_uni, uint32_t nuni,
                                    const uint32_t* d_ids, uint64_t ids_cap, const uint64_t* d_doc_tok,
                                    const uint64_t* d_ntok, uint32_t ndocs, const uint8_t* d_keep, uint32_t nkeep,
                                    uint32_t flags, const uint32_t* d_start, const uint32_t* d_end, void* stream,
                                    void* d_work, size_t nwork) {
    const char* who = "jb_colloc_add_device";
    if (const int rc = colloc_add_args(who, d_ids, ids_cap, d_doc_tok, d_keep, nkeep, flags, d_start, d_end, d_uni, nuni))
        return rc;
    if (!ctx || !d_ntok || (ids_cap && !d_work)) return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = colloc_table_args(who, d_table, ntable, d_uni, nuni)) return rc;
    if (((uintptr_t)d_work & 3u) != 0) return fail(JB_EINVAL, "%s: d_work must be 4-byte aligned", who);
    const size_t need = jb_colloc_work_bytes(ids_cap, ndocs);
    if (ids_cap && nwork < need)
        return fail(JB_EINVAL, "%s: a work buffer of %llu bytes, jb_colloc_work_bytes asks for %llu", who,
                    (unsigned long long)nwork, (unsigned long long)need);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    const bool combine = d->lc.colloc_combine != 0;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_colloc_add(d_table, ntable, d_uni, nuni, d_ids, ids_cap, d_doc_tok, d_ntok, ndocs, d_keep, nkeep, flags,
                              d_start, d_end, combine, d_work, d->ncu, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_colloc_add(d_table, ntable, d_uni, nuni, d_ids, ids_cap, d_doc_tok, d_ntok, ndocs, d_keep, nkeep, flags,
                          d_start, d_end, combine, d_work, d->ncu, s, nullptr));
    return JB_OK;
}

extern "C" int jb_colloc_score_device(jb_ctx* ctx, const void* d_table, size_t ntable, const uint64_t* d_uni, uint32_t nuni,
                                      int scorer, uint64_t min_count, float threshold, uint32_t* d_cand_a,
                                      uint32_t* d_cand_b, uint64_t* d_cand_cnt, float* d_cand_score, uint64_t ccap,
                                      uint64_t* d_ncand, void* stream) {
    const char* who = "jb_colloc_score_device";
    if (const int rc = colloc_score_args(who, d_uni, nuni, scorer, min_count)) return rc;
    if (!ctx || !d_ncand || (ccap && (!d_cand_a || !d_cand_b || !d_cand_cnt || !d_cand_score)))
        return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = colloc_table_args(who, d_table, ntable, d_uni, nuni)) return rc;
    if (((uintptr_t)d_ncand & 7u) != 0 || ((uintptr_t)d_cand_cnt & 7u) != 0 || ((uintptr_t)d_cand_a & 3u) != 0 ||
        ((uintptr_t)d_cand_b & 3u) != 0 || ((uintptr_t)d_cand_score & 3u) != 0)
        return fail(JB_EINVAL, "%s: a candidate array is not aligned to its entries", who);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    if (d->profile) {
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_colloc_score(d_table, ntable, colloc_room(ntable), d_uni, nuni, scorer, min_count, threshold, d_cand_a,
                                d_cand_b, d_cand_cnt, d_cand_score, ccap, d_ncand, d->ncu, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_colloc_score(d_table, ntable, colloc_room(ntable), d_uni, nuni, scorer, min_count, threshold, d_cand_a,
                            d_cand_b, d_cand_cnt, d_cand_score, ccap, d_ncand, d->ncu, s, nullptr));
    return JB_OK;
}

extern "C" int jb_colloc_read(jb_ctx* ctx, const void* d_table, size_t ntable, const uint64_t* d_uni, uint32_t nuni,
                              int scorer, uint64_t min_count, float threshold, uint64_t topn, void* stream,
                              jb_colloc_result* out) {
    const char* who = "jb_colloc_read";
    if (!ctx || !out) return fail(JB_EINVAL, "%s: null argument", who);
    memset(out, 0, sizeof *out);
    if (const int rc = colloc_score_args(who, d_uni, nuni, scorer, min_count)) return rc;
    if (const int rc = colloc_table_args(who, d_table, ntable, d_uni, nuni)) return rc;
    int ordinal;
    {
        std::shared_lock<std::shared_mutex> rl(ctx->lock);
        ordinal = ctx->devs[0]->ordinal;
    }
    HIPCHK(hipSetDevice(ordinal));
    const hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipStreamSynchronize(st));
    JbClHeader h;
    HIPCHK(hipMemcpy(&h, d_table, sizeof h, hipMemcpyDeviceToHost));
    if (h.magic != JB_CL_MAGIC || !jb_cl_slots_ok(h.nslots) || jb_cl_bytes(h.nslots) > ntable)
        return fail(JB_EINVAL, "%s: the buffer holds no table (jb_colloc_init_device)", who);
    // the candidates are at most the claimed keys; the buffer starts smaller and grows to the count once
    uint64_t ccap = std::max<uint64_t>(1u, std::min<uint64_t>(std::min<uint64_t>(h.ctr[JB_CL_DISTINCT], h.nslots), 1u << 16));
    uint64_t ncand = 0;
    uint8_t* buf = nullptr;
    auto run = [&]() -> int {
        for (int pass = 0; pass < 2; pass++) {
            // the candidate count, the counts (u64), then a, b (u32) and the scores (f32)
            HIPCHK(hipMalloc(&buf, 8u + ccap * 20u));
            uint64_t* dn = (uint64_t*)buf;
            uint64_t* cc = dn + 1;
            uint32_t* ca = (uint32_t*)(cc + ccap);
            if (const int rc = jb_colloc_score_device(ctx, d_table, ntable, d_uni, nuni, scorer, min_count, threshold, ca,
                                                      ca + ccap, cc, (float*)(ca + 2u * ccap), ccap, dn, stream))
                return rc;
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipMemcpy(&ncand, dn, 8, hipMemcpyDeviceToHost));
            if (ncand <= ccap) break;
            if (pass == 1) return fail(JB_EDEVICE, "%s: the table changed while it was read", who);
            (void)hipFree(buf);
            buf = nullptr;
            ccap = ncand;
        }
        if (const int rc = colloc_alloc(who, ncand, out)) return rc;
        if (ncand) {
            const uint64_t* cc = (const uint64_t*)buf + 1;
            const uint32_t* ca = (const uint32_t*)(cc + ccap);
            HIPCHK(hipMemcpy(out->count, cc, ncand * 8u, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(out->a, ca, ncand * 4u, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(out->b, ca + ccap, ncand * 4u, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(out->score, ca + 2u * ccap, ncand * 4u, hipMemcpyDeviceToHost));
        }
        return JB_OK;
    };
    int rc = run();
    if (buf) (void)hipFree(buf);
    if (rc == JB_OK) {
        try {
            colloc_sort(out, topn);
        } catch (const std::bad_alloc&) {
            rc = fail(JB_ENOMEM, "%s: out of host memory", who);
        }
    }
    if (rc) {
        jb_colloc_result_free(out);
        return rc;
    }
    out->tokens = h.ctr[JB_CL_TOKENS];
    out->known = h.ctr[JB_CL_KNOWN];
    out->pairs = h.ctr[JB_CL_PAIRS];
    out->dropped = h.ctr[JB_CL_DROPPED];
    out->distinct = h.ctr[JB_CL_DISTINCT];
    return JB_OK;
}

// ---------------------------------------------------------------------------
// Near-duplicate pairs (jb_neardup.hip; the host rule, jb_neardup, jb_neardup_labels, the argument checks, the
// work buffer's layout and the size helper are jb_neardup.cpp)
// ---------------------------------------------------------------------------
static_assert(JB_ND_TILE == kNdTile && JB_ND_MAXWIN == kNdMaxWin, "the header's constants are the kernels'");

extern "C" int jb_neardup_device(jb_ctx* ctx, const uint64_t* d_key, const uint32_t* d_sig, uint32_t ndocs, uint32_t B,
                                 uint32_t K, uint32_t W, uint32_t min_agree, uint32_t* d_pair_doc, uint32_t* d_pair_agree,
                                 uint64_t pcap, uint64_t* d_pair_off, uint64_t* d_npairs, uint64_t* d_stat, void* d_work,
                                 size_t nwork, void* stream) {
    const char* who = "jb_neardup_device";
    // (the limits come first: they need no ctx)
    if (const int rc = neardup_args(who, ndocs, B, K, W, min_agree)) return rc;
    if (!ctx || !d_pair_off || !d_npairs || !d_stat || !d_work || (ndocs && (!d_key || !d_sig)) ||
        (pcap && (!d_pair_doc || !d_pair_agree)))
        return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = neardup_alias(who, d_key, d_sig, d_pair_doc, d_pair_agree, d_pair_off, d_npairs, d_stat, d_work))
        return rc;
    if (((uintptr_t)d_work & 7u) != 0) return fail(JB_EINVAL, "%s: d_work must be 8-byte aligned", who);
    const size_t need = jb_neardup_work_bytes(ndocs, B);
    if (nwork < need)
        return fail(JB_EINVAL, "%s: a work buffer of %llu bytes, jb_neardup_work_bytes asks for %llu", who,
                    (unsigned long long)nwork, (unsigned long long)need);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const hipStream_t s = (hipStream_t)stream;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_neardup(d_key, d_sig, ndocs, B, K, W, min_agree, d_pair_doc, d_pair_agree, pcap, d_pair_off, d_npairs,
                           d_stat, d_work, s, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_neardup(d_key, d_sig, ndocs, B, K, W, min_agree, d_pair_doc, d_pair_agree, pcap, d_pair_off, d_npairs,
                       d_stat, d_work, s, nullptr));
    return JB_OK;
}

// ---------------------------------------------------------------------------
// BM25 search (jb_bm25.hip; the host rules, the argument checks, the work buffer's layout and the size helper
// are jb_bm25.cpp)
// ---------------------------------------------------------------------------
static_assert(JB_BM25_TILE == kBm25Tile && JB_BM25_MAXQ == kBm25MaxQ, "the header's constants are the kernels'");

extern "C" int jb_bm25_norms_device(jb_ctx* ctx, const uint32_t* d_doc_len, uint32_t ndocs, double k1, double b,
                                    double avgdl, void* stream, float* d_norm) {
    const char* who = "jb_bm25_norms_device";
    if (const int rc = bm25_params(who, k1, b)) return rc;
    if (const int rc = bm25_avgdl_ok(who, avgdl)) return rc;
    if (!ctx || (ndocs && (!d_doc_len || !d_norm))) return fail(JB_EINVAL, "%s: null argument", who);
    if (ndocs && (const void*)d_doc_len == (const void*)d_norm) return fail(JB_EINVAL, "%s: the output is the input", who);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_bm25_norms(d_doc_len, ndocs, k1, b, avgdl, d_norm, (hipStream_t)stream, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_bm25_norms(d_doc_len, ndocs, k1, b, avgdl, d_norm, (hipStream_t)stream, nullptr));
    return JB_OK;
}

extern "C" int jb_bm25_idf_device(jb_ctx* ctx, const uint64_t* d_post_off, uint32_t nids, uint64_t ndocs_total,
                                  void* stream, float* d_weight) {
    const char* who = "jb_bm25_idf_device";
    if (ndocs_total >= (1ull << 53))
        return fail(JB_ELIMIT, "%s: %llu documents (limit 2^53)", who, (unsigned long long)ndocs_total);
    if (!ctx || !d_post_off || (nids && !d_weight)) return fail(JB_EINVAL, "%s: null argument", who);
    if ((const void*)d_post_off == (const void*)d_weight) return fail(JB_EINVAL, "%s: the output is the input", who);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    if (d->profile) {
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_bm25_idf(d_post_off, nids, ndocs_total, d_weight, (hipStream_t)stream, &d->timer));
        return JB_OK;
    }
    HIPCHK(run_bm25_idf(d_post_off, nids, ndocs_total, d_weight, (hipStream_t)stream, nullptr));
    return JB_OK;
}

// The search, queued: the caller holds the ctx's lock (shared or exclusive) and has checked the arguments
// (jb_search_batch, in jb_batch.cpp, queues it too).
int bm25_queue(jb_ctx* ctx, const uint32_t* d_post_doc, const uint32_t* d_post_tf, const uint64_t* d_post_off,
               uint64_t npost, uint32_t nids, const float* d_norm, uint32_t ndocs, const float* d_weight,
               uint32_t nweights, double k1, const uint32_t* d_q_id, uint64_t q_cap, const uint64_t* d_q_off, uint32_t nq,
               uint32_t topk, hipStream_t s, uint32_t* d_res_doc, uint64_t* d_res_score, uint32_t* d_res_n, void* d_work) {
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    const uint32_t form = d->lc.bm25_form;
    if (d->profile) {  // (the timer's event lists are the device's, under its lock)
        std::lock_guard<std::mutex> g(d->mu);
        HIPCHK(run_bm25_search(d_post_doc, d_post_tf, d_post_off, npost, nids, d_norm, ndocs, d_weight, nweights, k1,
                               d_q_id, q_cap, d_q_off, nq, topk, form, d_res_doc, d_res_score, d_res_n, d_work, s,
                               &d->timer));
        return JB_OK;
    }
    HIPCHK(run_bm25_search(d_post_doc, d_post_tf, d_post_off, npost, nids, d_norm, ndocs, d_weight, nweights, k1, d_q_id,
                           q_cap, d_q_off, nq, topk, form, d_res_doc, d_res_score, d_res_n, d_work, s, nullptr));
    return JB_OK;
}

extern "C" int jb_bm25_search_device(jb_ctx* ctx, const uint32_t* d_post_doc, const uint32_t* d_post_tf,
                                     const uint64_t* d_post_off, uint64_t npost, uint32_t nids, const float* d_norm,
                                     uint32_t ndocs, const float* d_weight, uint32_t nweights, double k1,
                                     const uint32_t* d_q_id, uint64_t q_cap, const uint64_t* d_q_off, uint32_t nq,
                                     uint32_t topk, void* stream, uint32_t* d_res_doc, uint64_t* d_res_score,
                                     uint32_t* d_res_n, void* d_work, size_t nwork) {
    const char* who = "jb_bm25_search_device";
    // (the limits come first: they need no ctx)
    if (const int rc = bm25_topk(who, topk)) return rc;
    if (const int rc = bm25_params(who, k1, 0.0)) return rc;
    if (!ctx || !d_work) return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = bm25_search_args(who, d_post_doc, d_post_tf, d_post_off, npost, d_norm, ndocs, d_weight, nweights,
                                        d_q_id, q_cap, d_q_off, nq, d_res_doc, d_res_score, d_res_n, d_work))
        return rc;
    if (((uintptr_t)d_work & 7u) != 0) return fail(JB_EINVAL, "%s: d_work must be 8-byte aligned", who);
    const size_t need = jb_bm25_work_bytes(nq, ndocs, topk);
    if (nwork < need)
        return fail(JB_EINVAL, "%s: a work buffer of %llu bytes, jb_bm25_work_bytes asks for %llu", who,
                    (unsigned long long)nwork, (unsigned long long)need);
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    return bm25_queue(ctx, d_post_doc, d_post_tf, d_post_off, npost, nids, d_norm, ndocs, d_weight, nweights, k1, d_q_id,
                      q_cap, d_q_off, nq, topk, (hipStream_t)stream, d_res_doc, d_res_score, d_res_n, d_work);
}

namespace {
// The old index may be in use by kernels queued earlier, on any stream of the device (under the exclusive lock).
void index_drop(jb_ctx* ctx) {
    if (!ctx->index.base) return;
    (void)hipDeviceSynchronize();
    dfree(ctx->index.base);
    ctx->index = jb_ctx::Index{};
}
}  // namespace

extern "C" int jb_index_set(jb_ctx* ctx, const uint64_t* post_off, const uint32_t* post_doc, const uint32_t* post_tf,
                            uint64_t npost, uint32_t nids, const uint32_t* doc_len, uint64_t ndocs, double k1, double b) {
    const char* who = "jb_index_set";
    if (ndocs >= (1ull << 32)) return fail(JB_ELIMIT, "%s: %llu documents (limit 2^32)", who, (unsigned long long)ndocs);
    if (npost >= (1ull << 32)) return fail(JB_ELIMIT, "%s: %llu postings (limit 2^32)", who, (unsigned long long)npost);
    if (const int rc = bm25_params(who, k1, b)) return rc;
    if (!ctx || !post_off || (npost && (!post_doc || !post_tf)) || (ndocs && !doc_len))
        return fail(JB_EINVAL, "%s: null argument", who);
    double avgdl = 0;
    if (jb_bm25_avgdl(doc_len, (uint32_t)ndocs, &avgdl)) return fail(JB_EINVAL, "%s: an index without a token", who);
    const uint32_t nd = (uint32_t)ndocs;
    const size_t noff = ((size_t)nids + 1) * 8, np4 = std::max<size_t>(npost, 1) * 4, nd4 = (size_t)nd * 4,
                 nw4 = std::max<size_t>(nids, 1) * 4;
    std::unique_lock<std::shared_mutex> wl(ctx->lock);
    Device* d = ctx->devs[0].get();
    HIPCHK(hipSetDevice(d->ordinal));
    // built aside: on any error the old index stays attached
    void* base = nullptr;
    {
        const hipError_t e = hipMalloc(&base, r256(noff) + 2 * r256(np4) + 2 * r256(nd4) + r256(nw4));
        if (e != hipSuccess) return fail(JB_EDEVICE, "%s: allocating the index: %s", who, hipGetErrorString(e));
    }
    Arena a;
    a.p = (uint8_t*)base;
    jb_ctx::Index ix;
    ix.base = base;
    uint64_t* doff = (uint64_t*)a.take(noff);
    uint32_t* ddoc = (uint32_t*)a.take(np4);
    uint32_t* dtf = (uint32_t*)a.take(np4);
    uint32_t* dlen = (uint32_t*)a.take(nd4);
    float* dnorm = (float*)a.take(nd4);
    float* dwt = (float*)a.take(nw4);
    hipError_t e = hipMemcpy(doff, post_off, noff, hipMemcpyHostToDevice);
    if (e == hipSuccess && npost) e = hipMemcpy(ddoc, post_doc, (size_t)npost * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && npost) e = hipMemcpy(dtf, post_tf, (size_t)npost * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dlen, doc_len, nd4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = run_bm25_norms(dlen, nd, k1, b, avgdl, dnorm, nullptr, nullptr);
    if (e == hipSuccess) e = run_bm25_idf(doff, nids, ndocs, dwt, nullptr, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        dfree(base);
        return fail(JB_EDEVICE, "%s: uploading the index: %s", who, hipGetErrorString(e));
    }
    ix.post_off = doff;
    ix.post_doc = ddoc;
    ix.post_tf = dtf;
    ix.norm = dnorm;
    ix.weight = dwt;
    ix.npost = npost;
    ix.nids = nids;
    ix.ndocs = nd;
    ix.k1 = k1;
    ix.b = b;
    ix.avgdl = avgdl;
    index_drop(ctx);
    ctx->index = ix;
    return JB_OK;
}

extern "C" int jb_index_clear(jb_ctx* ctx) {
    if (!ctx) return fail(JB_EINVAL, "jb_index_clear: null ctx");
    std::unique_lock<std::shared_mutex> wl(ctx->lock);
    HIPCHK(hipSetDevice(ctx->devs[0]->ordinal));
    index_drop(ctx);
    return JB_OK;
}

extern "C" int jb_index_info(jb_ctx* ctx, uint64_t* ndocs, uint64_t* nids, uint64_t* npost, double* avgdl) {
    if (!ctx) return fail(JB_EINVAL, "jb_index_info: null ctx");
    std::shared_lock<std::shared_mutex> rl(ctx->lock);
    if (!ctx->index.base) return fail(JB_EINVAL, "jb_index_info: no index attached (jb_index_set)");
    if (ndocs) *ndocs = ctx->index.ndocs;
    if (nids) *nids = ctx->index.nids;
    if (npost) *npost = ctx->index.npost;
    if (avgdl) *avgdl = ctx->index.avgdl;
    return JB_OK;
}
