// jb_device.h — one device of a context: its image, workspace, streams, launch shape and graph
// cache, and the context that owns the devices.  Library-internal (jb_device.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/jiebahip.h"
#include "jb_batch.h"
#include "jb_err.h"
#include "jb_image.h"
#include "jb_kernels.h"

using namespace jb;

#pragma GCC visibility push(hidden)

struct jb_image {
    Dictionary dict;
    Emission emit;
    Image img;
    int dict_kind = 0;
};

// Per-launch HIP events, recorded on the launch stream.
struct EventTimer final : KernelTimer {
    struct Rec { int id; hipEvent_t a, b; };
    std::vector<hipEvent_t> pool;
    std::vector<Rec> recs;
    size_t used = 0;
    hipEvent_t cur_a = nullptr;
    double ms[K_NUM] = {0};
    uint64_t launches[K_NUM] = {0};
    hipEvent_t take() {
        if (used == pool.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            pool.push_back(e);
        }
        return pool[used++];
    }
    void begin(int, hipStream_t s) override {
        cur_a = take();
        if (cur_a) (void)hipEventRecord(cur_a, s);
    }
    void end(int id, hipStream_t s) override {
        hipEvent_t b = take();
        if (b && cur_a) {
            (void)hipEventRecord(b, s);
            recs.push_back(Rec{id, cur_a, b});
        }
    }
    void harvest() {
        for (const Rec& r : recs) {
            (void)hipEventSynchronize(r.b);
            float t = 0;
            if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
                ms[r.id] += t;
                launches[r.id]++;
            }
        }
        recs.clear();
        used = 0;
    }
    void reset() {
        harvest();
        for (int k = 0; k < K_NUM; k++) { ms[k] = 0; launches[k] = 0; }
    }
    ~EventTimer() override {
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    }
};

// One device's copy of the image (jb_common.h layout).
struct ImageBufs {
    uint16_t* pagemap = nullptr;
    double* emit = nullptr;
    uint64_t* cells = nullptr;
    uint32_t* code = nullptr;
    double* wtab = nullptr;
    uint64_t* l1row = nullptr;
    uint64_t* hot = nullptr;  // hot level-1 rows: JB_HOT_SLOTS u64 values, then u16 tags
};

struct SmallReq;  // (jb_small.cpp)

// Which list a cut returns: Cut's tokens, their search-mode expansion (run_search) or the full-mode
// list (run_full).  Each mode has its own captured graph.
enum CutMode { kModePlain = 0, kModeSearch = 1, kModeFull = 2 };

struct Device {
    int ordinal = 0;
    std::mutex mu;  // one pipeline at a time per device workspace
    hipStream_t stream = nullptr;
    ImageBufs ib{};  // the device image
    DevImage dim{};
    // workspace
    Work w{};
    // search mode (jb_cut_*_search): the expanded spans and the pass's workspace, allocated by the
    // first search call and again whenever the workspace grows (ensure_search)
    SearchOut srch{};
    uint64_t srch_gen = 0;  // work_gen they were sized for
    // full mode (jb_cut_*_full) shares them (both are valid only until the next call) and adds the
    // per-tile bases of its 64-bit offsets
    uint64_t* full_tbase = nullptr;
    uint64_t full_gen = 0;
    uint32_t maxlen = 1;  // the image's longest key, runes (full mode's look-back reach)
    uint8_t* text = nullptr;   // staging for host batches (padded)
    uint64_t* doc_off = nullptr;
    uint64_t text_cap = 0;
    uint64_t doc_cap = 0;
    // pinned host staging for host batches (full-speed DMA both ways)
    uint8_t* h_text = nullptr;
    uint64_t h_text_cap = 0;
    uint64_t* h_misc = nullptr;  // piece-relative doc offsets (u64)
    uint64_t h_misc_cap = 0;
    // host-batch pipeline (RangePipeline, jb_hostbatch.cpp): a batch is cut in pieces of whole documents;
    // piece k+1's text goes up on cstream while piece k runs on `stream` and the
    // spans / masks of earlier pieces come back on dstream
    hipStream_t cstream = nullptr, dstream = nullptr;
    std::vector<hipEvent_t> ev_h2d, ev_comp, ev_d2h;  // per piece
    static constexpr int kSets = 3;  // output sets in flight
    struct OutSet {
        uint32_t* ts = nullptr;  // device u32 spans and doc_tok of the piece
        uint32_t* te = nullptr;
        uint64_t* dt = nullptr;
        uint64_t cap_tok = 0, cap_docs = 0;  // entries of ts and te (they grow together), of dt
        uint32_t* hs = nullptr;  // pinned: starts then ends
        uint64_t* hdt = nullptr; // pinned doc_tok
        uint64_t hcap_tok = 0, hcap_docs = 0;
        // packed spans (span_pack): device u32 per token + block headers, side list; pinned copies
        uint16_t* pk = nullptr;
        uint32_t* phdr = nullptr;
        uint4* pside = nullptr;
        uint64_t cap_pk = 0, cap_phdr = 0, cap_pside = 0;
        uint16_t* hpk = nullptr;  // pinned copies
        uint32_t* hhdr = nullptr;
        uint4* hside = nullptr;
        uint64_t hcap_pk = 0, hcap_hdr = 0, hcap_side = 0;
    } outs[kSets];
    bool span_pack = true;  // host batches' spans come back packed, 2 B per token (JB_SPAN_PACK, default 1)
    uint32_t* h_pcnt = nullptr;  // mapped pinned: kSnapWords u32 per piece (k_snap writes them)
    uint32_t* d_pcnt = nullptr;  // its device address
    uint64_t h_pcnt_cap = 0;
    uint64_t* d_mask = nullptr;  // boundary masks of a range: starts then ends (u64 words)
    uint64_t* h_mask = nullptr;  // pinned copy
    uint64_t mask_cap = 0;       // u64 words of d_mask
    uint64_t mask_cap_h = 0;     // u64 words of h_mask
    uint8_t* h_zero = nullptr;   // 64 pinned zero bytes
    jb_stats acc{};              // counters summed over the pieces of the last host range
    bool acc_valid = false;      // the last run was such a range
    // k_small's pinned, mapped host buffers (coherent: the kernel reads and writes them directly)
    // per in-flight k_small batch (cut_small keeps up to kSmallSlots launched at once)
    struct SmallSlot {
        uint8_t* h_sin = nullptr;    // text (kSmallBytes + 128), then u64 doc offsets (kSmallDocs + 1)
        // header, spans, doc_tok (kSmallOutBytes), two of them: batches alternate, so the
        // slot's next batch runs while the callers of the last one get their spans
        uint32_t* h_sout[2] = {nullptr, nullptr};
        uint8_t* d_sin = nullptr;    // their device addresses
        uint32_t* d_sout[2] = {nullptr, nullptr};
        uint32_t ob = 0;             // the output buffer of the slot's current batch
        std::atomic<bool> reading[2] = {false, false};  // spans still being split out of h_sout[i]
        uint32_t seq = 0;            // the kernel writes this number last
        bool busy = false;
        hipStream_t st = nullptr;    // this slot's stream, masked to its own CU
    } slots[8];
    // jb_last_stats' view of the last batch: last_small, small_hdr and has_stats, under
    // stats_mu alone (a finished k_small batch publishes them without waiting for d->mu,
    // which a host-batch pipeline holds for its whole run; lock order: mu, then stats_mu)
    std::mutex stats_mu;
    bool last_small = false;     // the last batch took k_small (jb_last_stats reads small_hdr)
    // concurrent small calls, coalesced into shared k_small launches (cut_small)
    std::mutex small_mu;
    std::condition_variable small_cv;
    std::deque<SmallReq*> small_q;
    uint32_t small_sleepers = 0;         // callers asleep on small_cv (under small_mu)
    // JB_SMALL_TRACE=path (diagnostics): per batch its slot, calls, and the clocks (us) of
    // staging, launch return, completion word and split, written to path at jb_close
    std::vector<std::array<double, 6>> small_trace;
    uint32_t small_slots = 4;            // k_small batches in flight at most (JB_SMALL_SLOTS, 1..8)
    uint32_t small_hdr[kSmallHdr] = {0};
    uint32_t ncu = 0;
    uint64_t piece_bytes = 64ull << 20;  // host-batch pipeline piece (JB_PIECE_KIB)
    LaunchCfg lc{};  // launch shape, fixed at jb_open
    uint64_t last_nbytes = 0;  // batch size of the last pipeline run (jb_last_stats)
    bool has_stats = false;    // this device took part in the last cut (jb_last_stats skips it otherwise)
    // The workspace is shared by every stream a caller queues on (jb_cut_device): each
    // pipeline is recorded here, and a pipeline on another stream waits for it first.
    hipEvent_t ws_done = nullptr;
    EventTimer timer;
    bool profile = false;
    // replay cache: the whole pipeline captured as one HIP graph for the last
    // (buffers, sizes, grids) it ran with; any change re-captures
    struct GraphKey {
        const void* text; uint64_t nbytes; const void* doc_off; uint32_t ndocs; bool hmm;
        uint64_t work_gen; hipStream_t stream; const void* out_s; const void* out_e; const void* out_d;
        // search and full mode (CutMode): the pass's outputs (all null for a plain run) and, in full
        // mode, their capacity
        int mode; const void* so_s; const void* so_e; const void* so_d; const void* so_n; uint64_t so_cap;
        bool operator==(const GraphKey& o) const {
            return text == o.text && nbytes == o.nbytes && doc_off == o.doc_off && ndocs == o.ndocs &&
                   hmm == o.hmm && work_gen == o.work_gen && stream == o.stream && out_s == o.out_s &&
                   out_e == o.out_e && out_d == o.out_d && mode == o.mode && so_s == o.so_s &&
                   so_e == o.so_e && so_d == o.so_d && so_n == o.so_n && so_cap == o.so_cap;
        }
    };
    // one slot per CutMode, so that calls of the three modes on the same buffers each keep their
    // captured graph
    struct GraphSlot {
        GraphKey key{};
        hipGraphExec_t exec = nullptr;  // captured for key (null until the key repeats)
        uint64_t gen = 0;               // 0: no key yet
    } graphs[3];
    uint64_t work_gen = 0;  // bumped whenever the workspace is reallocated
    // The workspace's document bitmap may hold set bits: a new workspace, or a pipeline
    // launch that failed part way.  Pipelines leave it all zeros (k_docbits, k_nonzh).
    bool docbits_dirty = true;
    void drop_graphs() {
        for (GraphSlot& g : graphs) {
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
            g.exec = nullptr;
            g.gen = 0;
        }
    }
};

void dfree(void* p);
void hfree(void* p);
int env_int(const char* name, int dflt);

// The outputs of the pass that follows the pipeline's kernels in search and full mode.
struct PostOut {
    CutMode mode;
    SearchOut so;  // kModeSearch
    FullOut fo;    // kModeFull
};

// Where a run's spans go: arrays of the caller or of an output set instead of the device's own
// (ntok null: the device's own count word; cap: full mode only).
struct SpanDst {
    uint32_t *start, *end;
    uint64_t cap;
    uint64_t *doc_tok, *ntok;
};
// A mode's launch arguments: the workspace (a copy with other outputs for a plain run to `dst`),
// the mode's pass and where the spans end up.
struct SpanTarget {
    Work w;
    PostOut po;
    SpanDst at;
    const PostOut* post() const { return po.mode != kModePlain ? &po : nullptr; }
};
// After ensure_mode.  own_cap: the capacity of the ctx-owned full-mode arrays this run may use.
SpanTarget span_target(const Device* d, CutMode mode, const SpanDst* dst, uint64_t own_cap);

int stage_image(int ordinal, const Image& img, ImageBufs* b);
int install_image(Device* d, ImageBufs* b, const Image& img);
void free_image_bufs(ImageBufs* b);
int ensure_work(Device* d, uint64_t nbytes, uint32_t ndocs);
int ensure_mode(Device* d, CutMode mode);  // search and full mode's buffers (after ensure_work)
int launch(Device* d, const Work& w, const uint8_t* d_text, uint64_t nbytes, const uint64_t* d_doc_off,
           uint32_t ndocs, bool hmm, hipStream_t s, const MaskOut* mask = nullptr, const PostOut* po = nullptr);
int open_device(Device* d, int ordinal, const Image& img);
void close_device(Device* d);

// grow-only device / pinned buffers (a call never has work in flight on them when it grows them)
template <class T>
static int grow_dev(T** p, uint64_t* cap, uint64_t want) {
    if (want <= *cap && *p) return JB_OK;
    dfree(*p);
    *p = nullptr;
    *cap = 0;
    const uint64_t c = std::max<uint64_t>(want, 1);
    HIPCHK(hipMalloc(p, c * sizeof(T)));
    *cap = c;
    return JB_OK;
}
// two arrays of one capacity (they always grow together)
template <class T>
static int grow_dev_pair(T** a, T** b, uint64_t* cap, uint64_t want) {
    if (want <= *cap && *a && *b) return JB_OK;
    dfree(*a);
    dfree(*b);
    *a = *b = nullptr;
    *cap = 0;
    const uint64_t c = std::max<uint64_t>(want, 1);
    HIPCHK(hipMalloc(a, c * sizeof(T)));
    HIPCHK(hipMalloc(b, c * sizeof(T)));
    *cap = c;
    return JB_OK;
}
template <class T>
static int grow_pinned(T** p, uint64_t* cap, uint64_t want) {
    if (want <= *cap && *p) return JB_OK;
    const uint64_t c = std::max<uint64_t>(want, *cap * 3 / 2 + 1);
    hfree(*p);
    *p = nullptr;
    *cap = 0;
    HIPCHK(hipHostMalloc(p, c * sizeof(T), hipHostMallocDefault));
    *cap = c;
    return JB_OK;
}

// grow-only mapped (device-visible), coherent pinned memory: kernels write it directly
template <class T>
static int grow_mapped(T** p, T** dp, uint64_t* cap, uint64_t want) {
    if (want <= *cap && *p) return JB_OK;
    const uint64_t c = std::max<uint64_t>(want, *cap * 3 / 2 + 1);
    hfree(*p);
    *p = *dp = nullptr;
    *cap = 0;
    HIPCHK(hipHostMalloc(p, c * sizeof(T), hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer((void**)dp, *p, 0));
    *cap = c;
    return JB_OK;
}

struct jb_ctx {
    std::unique_ptr<jb_image> im;
    std::vector<std::unique_ptr<Device>> devs;
    std::shared_mutex lock;  // prefixDictionary.lock: cuts share, AddWord excludes
    // the caller's vocabulary (jb_vocab_set) and its copy on the first device; id calls read
    // them under the shared lock, jb_vocab_set replaces them under the exclusive one
    std::unique_ptr<Vocab> vocab;
    uint32_t* d_vslots = nullptr;
    uint8_t* d_vpool = nullptr;
    DevVocab dvocab{};
    // the caller's stop set (jb_stopwords_set): a second table under the same rules, read by jb_filter_device
    std::unique_ptr<Vocab> stopw;
    uint32_t* d_sslots = nullptr;
    uint8_t* d_spool = nullptr;
    DevVocab dstop{};
    // the host-text calls' device buffers on the first device (jb_batch.h: KwBuf names them) and the lock they
    // are used under
    std::mutex kw_mu;
    void* kw_buf[kArCount] = {};
    size_t kw_cap[kArCount] = {};
    // the rule of jb_batch_filter_set (under kw_mu); jb_batch.cpp lists the calls that filter by it
    bool bfilter_on = false;
    jb_filter_rule bfilter{0, 0, 0, 0};
    // the caller's index (jb_index_set) on the first device, one allocation: search calls read it under the
    // shared lock, jb_index_set and jb_index_clear replace it under the exclusive one
    struct Index {
        void* base = nullptr;
        const uint64_t* post_off = nullptr;
        const uint32_t *post_doc = nullptr, *post_tf = nullptr;
        const float *norm = nullptr, *weight = nullptr;
        uint64_t npost = 0;
        uint32_t nids = 0, ndocs = 0;
        double k1 = 0, b = 0, avgdl = 0;
    } index;
};

#pragma GCC visibility pop
