// jb_host.h — cutting batches that live in host memory: the k_small path (jb_small.cpp) and the
// sharded piece pipeline (jb_hostbatch.cpp).  Library-internal.
#pragma once
#include "jb_device.h"

#pragma GCC visibility push(hidden)

// growable malloc'd span arrays (handed to the caller as jb_spans)
struct SpanBuf {
    uint64_t* s = nullptr;
    uint64_t* e = nullptr;
    // external u32 arrays instead (jb_cut_batch_into32): token k is s32[k] = start - b32
    uint32_t* s32 = nullptr;
    uint32_t* e32 = nullptr;
    uint64_t b32 = 0;
    size_t n = 0, cap = 0;
    bool external = false;          // caller-owned arrays of fixed capacity
    std::vector<uint64_t> per_doc;  // tokens per document
    bool reserve(size_t want) {
        if (want <= cap) return true;
        if (external) return false;
        const size_t nc = std::max(want, cap * 3 / 2 + 1024);
        uint64_t* ns = (uint64_t*)realloc(s, nc * 8);
        if (!ns) return false;
        s = ns;
        uint64_t* ne = (uint64_t*)realloc(e, nc * 8);
        if (!ne) return false;
        e = ne;
        cap = nc;
        return true;
    }
    void release() {
        if (!external) {
            free(s);
            free(e);
        }
        s = e = nullptr;
        n = cap = 0;
    }
};

// Caller-owned boundary masks (jb_cut_batch_mask): bit i of s / e is byte batch0 + i.
struct MaskDst {
    uint64_t* s;
    uint64_t* e;
    uint64_t batch0;
};

// One small batch (at most lc.small_max bytes and kSmallDocs documents) through k_small, coalesced
// with other callers'; takes no device lock.
int cut_small(Device* d, const uint8_t* text, const uint64_t* doc_off, uint32_t nd, bool hmm, SpanBuf* out);

// Shard the batch over the devices and cut, one host thread per device (jb_plan.h: plan_units).
// sb[k] receives device k's spans and tokens per unit; *unit_doc (left empty when units are
// documents) maps units to documents.  The caller holds ctx->lock (shared for cuts, exclusive
// inside jb_add_word).
int cut_sharded(jb_ctx* ctx, const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, int hmm,
                std::vector<SpanBuf>* sbp, const MaskDst* mask = nullptr, std::vector<uint32_t>* unit_doc = nullptr,
                CutMode mode = kModePlain);
// doc_tok from the tokens per unit (in unit order over the devices' buffers)
void fill_doc_tok(const std::vector<SpanBuf>& sb, uint32_t ndocs, uint64_t* doc_tok,
                  const std::vector<uint32_t>& unit_doc);

// jb_host_alloc's allocations: a batch inside one is copied to the device without staging.
void host_register(const void* p, size_t n);
void host_unregister(const void* p);

#pragma GCC visibility pop
