// jb_kstages.h — the kernel units' enqueue functions (internal to csrc/): run_pipeline and
// the mode passes launch a kernel of another unit through these.  Each enqueues one launch
// on `stream` and nothing else; errors are left to the caller's hipGetLastError.
// The launch-timing macros live here and not with the device helpers in jb_kdev.h: they are host
// code, jb_pipeline.cpp is compiled without device code, and jb_terms.hip takes them from here
// without seeing jb_kdev.h's names.
#pragma once
#include "jb_kernels.h"

// A launch between the optional timer's events (`timer`, a KernelTimer*, and `stream` are the caller's).
#define JB_TIMED_ON(id, st, ...)                  \
    do {                                          \
        if (timer) timer->begin((id), (st));      \
        __VA_ARGS__;                              \
        if (timer) timer->end((id), (st));        \
    } while (0)
#define JB_TIMED(id, ...) JB_TIMED_ON(id, stream, __VA_ARGS__)

namespace jb {

// jb_kernels.hip: the mark stage
void enq_docbits(const Work& w, const uint64_t* d_doc_off, uint32_t ndocs, uint64_t nbytes, uint32_t nttiles,
                 hipStream_t stream);
void enq_mark_walk(const DevImage& im, const Work& w, const uint8_t* d_text, uint64_t nbytes, uint32_t ntiles,
                   uint32_t split, uint32_t diag, hipStream_t stream);

// jb_kernels.hip: k_zh, grid workgroups of 4 waves, or of kZhWgWide (wide)
void enq_zh(const DevImage& im, const Work& w, const uint8_t* d_text, uint64_t nbytes, bool hmm, bool wide,
            uint32_t grid, uint32_t grp, uint32_t g1, uint32_t sgrp, uint32_t diag, hipStream_t stream);

// jb_kernels.hip: the long-block family and k_nonzh; gseg workgroups of 256 segments; k_long's grid
// and whether it does k_nonzh's work (nzf) are the pipeline's choice
void enq_long_spec(const DevImage& im, const Work& w, const uint8_t* d_text, uint32_t spec, hipStream_t stream);
void enq_long_path(const Work& w, uint32_t want, uint32_t set, hipStream_t stream);
void enq_long_pbits(const Work& w, uint32_t gseg, hipStream_t stream);
void enq_long_dp(const DevImage& im, const Work& w, const uint8_t* d_text, bool hmm, uint32_t spec,
                 hipStream_t stream);
void enq_long_seg(const DevImage& im, const Work& w, const uint8_t* d_text, uint32_t gseg, hipStream_t stream);
void enq_long_tail(const DevImage& im, const Work& w, const uint8_t* d_text, bool hmm, uint32_t gseg,
                   hipStream_t stream);
void enq_long(const DevImage& im, const Work& w, const uint8_t* d_text, uint64_t nbytes, uint32_t ntiles,
              const uint64_t* d_doc_off, uint32_t ndocs, bool hmm, bool nzf, uint32_t grid, uint32_t spec,
              uint32_t wait_ticks, hipStream_t stream);
void enq_nonzh(const Work& w, const uint8_t* d_text, uint64_t nbytes, uint32_t ntiles, const uint64_t* d_doc_off,
               uint32_t ndocs, hipStream_t stream);

// jb_k_tok.hip
void enq_sup(const uint2* cnt, uint32_t n, uint2* sup, hipStream_t stream);  // (also the search pass's tile sums)
void enq_tok_count(const Work& w, uint64_t nwords, uint32_t nttiles, hipStream_t stream);
void enq_tok_write(const Work& w, uint64_t nwords, uint32_t nttiles, hipStream_t stream);
void enq_doc_tok(const Work& w, const uint64_t* d_doc_off, uint32_t ndocs, hipStream_t stream);
void enq_tok1(const Work& w, uint64_t nwords, uint32_t nttiles, const uint64_t* d_doc_off, uint32_t ndocs,
              hipStream_t stream);
void enq_mask_merge(const Work& w, uint64_t nbytes, const MaskOut& mask, hipStream_t stream);

}  // namespace jb
