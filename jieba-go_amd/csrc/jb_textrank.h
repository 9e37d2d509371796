// jb_textrank.h — what jb_textrank (jb_textrank.cpp), jb_textrank_device (jb_capi.cpp) and jb_textrank_batch
// (jb_batch.cpp) share.
// Library-internal, host only.
#pragma once
#include <cstdint>

#pragma GCC visibility push(hidden)

namespace jb {

// The limits of span, iters, topk and of the list lengths, in the order both calls report them:
// JB_OK, or JB_EINVAL / JB_ELIMIT with the thread's message set.  `who` names the entry point.
int textrank_args(const char* who, uint64_t ids_cap, uint64_t cap, uint32_t span, uint32_t iters, uint32_t topk);

}  // namespace jb

#pragma GCC visibility pop
