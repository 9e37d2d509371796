// jb_join.h — what jb_join (jb_join.cpp), jb_join_device (jb_capi.cpp) and jb_cut_batch_join (jb_batch.cpp) share.
// Library-internal, host only.
#pragma once
#include <cstdint>

#pragma GCC visibility push(hidden)

namespace jb {

// The limits of the separator, the terminator, the text and the span list, in the order the calls report
// them: JB_OK, or JB_EINVAL / JB_ELIMIT with the thread's message set.  `who` names the entry point.
int join_args(const char* who, uint64_t nbytes, uint64_t cap, const void* sep, uint32_t seplen, const void* term,
              uint32_t termlen);

}  // namespace jb

#pragma GCC visibility pop
