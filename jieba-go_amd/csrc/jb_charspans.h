// jb_charspans.h — what jb_charspans (jb_charspans.cpp), jb_charspans_device (jb_capi.cpp) and
// jb_cut_batch_charspans (jb_batch.cpp) share.  Library-internal, host only.
#pragma once
#include <cstdint>

#pragma GCC visibility push(hidden)

namespace jb {

// The limits of the unit, the text and the span list, in the order the calls report them: JB_OK, or
// JB_EINVAL / JB_ELIMIT with the thread's message set.  `who` names the entry point.
int charspans_args(const char* who, uint64_t nbytes, uint64_t cap, int unit);

}  // namespace jb

#pragma GCC visibility pop
