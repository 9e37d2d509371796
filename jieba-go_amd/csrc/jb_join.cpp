// jb_join.cpp — jb_join, the joined-text rule of jiebahip.h on host arrays, and the argument checks it
// shares with jb_join_device.  Host only, no HIP: the kernels of jb_join.hip are pinned to this function
// byte for byte.
#include "jb_join.h"

#include <algorithm>

#include "jb_err.h"
#include "jiebahip.h"

namespace jb {

int join_args(const char* who, uint64_t nbytes, uint64_t cap, const void* sep, uint32_t seplen, const void* term,
              uint32_t termlen) {
    if (seplen > JB_JOIN_MAXSEP)
        return fail(JB_ELIMIT, "%s: a separator of %u bytes (limit JB_JOIN_MAXSEP = %u)", who, seplen, JB_JOIN_MAXSEP);
    if (termlen > JB_JOIN_MAXSEP)
        return fail(JB_ELIMIT, "%s: a terminator of %u bytes (limit JB_JOIN_MAXSEP = %u)", who, termlen, JB_JOIN_MAXSEP);
    if ((seplen && !sep) || (termlen && !term)) return fail(JB_EINVAL, "%s: null separator or terminator", who);
    if (nbytes >= (1ull << 31)) return fail(JB_ELIMIT, "%s: a text of %llu bytes (limit 2 GiB)", who, (unsigned long long)nbytes);
    if (cap >= (1ull << 32) - JB_JOIN_TILE)
        return fail(JB_ELIMIT, "%s: a span list of %llu entries (limit 2^32 - %u)", who, (unsigned long long)cap,
                    JB_JOIN_TILE);
    return JB_OK;
}

}  // namespace jb

extern "C" int jb_join(const uint8_t* text, uint64_t nbytes, const uint32_t* start, const uint32_t* end,
                       const uint64_t* doc_tok, uint64_t ntok, uint64_t cap, uint32_t ndocs, const uint8_t* sep,
                       uint32_t seplen, const uint8_t* term, uint32_t termlen, uint8_t* out, uint64_t out_cap,
                       uint64_t* out_doc_off, uint64_t* nout) {
    if (const int rc = jb::join_args("jb_join", nbytes, cap, sep, seplen, term, termlen)) return rc;
    if (!doc_tok || !out_doc_off || !nout || (nbytes && !text) || (cap && (!start || !end)) || (out_cap && !out))
        return fail(JB_EINVAL, "jb_join: null argument");
    static const uint8_t kRepl[3] = {0xEF, 0xBF, 0xBD};
    const uint64_t n = std::min(ntok, cap);
    uint64_t pos = 0;
    // (a byte of the complete output: stored when it lies below out_cap, counted either way)
    auto put = [&](const uint8_t* p, uint64_t len) {
        if (len && pos < out_cap) std::copy(p, p + std::min(len, out_cap - pos), out + pos);
        pos += len;
    };
    for (uint32_t d = 0; d < ndocs; d++) {
        out_doc_off[d] = pos;
        const uint64_t a = std::min(doc_tok[d], n), b = std::min(doc_tok[d + 1], n);
        for (uint64_t k = a; k < b; k++) {
            if (k > a) put(sep, seplen);
            const uint64_t s = start[k], e = end[k];
            if (s >= e || e > nbytes) continue;  // (an empty key: no text byte is read)
            if (e - s == 1 && text[s] >= 0x80) put(kRepl, 3);
            else put(text + s, e - s);
        }
        put(term, termlen);
    }
    out_doc_off[ndocs] = pos;
    *nout = pos;
    return JB_OK;
}
