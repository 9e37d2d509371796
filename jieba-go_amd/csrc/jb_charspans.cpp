// jb_charspans.cpp — jb_charspans, the character-offset rule of jiebahip.h on host arrays, and the argument
// checks it shares with jb_charspans_device.  Host only, no HIP: the kernels of jb_charspans.hip are pinned
// to this function to the bit.
#include "jb_charspans.h"

#include <algorithm>
#include <new>
#include <vector>

#include "jb_common.h"
#include "jb_err.h"
#include "jiebahip.h"

namespace jb {

int charspans_args(const char* who, uint64_t nbytes, uint64_t cap, int unit) {
    if (unit != JB_UNIT_RUNE && unit != JB_UNIT_UTF16)
        return fail(JB_EINVAL, "%s: unit %d (JB_UNIT_RUNE or JB_UNIT_UTF16)", who, unit);
    if (nbytes >= (1ull << 31)) return fail(JB_ELIMIT, "%s: a text of %llu bytes (limit 2 GiB)", who, (unsigned long long)nbytes);
    if (cap >= (1ull << 32) - JB_JOIN_TILE)
        return fail(JB_ELIMIT, "%s: a span list of %llu entries (limit 2^32 - %u)", who, (unsigned long long)cap,
                    JB_JOIN_TILE);
    return JB_OK;
}

}  // namespace jb

extern "C" int jb_charspans(const uint8_t* text, uint64_t nbytes, const uint64_t* doc_off, uint32_t ndocs,
                            const uint32_t* start, const uint32_t* end, const uint64_t* doc_tok, uint64_t ntok,
                            uint64_t cap, int unit, uint32_t* cstart, uint32_t* cend, uint32_t* doc_units) {
    if (const int rc = jb::charspans_args("jb_charspans", nbytes, cap, unit)) return rc;
    if (!doc_off || !doc_tok || (nbytes && !text) || (cap && (!start || !end || !cstart || !cend)) || (ndocs && !doc_units))
        return fail(JB_EINVAL, "jb_charspans: null argument");
    if (doc_off[0] != 0) return fail(JB_EINVAL, "jb_charspans: doc_off[0] is %llu, not 0", (unsigned long long)doc_off[0]);
    for (uint32_t d = 0; d < ndocs; d++)
        if (doc_off[d] > doc_off[d + 1]) return fail(JB_EINVAL, "jb_charspans: doc_off decreases at %u", d);
    if (doc_off[ndocs] != nbytes)
        return fail(JB_EINVAL, "jb_charspans: doc_off[ndocs] is %llu, the text has %llu bytes",
                    (unsigned long long)doc_off[ndocs], (unsigned long long)nbytes);
    // at[p - so], for a byte p of document [so, eo): pos_d(p).  A byte inside a rune has that rune counted.
    std::vector<uint32_t> at;
    const uint64_t n = std::min(ntok, cap);
    uint64_t k = 0;
    auto none = [&](uint64_t upto) {  // the tokens below `upto` that no document has claimed
        for (; k < upto; k++) cstart[k] = cend[k] = JB_CHAR_NONE;
    };
    for (uint32_t d = 0; d < ndocs; d++) {
        const uint64_t so = doc_off[d], eo = doc_off[d + 1];
        try {
            at.assign((size_t)(eo - so) + 1, 0);
        } catch (const std::bad_alloc&) {
            return fail(JB_ENOMEM, "jb_charspans: out of host memory for a document of %llu bytes", (unsigned long long)(eo - so));
        }
        uint32_t units = 0;
        for (uint64_t i = so; i < eo;) {
            uint32_t x = 0, rune;
            const uint32_t lim = (uint32_t)std::min<uint64_t>(4, eo - i);
            for (uint32_t b = 0; b < lim; b++) x |= (uint32_t)text[i + b] << (8 * b);
            const uint32_t w = jb_decode(x, lim, &rune);
            at[i - so] = units;
            units += (unit == JB_UNIT_UTF16 && w == 4) ? 2u : 1u;  // (a valid four-byte form is U+10000 or above)
            for (uint32_t b = 1; b < w; b++) at[i - so + b] = units;
            i += w;
        }
        at[eo - so] = units;
        doc_units[d] = units;
        const uint64_t a = std::min(doc_tok[d], n), b = std::min(doc_tok[d + 1], n);
        none(std::min(a, b));
        // (a doc_tok that decreases, outside the contract, claims nothing here: the tokens stay for none())
        for (; k >= a && k < b; k++) {
            const uint64_t s = start[k], e = end[k];  // (both read before either output is written: in place)
            if (so <= s && s <= e && e <= eo) {
                cstart[k] = at[s - so];
                cend[k] = at[e - so];
            } else {
                cstart[k] = cend[k] = JB_CHAR_NONE;
            }
        }
    }
    none(n);
    return JB_OK;
}
