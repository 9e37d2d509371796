// jb_filter.h — the token filter's rule (jb_filter*, jiebahip.h): a token's class, its rune count and the
// decision, shared by the host rule (jb_filter.cpp) and the gfx950 kernels (jb_filter.hip), which run the
// code below over a byte pointer to the span's first byte.
//
// A span [s, e) with s >= e or e > nbytes is bad: it is never kept and none of its bytes is read.  Every
// other span has len = e - s >= 1 bytes at p = text + s, and kw[0..5], the little-endian words of its first
// min(len, 24) bytes, zero past the span's end.
#pragma once
#include "jb_vocab.h"
#include "jiebahip.h"

// Why a token was left out (0: it is kept); the order is the order of stats[1..4].
#define JB_FR_KEEP 0u
#define JB_FR_BAD 1u
#define JB_FR_CLASS 2u
#define JB_FR_LENGTH 3u
#define JB_FR_STOP 4u

#define JB_FILTER_MAXRUNES 255u  // the greatest min_runes / max_runes
#define JB_FILTER_SCAN 1024u     // a key longer than this counts 256 runes without being read
#define JB_FILTER_ALLCLASSES (JB_TC_HAN | JB_TC_ALNUM | JB_TC_NUM | JB_TC_OTHER | JB_TC_INVALID)

JB_HD bool jb_filter_bad(uint64_t s, uint64_t e, uint64_t nbytes) { return s >= e || e > nbytes; }

// The words of the first min(len, 24) bytes at p, as the kernels build them from aligned dwords.
JB_HD void jb_filter_words(const uint8_t* p, uint32_t len, uint32_t kw[6]) {
    for (uint32_t w = 0; w < 6u; w++) kw[w] = 0u;
    for (uint32_t i = 0; i < len && i < JB_VOCAB_INLINE; i++) kw[i >> 2] |= (uint32_t)p[i] << (8u * (i & 3u));
}

// The class of the span of len >= 1 bytes at p; x is kw[0].  Only an alnum key of at most 255 bytes is
// scanned (for a byte that is no digit); every other class follows from x alone.
JB_HD uint32_t jb_filter_class(uint32_t x, const uint8_t* p, uint32_t len) {
    const uint32_t b0 = x & 0xFFu;
    if (len == 1u && b0 >= 0x80u) return JB_TC_INVALID;
    if (jb_is_alnum(b0)) {
        if (len > JB_VOCAB_MAXKEY) return JB_TC_ALNUM;
        for (uint32_t i = 0; i < len; i++)
            if ((uint32_t)p[i] - (uint32_t)'0' >= 10u) return JB_TC_ALNUM;
        return JB_TC_NUM;
    }
    uint32_t r;
    (void)jb_decode(x, len < 4u ? len : 4u, &r);  // (a sequence cut short by the span's end is U+FFFD)
    return jb_is_han(r) ? JB_TC_HAN : JB_TC_OTHER;
}

// min(runes, sat) of the span at p, sat <= 256: runes is the number of bytes that are not 10xxxxxx,
// saturating at 256, and 256 for a span over JB_FILTER_SCAN bytes, which is not read (text that is valid
// UTF-8 has at least 256 runes in 1024 bytes, so only malformed spans see the difference).
JB_HD uint32_t jb_filter_runes(const uint8_t* p, uint32_t len, uint32_t sat) {
    if (len > JB_FILTER_SCAN) return sat;
    uint32_t c = 0;
    for (uint32_t i = 0; i < len && c < sat; i++) c += (p[i] & 0xC0u) != 0x80u;
    return c;
}

// The 10xxxxxx bytes among the four of w (bit 7 set and bit 6 clear).
JB_HD uint32_t jb_filter_cont4(uint32_t w) {
    const uint32_t m = (w >> 7) & ~(w >> 6) & 0x01010101u;
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(m);
#else
    return (uint32_t)__builtin_popcount(m);
#endif
}

// The decision for a span that is not bad: JB_FR_KEEP or the first reason that applies.  `stop` is read
// only with JB_FILTER_STOP in the rule's flags.
JB_HD uint32_t jb_filter_decide(const jb_filter_rule& r, const JbVocabView& stop, const uint32_t kw[6],
                                const uint8_t* p, uint32_t len) {
    const uint32_t cls = jb_filter_class(kw[0], p, len);
    if (r.drop_classes & cls) return JB_FR_CLASS;
    if (r.min_runes | r.max_runes) {
        // counting stops once both comparisons are decided
        const uint32_t sat = (r.min_runes > r.max_runes ? r.min_runes : r.max_runes) + 1u;
        uint32_t n;
        if (cls == JB_TC_INVALID) {
            n = 1u;
        } else if (len <= JB_VOCAB_INLINE) {  // the key is in kw, whose bytes past len are zero: no byte is read
            n = len;
            for (uint32_t w = 0; w < 6u; w++) n -= jb_filter_cont4(kw[w]);
        } else {
            n = jb_filter_runes(p, len, sat);
        }
        if (n < r.min_runes || (r.max_runes && n > r.max_runes)) return JB_FR_LENGTH;
    }
    if (r.flags & JB_FILTER_STOP) {
        if (cls == JB_TC_INVALID) {  // the key is "\xEF\xBF\xBD"
            const uint32_t kq[6] = {0x00BDBFEFu, 0u, 0u, 0u, 0u, 0u};
            if (jb_vocab_find(stop, kq, p, 3u) != JB_VOCAB_UNK) return JB_FR_STOP;
        } else if (jb_vocab_find(stop, kw, p, len) != JB_VOCAB_UNK) {  // (a key over stop.maxlen is not read)
            return JB_FR_STOP;
        }
    }
    return JB_FR_KEEP;
}

// The host side (jb_filter.cpp).
#pragma GCC visibility push(hidden)
namespace jb {

// The checks the host rule and the device calls share, in the order the calls report them: JB_OK, or
// JB_EINVAL / JB_ELIMIT with the thread's message set.  `who` names the entry point.
int filter_args(const char* who, uint64_t nbytes, uint64_t cap, const jb_filter_rule* rule, bool have_stop);
// Outputs must not alias inputs (or each other): JB_EINVAL when two of the non-null pointers are equal.
int filter_alias(const char* who, const void* start, const void* end, const void* doc_tok, const void* out_start,
                 const void* out_end, const void* out_src, const void* out_doc_tok);

// The work buffer of jb_filter_device: one bit per token in 64-bit words (kFiltTile / 64 per tile), 8 u32
// per tile (kept, bad, class, length, stop, 3 unused) and the tiles' exclusive prefixes (ntl + 1 u64).
struct FilterWork {
    uint64_t ntl;
    size_t words, cnt, base;  // byte offsets
    size_t bytes;
};
FilterWork filter_layout(uint64_t max_tokens);

}  // namespace jb
#pragma GCC visibility pop
