// jb_plan.cpp — the host layer's pure planners (jb_plan.h).  Host only, no HIP.
#include "jb_plan.h"

#include <algorithm>

#include "../../include/jiebahip.h"
#include "jb_common.h"
#include "jb_err.h"

PiecePlan plan_pieces(const uint64_t* doc_off, uint32_t d0, uint32_t d1, uint64_t piece_bytes) {
    PiecePlan pl;
    for (uint32_t a = d0; a < d1;) {
        uint32_t b = a + 1;
        while (b < d1 && doc_off[b + 1] - doc_off[a] <= piece_bytes) b++;
        const uint64_t len = doc_off[b] - doc_off[a];
        pl.pcs.push_back(Piece{a, b, pl.dev_bytes, pl.slots});
        pl.dev_bytes += (len + 64 + 255) & ~255ull;  // 64 zero bytes after each piece, 256-byte aligned starts
        pl.slots += b - a + 1;
        pl.maxb = std::max(pl.maxb, len);
        pl.maxd = std::max(pl.maxd, b - a);
        a = b;
    }
    return pl;
}

// Contiguous byte-balanced document ranges: part k owns
// documents [cut[k], cut[k+1]); cut[0] = 0, cut[nparts] = ndocs.  The cut
// before part k is the first document that does not end at or before byte
// total * k / nparts (jieba-go_amd/python/shard.py restates the rule for
// bench.py's one-process-per-GPU runs).
extern "C" int jb_shard_bounds(const uint64_t* doc_off, uint32_t ndocs, uint32_t nparts, uint32_t* cut) {
    if (!cut || nparts == 0 || (!doc_off && ndocs)) return fail(JB_EINVAL, "jb_shard_bounds: bad argument");
    for (uint32_t k = 0; k < ndocs; k++)
        if (doc_off[k + 1] < doc_off[k]) return fail(JB_EINVAL, "doc_off not monotonic at %u", k);
    for (uint32_t k = 0; k <= nparts; k++) cut[k] = ndocs;
    cut[0] = 0;
    const uint64_t total = ndocs ? doc_off[ndocs] - doc_off[0] : 0;
    for (uint32_t k = 1; k < nparts; k++) {
        // (total * k fits u64: total < 2^56 for any batch a host holds)
        const uint64_t target = (ndocs ? doc_off[0] : 0) + total * k / nparts;
        uint32_t lo = cut[k - 1];
        while (lo < ndocs && doc_off[lo + 1] <= target) lo++;
        cut[k] = lo;
    }
    return JB_OK;
}

// The first Han-run start of the document [lo, hi) at or after pos (and after lo):
// a position q where a Han rune begins (Go's DecodeRune over the document) and the
// rune before it is not Han; hi if there is none.  Cutting a document there is
// exact: splitText's blocks (tokenizer.go:165-210) are the same in both parts, and
// blocks are cut independently (tokenizer.go:158-160).  Decoding from lo lands on
// every lead byte of a valid sequence (a continuation byte is never a lead byte), so
// the rune before q is the valid 2-4 byte sequence that ends at q if there is one,
// else the single byte q-1.
uint64_t han_run_start(const uint8_t* t, uint64_t lo, uint64_t hi, uint64_t pos) {
    auto dec = [&](uint64_t q, uint32_t* r) -> uint32_t {
        const uint64_t lim = std::min<uint64_t>(4, hi - q);
        uint32_t x = 0;
        for (uint64_t k = 0; k < lim; k++) x |= (uint32_t)t[q + k] << (8 * k);
        return jb_decode(x, (uint32_t)lim, r);
    };
    for (uint64_t q = std::max(pos, lo + 1); q < hi; q++) {
        if (t[q] < 0xE0u) continue;  // Han runes are 3 or 4 bytes long
        uint32_t r;
        if (dec(q, &r) < 3 || !jb_is_han(r)) continue;
        bool prev_han = false;
        if (t[q - 1] >= 0x80u)
            for (uint32_t k = 2; k <= 4; k++) {
                uint32_t pr;
                if (q >= lo + k && dec(q - k, &pr) == k) {
                    prev_han = jb_is_han(pr);
                    break;
                }
            }
        if (!prev_han) return q;
    }
    return hi;
}

extern "C" int jb_split_points(const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, uint32_t nparts,
                               uint64_t* cut) {
    if (!cut || nparts == 0 || (!doc_off && ndocs)) return fail(JB_EINVAL, "jb_split_points: bad argument");
    for (uint32_t k = 0; k < ndocs; k++)
        if (doc_off[k + 1] < doc_off[k]) return fail(JB_EINVAL, "doc_off not monotonic at %u", k);
    const uint64_t b0 = ndocs ? doc_off[0] : 0, total = ndocs ? doc_off[ndocs] - b0 : 0;
    if (total && !text) return fail(JB_EINVAL, "jb_split_points: null text");
    cut[0] = b0;
    cut[nparts] = b0 + total;
    uint32_t j = 0;
    uint64_t known = 0, known_q = 0;  // in document j: the first Han-run start at or after `known` is known_q
    bool have = false;
    for (uint32_t k = 1; k < nparts; k++) {
        const uint64_t target = std::max(b0 + total * k / nparts, cut[k - 1]);
        const uint32_t j0 = j;
        while (j < ndocs && doc_off[j + 1] <= target) j++;
        if (j != j0) have = false;
        if (j >= ndocs) {
            cut[k] = b0 + total;
            continue;
        }
        if (doc_off[j] >= target) {
            cut[k] = doc_off[j];
            continue;
        }
        if (!have || target < known || target > known_q) {
            known = target;
            known_q = han_run_start(text, doc_off[j], doc_off[j + 1], target);
            have = true;
        }
        cut[k] = known_q;  // (the next document's start when the rest of this one has none)
    }
    return JB_OK;
}

int plan_units(const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, const uint64_t* piece_bytes, size_t nd,
               Units* unp, std::vector<uint64_t>* cutbp, bool* splitp) {
    Units& un = *unp;
    std::vector<uint64_t>& cutb = *cutbp;
    const uint64_t b0 = ndocs ? doc_off[0] : 0, b1 = ndocs ? doc_off[ndocs] : 0;
    bool split = nd > 1;
    for (uint32_t j = 0; j < ndocs && !split; j++) split = doc_off[j + 1] - doc_off[j] > piece_bytes[0];
    *splitp = split;
    un = Units{};
    cutb.assign(nd + 1, b0);
    cutb[nd] = b1;
    if (!split) return JB_OK;
    int rc0 = jb_split_points(text, doc_off, ndocs, (uint32_t)nd, cutb.data());
    if (rc0) return rc0;
    un.off.reserve((size_t)ndocs + 2 * nd + 1);
    un.doc.reserve((size_t)ndocs + 2 * nd);
    un.dev.assign(nd + 1, 0);
    size_t k = 0;
    auto dev_of = [&](uint64_t pos) {  // the last device whose range starts at or before pos
        while (k + 1 < nd && cutb[k + 1] <= pos && (cutb[k + 1] < b1 || pos >= b1)) {
            k++;
            un.dev[k] = (uint32_t)un.doc.size();
        }
    };
    for (uint32_t j = 0; j < ndocs; j++) {
        uint64_t pos = doc_off[j];
        const uint64_t de = doc_off[j + 1];
        for (;;) {
            dev_of(pos);
            const uint64_t end = std::min(de, k + 1 < nd && cutb[k + 1] > pos ? cutb[k + 1] : de);
            const uint64_t pb = piece_bytes[k];
            uint64_t u = pos;
            while (end - u > pb) {  // a longer part: pipeline pieces at Han-run starts
                const uint64_t q = han_run_start(text, doc_off[j], de, u + pb);
                if (q >= end) break;
                un.off.push_back(u);
                un.doc.push_back(j);
                u = q;
            }
            un.off.push_back(u);
            un.doc.push_back(j);
            if (end >= de) break;
            pos = end;
        }
    }
    un.off.push_back(b1);
    for (size_t q = k + 1; q <= nd; q++) un.dev[q] = (uint32_t)un.doc.size();
    if (un.doc.size() > 0xFFFFFFFFull) return fail(JB_ELIMIT, "too many cut units");
    return JB_OK;
}
