// jb_neardup.cpp — the host side of the near-duplicate call: jb_neardup, the rule of jiebahip.h on host arrays
// (what the kernels of jb_neardup.hip are pinned to, on every output), jb_neardup_labels, the size helper, the
// work buffer's layout and the argument checks shared with the device call.  Host only, no HIP.
#include "jb_neardup.h"

#include <stdlib.h>

#include <algorithm>
#include <new>
#include <vector>

#include "jb_err.h"

namespace jb {

int neardup_args(const char* who, uint32_t ndocs, uint32_t B, uint32_t K, uint32_t W, uint32_t min_agree) {
    if (B == 0 || K == 0 || W == 0 || min_agree == 0)
        return fail(JB_EINVAL, "%s: B = %u, K = %u, W = %u, min_agree = %u: none may be 0", who, B, K, W, min_agree);
    if (B > JB_MH_MAXK || K > JB_MH_MAXK)
        return fail(JB_ELIMIT, "%s: B = %u, K = %u (limit %u)", who, B, K, JB_MH_MAXK);
    if (W > JB_ND_MAXWIN) return fail(JB_ELIMIT, "%s: a window of %u (limit %u)", who, W, JB_ND_MAXWIN);
    if (min_agree > K) return fail(JB_ELIMIT, "%s: min_agree %u above K = %u", who, min_agree, K);
    if ((uint64_t)ndocs * B >= (1ull << 32) - JB_ND_TILE)
        return fail(JB_ELIMIT, "%s: %u documents x %u bands (limit 2^32 - %u entries)", who, ndocs, B, JB_ND_TILE);
    return JB_OK;
}

int neardup_alias(const char* who, const void* key, const void* sig, const void* pair_doc, const void* pair_agree,
                  const void* pair_off, const void* npairs, const void* stat, const void* work) {
    const void* in[3] = {key, sig, work};
    const void* out[5] = {pair_doc, pair_agree, pair_off, npairs, stat};
    for (int i = 0; i < 5; i++) {
        if (!out[i]) continue;
        for (int j = 0; j < 3; j++)
            if (out[i] == in[j]) return fail(JB_EINVAL, "%s: an output array is an input array", who);
        for (int j = i + 1; j < 5; j++)
            if (out[i] == out[j]) return fail(JB_EINVAL, "%s: two output arrays are the same", who);
    }
    return JB_OK;
}

NeardupWork neardup_layout(uint64_t nentries) {
    NeardupWork w;
    w.ntl = std::max<uint64_t>(1u, (nentries + JB_ND_TILE - 1u) / JB_ND_TILE);
    auto r256 = [](size_t x) { return (x + 255u) & ~(size_t)255u; };
    const size_t slots = (size_t)w.ntl * JB_ND_TILE;
    w.key[0] = 0;
    w.key[1] = w.key[0] + r256(slots * 8u);
    w.pay[0] = w.key[1] + r256(slots * 8u);
    w.pay[1] = w.pay[0] + r256(slots * 4u);
    w.cnt = w.pay[1] + r256(slots * 4u);
    w.tot = w.cnt + r256((size_t)w.ntl * 256u * 4u);
    w.part = w.tot + r256(256u * 4u);
    w.tbase = w.part + r256((size_t)w.ntl * 3u * 4u);
    w.bytes = w.tbase + r256((size_t)w.ntl * 8u);
    return w;
}

}  // namespace jb

extern "C" size_t jb_neardup_work_bytes(uint32_t ndocs, uint32_t B) {
    const uint64_t n = (uint64_t)ndocs * B;
    if (n > (1ull << 40)) return SIZE_MAX;
    return jb::neardup_layout(n).bytes;
}

namespace {
struct Kept {
    uint32_t e, i, agree;
};
}  // namespace

extern "C" int jb_neardup(const uint64_t* key, const uint32_t* sig, uint32_t ndocs, uint32_t B, uint32_t K, uint32_t W,
                          uint32_t min_agree, uint32_t* pair_doc, uint32_t* pair_agree, uint64_t pcap, uint64_t* pair_off,
                          uint64_t* npairs, uint64_t* stat) {
    const char* who = "jb_neardup";
    if (const int rc = jb::neardup_args(who, ndocs, B, K, W, min_agree)) return rc;
    if (!pair_off || !npairs || !stat || (ndocs && (!key || !sig)) || (pcap && (!pair_doc || !pair_agree)))
        return fail(JB_EINVAL, "%s: null argument", who);
    if (const int rc = jb::neardup_alias(who, key, sig, pair_doc, pair_agree, pair_off, npairs, stat, nullptr)) return rc;
    const uint32_t N = ndocs * B;
    std::vector<uint32_t> ord;
    std::vector<Kept> kept;
    uint64_t ncand = 0, ntrunc = 0;
    try {
        for (uint32_t e = 0; e < N; e++)
            if (key[e] != JB_MH_NOKEY) ord.push_back(e);
        // equal (band, key) together, documents ascending inside
        std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) {
            const uint32_t bx = jb_nd_band(x, B), by = jb_nd_band(y, B);
            if (bx != by) return bx < by;
            if (key[x] != key[y]) return key[x] < key[y];
            return x < y;
        });
        for (size_t r0 = 0; r0 < ord.size();) {
            size_t r1 = r0 + 1;
            while (r1 < ord.size() && jb_nd_same(ord[r0], key[ord[r0]], ord[r1], key[ord[r1]], B)) r1++;
            const uint32_t b = jb_nd_band(ord[r0], B);
            for (size_t m = r0; m < r1; m++) {
                const size_t rank = m - r0;
                if (rank > W) ntrunc++;
                const uint32_t e = ord[m], j = jb_nd_doc(e, B);
                for (size_t w = std::min<size_t>(rank, W); w-- > 0;) {  // the member w + 1 places below: i ascends
                    const uint32_t i = jb_nd_doc(ord[m - 1u - w], B);
                    if (!jb_nd_first(key, i, j, B, b)) continue;
                    ncand++;
                    uint32_t agree = 0;
                    for (uint32_t s = 0; s < K; s++) agree += jb_nd_eq(sig, i, j, K, s);
                    if (agree >= min_agree) kept.push_back(Kept{e, i, agree});
                }
            }
            r0 = r1;
        }
        // row j by (band, i): the entries in order, each entry's pairs as found
        std::stable_sort(kept.begin(), kept.end(), [](const Kept& x, const Kept& y) { return x.e < y.e; });
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "%s: out of host memory for %u entries", who, N);
    }
    for (uint64_t j = 0; j <= ndocs; j++) pair_off[j] = 0;
    for (const Kept& p : kept) pair_off[(uint64_t)jb_nd_doc(p.e, B) + 1u]++;
    for (uint64_t j = 0; j < ndocs; j++) pair_off[j + 1u] += pair_off[j];
    *npairs = kept.size();
    stat[JB_ND_NENTRIES] = ord.size();
    stat[JB_ND_NCAND] = ncand;
    stat[JB_ND_NTRUNC] = ntrunc;
    for (uint64_t k = 0; k < kept.size() && k < pcap; k++) {
        pair_doc[k] = kept[k].i;
        pair_agree[k] = kept[k].agree;
    }
    return JB_OK;
}

extern "C" int jb_neardup_labels(const uint64_t* pair_off, const uint32_t* pair_doc, uint64_t pcap, uint32_t ndocs,
                                 uint32_t* label) {
    const char* who = "jb_neardup_labels";
    if (!pair_off || (ndocs && !label) || (pcap && !pair_doc)) return fail(JB_EINVAL, "%s: null argument", who);
    // a union-find whose root is the least document of its set, so that a root is its set's label
    for (uint32_t d = 0; d < ndocs; d++) label[d] = d;
    auto find = [&](uint32_t d) {
        while (label[d] != d) {
            label[d] = label[label[d]];
            d = label[d];
        }
        return d;
    };
    for (uint32_t j = 0; j < ndocs; j++) {
        const uint64_t lo = std::min(pair_off[j], pcap), hi = std::min(pair_off[(uint64_t)j + 1u], pcap);
        for (uint64_t k = lo; k < hi; k++) {
            const uint32_t i = pair_doc[k];
            if (i >= j) continue;  // (a caller's CSR: not a pair of this row)
            const uint32_t a = find(i), c = find(j);
            if (a < c) label[c] = a;
            else label[a] = c;
        }
    }
    for (uint32_t d = 0; d < ndocs; d++) label[d] = find(d);
    return JB_OK;
}
