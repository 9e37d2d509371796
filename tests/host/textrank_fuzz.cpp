// jb_textrank (jieba-go_amd/csrc/jb_textrank.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer:
// seeded id lists with CSRs that are right, that lack ids, whose rows are unsorted, whose offsets pass cap
// or decrease, and token counts on either side of the id array's length.  Every array is a heap block of
// exactly the length the call is told, so a read or write outside one is a report.  A right CSR must give
// the same result twice and kw_n <= topk with the empty slots filled.
// usage: textrank_fuzz <rounds> <seed>; prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include "jiebahip.h"

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 50;
    std::mt19937_64 rng(argc > 2 ? std::atoll(argv[2]) : 1);
    auto pick = [&](uint64_t n) { return n ? rng() % n : 0; };
    for (int round = 0; round < rounds; round++) {
        const uint32_t ndocs = (uint32_t)pick(6), nvocab = 1 + (uint32_t)pick(30);
        std::vector<uint32_t> ids, term_id;
        std::vector<uint64_t> doc_tok(1, 0), term_off(1, 0);
        for (uint32_t d = 0; d < ndocs; d++) {
            const uint64_t len = pick(4) == 0 ? 0 : pick(200);
            std::set<uint32_t> seen;
            for (uint64_t k = 0; k < len; k++) {
                const uint32_t id = pick(10) == 0 ? JB_ID_UNK : (uint32_t)pick(nvocab + 3);
                ids.push_back(id);
                if (id != JB_ID_UNK) seen.insert(id);
            }
            doc_tok.push_back(ids.size());
            term_id.insert(term_id.end(), seen.begin(), seen.end());
            term_off.push_back(term_id.size());
        }
        std::vector<uint8_t> keep(nvocab);
        for (auto& k : keep) k = pick(5) != 0;
        const uint32_t span = 2 + (uint32_t)pick(31), iters = (uint32_t)pick(12), topk = 1 + (uint32_t)pick(64);
        uint64_t ntok = ids.size(), ids_cap = ids.size(), cap = term_id.size();
        const int kind = (int)pick(6);
        bool right = kind == 0;
        if (kind == 1 && !term_id.empty()) term_id.erase(term_id.begin() + (long)pick(term_id.size())), term_off.back()--, cap--;
        if (kind == 2) std::shuffle(term_id.begin(), term_id.end(), rng);
        if (kind == 3) cap = pick(cap + 1);       // an overflowed CSR
        if (kind == 4 && ndocs) term_off[1 + pick(ndocs)] = pick(2 * cap + 2);  // offsets out of order or past cap
        if (kind == 5) {
            ntok = pick(2 * ids.size() + 2);
            ids_cap = pick(ids.size() + 1);
        }
        ids.resize(ids_cap);
        term_id.resize(std::min<uint64_t>(cap, term_id.size()));
        cap = term_id.size() < cap ? term_id.size() : cap;
        auto p_ids = exact(ids);
        auto p_tid = exact(term_id);
        auto p_doc = exact(doc_tok);
        auto p_off = exact(term_off);
        auto p_keep = exact(keep);
        std::vector<std::unique_ptr<uint32_t[]>> oid, on;
        std::vector<std::unique_ptr<float[]>> osc;
        for (int rep = 0; rep < 2; rep++) {
            oid.emplace_back(new uint32_t[(size_t)ndocs * topk]);
            osc.emplace_back(new float[(size_t)ndocs * topk]);
            on.emplace_back(new uint32_t[ndocs]);
            const int rc = jb_textrank(p_ids.get(), ids_cap, p_doc.get(), ntok, ndocs, p_tid.get(), p_off.get(), cap,
                                       p_keep.get(), nvocab, span, iters, topk, oid[rep].get(), osc[rep].get(), on[rep].get());
            if (rc != JB_OK) {
                std::fprintf(stderr, "round %d: %s\n", round, jb_last_error());
                return 1;
            }
        }
        if (ndocs && (std::memcmp(oid[0].get(), oid[1].get(), (size_t)ndocs * topk * 4) != 0 ||
                      std::memcmp(osc[0].get(), osc[1].get(), (size_t)ndocs * topk * 4) != 0 ||
                      std::memcmp(on[0].get(), on[1].get(), (size_t)ndocs * 4) != 0)) {
            std::fprintf(stderr, "round %d: two calls differ\n", round);
            return 1;
        }
        for (uint32_t d = 0; d < ndocs; d++) {
            const uint32_t n = on[0][d];
            if (n > topk) return 1;
            for (uint32_t k = 0; k < topk; k++) {
                const uint32_t id = oid[0][(size_t)d * topk + k];
                const float sc = osc[0][(size_t)d * topk + k];
                if (k >= n ? (id != JB_ID_UNK || sc != 0.0f) : (id == JB_ID_UNK || (right && !(sc > 0.0f && sc <= 1.0f)))) {
                    std::fprintf(stderr, "round %d: document %u slot %u is (%u, %g) with kw_n %u\n", round, d, k, id, (double)sc, n);
                    return 1;
                }
                if (right && k > 0 && k < n && sc > osc[0][(size_t)d * topk + k - 1]) return 1;
            }
            if (right && n > 0 && osc[0][(size_t)d * topk] != 1.0f) return 1;
        }
    }
    std::printf("ok\n");
    return 0;
}
