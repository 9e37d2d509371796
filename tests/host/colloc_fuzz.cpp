// The collocation rule's host code (jieba-go_amd/csrc/jb_colloc.cpp) and the code jb_colloc.h shares between host
// and kernels under AddressSanitizer + UndefinedBehaviorSanitizer.  Each round draws a seeded id list of arbitrary
// u32 (small ids so that pairs repeat, JB_ID_UNK, ids at and past nuni), a doc_tok that is sorted in most rounds
// and hostile in the others (decreasing, past the list), an ntok on either side of ids_cap, a keep mask shorter
// than nuni, spans of arbitrary bits, and runs jb_colloc_count with and without a slot limit.  The result is
// compared with the rule restated here document by document (sorted doc_tok), and the identities are checked in
// every round; then jb_colloc_score runs over the pairs with a hostile uni and N.  Every array, the outputs
// included, is a heap block of exactly the length the call is told, so a read or write outside one is a report.
// usage: colloc_fuzz <rounds> <seed>; prints "ok".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <vector>

#include "jb_colloc.h"
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
    auto die = [&](int round, const char* what) {
        std::fprintf(stderr, "round %d: %s (%s)\n", round, what, jb_last_error());
        std::exit(1);
    };
    for (int round = 0; round < rounds; round++) {
        const uint64_t cap = pick(6) == 0 ? pick(3) : pick(700);
        const uint32_t nuni = pick(8) == 0 ? 0u : 1u + (uint32_t)pick(12);
        const uint32_t ndocs = (uint32_t)pick(pick(4) == 0 ? 2 : 40);
        const uint64_t ntok = pick(3) == 0 ? cap + pick(50) : pick(cap + 1);
        const uint64_t n = std::min(ntok, cap);
        std::vector<uint32_t> ids(cap), st(cap), en(cap);
        for (auto& v : ids) {
            const uint64_t k = pick(20);
            v = k == 0 ? JB_ID_UNK : k == 1 ? nuni + (uint32_t)pick(3) : k == 2 ? (uint32_t)rng() : (uint32_t)pick(nuni ? nuni : 1);
        }
        uint32_t pos = 0;
        for (uint64_t k = 0; k < cap; k++) {  // mostly touching spans, with gaps, overlaps and noise
            st[k] = pick(30) == 0 ? (uint32_t)rng() : pos;
            en[k] = st[k] + 1u + (uint32_t)pick(4);
            pos = en[k] + (pick(5) == 0 ? 1u : 0u) - (pick(9) == 0 ? 1u : 0u);
        }
        const bool sorted = pick(4) != 0;
        std::vector<uint64_t> dt((size_t)ndocs + 1);
        for (auto& v : dt) v = pick(12) == 0 ? cap + pick(9) : pick(7) == 0 ? rng() : pick(cap + 1);
        if (sorted) std::sort(dt.begin(), dt.end());
        const uint32_t nkeep = pick(3) == 0 ? 0u : (uint32_t)pick(nuni + 2u);
        std::vector<uint8_t> keep(nkeep);
        for (auto& v : keep) v = pick(4) == 0 ? 0 : (uint8_t)(1u + pick(255));
        const uint32_t flags = pick(2) ? JB_COLLOC_CONTIG : 0u;
        const auto p_ids = exact(ids), p_st = exact(st), p_en = exact(en);
        const auto p_dt = exact(dt);
        const auto p_keep = exact(keep);
        const bool spans = flags || pick(2);
        for (int limited = 0; limited < 2; limited++) {
            const uint64_t nslots = limited ? 8ull << pick(4) : 0;
            std::vector<uint64_t> base(nuni);
            for (auto& v : base) v = pick(1000);
            auto p_uni = exact(base);
            jb_colloc_result r;
            if (jb_colloc_count(cap ? p_ids.get() : nullptr, cap, p_dt.get(), ntok, ndocs, nkeep ? p_keep.get() : nullptr, nkeep,
                                flags, spans ? p_st.get() : nullptr, spans ? p_en.get() : nullptr, nslots,
                                nuni ? p_uni.get() : nullptr, nuni, &r) != JB_OK)
                die(round, "jb_colloc_count failed");
            uint64_t sum = 0, added = 0;
            for (uint64_t i = 0; i < r.n; i++) {
                sum += r.count[i];
                if (r.count[i] == 0 || r.a[i] >= nuni || r.b[i] >= nuni) die(round, "a pair that cannot be");
                if (i && jb_cl_key(r.a[i - 1], r.b[i - 1]) >= jb_cl_key(r.a[i], r.b[i])) die(round, "not sorted by key");
                if (r.score[i] != (float)(double)r.count[i]) die(round, "the score is not the count");
            }
            for (uint32_t t = 0; t < nuni; t++) added += p_uni[t] - base[t];
            if (sum + r.dropped != r.pairs || added != r.known || r.tokens != n || r.distinct != r.n)
                die(round, "an identity does not hold");
            if (limited && r.n > nslots / 2u) die(round, "more keys than the half");
            if (!limited && r.dropped) die(round, "dropped without a limit");
            if (sorted) {  // the rule once more, document by document
                std::map<uint64_t, uint64_t> want;
                std::vector<uint64_t> uni(nuni, 0);
                uint64_t known = 0, pairs = 0, dropped = 0;
                auto kept = [&](uint32_t t) { return t < nuni && (nkeep == 0 || (t < nkeep && keep[t] != 0)); };
                for (uint32_t d = 0; d < ndocs; d++) {
                    const uint64_t lo = std::min(dt[d], n), hi = std::min(dt[d + 1], n);
                    for (uint64_t k = lo; k < hi; k++) {
                        if (ids[k] < nuni) {
                            uni[ids[k]]++;
                            known++;
                        }
                        if (k + 1 >= hi || !kept(ids[k]) || !kept(ids[k + 1])) continue;
                        if (flags && en[k] != st[k + 1]) continue;
                        pairs++;
                        const uint64_t key = jb_cl_key(ids[k], ids[k + 1]);
                        if (want.count(key)) want[key]++;
                        else if (!limited || want.size() < nslots / 2u) want[key] = 1;
                        else dropped++;
                    }
                }
                if (known != r.known || pairs != r.pairs || dropped != r.dropped || want.size() != r.n)
                    die(round, "the totals differ from the restated rule");
                uint64_t i = 0;
                for (const auto& kv : want) {
                    if (jb_cl_key(r.a[i], r.b[i]) != kv.first || r.count[i] != kv.second) die(round, "a pair differs");
                    i++;
                }
                for (uint32_t t = 0; t < nuni; t++)
                    if (p_uni[t] - base[t] != uni[t]) die(round, "uni differs");
            }
            // the scores over these pairs, with a hostile uni and N; the pairs' arrays as exact blocks again
            std::vector<uint32_t> a(r.a, r.a + r.n), b(r.b, r.b + r.n);
            std::vector<uint64_t> c(r.count, r.count + r.n), hu(nuni);
            for (auto& v : a)
                if (pick(9) == 0) v = (uint32_t)rng();
            for (auto& v : c)
                if (pick(9) == 0) v = rng() >> pick(64);
            for (auto& v : hu) v = pick(5) == 0 ? rng() >> pick(64) : pick(4) == 0 ? 0 : 1u + pick(900);
            const auto pa = exact(a), pb = exact(b);
            const auto pc = exact(c), pu = exact(hu);
            const uint32_t snuni = (uint32_t)pick(nuni + 1u);
            const uint64_t N = pick(6) == 0 ? rng() >> pick(64) : 1u + pick(5000), m = 1u + pick(4), topn = pick(3) ? 0 : pick(r.n + 2);
            const float thr = pick(5) == 0 ? NAN : pick(5) == 0 ? -INFINITY : (float)pick(200) / 100.0f - 1.0f;
            for (int scorer = 0; scorer < 3; scorer++) {
                jb_colloc_result s;
                if (jb_colloc_score(r.n ? pa.get() : nullptr, r.n ? pb.get() : nullptr, r.n ? pc.get() : nullptr, r.n,
                                    snuni ? pu.get() : nullptr, snuni, N, scorer, m, thr, topn, &s) != JB_OK)
                    die(round, "jb_colloc_score failed");
                if (s.n > r.n || (topn && s.n > topn)) die(round, "more candidates than pairs or topn");
                for (uint64_t i = 0; i < s.n; i++) {
                    if (!(s.score[i] >= thr) || s.count[i] < m || s.a[i] >= snuni || s.b[i] >= snuni || s.count[i] >= N)
                        die(round, "a candidate that is none");
                    if (i && jb_cl_before(s.score[i], s.count[i], jb_cl_key(s.a[i], s.b[i]), s.score[i - 1], s.count[i - 1],
                                          jb_cl_key(s.a[i - 1], s.b[i - 1])))
                        die(round, "the order");
                }
                jb_colloc_result_free(&s);
            }
            jb_colloc_result_free(&r);
        }
    }
    std::printf("ok\n");
    return 0;
}
