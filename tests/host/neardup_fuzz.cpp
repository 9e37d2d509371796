// The near-duplicate rule's host code (jieba-go_amd/csrc/jb_neardup.cpp) and the code jb_neardup.h shares between
// host and kernels under AddressSanitizer + UndefinedBehaviorSanitizer.  Each round draws seeded keys and slots:
// arbitrary bit patterns, values from small pools so that buckets form, JB_MH_NOKEY, any B, K, W and min_agree
// inside the limits and a pcap up to past the count, and runs jb_neardup on them.  The result is compared with
// the rule restated here (all pairs i < j, the first common band, the rank difference by counting), and
// jb_neardup_labels with a flood fill; then the labels run on a hostile CSR.  Every array, the outputs included,
// is a heap block of exactly the length the call is told, so a read or write outside one is a report.
// usage: neardup_fuzz <rounds> <seed>; prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "jb_neardup.h"
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
        const uint32_t nd = pick(5) == 0 ? (uint32_t)pick(3) : (uint32_t)pick(90);
        const uint32_t B = pick(8) == 0 ? JB_MH_MAXK : 1u + (uint32_t)pick(6);
        const uint32_t K = pick(8) == 0 ? JB_MH_MAXK : 1u + (uint32_t)pick(70);
        const uint32_t W = pick(3) == 0 ? JB_ND_MAXWIN : 1u + (uint32_t)pick(5);
        const uint32_t m = pick(4) == 0 ? K : 1u + (uint32_t)pick(K);
        const uint64_t npool = 1u + pick(8);
        std::vector<uint64_t> pool(npool);
        for (auto& v : pool) v = pick(6) == 0 ? (JB_MH_NOKEY - pick(2)) : rng() >> pick(64);
        std::vector<uint64_t> key((size_t)nd * B);
        for (auto& k : key) k = pick(10) == 0 ? rng() : pool[pick(npool)];
        std::vector<uint32_t> proto(K * 3u), sig((size_t)nd * K);
        for (auto& v : proto) v = (uint32_t)rng();
        for (uint32_t d = 0; d < nd; d++) {
            const uint32_t which = (uint32_t)pick(3);
            for (uint32_t s = 0; s < K; s++) sig[(size_t)d * K + s] = pick(6) == 0 ? (uint32_t)rng() : proto[which * K + s];
        }
        // the rule once more: all pairs, the first common band, the rank difference in that bucket
        struct Pair {
            uint32_t j, b, i, agree;
        };
        std::vector<Pair> want;
        uint64_t nent = 0, ncand = 0, ntrunc = 0;
        for (uint32_t j = 0; j < nd; j++)
            for (uint32_t b = 0; b < B; b++) {
                const uint64_t kj = key[(size_t)j * B + b];
                if (kj == JB_MH_NOKEY) continue;
                nent++;
                uint32_t rank = 0;
                for (uint32_t i = 0; i < j; i++) rank += key[(size_t)i * B + b] == kj;
                if (rank > W) ntrunc++;
            }
        for (uint32_t j = 0; j < nd; j++)
            for (uint32_t i = 0; i < j; i++) {
                uint32_t b = 0;
                while (b < B && !(key[(size_t)i * B + b] == key[(size_t)j * B + b] && key[(size_t)i * B + b] != JB_MH_NOKEY)) b++;
                if (b == B) continue;
                uint32_t between = 0;  // members above i and up to j: rank(j) - rank(i)
                for (uint32_t d = i + 1; d <= j; d++) between += key[(size_t)d * B + b] == key[(size_t)j * B + b];
                if (between > W) continue;
                ncand++;
                uint32_t agree = 0;
                for (uint32_t s = 0; s < K; s++) agree += sig[(size_t)i * K + s] == sig[(size_t)j * K + s];
                if (agree >= m) want.push_back(Pair{j, b, i, agree});
            }
        std::sort(want.begin(), want.end(), [](const Pair& x, const Pair& y) {
            return x.j != y.j ? x.j < y.j : x.b != y.b ? x.b < y.b : x.i < y.i;
        });
        const uint64_t pcap = pick(3) == 0 ? pick(want.size() + 1) : want.size() + pick(3);
        auto p_key = exact(key);
        auto p_sig = exact(sig);
        std::unique_ptr<uint32_t[]> pd(new uint32_t[pcap]), pa(new uint32_t[pcap]);
        std::unique_ptr<uint64_t[]> po(new uint64_t[(size_t)nd + 1]), np(new uint64_t[1]), st(new uint64_t[JB_ND_NSTAT]);
        if (jb_neardup(p_key.get(), p_sig.get(), nd, B, K, W, m, pd.get(), pa.get(), pcap, po.get(), np.get(), st.get()) !=
            JB_OK)
            die(round, "jb_neardup failed");
        if (np[0] != want.size() || po[nd] != want.size() || po[0] != 0) die(round, "the count is wrong");
        if (st[JB_ND_NENTRIES] != nent || st[JB_ND_NCAND] != ncand || st[JB_ND_NTRUNC] != ntrunc) die(round, "a counter is wrong");
        uint64_t at = 0;
        for (uint32_t j = 0; j < nd; j++) {
            if (po[j] != at) die(round, "a row offset is wrong");
            while (at < want.size() && want[at].j == j) at++;
        }
        for (uint64_t k = 0; k < want.size() && k < pcap; k++)
            if (pd[k] != want[k].i || pa[k] != want[k].agree) die(round, "a pair is wrong");
        // the labels: the least document reachable over the kept pairs
        if (pcap >= want.size()) {
            std::unique_ptr<uint32_t[]> label(new uint32_t[nd]);
            if (jb_neardup_labels(po.get(), pd.get(), pcap, nd, label.get()) != JB_OK) die(round, "jb_neardup_labels failed");
            std::vector<uint32_t> comp(nd);
            for (uint32_t d = 0; d < nd; d++) comp[d] = d;
            for (bool moved = true; moved;) {
                moved = false;
                for (const Pair& p : want) {
                    const uint32_t lo = std::min(comp[p.i], comp[p.j]);
                    if (comp[p.i] != lo || comp[p.j] != lo) comp[p.i] = comp[p.j] = lo, moved = true;
                }
            }
            for (uint32_t d = 0; d < nd; d++)
                if (label[d] != comp[d]) die(round, "a label is wrong");
        }
        // a hostile CSR: any offsets, any documents, any pcap up to the array
        const uint64_t hlen = pick(60);
        std::vector<uint32_t> hd(hlen);
        std::vector<uint64_t> ho((size_t)nd + 1);
        for (auto& v : hd) v = pick(4) == 0 ? (uint32_t)rng() : (uint32_t)pick((uint64_t)nd + 3);
        for (auto& v : ho) v = pick(4) == 0 ? rng() : pick(hlen + 5);
        auto p_hd = exact(hd);
        auto p_ho = exact(ho);
        std::unique_ptr<uint32_t[]> hl(new uint32_t[nd]);
        if (jb_neardup_labels(p_ho.get(), p_hd.get(), pick(hlen + 1), nd, hl.get()) != JB_OK) die(round, "labels on a hostile CSR");
        for (uint32_t d = 0; d < nd; d++)
            if (hl[d] > d) die(round, "a label above its document");
    }
    // the shared helpers and the limits
    const uint64_t k2[4] = {5, JB_MH_NOKEY, 5, JB_MH_NOKEY};
    if (jb_nd_doc(7, 3) != 2 || jb_nd_band(7, 3) != 1 || !jb_nd_same(0, 5, 3, 5, 3) || jb_nd_same(0, 5, 4, 5, 3) ||
        jb_nd_same(0, 5, 3, 6, 3) || jb_nd_same(0, JB_MH_NOKEY, 3, JB_MH_NOKEY, 3))
        die(-1, "the entry helpers");
    if (!jb_nd_first(k2, 0, 1, 2, 0) || jb_nd_first(k2, 0, 1, 2, 1) || !jb_nd_first(k2 + 1, 0, 1, 1, 0)) die(-1, "jb_nd_first");
    const uint32_t s2[4] = {1, 2, 1, 3};
    if (jb_nd_eq(s2, 0, 1, 2, 0) != 1 || jb_nd_eq(s2, 0, 1, 2, 1) != 0 || jb_nd_eq(s2, 0, 1, 2, 2) != 0) die(-1, "jb_nd_eq");
    uint64_t po1[1] = {9}, n1 = 9, st1[JB_ND_NSTAT] = {9, 9, 9};
    if (jb_neardup(nullptr, nullptr, 0, 1, 1, 1, 1, nullptr, nullptr, 0, po1, &n1, st1) != JB_OK || po1[0] != 0 || n1 != 0 ||
        st1[0] != 0)
        die(-1, "empty input");
    if (jb_neardup(nullptr, nullptr, 0, 0, 1, 1, 1, nullptr, nullptr, 0, po1, &n1, st1) != JB_EINVAL) die(-1, "B = 0");
    if (jb_neardup(nullptr, nullptr, 0, 1, 1, JB_ND_MAXWIN + 1, 1, nullptr, nullptr, 0, po1, &n1, st1) != JB_ELIMIT) die(-1, "W");
    if (jb_neardup(nullptr, nullptr, 0, 1, 1, 1, 2, nullptr, nullptr, 0, po1, &n1, st1) != JB_ELIMIT) die(-1, "min_agree > K");
    if (jb_neardup(nullptr, nullptr, 0xFFFFFFFFu, JB_MH_MAXK, 1, 1, 1, nullptr, nullptr, 0, po1, &n1, st1) != JB_ELIMIT)
        die(-1, "entries at the limit");
    if (jb_neardup(nullptr, nullptr, 1, 1, 1, 1, 1, nullptr, nullptr, 0, po1, &n1, st1) != JB_EINVAL) die(-1, "null key");
    if (jb_neardup_work_bytes(0, 0) == 0 || jb_neardup_work_bytes(0xFFFFFFFFu, 0xFFFFFFFFu) == 0) die(-1, "size helper");
    std::printf("ok\n");
    return 0;
}
