// The postings rule's host code (jieba-go_amd/csrc/jb_postings.cpp) and the code jb_postings.h shares between
// host and kernels under AddressSanitizer + UndefinedBehaviorSanitizer.  Each round draws a seeded CSR: ids on
// either side of nids (and 0xFFFFFFFF), counts on either side of the arrays' length, a term_off that is
// non-decreasing from 0, or reaches past the list, or decreases, a doc_base up to the limit and a pcap up to
// cap, and runs jb_postings on it.  With trusted offsets the result is compared with the rule restated here (a
// std::stable_sort); with broken ones only the counts are.  Every array, the outputs included, is a heap block
// of exactly the length the call is told, so a read or write outside one is a report.
// usage: postings_fuzz <rounds> <seed>; prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "jb_postings.h"
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
        const uint64_t len = pick(4) == 0 ? pick(8) : pick(10) == 0 ? 4000 + pick(5000) : pick(700);
        const uint32_t nids = pick(6) == 0 ? (uint32_t)pick(3) : pick(5) == 0 ? 60000u + (uint32_t)pick(10000) : 1u + (uint32_t)pick(300);
        std::vector<uint32_t> id(len), cnt(len);
        for (uint64_t i = 0; i < len; i++) {
            id[i] = pick(40) == 0 ? 0xFFFFFFFFu : (uint32_t)pick((uint64_t)nids + nids / 4 + 2);
            cnt[i] = (uint32_t)rng();
        }
        uint64_t nterms = len, cap = len;
        const int kind = (int)pick(3);
        if (kind == 1) nterms = pick(2 * len + 2), cap = pick(len + 1);
        if (kind == 2) nterms = pick(len + 1);
        id.resize(cap);
        cnt.resize(cap);
        const uint32_t ndocs = (uint32_t)pick(pick(3) == 0 ? 3 : 60);
        std::vector<uint64_t> off(ndocs + 1);
        for (auto& t : off) t = pick(len + 1);
        std::sort(off.begin(), off.end());
        off[0] = 0;
        const int okind = (int)pick(6);  // 0-2 a full cover, 3 short of the list, 4 past it, 5 decreasing
        if (okind <= 2) off[ndocs] = ndocs ? len : 0;
        if (okind == 4) off[ndocs] = ndocs ? len + 1 + pick(1000) : 0;
        const bool trusted = okind != 5;
        if (!trusted) {
            std::sort(off.begin(), off.end(), [](uint64_t a, uint64_t b) { return a > b; });
            if (pick(2)) off[ndocs] = ~0ull;
        }
        const uint32_t doc_base = pick(3) == 0 ? 0xFFFFFFFFu - ndocs + 1u : (uint32_t)pick(1u << 20);
        const uint64_t pcap = pick(3) == 0 ? pick(cap + 1) : cap;
        auto p_id = exact(id);
        auto p_cnt = exact(cnt);
        auto p_off = exact(off);
        std::unique_ptr<uint32_t[]> pd(new uint32_t[pcap]), pt(new uint32_t[pcap]);
        std::unique_ptr<uint64_t[]> po(new uint64_t[(size_t)nids + 1]), np(new uint64_t[1]);
        if (jb_postings(p_id.get(), p_cnt.get(), p_off.get(), nterms, cap, ndocs, nids, doc_base, pd.get(), pt.get(), pcap,
                        po.get(), np.get()) != JB_OK)
            die(round, "jb_postings failed");
        // the rule once more
        const uint64_t n = std::min(std::min(nterms, cap), off[ndocs]);
        std::vector<uint64_t> take;
        for (uint64_t i = 0; i < n; i++)
            if (id[i] < nids) take.push_back(i);
        std::stable_sort(take.begin(), take.end(), [&](uint64_t a, uint64_t b) { return id[a] < id[b]; });
        if (np[0] != take.size() || po[nids] != take.size() || po[0] != 0) die(round, "the count is wrong");
        uint64_t at = 0;
        for (uint32_t t = 0; t < nids; t++) {
            if (po[t] != at) die(round, "a list offset is wrong");
            while (at < take.size() && id[take[at]] == t) at++;
        }
        if (!trusted) continue;
        for (uint64_t k = 0; k < take.size() && k < pcap; k++) {
            const uint64_t i = take[k];
            const uint64_t row = jb_postings_row_ub(off.data(), i, 0, (uint64_t)ndocs + 1u) - 1u;
            if (!(off[row] <= i && i < off[row + 1])) die(round, "the row search is wrong");
            if (pd[k] != doc_base + (uint32_t)row) die(round, "a document is wrong");
            if (pt[k] != cnt[i]) die(round, "a term frequency is wrong");
        }
    }
    // the shared helpers and the limits
    if (jb_postings_passes(0) != 1 || jb_postings_passes(1) != 1 || jb_postings_passes(255) != 1 ||
        jb_postings_passes(256) != 2 || jb_postings_passes(65535) != 2 || jb_postings_passes(65536) != 3 ||
        jb_postings_passes((1u << 24) - 1u) != 3 || jb_postings_passes(1u << 24) != 4 || jb_postings_passes(0xFFFFFFFFu) != 4)
        die(-1, "jb_postings_passes");
    if (jb_postings_key(5, 3, 4, 6) != 5 || jb_postings_key(6, 3, 4, 6) != 6 || jb_postings_key(5, 4, 4, 6) != 6)
        die(-1, "jb_postings_key");
    const uint64_t off1[2] = {0, 0};
    uint64_t po1[1] = {9}, n1 = 9;
    if (jb_postings(nullptr, nullptr, off1, 0, 0, 1, 0, 0, nullptr, nullptr, 0, po1, &n1) != JB_OK || po1[0] != 0 || n1 != 0)
        die(-1, "empty input");
    if (jb_postings(nullptr, nullptr, off1, 0, (1ull << 32) - JB_POSTINGS_TILE, 1, 0, 0, nullptr, nullptr, 0, po1, &n1) !=
        JB_ELIMIT)
        die(-1, "cap at the limit");
    if (jb_postings(nullptr, nullptr, off1, 0, 0, 2, 0, 0xFFFFFFFFu, nullptr, nullptr, 0, po1, &n1) != JB_ELIMIT)
        die(-1, "doc_base + ndocs past 2^32");
    if (jb_postings(nullptr, nullptr, nullptr, 0, 0, 1, 0, 0, nullptr, nullptr, 0, po1, &n1) != JB_EINVAL)
        die(-1, "null term_off");
    if (jb_postings_work_bytes(0, 0, 0) == 0 || jb_postings_work_bytes(~0ull, ~0ull, 0xFFFFFFFFu) == 0) die(-1, "size helper");
    std::printf("ok\n");
    return 0;
}
