// The token filter's host code (jieba-go_amd/csrc/jb_filter.cpp) and the code jb_filter.h shares between host
// and kernels (class, rune count, decision) under AddressSanitizer + UndefinedBehaviorSanitizer.  Each round
// draws a seeded span list with ordered, overlapping and bad spans (start >= end, end past the text, start near
// 2^32), keys on either side of 8, 24, 255 and 1024 bytes, token counts on either side of the span arrays'
// length, a doc_tok that is sorted, or not, or reaches past the list, a rule and a stop set, and runs jb_filter
// on it; the result is compared with the rule restated here.  Every array, the outputs included, is a heap
// block of exactly the length the call is told, so a read or write outside one is a report.
// usage: filter_fuzz <rounds> <seed>; prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "jb_filter.h"
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
    static const char* const kAlpha[] = {"a", "7", "\xe4\xb8\xad", "\xe7\x9a\x84", "\xef\xbc\x8c", "\x80", "\xe4", " ", "Q"};
    for (int round = 0; round < rounds; round++) {
        std::vector<uint8_t> text;
        const uint64_t want = pick(3) == 0 ? pick(40) : pick(20) == 0 ? 1500 + pick(2000) : pick(600);
        while (text.size() < want) {
            const char* a = kAlpha[pick(9)];
            const uint64_t rep = pick(50) == 0 ? 300 + pick(1200) : 1;  // (long runs: keys past 255 and 1024 bytes)
            for (uint64_t r = 0; r < rep; r++) text.insert(text.end(), a, a + std::strlen(a));
        }
        const uint64_t nbytes = text.size();
        const uint64_t n = pick(300);
        std::vector<uint32_t> start(n), end(n);
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t s = pick(nbytes + 1);
            const uint64_t len = pick(3) == 0 ? 1 : pick(10) == 0 ? 6 + pick(22) : pick(30) == 0 ? 250 + pick(10)
                                 : pick(30) == 0 ? 1020 + pick(10) : pick(7);
            start[k] = (uint32_t)s;
            end[k] = (uint32_t)std::min<uint64_t>(s + len, nbytes);
            const uint64_t kind = pick(20);
            if (kind == 0) end[k] = start[k];
            if (kind == 1) std::swap(start[k], end[k]);
            if (kind == 2) end[k] = (uint32_t)(nbytes + 1 + pick(1000));
            if (kind == 3) start[k] = 0xFFFFFFF0u, end[k] = 0xFFFFFFFFu;
        }
        uint64_t ntok = n, cap = n;
        const int kind = (int)pick(3);
        if (kind == 1) ntok = pick(2 * n + 2), cap = pick(n + 1);
        if (kind == 2) ntok = pick(n + 1);
        start.resize(cap);
        end.resize(cap);
        const uint32_t ndocs = (uint32_t)pick(12);
        std::vector<uint64_t> tok(ndocs + 1);
        for (auto& t : tok) t = pick(8) == 0 ? pick(4 * n + 9) : pick(n + 3);
        const bool sorted = pick(4) != 0;
        if (sorted) std::sort(tok.begin(), tok.end());
        else std::sort(tok.begin(), tok.end(), [](uint64_t a, uint64_t b) { return a > b; });
        if (pick(9) == 0) tok[ndocs] = ~0ull;
        // a stop set of some of the list's own keys (and the replacement character), unless there is none
        std::set<std::string> stopset;
        const bool have_stop = pick(4) != 0;
        if (have_stop) {
            if (pick(2)) stopset.insert("\xef\xbf\xbd");
            for (uint64_t k = 0; k < cap; k++) {
                const uint64_t s = start[k], e = end[k];
                if (s < e && e <= nbytes && e - s <= 255 && pick(3) == 0 && !(e - s == 1 && text[s] >= 0x80))
                    stopset.insert(std::string(text.begin() + s, text.begin() + e));
            }
        }
        std::vector<uint8_t> keys;
        std::vector<uint64_t> koff(1, 0);
        for (const auto& k : stopset) {
            keys.insert(keys.end(), k.begin(), k.end());
            koff.push_back(keys.size());
        }
        jb_vocab stop;
        std::string err;
        if (jb::vocab_build(keys.data(), koff.data(), (uint32_t)stopset.size(), &stop.v, &err) != 0) die(round, err.c_str());
        jb_filter_rule rule;
        rule.flags = have_stop && pick(3) ? JB_FILTER_STOP : 0u;
        rule.drop_classes = (uint32_t)pick(32);
        rule.min_runes = pick(3) ? (uint32_t)pick(4) : pick(2) ? 255u : (uint32_t)pick(256);
        rule.max_runes = pick(3) ? (uint32_t)pick(6) : pick(2) ? 255u : (uint32_t)pick(256);
        const uint64_t out_cap = pick(4) == 0 ? pick(cap + 1) : cap;
        const bool with_src = pick(3) != 0;
        auto p_text = exact(text);
        auto p_s = exact(start);
        auto p_e = exact(end);
        auto p_tok = exact(tok);
        std::unique_ptr<uint32_t[]> os(new uint32_t[out_cap]), oe(new uint32_t[out_cap]), osrc(new uint32_t[out_cap]);
        std::unique_ptr<uint64_t[]> odt(new uint64_t[ndocs + 1]), cnt(new uint64_t[1]), stats(new uint64_t[5]);
        if (jb_filter(p_text.get(), nbytes, p_s.get(), p_e.get(), p_tok.get(), ntok, cap, ndocs, &rule,
                      have_stop ? &stop : nullptr, os.get(), oe.get(), with_src ? osrc.get() : nullptr, out_cap, odt.get(),
                      cnt.get(), stats.get()) != JB_OK)
            die(round, "jb_filter failed");
        // the rule once more
        const uint64_t nt = std::min(ntok, cap);
        std::vector<uint64_t> R(nt + 1, 0);
        uint64_t why_n[5] = {0, 0, 0, 0, 0};
        for (uint64_t k = 0; k < nt; k++) {
            const uint64_t s = start[k], e = end[k];
            int why = 1;
            if (s < e && e <= nbytes) {
                const uint8_t* p = text.data() + s;
                const uint64_t len = e - s;
                uint32_t cls;
                auto alnum = [](uint8_t b) { return (b >= '0' && b <= '9') || (b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z'); };
                if (len == 1 && p[0] >= 0x80) cls = JB_TC_INVALID;
                else if (alnum(p[0])) {
                    cls = len <= 255 && std::all_of(p, p + len, [](uint8_t b) { return b >= '0' && b <= '9'; }) ? JB_TC_NUM
                                                                                                               : JB_TC_ALNUM;
                } else {
                    // (the alphabet's only lead bytes are E4, E7 and EF: a 3-byte rune of the BMP, or U+FFFD)
                    uint32_t r = 0xFFFD;
                    if (len >= 3 && (p[0] == 0xE4 || p[0] == 0xE7 || p[0] == 0xEF) && (p[1] & 0xC0) == 0x80 &&
                        (p[2] & 0xC0) == 0x80)
                        r = ((p[0] & 0x0Fu) << 12) | ((p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu);
                    const bool han = (r >= 0x3400 && r <= 0x4DBF) || (r >= 0x4E00 && r <= 0x9FFC) ||
                                     (r >= 0xF900 && r <= 0xFA6D) || (r >= 0xFA70 && r <= 0xFAD9);
                    cls = han ? JB_TC_HAN : JB_TC_OTHER;
                }
                uint64_t runes = 0;
                if (cls == JB_TC_INVALID) runes = 1;
                else if (len > 1024) runes = 256;
                else {
                    for (uint64_t i = 0; i < len; i++) runes += (p[i] & 0xC0) != 0x80;
                    runes = std::min<uint64_t>(runes, 256);
                }
                const std::string key = cls == JB_TC_INVALID ? std::string("\xef\xbf\xbd") : std::string(p, p + len);
                if (rule.drop_classes & cls) why = 2;
                else if (runes < rule.min_runes || (rule.max_runes && runes > rule.max_runes)) why = 3;
                else if ((rule.flags & JB_FILTER_STOP) && stopset.count(key)) why = 4;
                else why = 0;
            }
            if (why == 0 && R[k] < out_cap) {
                if (os[R[k]] != s || oe[R[k]] != e) die(round, "a kept span is wrong");
                if (with_src && osrc[R[k]] != k) die(round, "a source index is wrong");
            }
            why_n[why]++;
            R[k + 1] = R[k] + (why == 0);
        }
        if (cnt[0] != R[nt]) die(round, "the count is wrong");
        if (stats[0] != nt) die(round, "stats[0] is wrong");
        for (int q = 1; q < 5; q++)
            if (stats[q] != why_n[q]) die(round, "a reason count is wrong");
        for (uint32_t d = 0; d <= ndocs; d++)
            if (odt[d] != R[std::min(tok[d], nt)]) die(round, "a document offset is wrong");
    }
    // the limits
    uint64_t one[5] = {9, 9, 9, 9, 9}, c = 9;
    const uint64_t tok2[2] = {0, 0};
    uint64_t odt2[2] = {9, 9};
    jb_filter_rule r = {0, 0, 0, 0};
    if (jb_filter(nullptr, 0, nullptr, nullptr, tok2, 0, 0, 1, &r, nullptr, nullptr, nullptr, nullptr, 0, odt2, &c, one) != JB_OK ||
        c != 0 || odt2[0] != 0 || odt2[1] != 0 || one[0] != 0)
        die(-1, "empty input");
    r.flags = JB_FILTER_STOP;
    if (jb_filter(nullptr, 0, nullptr, nullptr, tok2, 0, 0, 1, &r, nullptr, nullptr, nullptr, nullptr, 0, odt2, &c, one) != JB_EINVAL)
        die(-1, "JB_FILTER_STOP without a set");
    r.flags = 0;
    r.min_runes = 256;
    if (jb_filter(nullptr, 0, nullptr, nullptr, tok2, 0, 0, 1, &r, nullptr, nullptr, nullptr, nullptr, 0, odt2, &c, one) != JB_ELIMIT)
        die(-1, "min_runes = 256");
    if (jb_filter_work_bytes(0, 0) == 0 || jb_filter_work_bytes(~0ull, 0) == 0) die(-1, "size helper");
    std::printf("ok\n");
    return 0;
}
