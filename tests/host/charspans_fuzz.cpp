// jb_charspans (jieba-go_amd/csrc/jb_charspans.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer:
// seeded texts of valid runes, malformed sequences and leads cut short, documents cut at any byte (inside
// runes, empty ones in a row), spans that are ordered, reversed, past their document, before it or far
// outside, token counts on either side of the span arrays' length and doc_tok running past the count.  Every
// array is a heap block of exactly the length the call is told, so a read or write outside one is a report.
// Checked besides: every entry below min(ntok, cap) is written, a valid span gives cstart <= cend <=
// 2 * nbytes, nothing at or past that bound is written, the in-place call gives the same, and over the whole
// batch UTF-16 counts at least the runes and the runes at most the bytes.
// usage: charspans_fuzz <rounds> <seed>; prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
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
    static const char* const kPieces[] = {"a", " ", "\xc3\xa9", "\xe4\xb8\xad", "\xf0\xa0\x80\x80", "\xf0\x9f\x98\x80",
                                          "\xc3", "\xe4\xb8", "\xf0\xa0\x80", "\xc0\x80", "\xed\xa0\x80", "\xf4\x90\x80\x80",
                                          "\xf5\x80", "\xff", "\x80", "\xbf\xbf"};
    for (int round = 0; round < rounds; round++) {
        const uint64_t nbytes = pick(300);
        std::vector<uint8_t> text;
        const bool valid = pick(4) == 0;  // (the first six pieces only: valid UTF-8)
        while (text.size() < nbytes) {
            const char* p = kPieces[pick(valid ? 6 : 16)];
            const size_t len = std::strlen(p);
            if (text.size() + len > nbytes) {
                text.push_back('x');
                continue;
            }
            text.insert(text.end(), p, p + len);
        }
        const uint32_t ndocs = (uint32_t)pick(8);
        std::vector<uint64_t> doc_off(ndocs + 1, 0);
        for (uint32_t d = 1; d < ndocs; d++) doc_off[d] = pick(4) == 0 ? doc_off[d - 1] : pick(nbytes + 1);
        doc_off[ndocs] = ndocs ? nbytes : 0;
        std::sort(doc_off.begin(), doc_off.end());
        const uint64_t tb = ndocs ? nbytes : 0;  // (no document: no text)
        const uint64_t n = pick(200);
        std::vector<uint32_t> start(n), end(n);
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t s = pick(tb + 1);
            start[k] = (uint32_t)s;
            end[k] = (uint32_t)std::min<uint64_t>(s + pick(12), tb);
            const uint64_t kind = pick(20);
            if (kind == 0) std::swap(start[k], end[k]);
            if (kind == 1) end[k] = (uint32_t)(tb + 1 + pick(1000));
            if (kind == 2) start[k] = 0xFFFFFFF0u, end[k] = 0xFFFFFFFFu;
        }
        std::vector<uint64_t> doc_tok(ndocs + 1, 0);
        doc_tok[0] = pick(4) == 0 ? pick(3) : 0;
        for (uint32_t d = 1; d <= ndocs; d++) doc_tok[d] = doc_tok[d - 1] + (pick(3) == 0 ? 0 : pick(2 * n / ndocs + 2));
        uint64_t ntok = n, cap = n;
        const int kind = (int)pick(3);
        if (kind == 1) ntok = pick(2 * n + 2), cap = pick(n + 1);
        if (kind == 2) ntok = pick(n + 1);
        start.resize(cap);
        end.resize(cap);
        const uint64_t m = std::min(ntok, cap);
        auto p_text = exact(text);
        auto p_off = exact(doc_off);
        auto p_d = exact(doc_tok);
        uint64_t sum[2] = {0, 0};
        for (int unit = 0; unit < 2; unit++) {
            auto p_s = exact(start);
            auto p_e = exact(end);
            std::unique_ptr<uint32_t[]> cs(new uint32_t[cap]), ce(new uint32_t[cap]), un(new uint32_t[ndocs]);
            std::fill(cs.get(), cs.get() + cap, 0xFFFFFFFEu);
            std::fill(ce.get(), ce.get() + cap, 0xFFFFFFFEu);
            auto call = [&](uint32_t* o_s, uint32_t* o_e, uint32_t* o_u) {
                const int rc = jb_charspans(tb ? p_text.get() : nullptr, tb, p_off.get(), ndocs, cap ? p_s.get() : nullptr,
                                            cap ? p_e.get() : nullptr, p_d.get(), ntok, cap, unit, cap ? o_s : nullptr,
                                            cap ? o_e : nullptr, ndocs ? o_u : nullptr);
                if (rc != JB_OK) {
                    std::fprintf(stderr, "round %d: %s\n", round, jb_last_error());
                    std::exit(1);
                }
            };
            call(cs.get(), ce.get(), un.get());
            for (uint64_t k = 0; k < cap; k++) {
                const bool none = cs[k] == JB_CHAR_NONE;
                bool ok = k < m ? (none == (ce[k] == JB_CHAR_NONE) && cs[k] != 0xFFFFFFFEu && ce[k] != 0xFFFFFFFEu)
                                : (cs[k] == 0xFFFFFFFEu && ce[k] == 0xFFFFFFFEu);
                if (ok && k < m && !none) ok = cs[k] <= ce[k] && ce[k] <= 2 * tb;
                if (!ok) {
                    std::fprintf(stderr, "round %d unit %d: token %llu is (%u, %u)\n", round, unit, (unsigned long long)k,
                                 cs[k], ce[k]);
                    return 1;
                }
            }
            for (uint32_t d = 0; d < ndocs; d++) sum[unit] += un[d];
            // in place: the outputs are the span arrays themselves
            std::unique_ptr<uint32_t[]> un2(new uint32_t[ndocs]);
            call(p_s.get(), p_e.get(), un2.get());
            if (std::memcmp(un.get(), un2.get(), ndocs * 4) != 0 || std::memcmp(p_s.get(), cs.get(), m * 4) != 0 ||
                std::memcmp(p_e.get(), ce.get(), m * 4) != 0 ||
                !std::equal(start.begin() + m, start.end(), p_s.get() + m) || !std::equal(end.begin() + m, end.end(), p_e.get() + m)) {
                std::fprintf(stderr, "round %d unit %d: the in-place call differs\n", round, unit);
                return 1;
            }
        }
        if (sum[1] < sum[0] || sum[0] > tb) {
            std::fprintf(stderr, "round %d: %llu runes, %llu UTF-16 units in %llu bytes\n", round, (unsigned long long)sum[0],
                         (unsigned long long)sum[1], (unsigned long long)tb);
            return 1;
        }
    }
    std::printf("ok\n");
    return 0;
}
