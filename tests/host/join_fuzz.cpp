// jb_join (jieba-go_amd/csrc/jb_join.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: seeded span
// lists with ordered, overlapping and malformed spans (start >= end, end past the text), token counts on
// either side of the span arrays' length, doc_tok running past the count, empty documents, separators and
// terminators of 0 to 8 bytes, and output capacities around the complete size.  Every array is a heap block
// of exactly the length the call is told, so a read or write outside one is a report.  The offsets must be
// non-decreasing from 0 to nout, nout must not depend on out_cap, and a truncated output must be a prefix of
// the complete one.
// usage: join_fuzz <rounds> <seed>; prints "ok".
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
    for (int round = 0; round < rounds; round++) {
        const uint64_t nbytes = pick(300);
        std::vector<uint8_t> text(nbytes);
        for (auto& b : text) b = pick(6) == 0 ? (uint8_t)(0x80 + pick(128)) : (uint8_t)(0x20 + pick(95));
        const uint64_t n = pick(200);
        std::vector<uint32_t> start(n), end(n);
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t s = pick(nbytes + 1), len = pick(3) == 0 ? 1 : pick(40);
            start[k] = (uint32_t)s;
            end[k] = (uint32_t)std::min<uint64_t>(s + len, nbytes);
            const uint64_t kind = pick(20);
            if (kind == 0) end[k] = start[k];
            if (kind == 1) std::swap(start[k], end[k]);
            if (kind == 2) end[k] = (uint32_t)(nbytes + 1 + pick(1000));
            if (kind == 3) start[k] = 0xFFFFFFF0u, end[k] = 0xFFFFFFFFu;
        }
        const uint32_t ndocs = (uint32_t)pick(8);
        std::vector<uint64_t> doc_tok(ndocs + 1, 0);
        for (uint32_t d = 1; d <= ndocs; d++) doc_tok[d] = doc_tok[d - 1] + (pick(3) == 0 ? 0 : pick(2 * n / ndocs + 2));
        uint64_t ntok = n, cap = n;
        const int kind = (int)pick(3);
        if (kind == 1) ntok = pick(2 * n + 2), cap = pick(n + 1);
        if (kind == 2) ntok = pick(n + 1);
        start.resize(cap);
        end.resize(cap);
        const uint32_t seplen = (uint32_t)pick(9), termlen = (uint32_t)pick(9);
        std::vector<uint8_t> sep(seplen, '_'), term(termlen, '\n');
        auto p_text = exact(text);
        auto p_s = exact(start);
        auto p_e = exact(end);
        auto p_d = exact(doc_tok);
        auto p_sep = exact(sep);
        auto p_term = exact(term);
        auto call = [&](uint8_t* out, uint64_t out_cap, uint64_t* off, uint64_t* nout) {
            const int rc = jb_join(nbytes ? p_text.get() : nullptr, nbytes, cap ? p_s.get() : nullptr, cap ? p_e.get() : nullptr,
                                   p_d.get(), ntok, cap, ndocs, seplen ? p_sep.get() : nullptr, seplen,
                                   termlen ? p_term.get() : nullptr, termlen, out, out_cap, off, nout);
            if (rc != JB_OK) {
                std::fprintf(stderr, "round %d: %s\n", round, jb_last_error());
                std::exit(1);
            }
        };
        std::unique_ptr<uint64_t[]> off0(new uint64_t[ndocs + 1]), off1(new uint64_t[ndocs + 1]);
        uint64_t nout = 0;
        call(nullptr, 0, off0.get(), &nout);
        if (off0[0] != 0 || off0[ndocs] != nout || !std::is_sorted(off0.get(), off0.get() + ndocs + 1)) {
            std::fprintf(stderr, "round %d: offsets are not non-decreasing from 0 to nout\n", round);
            return 1;
        }
        std::unique_ptr<uint8_t[]> full(new uint8_t[nout ? nout : 1]);
        uint64_t n1 = 0;
        call(nout ? full.get() : nullptr, nout, off1.get(), &n1);
        const uint64_t caps[4] = {1, nout ? nout - 1 : 0, nout + 5, pick(nout + 1)};
        for (uint64_t oc : caps) {
            std::unique_ptr<uint8_t[]> part(new uint8_t[oc ? oc : 1]);
            std::memset(part.get(), 0x5A, oc ? oc : 1);
            uint64_t n2 = 0;
            call(oc ? part.get() : nullptr, oc, off1.get(), &n2);
            const uint64_t m = std::min(oc, nout);
            if (n1 != nout || n2 != nout || std::memcmp(off0.get(), off1.get(), (ndocs + 1) * 8) != 0 ||
                std::memcmp(part.get(), full.get(), m) != 0 ||
                std::any_of(part.get() + m, part.get() + oc, [](uint8_t b) { return b != 0x5A; })) {
                std::fprintf(stderr, "round %d: out_cap %llu changes the result\n", round, (unsigned long long)oc);
                return 1;
            }
        }
    }
    std::printf("ok\n");
    return 0;
}
