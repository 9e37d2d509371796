// The MinHash host code (jieba-go_amd/csrc/jb_minhash.cpp) and the code jb_minhash.h shares between host and
// kernels (hash family, shingle fold, slot, band key) under AddressSanitizer + UndefinedBehaviorSanitizer.
// Each round draws a seeded span list with ordered, overlapping and malformed spans (start >= end, end past
// the text, start near 2^32), keys on either side of 24 and of 255 bytes, token counts on either side of the
// span arrays' length, and a doc_tok that is sorted, or not, or reaches past the list; it runs jb_minhash,
// jb_minhash_params and jb_minhash_bands on it.  With a sorted doc_tok the result is compared with the rule
// restated here over the shared code; with a decreasing one only the memory matters.  Every array, the outputs
// included, is a heap block of exactly the length the call is told, so a read or write outside one is a report.
// usage: minhash_fuzz <rounds> <seed>; prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "jb_minhash.h"
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
        const uint64_t nbytes = pick(3) == 0 ? pick(40) : pick(1500);
        std::vector<uint8_t> text(nbytes);
        for (auto& b : text) b = pick(6) == 0 ? (uint8_t)(0x80 + pick(128)) : (uint8_t)(0x61 + pick(3));
        const uint64_t n = pick(300);
        std::vector<uint32_t> start(n), end(n);
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t s = pick(nbytes + 1);
            const uint64_t len = pick(3) == 0 ? 1 : pick(10) == 0 ? 20 + pick(12) : pick(40) == 0 ? 250 + pick(10) : pick(5);
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
        else if (ndocs) std::sort(tok.begin(), tok.end(), [](uint64_t a, uint64_t b) { return a > b; });
        if (pick(9) == 0 && ndocs) tok[ndocs] = ~0ull;
        const uint32_t nn = 1 + (uint32_t)pick(JB_MH_MAXN), K = pick(5) == 0 ? JB_MH_MAXK : 1 + (uint32_t)pick(JB_MH_MAXK);
        const uint64_t seed = rng();
        auto p_text = exact(text);
        auto p_s = exact(start);
        auto p_e = exact(end);
        auto p_tok = exact(tok);
        std::unique_ptr<uint32_t[]> sig(new uint32_t[(size_t)ndocs * K]), dn(new uint32_t[ndocs]);
        std::unique_ptr<uint64_t[]> a(new uint64_t[K]), b(new uint64_t[K]);
        if (jb_minhash(p_text.get(), nbytes, p_s.get(), p_e.get(), p_tok.get(), ntok, cap, ndocs, nn, K, seed, sig.get(),
                       dn.get()) != JB_OK)
            die(round, "jb_minhash failed");
        if (jb_minhash_params(seed, K, a.get(), b.get()) != JB_OK) die(round, "jb_minhash_params failed");
        const uint32_t R = 1 + (uint32_t)pick(K), B = 1 + (uint32_t)pick(K / R);
        std::unique_ptr<uint64_t[]> keys(new uint64_t[(size_t)ndocs * B]);
        if (jb_minhash_bands(sig.get(), dn.get(), ndocs, K, B, R, keys.get()) != JB_OK) die(round, "jb_minhash_bands failed");
        for (uint32_t d = 0; d < ndocs; d++)
            for (uint32_t band = 0; band < B; band++)
                if ((keys[(size_t)d * B + band] == JB_MH_NOKEY) != (dn[d] == 0)) die(round, "a band key is wrong");
        if (!sorted) continue;
        // the rule once more: token hashes, then every document's shingles
        const uint64_t nt = std::min(ntok, cap);
        std::vector<uint64_t> t(nt);
        for (uint64_t k = 0; k < nt; k++) {
            const uint64_t s = start[k], e = end[k];
            std::vector<uint8_t> key;
            if (s < e && e <= nbytes) {
                if (e - s == 1 && text[s] >= 0x80) key = {0xEF, 0xBF, 0xBD};
                else key.assign(text.begin() + s, text.begin() + std::min(e, s + JB_VOCAB_MAXKEY));
            }
            key.resize(key.size() + 8, 0);  // (zero padding for the word reads below)
            const uint32_t len = (uint32_t)key.size() - 8u;
            uint64_t h = jb_vocab_hash_init(len);
            for (uint32_t p = 0; p < std::max(len, 1u); p += 8) {
                uint64_t w = 0;
                for (uint32_t i = 0; i < 8 && p + i < len; i++) w |= (uint64_t)key[p + i] << (8 * i);
                h = jb_vocab_mix(h, w);
            }
            t[k] = jb_vocab_hash_fin(h);
        }
        for (uint32_t d = 0; d < ndocs; d++) {
            const uint64_t lo = std::min(tok[d], nt), hi = std::min(tok[d + 1], nt), m = hi - lo;
            const uint64_t cnt = m == 0 ? 0 : m < nn ? 1 : m - nn + 1, c = std::min<uint64_t>(m, nn);
            if (dn[d] != cnt) die(round, "a shingle count is wrong");
            for (uint32_t j = 0; j < K; j++) {
                uint32_t mn = JB_MH_EMPTY;
                for (uint64_t i = 0; i < cnt; i++) {
                    uint64_t g = jb_vocab_hash_init((uint32_t)c);
                    for (uint64_t q = 0; q < c; q++) g = jb_vocab_mix(g, t[lo + i + q]);
                    const uint32_t x = (uint32_t)jb_vocab_hash_fin(g);
                    mn = std::min(mn, (uint32_t)((a[j] * (uint64_t)x + b[j]) >> 32));
                }
                if (sig[(size_t)d * K + j] != mn) die(round, "a slot is wrong");
            }
        }
    }
    // the limits
    uint32_t one = 0;
    const uint64_t tok2[2] = {0, 0};
    if (jb_minhash(nullptr, 0, nullptr, nullptr, tok2, 0, 0, 1, 1, 1, 1, &one, &one) != JB_OK || one != 0) die(-1, "empty input");
    if (jb_minhash(nullptr, 0, nullptr, nullptr, tok2, 0, 0, 1, 0, 1, 1, &one, &one) != JB_EINVAL) die(-1, "n = 0");
    if (jb_minhash(nullptr, 0, nullptr, nullptr, tok2, 0, 0, 1, 9, 1, 1, &one, &one) != JB_ELIMIT) die(-1, "n = 9");
    if (jb_minhash(nullptr, 0, nullptr, nullptr, tok2, 0, 0, 1, 1, 257, 1, &one, &one) != JB_ELIMIT) die(-1, "K = 257");
    if (jb_minhash_work_bytes(0, 0) == 0 || jb_minhash_work_bytes(~0ull, 0) == 0) die(-1, "size helper");
    std::printf("ok\n");
    return 0;
}
