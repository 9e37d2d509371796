// The word counts' host code (jieba-go_amd/csrc/jb_wc.cpp) and the code jb_wc.h shares between host and
// kernels (fingerprint, probe, key store, key compare) under AddressSanitizer + UndefinedBehaviorSanitizer.
// Each round draws a seeded span list with ordered, overlapping and malformed spans (start >= end, end past
// the text, start near 2^32), keys on either side of 24 and of 255 bytes, and token counts on either side of
// the span arrays' length; it runs jb_wc_count on it, then adds the same tokens one by one to a table in a
// heap block of exactly jb_wc_table_bytes bytes through the shared code (wc_host_add) and reads the block
// back (wc_read_host).  With room for every key the two results must be the same; with a table or a pool
// that is too small, or a fingerprint narrowed to a few bits, every count must be at most jb_wc_count's and
// the accounting must hold.  Every array is a heap block of exactly the length the call is told, so a read
// or write outside one is a report.
// usage: wc_fuzz <rounds> <seed>; prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "jb_wc.h"
#include "jiebahip.h"

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

static std::map<std::string, uint64_t> as_map(const jb_wc_result& r) {
    std::map<std::string, uint64_t> m;
    for (uint64_t i = 0; i < r.nkeys; i++)
        m[std::string((const char*)r.keys + r.key_off[i], (size_t)(r.key_off[i + 1] - r.key_off[i]))] = r.counts[i];
    return m;
}

static bool ordered(const jb_wc_result& r) {
    for (uint64_t i = 0; i + 1 < r.nkeys; i++) {
        const std::string a((const char*)r.keys + r.key_off[i], (size_t)(r.key_off[i + 1] - r.key_off[i]));
        const std::string b((const char*)r.keys + r.key_off[i + 1], (size_t)(r.key_off[i + 2] - r.key_off[i + 1]));
        if (r.counts[i] < r.counts[i + 1] || (r.counts[i] == r.counts[i + 1] && a.compare(b) >= 0)) return false;
    }
    return r.key_off[0] == 0;
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
        auto p_text = exact(text);
        auto p_s = exact(start);
        auto p_e = exact(end);
        const uint64_t min_count = pick(3), max_keys = pick(2) ? 0 : pick(6);
        jb_wc_result all, part;
        if (jb_wc_count(nbytes ? p_text.get() : nullptr, nbytes, cap ? p_s.get() : nullptr, cap ? p_e.get() : nullptr, ntok, cap,
                        1, 0, &all) != JB_OK ||
            jb_wc_count(nbytes ? p_text.get() : nullptr, nbytes, cap ? p_s.get() : nullptr, cap ? p_e.get() : nullptr, ntok, cap,
                        min_count, max_keys, &part) != JB_OK)
            die(round, "jb_wc_count failed");
        const uint64_t took = std::min(ntok, cap);
        uint64_t sum = 0;
        for (uint64_t i = 0; i < all.nkeys; i++) sum += all.counts[i];
        if (!ordered(all) || !ordered(part) || all.ntokens != took || sum + all.nbad + all.nlong != took || all.ndropped ||
            all.ncollided || part.nbad != all.nbad || part.nlong != all.nlong || part.ntokens != took)
            die(round, "jb_wc_count: order or accounting");
        {  // the filtered result is the head of the complete one
            uint64_t want = 0;
            while (want < all.nkeys && all.counts[want] >= min_count && (!max_keys || want < max_keys)) want++;
            if (part.nkeys != want || std::memcmp(part.counts, all.counts, want * 8) != 0 ||
                std::memcmp(part.key_off, all.key_off, (want + 1) * 8) != 0 ||
                std::memcmp(part.keys, all.keys, (size_t)all.key_off[want]) != 0)
                die(round, "jb_wc_count: the filters");
        }
        // the same tokens through the table's shared code, in a block of exactly the table's size
        const int shape = (int)pick(4);  // 0: room for all; 1: few slots; 2: a small pool; 3: a narrow fingerprint
        const uint64_t nslots = shape == 1 ? 8 : 1024, pool = shape == 2 ? pick(300) : 65536;
        const uint32_t bits = shape == 3 ? 1 + (uint32_t)pick(6) : 64;
        const size_t ntable = jb_wc_table_bytes(nslots, pool);
        if (jb::wc_sizes("wc_fuzz", nslots, pool) != JB_OK || ntable < jb_wc_bytes(nslots, pool)) die(round, "sizes");
        std::unique_ptr<uint64_t[]> block(new uint64_t[ntable / 8]);  // (8-byte aligned, ntable is a multiple of 8)
        std::memset(block.get(), 0, ntable);
        const JbWcView v = jb_wc_view(block.get(), nslots, pool);
        v.hdr->magic = JB_WC_MAGIC;
        v.hdr->nslots = nslots;
        v.hdr->pool_bytes = pool;
        for (uint64_t s = 0; s < nslots; s++) v.key[s * JB_VOCAB_SLOT_WORDS + 1] = JB_WC_NOREP;
        for (uint64_t k = 0; k < took; k++) {
            const uint64_t s = p_s[k], e = p_e[k];
            if (s >= e || e > nbytes) {
                v.hdr->ctr[JB_WC_TOKENS]++;
                v.hdr->ctr[JB_WC_BAD]++;
            } else if (e - s > JB_VOCAB_MAXKEY) {
                v.hdr->ctr[JB_WC_TOKENS]++;
                v.hdr->ctr[JB_WC_LONG]++;
            } else if (e - s == 1 && p_text[s] >= 0x80) {
                static const uint8_t kRepl[3] = {0xEF, 0xBF, 0xBD};
                std::unique_ptr<uint8_t[]> key(new uint8_t[3]);
                std::memcpy(key.get(), kRepl, 3);
                jb::wc_host_add(v, key.get(), 3, (uint32_t)k, bits);
            } else {
                std::unique_ptr<uint8_t[]> key(new uint8_t[e - s]);  // (a block of exactly the key's length)
                std::memcpy(key.get(), p_text.get() + s, e - s);
                jb::wc_host_add(v, key.get(), (uint32_t)(e - s), (uint32_t)k, bits);
                if (jb_wc_fp(key.get(), e - s, bits) == 0) die(round, "jb_wc_fp");
            }
        }
        jb_wc_result tab;
        std::memset(&tab, 0, sizeof tab);
        if (jb::wc_read_host(block.get(), ntable, 1, 0, &tab) != JB_OK) die(round, "wc_read_host failed");
        uint64_t tsum = 0;
        for (uint64_t i = 0; i < tab.nkeys; i++) tsum += tab.counts[i];
        if (!ordered(tab) || tab.ntokens != took || tab.nbad != all.nbad || tab.nlong != all.nlong ||
            tsum + tab.nbad + tab.nlong + tab.ndropped + tab.ncollided != took)
            die(round, "the table: order or accounting");
        const auto truth = as_map(all);
        for (const auto& kv : as_map(tab)) {
            const auto it = truth.find(kv.first);
            if (it == truth.end() || kv.second > it->second) die(round, "the table credits a key with tokens it does not have");
        }
        if (shape == 0 && (tab.ndropped || tab.ncollided || as_map(tab) != truth)) die(round, "the table differs from jb_wc_count");
        if (shape != 1 && shape != 2 && tab.ndropped) die(round, "dropped with room");
        if (shape != 3 && tab.ncollided) die(round, "a collision at 64 bits");
        // a reader of a block that holds no table, or less of it than its header says, refuses
        jb_wc_result none;
        std::memset(&none, 0, sizeof none);
        if (jb::wc_read_host(block.get(), ntable - 8, 1, 0, &none) != JB_EINVAL) die(round, "a short block was read");
        v.hdr->magic = 0;
        if (jb::wc_read_host(block.get(), ntable, 1, 0, &none) != JB_EINVAL) die(round, "a block without a table was read");
        jb_wc_result_free(&all);
        jb_wc_result_free(&part);
        jb_wc_result_free(&tab);
    }
    std::printf("ok\n");
    return 0;
}
