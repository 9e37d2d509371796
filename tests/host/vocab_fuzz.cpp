// vocab_fuzz — jieba-go_amd/csrc/jb_vocab.cpp under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_vocab_sanitize.py builds and runs it): seeded builds and lookups against a std::map,
// then malformed inputs: key_off arrays that decrease, start past 0 or hold empty and oversized
// keys, duplicates, zero-length inputs and null arrays.  Prints "ok" and exits 0.
//   vocab_fuzz <rounds> <seed>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <random>
#include <string>
#include <vector>

#include "jb_vocab.h"
#include "jiebahip.h"

using namespace jb;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static std::string rand_key(std::mt19937_64& g, uint32_t maxlen, uint32_t alphabet) {
    // (exact-size heap copies below, so that a read past a key's end is a report)
    const uint32_t len = 1u + (uint32_t)(g() % maxlen);
    std::string k(len, '\0');
    for (auto& c : k) c = (char)(alphabet == 256u ? g() & 255u : 'a' + g() % alphabet);
    return k;
}

static uint32_t lookup_exact(const Vocab& v, const std::string& t) {
    std::vector<uint8_t> copy(t.begin(), t.end());  // no byte past the token is readable
    return vocab_lookup(v, copy.data(), copy.size());
}

static int build(const std::vector<std::string>& keys, Vocab* v, std::string* err) {
    std::vector<uint8_t> buf;
    std::vector<uint64_t> off{0};
    for (const auto& k : keys) {
        buf.insert(buf.end(), k.begin(), k.end());
        off.push_back(buf.size());
    }
    return vocab_build(buf.data(), off.data(), (uint32_t)keys.size(), v, err);
}

static void round_ok(std::mt19937_64& g) {
    // small alphabets and short keys give shared prefixes, near misses and long probe chains
    const uint32_t alphabet = (g() & 1u) ? 256u : 2u + (uint32_t)(g() % 3u);
    const uint32_t maxlen = (g() & 1u) ? 255u : 1u + (uint32_t)(g() % 40u);
    const uint32_t want = (uint32_t)(g() % 3000u);
    std::map<std::string, uint32_t> ref;
    std::vector<std::string> keys;
    for (uint32_t i = 0; i < want; i++) {
        std::string k = rand_key(g, maxlen, alphabet);
        if (ref.emplace(k, (uint32_t)keys.size()).second) keys.push_back(k);
    }
    Vocab v;
    std::string err;
    CHECK(build(keys, &v, &err) == JB_OK);
    CHECK(v.nkeys == keys.size() && v.nslots >= 2ull * keys.size() && (v.nslots & (v.nslots - 1u)) == 0);
    uint32_t ml = 0;
    for (const auto& k : keys) ml = std::max<uint32_t>(ml, (uint32_t)k.size());
    CHECK(v.maxlen == ml);
    for (uint32_t i = 0; i < keys.size(); i++) CHECK(lookup_exact(v, keys[i]) == i);
    for (uint32_t i = 0; i < 2000u; i++) {
        std::string t = keys.empty() || (g() & 3u) == 0 ? rand_key(g, maxlen + 20u, alphabet) : keys[g() % keys.size()];
        switch (g() % 4u) {
        case 0: t.back() = (char)(t.back() + 1); break;
        case 1: t.erase(g() % t.size(), 1); break;
        case 2: t.push_back((char)(g() & 255u)); break;
        default: break;
        }
        auto it = ref.find(t);
        CHECK(lookup_exact(v, t) == (it == ref.end() ? JB_VOCAB_UNK : it->second));
    }
    CHECK(vocab_lookup(v, nullptr, 0) == JB_VOCAB_UNK);
    const std::string big(300, 'x');
    CHECK(lookup_exact(v, big) == JB_VOCAB_UNK);
    // the same key twice: an error that names both
    if (!keys.empty()) {
        std::vector<std::string> dup = keys;
        const uint32_t a = (uint32_t)(g() % keys.size());
        dup.push_back(keys[a]);
        Vocab w;
        CHECK(build(dup, &w, &err) == JB_EINVAL);
        CHECK(err.find(std::to_string(a)) != std::string::npos &&
              err.find(std::to_string(keys.size())) != std::string::npos);
    }
}

static void round_malformed(std::mt19937_64& g) {
    const uint32_t n = 1u + (uint32_t)(g() % 50u);
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t i = 1; i <= n; i++) off[i] = off[i - 1] + 1u + g() % 30u;
    std::vector<uint8_t> buf(off[n]);
    for (uint32_t i = 0; i < n; i++) {  // distinct keys: their first bytes hold the index
        for (uint64_t p = off[i]; p < off[i + 1]; p++) buf[p] = (uint8_t)g();
        buf[off[i]] = (uint8_t)i;
    }
    Vocab v;
    std::string err;
    const uint32_t i = 1u + (uint32_t)(g() % n);  // in 1..n
    std::vector<uint64_t> bad = off;
    int want = JB_EINVAL;
    switch (g() % 5u) {
    case 0: bad[0] = 1; break;            // does not start at 0
    case 1: bad[i] = bad[i - 1]; break;   // an empty key
    case 2:                               // decreasing (key 0 cannot end before 0: it does not start there)
        if (i == 1) bad[0] = 1;
        else bad[i] = bad[i - 1] - 1u;
        break;
    case 3:  // a key over 255 bytes (no key byte is read: the lengths are checked first)
        for (uint32_t k = i; k <= n; k++) bad[k] += 300u;
        want = JB_ELIMIT;
        break;
    default:  // an offset far past the buffer
        bad[i] = ~0ull - (g() % 4u);
        want = JB_ELIMIT;
        break;
    }
    CHECK(vocab_build(buf.data(), bad.data(), n, &v, &err) == want);
    CHECK(!err.empty());
    CHECK(v.nkeys == 0 && v.slots.empty());  // nothing was written on failure
    CHECK(vocab_build(buf.data(), off.data(), n, &v, &err) == JB_OK && v.nkeys == n);  // the intact arrays build
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 100;
    std::mt19937_64 g(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    // zero-length inputs and null arrays
    Vocab v;
    std::string err;
    CHECK(vocab_build(nullptr, nullptr, 0, &v, &err) == JB_OK && v.nkeys == 0 && v.maxlen == 0);
    CHECK(vocab_lookup(v, (const uint8_t*)"a", 1) == JB_VOCAB_UNK && vocab_lookup(v, nullptr, 0) == JB_VOCAB_UNK);
    const uint64_t zero = 0;
    CHECK(vocab_build((const uint8_t*)"", &zero, 0, &v, &err) == JB_OK && v.nkeys == 0);
    CHECK(vocab_build(nullptr, nullptr, 2, &v, &err) == JB_EINVAL);
    CHECK(vocab_build((const uint8_t*)"ab", nullptr, 2, &v, &err) == JB_EINVAL);
    CHECK(vocab_build((const uint8_t*)"ab", &zero, 0, nullptr, &err) == JB_EINVAL);
    CHECK(vocab_build(nullptr, nullptr, 0, &v, nullptr) == JB_OK);  // no message wanted
    const uint64_t empty_key[2] = {0, 0};
    CHECK(vocab_build((const uint8_t*)"", empty_key, 1, &v, nullptr) == JB_EINVAL);
    for (int r = 0; r < rounds; r++) {
        round_ok(g);
        for (int k = 0; k < 20; k++) round_malformed(g);
    }
    puts("ok");
    return 0;
}
