// The C++ mirror's MinHash (jieba-go_amd/host/tokenizer.hpp) against jb_minhash, the host form of the rule, fed
// the mirror's own Cut / CutForSearch / CutAll tokens laid out back to back (a signature depends on the tokens'
// bytes alone).  usage: cpp_minhash_smoke <mini_dict.txt> <prob_emit.json>.  Exits non-zero on a mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tokenizer.hpp"

using jiebago::Tokenizer;

static bool same(const Tokenizer::MinHashResult& got, const std::vector<std::vector<std::string>>& docs, uint32_t n,
                 uint32_t K, uint64_t seed) {
    std::string text;
    std::vector<uint32_t> s, e;
    std::vector<uint64_t> tok(1, 0);
    for (const auto& d : docs) {
        for (const auto& t : d) {
            s.push_back((uint32_t)text.size());
            text += t;
            e.push_back((uint32_t)text.size());
        }
        tok.push_back(s.size());
    }
    std::vector<uint32_t> sig(docs.size() * K + 1), dn(docs.size() + 1);
    if (jb_minhash((const uint8_t*)text.data(), text.size(), s.data(), e.data(), tok.data(), s.size(), s.size(),
                   (uint32_t)docs.size(), n, K, seed, sig.data(), dn.data()) != JB_OK)
        return false;
    sig.resize(docs.size() * K);
    dn.resize(docs.size());
    return got.sig == sig && got.docN == dn;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s mini_dict.txt prob_emit.json\n", argv[0]);
        return 2;
    }
    jb_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.dict_path = argv[1];
    cfg.dict_kind = JB_DICT_TXT;
    cfg.emit_path = argv[2];
    cfg.ndevices = 1;
    const std::vector<std::string> docs = {"abc \xFF这一刹那 abc", "", "今天天氣很好，2024 abc", "abc \xFF这一刹那 abc"};
    try {
        auto tk = Tokenizer::Open(cfg);
        for (int rep = 0; rep < 2; rep++) {
            for (bool hmm : {false, true}) {
                std::vector<std::vector<std::string>> c, s, f;
                for (const auto& d : docs) {
                    c.push_back(tk->Cut(d, hmm));
                    s.push_back(tk->CutForSearch(d, hmm));
                    f.push_back(tk->CutAll(d));
                }
                for (uint32_t n : {1u, 2u, 5u}) {
                    if (!same(tk->MinHash(docs, n, 64, 3, hmm), c, n, 64, 3)) return 1;
                    if (!same(tk->MinHash(docs, n, 128, 4, hmm, JB_MODE_SEARCH), s, n, 128, 4)) return 1;
                    if (!same(tk->MinHash(docs, n, 7, 5, hmm, JB_MODE_FULL), f, n, 7, 5)) return 1;
                }
            }
            auto r = tk->MinHash(docs);
            if (r.sig.size() != docs.size() * 128 || r.docN.size() != docs.size() || r.docN[1] != 0 || r.docN[0] < 1 ||
                r.docN[0] != r.docN[3])
                return 1;
            for (uint32_t j = 0; j < 128; j++)
                if (r.sig[j] != r.sig[3 * 128 + j] || r.sig[128 + j] != JB_MH_EMPTY) return 1;
        }
        auto none = tk->MinHash({});
        if (!none.sig.empty() || !none.docN.empty()) return 1;
        try {
            tk->MinHash(docs, 5, 128, 1, true, 7);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
        try {
            tk->MinHash(docs, 9);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_ELIMIT) return 1;
        }
        try {
            tk->MinHash(docs, 5, 0);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("minhash ok\n");
    return 0;
}
