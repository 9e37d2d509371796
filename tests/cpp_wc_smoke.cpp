// The C++ mirror's WordCounts (jieba-go_amd/host/tokenizer.hpp) against counts written out by hand and against
// the mirror's own Cut / CutForSearch / CutAll counted on the host, and a vocabulary fitted from it.
// usage: cpp_wc_smoke <mini_dict.txt> <prob_emit.json>.  Exits non-zero on a mismatch.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "tokenizer.hpp"

using jiebago::Tokenizer;
using WC = Tokenizer::WordCount;

static std::vector<WC> counted(const std::vector<std::vector<std::string>>& docs) {
    std::map<std::string, uint64_t> m;
    for (const auto& d : docs)
        for (const auto& t : d) m[t]++;
    std::vector<WC> v;
    for (const auto& kv : m) v.push_back({kv.first, kv.second});
    std::stable_sort(v.begin(), v.end(), [](const WC& a, const WC& b) { return a.count > b.count; });  // (the map is by bytes)
    return v;
}

static bool same(const std::vector<WC>& a, const std::vector<WC>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].word != b[i].word || a[i].count != b[i].count) return false;
    return true;
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
    const std::vector<std::string> docs = {"abc \xFF这一刹那 abc", "", "今天天氣很好，2024 abc"};
    try {
        auto tk = Tokenizer::Open(cfg);
        for (int rep = 0; rep < 2; rep++) {
            auto got = tk->WordCounts(docs, false);
            if (got.empty() || got[0].word != "abc" || got[0].count != 3) {
                std::fprintf(stderr, "WordCounts: %zu words\n", got.size());
                return 1;
            }
            for (bool hmm : {false, true}) {
                std::vector<std::vector<std::string>> c, s, f;
                for (const auto& d : docs) {
                    c.push_back(tk->Cut(d, hmm));
                    s.push_back(tk->CutForSearch(d, hmm));
                    f.push_back(tk->CutAll(d));
                }
                if (!same(tk->WordCounts(docs, hmm), counted(c))) return 1;
                if (!same(tk->WordCounts(docs, hmm, JB_MODE_SEARCH), counted(s))) return 1;
                if (!same(tk->WordCounts(docs, hmm, JB_MODE_FULL), counted(f))) return 1;
            }
            auto top = tk->WordCounts(docs, false, JB_MODE_CUT, 2, 1);
            if (top.size() != 1 || top[0].word != "abc") return 1;
        }
        if (!tk->WordCounts({}).empty()) return 1;
        // a fitted vocabulary knows every token of the text it was fitted on
        std::vector<std::string> keys;
        for (const auto& w : tk->WordCounts(docs, true)) keys.push_back(w.word);
        tk->SetVocab(keys);
        for (const auto& d : docs) {
            std::vector<uint32_t> ids;
            auto toks = tk->CutIds(d, true, &ids);
            for (size_t k = 0; k < toks.size(); k++)
                if (ids[k] == JB_ID_UNK || keys[ids[k]] != toks[k]) return 1;
        }
        try {
            tk->WordCounts(docs, false, JB_MODE_CUT, 1, 0, 8, 0);  // 4 words fit, the text has more
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_ELIMIT) return 1;
        }
        if (tk->WordCounts(docs, false, JB_MODE_CUT, 1, 0, 8, 0, false).empty()) return 1;
        try {
            tk->WordCounts(docs, true, 7);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
        try {
            tk->WordCounts(docs, true, JB_MODE_CUT, 1, 0, 1000);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("wc ok\n");
    return 0;
}
