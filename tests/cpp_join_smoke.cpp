// The C++ mirror's CutJoin (jieba-go_amd/host/tokenizer.hpp) against strings written out by hand and against
// the mirror's own Cut / CutForSearch / CutAll joined on the host.
// usage: cpp_join_smoke <mini_dict.txt> <prob_emit.json>.  Exits non-zero on a mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tokenizer.hpp"

using jiebago::Tokenizer;

static std::string joined(const std::vector<std::string>& toks, const std::string& sep) {
    std::string s;
    for (size_t k = 0; k < toks.size(); k++) s += (k ? sep : "") + toks[k];
    return s;
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
    const std::vector<std::string> docs = {"abc \xFF这一刹那", "", "今天天氣很好，2024"};
    try {
        auto tk = Tokenizer::Open(cfg);
        for (int rep = 0; rep < 2; rep++) {
            auto got = tk->CutJoin(docs, " ", false);
            if (got.size() != 3 || got[0] != "abc \xEF\xBF\xBD 这 一刹那" || got[1] != "" || got[2] != "今天 天 氣 很 好 ， 2024") {
                std::fprintf(stderr, "CutJoin: %s / %s / %s\n", got[0].c_str(), got[1].c_str(), got[2].c_str());
                return 1;
            }
            got = tk->CutJoin(docs, "／", false, JB_MODE_SEARCH);
            if (got[0] != "abc／\xEF\xBF\xBD／这／一刹／刹那／一刹那") return 1;
            got = tk->CutJoin(docs, "", false, JB_MODE_FULL);
            if (got[0] != "abc\xEF\xBF\xBD这一刹一刹那刹那" || got[2] != "今天天天氣很好，2024") return 1;
            for (bool hmm : {false, true})
                for (size_t d = 0; d < docs.size(); d++) {
                    if (tk->CutJoin(docs, "<=>", hmm)[d] != joined(tk->Cut(docs[d], hmm), "<=>")) return 1;
                    if (tk->CutJoin(docs, "<=>", hmm, JB_MODE_SEARCH)[d] != joined(tk->CutForSearch(docs[d], hmm), "<=>")) return 1;
                    if (tk->CutJoin(docs, "<=>", hmm, JB_MODE_FULL)[d] != joined(tk->CutAll(docs[d]), "<=>")) return 1;
                }
        }
        if (!tk->CutJoin({}).empty()) return 1;
        try {
            tk->CutJoin(docs, "123456789");
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_ELIMIT) return 1;
        }
        try {
            tk->CutJoin(docs, " ", true, 7);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("join ok\n");
    return 0;
}
