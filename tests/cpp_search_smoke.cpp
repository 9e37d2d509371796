// The C++ mirror's CutForSearch (jieba-go_amd/host/tokenizer.hpp) on a hand-checked example.
// usage: cpp_search_smoke <dict.txt> <prob_emit.json>, the dictionary being
//   甲 10 / 甲乙 20 / 甲乙丙 30 / 甲乙丙丁 40 / 乙 0 / 乙丙 50 / 丙 5 / 丙丁 60 / 丁 7
// Exits non-zero on a mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tokenizer.hpp"

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s dict.txt prob_emit.json\n", argv[0]);
        return 2;
    }
    jb_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.dict_path = argv[1];
    cfg.dict_kind = JB_DICT_TXT;
    cfg.emit_path = argv[2];
    cfg.ndevices = 1;
    try {
        auto tk = jiebago::Tokenizer::Open(cfg);
        const std::vector<std::string> want = {"x", "甲乙", "丙丁", "甲乙丙", "甲乙丙丁", "y", "甲乙", "丙丁",
                                               "甲乙丙", "甲乙丙丁", "丁"};
        for (bool hmm : {false, true}) {
            const std::vector<std::string> got = tk->CutForSearch("x甲乙丙丁y 甲乙丙丁丁", hmm);
            if (got != want) {
                std::fprintf(stderr, "CutForSearch(hmm=%d):", (int)hmm);
                for (const auto& t : got) std::fprintf(stderr, " %s", t.c_str());
                std::fprintf(stderr, "\n");
                return 1;
            }
            if (tk->CutForSearch("", hmm) != std::vector<std::string>{}) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("search ok\n");
    return 0;
}
