// The C++ mirror's CutAll (jieba-go_amd/host/tokenizer.hpp) on a hand-worked example.
// usage: cpp_full_smoke <dict.txt> <prob_emit.json>, the dictionary being
//   甲 5 / 甲乙 5 / 甲乙丙 0 / 甲乙丙丁 5 / 乙 5 / 乙丙 5 / 丙 5 / 丁 5
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
        const std::vector<std::string> want = {"x", "甲乙", "甲乙丙丁", "乙丙", "丁", "戊", "丁", "y", "甲乙"};
        for (int rep = 0; rep < 2; rep++) {
            const std::vector<std::string> got = tk->CutAll("x甲乙丙丁戊丁y 甲乙");
            if (got != want) {
                std::fprintf(stderr, "CutAll:");
                for (const auto& t : got) std::fprintf(stderr, " %s", t.c_str());
                std::fprintf(stderr, "\n");
                return 1;
            }
            if (tk->CutAll("") != std::vector<std::string>{}) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("full ok\n");
    return 0;
}
