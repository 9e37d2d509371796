// The C++ mirror's SetVocab and CutIds (jieba-go_amd/host/tokenizer.hpp) on hand-worked examples.
// usage: cpp_ids_smoke <mini_dict.txt> <prob_emit.json>.  Exits non-zero on a mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tokenizer.hpp"

using jiebago::Tokenizer;

static bool same(const char* what, const std::vector<std::string>& toks, const std::vector<uint32_t>& ids,
                 const std::vector<std::string>& wt, const std::vector<uint32_t>& wi) {
    if (toks == wt && ids == wi) return true;
    std::fprintf(stderr, "%s:", what);
    for (size_t k = 0; k < toks.size(); k++) std::fprintf(stderr, " %s=%u", toks[k].c_str(), k < ids.size() ? ids[k] : 0u);
    std::fprintf(stderr, "\n");
    return false;
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
    const uint32_t U = JB_ID_UNK;
    try {
        auto tk = Tokenizer::Open(cfg);
        std::vector<uint32_t> ids;
        try {  // no vocabulary yet
            tk->CutIds("abc", false, &ids);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
        tk->SetVocab({"abc", "今天", "\xEF\xBF\xBD", "一刹那", "刹那", "这", "天天"});
        for (int rep = 0; rep < 2; rep++) {
            auto t = tk->CutIds("abc \xFF今天天氣 这一刹那", false, &ids);
            if (!same("cut", t, ids, {"abc", "\xEF\xBF\xBD", "今天", "天", "氣", "这", "一刹那"}, {0, 2, 1, U, U, 5, 3})) return 1;
            t = tk->CutIds("这一刹那", false, &ids, Tokenizer::Mode::Search);
            if (!same("search", t, ids, {"这", "一刹", "刹那", "一刹那"}, {5, U, 4, 3})) return 1;
            t = tk->CutIds("今天天氣这一刹那", false, &ids, Tokenizer::Mode::Full);
            if (!same("full", t, ids, {"今天", "天天", "氣", "这", "一刹", "一刹那", "刹那"}, {1, 6, U, 5, U, 3, 4})) return 1;
            t = tk->CutIds("", false, &ids);
            if (!t.empty() || !ids.empty()) return 1;
        }
        tk->SetVocab({});  // an empty vocabulary: everything is unknown
        auto t = tk->CutIds("abc", false, &ids);
        if (!same("empty", t, ids, {"abc"}, {U})) return 1;
        try {
            tk->SetVocab({"a", "a"});
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("ids ok\n");
    return 0;
}
