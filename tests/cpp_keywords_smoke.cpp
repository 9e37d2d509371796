// The C++ mirror's ExtractTags (jieba-go_amd/host/tokenizer.hpp) on hand-worked examples.
// usage: cpp_keywords_smoke <mini_dict.txt> <prob_emit.json>.  Exits non-zero on a mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tokenizer.hpp"

using jiebago::Tokenizer;
using Tag = jiebago::Tokenizer::Tag;

static bool same(const char* what, const std::vector<Tag>& got, const std::vector<Tag>& want) {
    bool ok = got.size() == want.size();
    for (size_t k = 0; ok && k < got.size(); k++)
        ok = got[k].id == want[k].id && got[k].score == want[k].score && got[k].count == want[k].count;
    if (ok) return true;
    std::fprintf(stderr, "%s:", what);
    for (const auto& t : got) std::fprintf(stderr, " (%u, %g, %u)", t.id, (double)t.score, t.count);
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
    // ids:                           abc   今天  U+FFFD 一刹那 刹那  这    天天
    const std::vector<float> weights = {1.0f, 1.5f, 0.5f, 2.0f, 1.0f, 0.0f, 1.0f};
    try {
        auto tk = Tokenizer::Open(cfg);
        try {  // no vocabulary yet
            tk->ExtractTags({"abc"}, weights);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
        tk->SetVocab({"abc", "今天", "\xEF\xBF\xBD", "一刹那", "刹那", "这", "天天"});
        for (int rep = 0; rep < 2; rep++) {
            // abc, U+FFFD, 今天, 天, 氣, 这, 一刹那 = ids 0 2 1 U U 5 3;   abc, abc, 今天 = ids 0 0 1;   nothing
            auto tags = tk->ExtractTags({"abc \xFF今天天氣 这一刹那", "abc abc 今天", ""}, weights, 3, false);
            if (tags.size() != 3) return 1;
            if (!same("document 0", tags[0], {{3, 2.0f, 1}, {1, 1.5f, 1}, {0, 1.0f, 1}})) return 1;
            if (!same("document 1", tags[1], {{0, 2.0f, 2}, {1, 1.5f, 1}})) return 1;
            if (!same("document 2", tags[2], {})) return 1;
        }
        if (!tk->ExtractTags({}, weights).empty()) return 1;
        try {
            tk->ExtractTags({"abc"}, weights, JB_KW_MAXK + 1);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_ELIMIT) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("keywords ok\n");
    return 0;
}
