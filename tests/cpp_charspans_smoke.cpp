// The C++ mirror's Tokenize (jieba-go_amd/host/tokenizer.hpp) against offsets written out by hand and against
// the mirror's own Cut / CutForSearch / CutAll.
// usage: cpp_charspans_smoke <mini_dict.txt> <prob_emit.json>.  Exits non-zero on a mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tokenizer.hpp"

using jiebago::Tokenizer;

static bool same(const std::vector<Tokenizer::Token>& got, const std::vector<std::string>& words,
                 const std::vector<uint32_t>& bounds) {
    if (got.size() != words.size() || (!bounds.empty() && bounds.size() != 2 * words.size())) return false;
    for (size_t k = 0; k < got.size(); k++) {
        if (got[k].word != words[k]) return false;
        if (!bounds.empty() && (got[k].start != bounds[2 * k] || got[k].end != bounds[2 * k + 1])) return false;
    }
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
    // (U+20000 and the emoji are one rune and two UTF-16 units each; \xFF is an invalid byte, one of either;
    // the emoji is a token because its block has an alnum byte)
    const std::vector<std::string> docs = {"abc \xFF这一刹那", "", "\xF0\xA0\x80\x80今天a\xF0\x9F\x98\x80天氣"};
    try {
        auto tk = Tokenizer::Open(cfg);
        for (int rep = 0; rep < 2; rep++) {
            auto got = tk->Tokenize(docs, false);
            if (got.size() != 3 || !got[1].empty()) return 1;
            if (!same(got[0], {"abc", "\xEF\xBF\xBD", "这", "一刹那"}, {0, 3, 4, 5, 5, 6, 6, 9})) return 1;
            if (!same(got[2], {"\xF0\xA0\x80\x80", "今天", "a", "\xF0\x9F\x98\x80", "天", "氣"},
                      {0, 1, 1, 3, 3, 4, 4, 5, 5, 6, 6, 7}))
                return 1;
            got = tk->Tokenize(docs, false, JB_MODE_CUT, JB_UNIT_UTF16);
            if (!same(got[0], {"abc", "\xEF\xBF\xBD", "这", "一刹那"}, {0, 3, 4, 5, 5, 6, 6, 9})) return 1;
            if (!same(got[2], {"\xF0\xA0\x80\x80", "今天", "a", "\xF0\x9F\x98\x80", "天", "氣"},
                      {0, 2, 2, 4, 4, 5, 5, 7, 7, 8, 8, 9}))
                return 1;
            got = tk->Tokenize(docs, false, JB_MODE_SEARCH);
            if (!same(got[0], {"abc", "\xEF\xBF\xBD", "这", "一刹", "刹那", "一刹那"}, {0, 3, 4, 5, 5, 6, 6, 8, 7, 9, 6, 9})) return 1;
            for (bool hmm : {false, true})
                for (int unit : {JB_UNIT_RUNE, JB_UNIT_UTF16})
                    for (size_t d = 0; d < docs.size(); d++) {
                        if (!same(tk->Tokenize(docs, hmm, JB_MODE_CUT, unit)[d], tk->Cut(docs[d], hmm), {})) return 1;
                        if (!same(tk->Tokenize(docs, hmm, JB_MODE_SEARCH, unit)[d], tk->CutForSearch(docs[d], hmm), {})) return 1;
                        if (!same(tk->Tokenize(docs, hmm, JB_MODE_FULL, unit)[d], tk->CutAll(docs[d]), {})) return 1;
                    }
        }
        if (!tk->Tokenize({}).empty()) return 1;
        for (int bad = 0; bad < 2; bad++) {
            try {
                tk->Tokenize(docs, true, bad ? JB_MODE_CUT : 7, bad ? 2 : JB_UNIT_RUNE);
                return 1;
            } catch (const jiebago::Error& e) {
                if (e.code != JB_EINVAL) return 1;
            }
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("charspans ok\n");
    return 0;
}
