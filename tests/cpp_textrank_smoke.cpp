// The C++ mirror's TextRank (jieba-go_amd/host/tokenizer.hpp) against jb_textrank, the host form of the
// rule, on ids worked out by hand.
// usage: cpp_textrank_smoke <mini_dict.txt> <prob_emit.json>.  Exits non-zero on a mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tokenizer.hpp"

using jiebago::Tokenizer;
using Rank = jiebago::Tokenizer::Rank;

static bool same(const char* what, const std::vector<Rank>& got, const uint32_t* id, const float* score, uint32_t n) {
    bool ok = got.size() == n;
    for (size_t k = 0; ok && k < got.size(); k++) ok = got[k].id == id[k] && std::memcmp(&got[k].score, &score[k], 4) == 0;
    if (ok) return true;
    std::fprintf(stderr, "%s:", what);
    for (const auto& t : got) std::fprintf(stderr, " (%u, %g)", t.id, (double)t.score);
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
    // ids:                           abc 今天 U+FFFD 一刹那 刹那 这 天天
    const std::vector<uint8_t> keep = {1, 1, 1, 1, 1, 0, 1};
    // abc, U+FFFD, 今天, 天, 氣, 这, 一刹那 = ids 0 2 1 U U 5 3;   abc, abc, 今天 = ids 0 0 1;   nothing
    const uint32_t U = JB_ID_UNK;
    const uint32_t ids[] = {0, 2, 1, U, U, 5, 3, 0, 0, 1}, term_id[] = {0, 1, 2, 3, 5, 0, 1};
    const uint64_t doc_tok[] = {0, 7, 10, 10}, term_off[] = {0, 5, 7, 7};
    uint32_t hid[9], hn[3];
    float hsc[9];
    if (jb_textrank(ids, 10, doc_tok, 10, 3, term_id, term_off, 7, keep.data(), 7, 4, 6, 3, hid, hsc, hn) != JB_OK) return 1;
    if (hn[0] != 3 || hn[1] != 2 || hn[2] != 0) return 1;
    try {
        auto tk = Tokenizer::Open(cfg);
        try {  // no vocabulary yet
            tk->TextRank({"abc"}, keep);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
        tk->SetVocab({"abc", "今天", "\xEF\xBF\xBD", "一刹那", "刹那", "这", "天天"});
        for (int rep = 0; rep < 2; rep++) {
            auto ranks = tk->TextRank({"abc \xFF今天天氣 这一刹那", "abc abc 今天", ""}, keep, 3, 4, 6, false);
            if (ranks.size() != 3) return 1;
            if (!same("document 0", ranks[0], hid, hsc, hn[0])) return 1;
            if (!same("document 1", ranks[1], hid + 3, hsc + 3, hn[1])) return 1;
            if (!same("document 2", ranks[2], hid + 6, hsc + 6, hn[2])) return 1;
        }
        if (!tk->TextRank({}, keep).empty()) return 1;
        try {
            tk->TextRank({"abc"}, keep, JB_KW_MAXK + 1);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_ELIMIT) return 1;
        }
        try {
            tk->TextRank({"abc"}, keep, 20, 1);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("textrank ok\n");
    return 0;
}
