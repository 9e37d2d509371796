// The C++ mirror's FitIdf (jieba-go_amd/host/tokenizer.hpp) on a hand-worked example, and ExtractTags with
// the fitted weights.  usage: cpp_df_smoke <mini_dict.txt> <prob_emit.json>.  Exits non-zero on a mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tokenizer.hpp"

using jiebago::Tokenizer;

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
    // the documents of tests/c_abi_df.c, hmm off:
    //   abc, abc, 今天 | abc, U+FFFD, 今天, 天, 氣, 这, 一刹那 | 这, 一刹那, 今天 | nothing | 刹那, abc
    const std::vector<std::vector<std::string>> batches = {
        {"abc abc 今天", "abc \xFF今天天氣 这一刹那"}, {}, {"这一刹那 今天", "", "刹那 abc"}};
    // ids:                          abc 今天 U+FFFD 一刹那 刹那 这 天天
    const std::vector<uint32_t> want = {3, 3, 1, 2, 1, 2, 0};
    try {
        auto tk = Tokenizer::Open(cfg);
        try {  // no vocabulary yet
            tk->FitIdf(batches);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
        tk->SetVocab({"abc", "今天", "\xEF\xBF\xBD", "一刹那", "刹那", "这", "天天"});
        for (int rep = 0; rep < 2; rep++) {  // twice: a fit starts from zero
            const auto fit = tk->FitIdf(batches, false);
            if (fit.ndocs != 5 || fit.df != want) {
                std::fprintf(stderr, "ndocs %llu, df:", (unsigned long long)fit.ndocs);
                for (uint32_t f : fit.df) std::fprintf(stderr, " %u", f);
                std::fprintf(stderr, "\n");
                return 1;
            }
            std::vector<float> w(want.size(), -1.0f);
            if (jb_idf(want.data(), (uint32_t)want.size(), 5, 1, JB_DF_NOMAX, nullptr, w.data()) != JB_OK) return 1;
            if (std::memcmp(w.data(), fit.weights.data(), w.size() * sizeof(float)) != 0 || w[6] != 0.0f || !(w[2] > w[0]) ||
                w[0] <= 1.0f) {
                std::fprintf(stderr, "the weights are not jb_idf's\n");
                return 1;
            }
            // the rarest known term of the second document leads it: U+FFFD (df 1)
            const auto tags = tk->ExtractTags({"abc \xFF今天天氣 这一刹那"}, fit.weights, 2, false);
            if (tags.size() != 1 || tags[0].size() != 2 || tags[0][0].id != 2 || tags[0][0].score != w[2] ||
                tags[0][0].count != 1)
                return 1;
            // filters: minDf 2 and the keep bytes leave 今天 (kept, df 3) and 这 (kept, df 2)
            const auto cut = tk->FitIdf(batches, false, 2, JB_DF_NOMAX, {0, 1, 1, 0, 1, 1, 1});
            for (size_t i = 0; i < want.size(); i++)
                if ((cut.weights[i] != 0.0f) != (i == 1 || i == 5) || (cut.weights[i] != 0.0f && cut.weights[i] != w[i]))
                    return 1;
        }
        try {
            tk->FitIdf(batches, false, 1, JB_DF_NOMAX, {1, 1});
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("df ok\n");
    return 0;
}
