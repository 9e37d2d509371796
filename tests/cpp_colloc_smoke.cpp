// The C++ mirror's Collocations (jieba-go_amd/host/tokenizer.hpp) against pairs counted here over the mirror's
// own Tokenize (the cut drops the fullwidth comma, so not every adjacent pair touches), scored by jb_colloc_score,
// the host form of the rule.  usage: cpp_colloc_smoke <mini_dict.txt>
// <prob_emit.json>.  Exits non-zero on a mismatch.
#include <cstdio>
#include <cstring>
#include <map>
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
    const std::vector<std::string> docs = {"我昨天去上海交通大學", "今天天氣很好，我去上海", "", "我去上海，我去上海，我昨天去上海",
                                           "今天很好今天很好abc"};
    try {
        auto tk = Tokenizer::Open(cfg);
        // the vocabulary: the distinct words of the cut, by count
        std::vector<std::string> keys;
        for (const auto& w : tk->WordCounts(docs, false)) keys.push_back(w.word);
        tk->SetVocab(keys);
        std::map<std::string, uint32_t> id;
        for (uint32_t i = 0; i < keys.size(); i++) id[keys[i]] = i;
        // the rule by hand, over the tokens with their offsets: [0] every adjacent pair, [1] those that touch
        std::map<std::pair<uint32_t, uint32_t>, uint64_t> pairs[2];
        std::vector<uint64_t> uni(keys.size(), 0);
        uint64_t known = 0;
        for (const auto& toks : tk->Tokenize(docs, false)) {
            for (size_t k = 0; k < toks.size(); k++) {
                uni[id.at(toks[k].word)]++;
                known++;
                if (k + 1 == toks.size()) continue;
                const std::pair<uint32_t, uint32_t> key{id.at(toks[k].word), id.at(toks[k + 1].word)};
                pairs[0][key]++;
                if (toks[k].end == toks[k + 1].start) pairs[1][key]++;
            }
        }
        if (pairs[1].size() >= pairs[0].size() || pairs[1].size() < 3) return 1;
        const int scorers[3] = {JB_COLLOC_NPMI, JB_COLLOC_RATIO, JB_COLLOC_COUNT};
        for (int s = 0; s < 3; s++)
            for (int contiguous = 0; contiguous < 2; contiguous++) {
                std::vector<uint32_t> a, b;
                std::vector<uint64_t> c;
                for (const auto& kv : pairs[contiguous]) {
                    a.push_back(kv.first.first);
                    b.push_back(kv.first.second);
                    c.push_back(kv.second);
                }
                jb_colloc_result want;
                if (jb_colloc_score(a.data(), b.data(), c.data(), a.size(), uni.data(), (uint32_t)uni.size(), known, scorers[s],
                                    2, 0.0f, 0, &want) != JB_OK)
                    return 1;
                const auto got = tk->Collocations(docs, keys, scorers[s], 2, 0.0f, 0, contiguous != 0, {}, false, 1024);
                bool same = got.size() == want.n && want.n >= 3;
                for (uint64_t i = 0; same && i < want.n; i++)
                    same = got[i].a == keys[want.a[i]] && got[i].b == keys[want.b[i]] && got[i].count == want.count[i] &&
                           std::memcmp(&got[i].score, &want.score[i], 4) == 0;
                jb_colloc_result_free(&want);
                if (!same) {
                    std::fprintf(stderr, "scorer %d contiguous %d: the mirror's result differs from the host rule's\n", scorers[s],
                                 contiguous);
                    return 1;
                }
            }
        const auto top = tk->Collocations(docs, keys, JB_COLLOC_COUNT, 1, 0.0f, 1, false, {}, false, 1024);
        if (top.size() != 1 || top[0].a + top[0].b != "去上海" || top[0].count != 5) return 1;
        bool threw = false;
        try {
            tk->Collocations(docs, keys, JB_COLLOC_COUNT, 1, 0.0f, 0, false, {}, false, 8);  // (too small: pairs are dropped)
        } catch (const jiebago::Error&) {
            threw = true;
        }
        if (!threw) return 1;
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    std::printf("colloc ok\n");
    return 0;
}
