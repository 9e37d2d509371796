// The C++ mirror's SetStopWords, CutFiltered and SetBatchFilter (jieba-go_amd/host/tokenizer.hpp) against a filter
// written out here over the mirror's own Cut / CutForSearch / CutAll tokens: no stop word, no token of one rune,
// no punctuation, no replaced byte.  usage: cpp_filter_smoke <mini_dict.txt> <prob_emit.json>.  Exits non-zero on
// a mismatch.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "tokenizer.hpp"

using jiebago::Tokenizer;

static size_t runes(const std::string& w) {
    size_t n = 0;
    for (unsigned char c : w) n += (c & 0xC0) != 0x80;
    return n;
}

// (every token of the documents below is ASCII alnum, Han, a replaced byte or punctuation)
static std::vector<std::string> keep(const std::vector<std::string>& toks, const std::set<std::string>& stop) {
    std::vector<std::string> out;
    for (const auto& w : toks) {
        const unsigned char c = (unsigned char)w[0];
        const bool alnum = (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z');
        const bool han = c >= 0xE4 && c <= 0xE9 && w.size() >= 3;
        if (w == "\xEF\xBF\xBD" || !(alnum || han)) continue;
        if (runes(w) < 2 || stop.count(w)) continue;
        out.push_back(w);
    }
    return out;
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
    const std::vector<std::string> docs = {"abc \xFF这一刹那 abc", "", "今天天氣很好，2024 abc 上海", "abc \xFF这一刹那 abc"};
    const std::vector<std::string> stops = {"上海", "abc", "一刹"};
    const std::set<std::string> stopset(stops.begin(), stops.end());
    const jb_filter_rule rule = {JB_FILTER_STOP, JB_TC_OTHER | JB_TC_INVALID, 2, 0};
    try {
        auto tk = Tokenizer::Open(cfg);
        try {  // JB_FILTER_STOP without a stop set
            tk->CutFiltered(docs, rule);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
        tk->SetStopWords(stops);
        for (int rep = 0; rep < 2; rep++) {
            for (bool hmm : {false, true}) {
                const auto c = tk->CutFiltered(docs, rule, hmm);
                const auto s = tk->CutFiltered(docs, rule, hmm, JB_MODE_SEARCH);
                const auto f = tk->CutFiltered(docs, rule, hmm, JB_MODE_FULL);
                if (c.size() != docs.size() || s.size() != docs.size() || f.size() != docs.size()) return 1;
                for (size_t d = 0; d < docs.size(); d++) {
                    if (c[d] != keep(tk->Cut(docs[d], hmm), stopset)) return 1;
                    if (s[d] != keep(tk->CutForSearch(docs[d], hmm), stopset)) return 1;
                    if (f[d] != keep(tk->CutAll(docs[d]), stopset)) return 1;
                }
                if (c[0].empty() || !c[1].empty() || c[0] != c[3]) return 1;
            }
        }
        // the default rule drops punctuation and replaced bytes only
        const auto def = tk->CutFiltered(docs);
        size_t nd = 0, nc = 0;
        for (const auto& d : def) nd += d.size();
        for (const auto& d : docs) nc += tk->Cut(d, true).size();
        if (nd == 0 || nd >= nc) return 1;
        // the batch filter and CutJoin
        const auto before = tk->CutJoin(docs, " ");
        tk->SetBatchFilter(rule);
        const auto joined = tk->CutJoin(docs, " ");
        for (size_t d = 0; d < docs.size(); d++) {
            std::string want;
            for (const auto& w : keep(tk->Cut(docs[d], true), stopset)) want += (want.empty() ? "" : " ") + w;
            if (joined[d] != want) return 1;
        }
        tk->ClearBatchFilter();
        if (tk->CutJoin(docs, " ") != before || before == joined) return 1;
        if (!tk->CutFiltered({}).empty()) return 1;
        try {
            tk->CutFiltered(docs, rule, true, 7);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
        try {
            tk->SetBatchFilter({0, 0, 256, 0});
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_ELIMIT) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("filter ok\n");
    return 0;
}
