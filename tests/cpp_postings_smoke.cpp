// The C++ mirror's Postings (jieba-go_amd/host/tokenizer.hpp) against an index built here from the mirror's own
// CutIds: per id a list of (document, count) filled document by document.  Two batches with a running docBase
// must concatenate per id into the index of all documents.  usage: cpp_postings_smoke <mini_dict.txt>
// <prob_emit.json>.  Exits non-zero on a mismatch.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "tokenizer.hpp"

using jiebago::Tokenizer;

struct Ref {
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> lists;  // per id: (document, tf)
    std::vector<uint32_t> docLen;
};

static Ref build(Tokenizer& tk, const std::vector<std::string>& docs, size_t nkeys, bool hmm, uint32_t base) {
    Ref r;
    r.lists.resize(nkeys);
    for (size_t d = 0; d < docs.size(); d++) {
        std::vector<uint32_t> ids;
        const auto toks = tk.CutIds(docs[d], hmm, &ids);
        r.docLen.push_back((uint32_t)toks.size());
        std::map<uint32_t, uint32_t> cnt;
        for (uint32_t id : ids)
            if (id != JB_ID_UNK) cnt[id]++;
        for (const auto& kv : cnt) r.lists[kv.first].push_back({base + (uint32_t)d, kv.second});
    }
    return r;
}

static bool same(const Tokenizer::Index& ix, const Ref& r) {
    if (ix.off.size() != r.lists.size() + 1 || ix.off[0] != 0 || ix.docLen != r.docLen) return false;
    if (ix.doc.size() != ix.off.back() || ix.tf.size() != ix.off.back()) return false;
    for (size_t t = 0; t < r.lists.size(); t++) {
        if (ix.off[t + 1] - ix.off[t] != r.lists[t].size()) return false;
        for (size_t k = 0; k < r.lists[t].size(); k++)
            if (ix.doc[ix.off[t] + k] != r.lists[t][k].first || ix.tf[ix.off[t] + k] != r.lists[t][k].second) return false;
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
    const std::vector<std::string> a = {"abc abc 今天", "abc \xFF今天天氣 这一刹那", "这一刹那 今天", "", "刹那 abc"};
    const std::vector<std::string> b = {"今天 abc 今天 今天", "天天 上海"};
    const std::vector<std::string> keys = {"abc", "今天", "\xEF\xBF\xBD", "一刹那", "刹那", "这", "天天", "absent"};
    try {
        auto tk = Tokenizer::Open(cfg);
        try {  // no vocabulary
            tk->Postings(a);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
        tk->SetVocab(keys);
        for (int rep = 0; rep < 2; rep++) {
            for (bool hmm : {false, true}) {
                const auto ia = tk->Postings(a, hmm);
                const auto ib = tk->Postings(b, hmm, (uint32_t)a.size());
                if (!same(ia, build(*tk, a, keys.size(), hmm, 0))) return 1;
                if (!same(ib, build(*tk, b, keys.size(), hmm, (uint32_t)a.size()))) return 1;
                if (ia.doc.empty() || ia.off[1] - ia.off[0] != 3 || ia.off[8] != ia.off[7]) return 1;  // "abc", "absent"
                // both batches as one
                std::vector<std::string> ab(a);
                ab.insert(ab.end(), b.begin(), b.end());
                const auto iab = tk->Postings(ab, hmm);
                if (!same(iab, build(*tk, ab, keys.size(), hmm, 0))) return 1;
                for (size_t t = 0; t < keys.size(); t++) {
                    std::vector<uint32_t> doc(ia.doc.begin() + ia.off[t], ia.doc.begin() + ia.off[t + 1]);
                    doc.insert(doc.end(), ib.doc.begin() + ib.off[t], ib.doc.begin() + ib.off[t + 1]);
                    if (doc != std::vector<uint32_t>(iab.doc.begin() + iab.off[t], iab.doc.begin() + iab.off[t + 1])) return 1;
                }
            }
        }
        const auto none = tk->Postings({});
        if (none.off.size() != keys.size() + 1 || none.off.back() != 0 || !none.doc.empty()) return 1;
        try {  // document numbers past 2^32
            tk->Postings(a, true, 0xFFFFFFFFu);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_ELIMIT) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("postings ok\n");
    return 0;
}
