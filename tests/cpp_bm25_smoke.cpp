// The C++ mirror's SetIndex and Search (jieba-go_amd/host/tokenizer.hpp) against the C ABI's host rule:
// Postings' index of a few documents is attached, queries are searched, and the hits must be those of
// jb_bm25_search over jb_bm25_norms, jb_bm25_idf and the mirror's own CutIds of each query.
// usage: cpp_bm25_smoke <mini_dict.txt> <prob_emit.json>.  Exits non-zero on a mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tokenizer.hpp"

using jiebago::Tokenizer;

static bool check(Tokenizer& tk, const Tokenizer::Index& ix, const std::vector<std::string>& queries, uint32_t topK,
                  double k1, double b, bool hmm) {
    const uint32_t nids = (uint32_t)(ix.off.size() - 1), ndocs = (uint32_t)ix.docLen.size();
    double avgdl = 0;
    if (jb_bm25_avgdl(ix.docLen.data(), ndocs, &avgdl) != JB_OK) return false;
    std::vector<float> norm(ndocs), weight(nids);
    if (jb_bm25_norms(ix.docLen.data(), ndocs, k1, b, avgdl, norm.data()) != JB_OK) return false;
    if (jb_bm25_idf(ix.off.data(), nids, ndocs, weight.data()) != JB_OK) return false;
    std::vector<uint32_t> qid;
    std::vector<uint64_t> qoff(1, 0);
    for (const auto& q : queries) {
        std::vector<uint32_t> ids;
        if (!q.empty()) tk.CutIds(q, hmm, &ids);
        qid.insert(qid.end(), ids.begin(), ids.end());
        qoff.push_back(qid.size());
    }
    const uint32_t nq = (uint32_t)queries.size();
    std::vector<uint32_t> rd((size_t)nq * topK + 1), rn(nq + 1);
    std::vector<uint64_t> rs((size_t)nq * topK + 1);
    qid.push_back(0);  // (never an empty array: its address is passed)
    if (jb_bm25_search(ix.doc.data(), ix.tf.data(), ix.off.data(), ix.doc.size(), nids, norm.data(), ndocs, weight.data(),
                       nids, k1, qid.data(), qid.size() - 1, qoff.data(), nq, topK, rd.data(), rs.data(), rn.data()) != JB_OK)
        return false;
    const auto hits = tk.Search(queries, topK, hmm);
    if (hits.size() != nq) return false;
    for (uint32_t q = 0; q < nq; q++) {
        if (hits[q].size() != rn[q]) return false;
        for (uint32_t r = 0; r < rn[q]; r++)
            if (hits[q][r].doc != rd[(size_t)q * topK + r] || hits[q][r].score != rs[(size_t)q * topK + r] ||
                !(hits[q][r].Score() > 0.0))
                return false;
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
    const std::vector<std::string> docs = {"abc abc 今天", "abc \xFF今天天氣 这一刹那", "这一刹那 今天", "", "刹那 abc",
                                           "今天 abc 今天 今天", "天天 上海"};
    const std::vector<std::string> keys = {"abc", "今天", "\xEF\xBF\xBD", "一刹那", "刹那", "这", "天天", "absent"};
    const std::vector<std::string> queries = {"abc", "今天 abc", "", "absent", "一刹那 天天 刹那", "zzz", "abc abc abc"};
    try {
        auto tk = Tokenizer::Open(cfg);
        tk->SetVocab(keys);
        try {  // no index
            tk->Search(queries);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
        const auto ix = tk->Postings(docs);
        for (int rep = 0; rep < 2; rep++) {
            tk->SetIndex(ix);
            for (uint32_t topK : {1u, 3u, 64u})
                if (!check(*tk, ix, queries, topK, 1.2, 0.75, true)) return 1;
            tk->SetIndex(ix, 0.0, 1.0);
            if (!check(*tk, ix, queries, 5, 0.0, 1.0, false)) return 1;
        }
        tk->SetIndex(ix);
        const auto hits = tk->Search({"abc"}, 10);
        if (hits.size() != 1 || hits[0].size() != 4) return 1;  // documents 0, 1, 4 and 5 hold "abc"
        if (!tk->Search({}, 3).empty()) return 1;
        try {
            tk->Search(queries, JB_KW_MAXK + 1);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_ELIMIT) return 1;
        }
        try {
            tk->SetIndex(ix, 65.0, 0.5);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
        tk->ClearIndex();
        try {
            tk->Search(queries);
            return 1;
        } catch (const jiebago::Error& e) {
            if (e.code != JB_EINVAL) return 1;
        }
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("bm25 ok\n");
    return 0;
}
