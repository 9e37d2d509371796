// The C++ mirror's NearDuplicates (jieba-go_amd/host/tokenizer.hpp) against the host rule run here on the
// mirror's own MinHash signatures: jb_minhash_bands -> jb_neardup -> jb_neardup_labels.  Exact copies must share
// a label and agree in all K slots.  usage: cpp_neardup_smoke <mini_dict.txt> <prob_emit.json>.  Exits non-zero
// on a mismatch.
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
    std::vector<std::string> docs;
    for (int d = 0; d < 12; d++) {
        std::string s;
        for (int k = 0; k < 40; k++) s += "w" + std::to_string((d * 7919 + k * 104729) % 997) + (k % 5 ? " " : " 今天天氣 ");
        docs.push_back(s);
    }
    docs[5] = docs[1];
    docs[9] = docs[1];
    docs[11] = docs[2];
    docs[7] = "";
    const uint32_t n = 3, K = 64, B = 16, R = 4, W = 64, m = 51;
    try {
        auto tk = Tokenizer::Open(cfg);
        const auto mh = tk->MinHash(docs, n, K);
        const auto r = tk->NearDuplicates(docs, n, K, B, R, W);  // (minAgree 0: the integer nearest 0.8 K = 51)
        const uint32_t nd = (uint32_t)docs.size();
        std::vector<uint64_t> keys((size_t)nd * B), off(nd + 1), stat(JB_ND_NSTAT);
        std::vector<uint32_t> pd(256), pa(256), label(nd);
        uint64_t np = 0;
        if (jb_minhash_bands(mh.sig.data(), mh.docN.data(), nd, K, B, R, keys.data()) != JB_OK) return 1;
        if (jb_neardup(keys.data(), mh.sig.data(), nd, B, K, W, m, pd.data(), pa.data(), pd.size(), off.data(), &np,
                       stat.data()) != JB_OK || np > pd.size())
            return 1;
        pd.resize(np);
        pa.resize(np);
        if (jb_neardup_labels(off.data(), pd.data(), np, nd, label.data()) != JB_OK) return 1;
        if (r.pairOff != off || r.pairDoc != pd || r.pairAgree != pa || r.label != label) {
            std::fprintf(stderr, "the mirror's result differs from the host rule's\n");
            return 1;
        }
        for (uint32_t k = 0; k < JB_ND_NSTAT; k++)
            if (r.stat[k] != stat[k]) return 1;
        if (label[5] != 1 || label[9] != 1 || label[11] != 2 || label[7] != 7 || label[0] != 0 || np < 4) return 1;
        for (uint64_t k = off[9]; k < off[10]; k++)
            if (pa[k] != K) return 1;  // (document 9's pairs are its exact copies 1 and 5)
        if (off[10] - off[9] != 2) return 1;
        const auto none = tk->NearDuplicates({});
        if (!none.label.empty() || none.pairOff.size() != 1 || none.pairOff[0] != 0) return 1;
    } catch (const jiebago::Error& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    std::printf("neardup ok\n");
    return 0;
}
