// tokenizer.cpp — C++ mirror of jieba-go's Tokenizer over the C ABI.
#include "tokenizer.hpp"

#include <algorithm>
#include <cstring>

namespace jiebago {

static void check(int rc) {
    if (rc != JB_OK) throw Error(rc, jb_last_error());
}

std::unique_ptr<Tokenizer> Tokenizer::Open(const jb_config& cfg) {
    jb_ctx* c = nullptr;
    check(jb_open(&cfg, &c));
    return std::unique_ptr<Tokenizer>(new Tokenizer(c));
}

std::unique_ptr<Tokenizer> Tokenizer::NewTokenizer(const std::string& dictionaryFile, int device) {
    jb_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.dict_path = dictionaryFile.c_str();
    cfg.dict_kind = JB_DICT_TXT;
    cfg.emit_path = "prob_emit.json";
    cfg.device = device;
    cfg.ndevices = 1;
    return Open(cfg);
}

std::unique_ptr<Tokenizer> Tokenizer::NewJiebaTokenizer(int device) {
    jb_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.dict_path = "prefix_dictionary.gob";
    cfg.dict_kind = JB_DICT_GOB;  // size 60,101,967 (tokenizer.go:454)
    cfg.emit_path = "prob_emit.json";
    cfg.device = device;
    cfg.ndevices = 1;
    return Open(cfg);
}

std::unique_ptr<Tokenizer> Tokenizer::FromImage(const std::string& path, int device) {
    jb_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.dict_path = path.c_str();
    cfg.dict_kind = JB_DICT_IMAGE;
    cfg.device = device;
    cfg.ndevices = 1;
    return Open(cfg);
}

Tokenizer::~Tokenizer() { jb_close(ctx_); }

static std::string token_at(const std::string& text, uint64_t s, uint64_t e) {
    // an invalid UTF-8 byte is emitted as "�" by the reference's range loop
    if (e - s == 1 && (unsigned char)text[s] >= 0x80) return "\xEF\xBF\xBD";
    return text.substr(s, e - s);
}

std::vector<std::string> Tokenizer::Cut(const std::string& text, bool useHmm) {
    jb_spans sp;
    check(jb_cut(ctx_, (const uint8_t*)text.data(), text.size(), useHmm ? 1 : 0, &sp));
    std::vector<std::string> out;
    out.reserve(sp.ntokens);
    for (uint64_t k = 0; k < sp.ntokens; k++) out.push_back(token_at(text, sp.start[k], sp.end[k]));
    jb_spans_free(&sp);
    return out;
}

std::vector<std::string> Tokenizer::CutForSearch(const std::string& text, bool useHmm) {
    jb_spans sp;
    check(jb_cut_search(ctx_, (const uint8_t*)text.data(), text.size(), useHmm ? 1 : 0, &sp));
    std::vector<std::string> out;
    out.reserve(sp.ntokens);
    for (uint64_t k = 0; k < sp.ntokens; k++) out.push_back(token_at(text, sp.start[k], sp.end[k]));
    jb_spans_free(&sp);
    return out;
}

std::vector<std::string> Tokenizer::CutAll(const std::string& text) {
    jb_spans sp;
    check(jb_cut_full(ctx_, (const uint8_t*)text.data(), text.size(), &sp));
    std::vector<std::string> out;
    out.reserve(sp.ntokens);
    for (uint64_t k = 0; k < sp.ntokens; k++) out.push_back(token_at(text, sp.start[k], sp.end[k]));
    jb_spans_free(&sp);
    return out;
}

void Tokenizer::SetVocab(const std::vector<std::string>& keys) {
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& k : keys) {
        all += k;
        off.push_back(all.size());
    }
    // (keys.data() of an empty list may be null, which would remove the vocabulary: pass a byte)
    check(jb_vocab_set(ctx_, (const uint8_t*)(all.empty() ? "" : all.data()), off.data(), (uint32_t)keys.size()));
}

std::vector<std::string> Tokenizer::CutIds(const std::string& text, bool useHmm, std::vector<uint32_t>* ids,
                                           Mode mode) {
    jb_spans sp;
    const uint8_t* t = (const uint8_t*)text.data();
    if (mode == Mode::Full) check(jb_cut_full(ctx_, t, text.size(), &sp));
    else if (mode == Mode::Search) check(jb_cut_search(ctx_, t, text.size(), useHmm ? 1 : 0, &sp));
    else check(jb_cut(ctx_, t, text.size(), useHmm ? 1 : 0, &sp));
    std::vector<std::string> out;
    out.reserve(sp.ntokens);
    for (uint64_t k = 0; k < sp.ntokens; k++) out.push_back(token_at(text, sp.start[k], sp.end[k]));
    int rc = JB_OK;
    if (ids) {
        ids->assign(sp.ntokens, JB_ID_UNK);
        rc = jb_spans_ids(ctx_, t, &sp, ids->data());
    }
    jb_spans_free(&sp);
    check(rc);
    return out;
}

std::vector<std::vector<Tokenizer::Tag>> Tokenizer::ExtractTags(const std::vector<std::string>& docs,
                                                                const std::vector<float>& weights, uint32_t topK,
                                                                bool useHmm) {
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& d : docs) {
        all += d;
        off.push_back(all.size());
    }
    const size_t nd = docs.size(), nrec = nd * (size_t)topK;
    std::vector<uint32_t> id(nrec + 1), cnt(nrec + 1), n(nd + 1);
    std::vector<float> score(nrec + 1);
    check(jb_keywords_batch(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)nd, useHmm ? 1 : 0, weights.data(),
                            (uint32_t)weights.size(), topK, id.data(), score.data(), cnt.data(), n.data()));
    std::vector<std::vector<Tag>> out(nd);
    for (size_t d = 0; d < nd; d++)
        for (uint32_t r = 0; r < n[d]; r++) out[d].push_back(Tag{id[d * topK + r], score[d * topK + r], cnt[d * topK + r]});
    return out;
}

Tokenizer::IdfFit Tokenizer::FitIdf(const std::vector<std::vector<std::string>>& batches, bool useHmm, uint32_t minDf,
                                    uint32_t maxDf, const std::vector<uint8_t>& keep) {
    const int64_t nv = jb_vocab_size(ctx_);
    if (nv < 0) throw Error(JB_EINVAL, "FitIdf: no vocabulary attached (SetVocab)");
    if (!keep.empty() && keep.size() != (size_t)nv) throw Error(JB_EINVAL, "FitIdf: keep holds one byte per id");
    IdfFit fit{std::vector<float>((size_t)nv), std::vector<uint32_t>((size_t)nv, 0u), 0};
    for (const auto& docs : batches) {
        if (docs.empty()) continue;
        std::string all;
        std::vector<uint64_t> off(1, 0);
        for (const auto& d : docs) {
            all += d;
            off.push_back(all.size());
        }
        check(jb_df_batch(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)docs.size(), useHmm ? 1 : 0,
                          fit.df.data(), (uint32_t)nv));
        fit.ndocs += docs.size();
    }
    check(jb_idf(fit.df.data(), (uint32_t)nv, fit.ndocs, minDf, maxDf, keep.empty() ? nullptr : keep.data(),
                 fit.weights.data()));
    return fit;
}

Tokenizer::Index Tokenizer::Postings(const std::vector<std::string>& docs, bool useHmm, uint32_t docBase) {
    const int64_t nv = jb_vocab_size(ctx_);
    if (nv < 0) throw Error(JB_EINVAL, "Postings: no vocabulary attached (SetVocab)");
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& d : docs) {
        all += d;
        off.push_back(all.size());
    }
    Index ix;
    ix.off.assign((size_t)nv + 1, 0);
    ix.docLen.assign(docs.size(), 0);
    // (a first guess of one posting per four bytes; the full count comes back with JB_ELIMIT)
    uint64_t n = 0, pcap = all.size() / 4 + 16;
    for (int pass = 0; pass < 2; pass++) {
        ix.doc.resize(pcap);
        ix.tf.resize(pcap);
        const int rc = jb_postings_batch(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)docs.size(), useHmm ? 1 : 0,
                                         docBase, pcap, ix.off.data(), (uint32_t)nv, ix.doc.data(), ix.tf.data(), &n,
                                         ix.docLen.data());
        if (rc == JB_ELIMIT && n > pcap && pass == 0) {
            pcap = n;
            continue;
        }
        check(rc);
        break;
    }
    ix.doc.resize(n);
    ix.tf.resize(n);
    return ix;
}

void Tokenizer::SetIndex(const Index& ix, double k1, double b) {
    if (ix.off.empty() || ix.doc.size() != ix.tf.size())
        throw Error(JB_EINVAL, "SetIndex: an index without offsets, or doc and tf of different lengths");
    check(jb_index_set(ctx_, ix.off.data(), ix.doc.data(), ix.tf.data(), ix.doc.size(), (uint32_t)(ix.off.size() - 1),
                       ix.docLen.data(), ix.docLen.size(), k1, b));
}

void Tokenizer::ClearIndex() { check(jb_index_clear(ctx_)); }

std::vector<std::vector<Tokenizer::Hit>> Tokenizer::Search(const std::vector<std::string>& queries, uint32_t topK,
                                                           bool useHmm) {
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& q : queries) {
        all += q;
        off.push_back(all.size());
    }
    const size_t nq = queries.size(), k = topK ? topK : 1;
    std::vector<uint32_t> doc(nq * k + 1), n(nq + 1);
    std::vector<uint64_t> score(nq * k + 1);
    check(jb_search_batch(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)nq, useHmm ? 1 : 0, topK, doc.data(),
                          score.data(), n.data()));
    std::vector<std::vector<Hit>> out(nq);
    for (size_t q = 0; q < nq; q++)
        for (uint32_t r = 0; r < n[q]; r++) out[q].push_back(Hit{doc[q * k + r], score[q * k + r]});
    return out;
}

std::vector<std::vector<Tokenizer::Rank>> Tokenizer::TextRank(const std::vector<std::string>& docs,
                                                              const std::vector<uint8_t>& keep, uint32_t topK,
                                                              uint32_t span, uint32_t iters, bool useHmm) {
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& d : docs) {
        all += d;
        off.push_back(all.size());
    }
    const size_t nd = docs.size(), nrec = nd * (size_t)topK;
    std::vector<uint32_t> id(nrec + 1), n(nd + 1);
    std::vector<float> score(nrec + 1);
    check(jb_textrank_batch(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)nd, useHmm ? 1 : 0, keep.data(),
                            (uint32_t)keep.size(), span, iters, topK, id.data(), score.data(), n.data()));
    std::vector<std::vector<Rank>> out(nd);
    for (size_t d = 0; d < nd; d++)
        for (uint32_t r = 0; r < n[d]; r++) out[d].push_back(Rank{id[d * topK + r], score[d * topK + r]});
    return out;
}

std::vector<std::string> Tokenizer::CutJoin(const std::vector<std::string>& docs, const std::string& sep, bool useHmm,
                                            int mode) {
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& d : docs) {
        all += d;
        off.push_back(all.size());
    }
    jb_joined j;
    check(jb_cut_batch_join(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)docs.size(), useHmm ? 1 : 0, mode,
                            (const uint8_t*)sep.data(), (uint32_t)sep.size(), nullptr, 0, &j));
    std::vector<std::string> out;
    out.reserve(docs.size());
    for (size_t d = 0; d < docs.size(); d++)
        out.emplace_back((const char*)j.text + j.doc_off[d], (size_t)(j.doc_off[d + 1] - j.doc_off[d]));
    jb_joined_free(&j);
    return out;
}

void Tokenizer::SetStopWords(const std::vector<std::string>& keys) {
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& k : keys) {
        all += k;
        off.push_back(all.size());
    }
    // (keys.data() of an empty list may be null, which would remove the set: pass a byte)
    check(jb_stopwords_set(ctx_, (const uint8_t*)(all.empty() ? "" : all.data()), off.data(), (uint32_t)keys.size()));
}

std::vector<std::vector<std::string>> Tokenizer::CutFiltered(const std::vector<std::string>& docs,
                                                             const jb_filter_rule& rule, bool useHmm, int mode) {
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& d : docs) {
        all += d;
        off.push_back(all.size());
    }
    // (a plain or search cut has at most one span per byte; full mode's count comes back with JB_ELIMIT)
    std::vector<uint32_t> s(all.size() + 1), e(all.size() + 1);
    std::vector<uint64_t> tok(docs.size() + 1);
    uint64_t n = 0;
    int rc = jb_cut_batch_filter(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)docs.size(), useHmm ? 1 : 0, mode,
                                 &rule, s.data(), e.data(), s.size(), tok.data(), &n, nullptr);
    if (rc == JB_ELIMIT && n > s.size()) {
        s.resize(n);
        e.resize(n);
        rc = jb_cut_batch_filter(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)docs.size(), useHmm ? 1 : 0, mode,
                                 &rule, s.data(), e.data(), s.size(), tok.data(), &n, nullptr);
    }
    check(rc);
    std::vector<std::vector<std::string>> out(docs.size());
    for (size_t d = 0; d < docs.size(); d++)
        for (uint64_t k = tok[d]; k < tok[d + 1]; k++) out[d].push_back(token_at(all, s[k], e[k]));
    return out;
}

void Tokenizer::SetBatchFilter(const jb_filter_rule& rule) { check(jb_batch_filter_set(ctx_, &rule)); }
void Tokenizer::ClearBatchFilter() { check(jb_batch_filter_set(ctx_, nullptr)); }

std::vector<Tokenizer::WordCount> Tokenizer::WordCounts(const std::vector<std::string>& docs, bool useHmm, int mode,
                                                        uint64_t minCount, uint64_t maxKeys, uint64_t nslots,
                                                        uint64_t poolBytes, bool strict) {
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& d : docs) {
        all += d;
        off.push_back(all.size());
    }
    const size_t ntable = jb_wc_table_bytes(nslots, poolBytes);
    void* table = nullptr;
    check(jb_device_alloc(ctx_, ntable, &table));
    jb_wc_result r;
    int rc = jb_wc_init_device(ctx_, table, ntable, nslots, poolBytes, nullptr);
    if (rc == JB_OK)
        rc = jb_wc_batch(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)docs.size(), useHmm ? 1 : 0, mode, table,
                         ntable);
    if (rc == JB_OK) rc = jb_wc_read(ctx_, table, ntable, nullptr, minCount, maxKeys, &r);
    jb_device_free(ctx_, table);
    check(rc);
    std::vector<WordCount> out;
    out.reserve(r.nkeys);
    for (uint64_t i = 0; i < r.nkeys; i++)
        out.push_back({std::string((const char*)r.keys + r.key_off[i], (size_t)(r.key_off[i + 1] - r.key_off[i])), r.counts[i]});
    const uint64_t dropped = r.ndropped, collided = r.ncollided;
    jb_wc_result_free(&r);
    if (strict && (dropped || collided))
        throw Error(JB_ELIMIT, "WordCounts: " + std::to_string(dropped) + " tokens dropped for lack of room and " +
                                   std::to_string(collided) + " in fingerprint collisions: the counts are lower bounds");
    return out;
}

Tokenizer::MinHashResult Tokenizer::MinHash(const std::vector<std::string>& docs, uint32_t n, uint32_t K, uint64_t seed,
                                            bool useHmm, int mode) {
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& d : docs) {
        all += d;
        off.push_back(all.size());
    }
    MinHashResult r;
    r.sig.resize(docs.size() * (size_t)K + 1);  // (+ 1: never an empty vector, its address is passed)
    r.docN.resize(docs.size() + 1);
    check(jb_minhash_batch(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)docs.size(), useHmm ? 1 : 0, mode, n, K,
                           seed, r.sig.data(), r.docN.data()));
    r.sig.resize(docs.size() * (size_t)K);
    r.docN.resize(docs.size());
    return r;
}

Tokenizer::NearDupResult Tokenizer::NearDuplicates(const std::vector<std::string>& docs, uint32_t n, uint32_t K, uint32_t B,
                                                   uint32_t R, uint32_t W, uint32_t minAgree, uint64_t seed, bool useHmm,
                                                   int mode) {
    const MinHashResult mh = MinHash(docs, n, K, seed, useHmm, mode);
    const uint32_t nd = (uint32_t)docs.size();
    if (minAgree == 0) minAgree = std::max<uint32_t>(1, (4 * K + 2) / 5);
    NearDupResult r;
    r.pairOff.resize((size_t)nd + 1);
    r.label.resize((size_t)nd + 1);  // (+ 1: never an empty vector, its address is passed)
    uint64_t np = 0, cap = std::max<uint64_t>(1024, 4ull * nd);
    for (int pass = 0; pass < 2; pass++) {
        r.pairDoc.resize(cap);
        r.pairAgree.resize(cap);
        const int rc = jb_neardup_sig(ctx_, mh.sig.data(), mh.docN.data(), nd, K, B, R, W, minAgree, r.pairDoc.data(),
                                      r.pairAgree.data(), cap, r.pairOff.data(), &np, r.stat);
        if (rc == JB_ELIMIT && np > cap && pass == 0) {  // (the arrays were too small: the count is known now)
            cap = np;
            continue;
        }
        check(rc);
        break;
    }
    r.pairDoc.resize(np);
    r.pairAgree.resize(np);
    check(jb_neardup_labels(r.pairOff.data(), r.pairDoc.data(), np, nd, r.label.data()));
    r.label.resize(nd);
    return r;
}

std::vector<Tokenizer::Colloc> Tokenizer::Collocations(const std::vector<std::string>& docs,
                                                       const std::vector<std::string>& keys, int scorer,
                                                       uint64_t minCount, float threshold, uint64_t topn, bool contiguous,
                                                       const std::vector<uint8_t>& keep, bool useHmm, uint64_t nslots) {
    const int64_t nv = jb_vocab_size(ctx_);
    if (nv < 0) throw Error(JB_EINVAL, "Collocations: no vocabulary attached (SetVocab)");
    if ((uint64_t)nv != keys.size()) throw Error(JB_EINVAL, "Collocations: keys are not the attached vocabulary's");
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& d : docs) {
        all += d;
        off.push_back(all.size());
    }
    const uint32_t nuni = (uint32_t)nv;
    const size_t ntable = jb_colloc_table_bytes(nslots);
    void *table = nullptr, *uni = nullptr;
    check(jb_device_alloc(ctx_, ntable, &table));
    int rc = jb_device_alloc(ctx_, (size_t)nuni * 8 + 8, &uni);
    jb_colloc_result r;
    if (rc == JB_OK) rc = jb_colloc_init_device(ctx_, table, ntable, nslots, (uint64_t*)uni, nuni, nullptr);
    if (rc == JB_OK)
        rc = jb_colloc_batch(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)docs.size(), useHmm ? 1 : 0,
                             keep.empty() ? nullptr : keep.data(), (uint32_t)keep.size(), contiguous ? JB_COLLOC_CONTIG : 0u,
                             table, ntable, (uint64_t*)uni, nuni);
    if (rc == JB_OK)
        rc = jb_colloc_read(ctx_, table, ntable, (const uint64_t*)uni, nuni, scorer, minCount, threshold, topn, nullptr, &r);
    jb_device_free(ctx_, uni);
    jb_device_free(ctx_, table);
    check(rc);
    std::vector<Colloc> out;
    out.reserve(r.n);
    for (uint64_t i = 0; i < r.n; i++) out.push_back({keys[r.a[i]], keys[r.b[i]], r.count[i], r.score[i]});
    const uint64_t dropped = r.dropped;
    jb_colloc_result_free(&r);
    if (dropped)
        throw Error(JB_ELIMIT, "Collocations: " + std::to_string(dropped) + " pairs dropped for lack of room: pairs are missing");
    return out;
}

std::vector<std::vector<Tokenizer::Token>> Tokenizer::Tokenize(const std::vector<std::string>& docs, bool useHmm, int mode,
                                                               int unit) {
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& d : docs) {
        all += d;
        off.push_back(all.size());
    }
    const uint32_t nd = (uint32_t)docs.size();
    std::vector<uint32_t> cs(std::max<size_t>(all.size() / 2, 16)), ce(cs.size()), units(nd + 1);
    std::vector<uint64_t> tok(nd + 1);
    uint64_t n = 0;
    int rc = jb_cut_batch_charspans(ctx_, (const uint8_t*)all.data(), off.data(), nd, useHmm ? 1 : 0, mode, unit, cs.data(),
                                    ce.data(), cs.size(), tok.data(), &n, units.data());
    if (rc == JB_ELIMIT && n > cs.size()) {  // (the arrays were too small: the count is known now)
        cs.resize(n);
        ce.resize(n);
        rc = jb_cut_batch_charspans(ctx_, (const uint8_t*)all.data(), off.data(), nd, useHmm ? 1 : 0, mode, unit, cs.data(),
                                    ce.data(), cs.size(), tok.data(), &n, units.data());
    }
    check(rc);
    // the words: the host form of the rule over one span per byte says which bytes start a rune (the span
    // [i, i + 1) has a length of its own exactly there) and at which unit, so no decoder is restated here.
    // With one span per byte, doc_off is also the spans' doc_tok.  It costs a second host pass and 8 bytes
    // per text byte, which a mirror can afford.  In UTF-16 at[u + 1] of a surrogate pair is never set: the
    // library's own cuts put no token bound inside a rune, so no token indexes it.
    const size_t nb = all.size();
    std::vector<uint32_t> bs(nb), be(nb);
    for (size_t i = 0; i < nb; i++) {
        bs[i] = (uint32_t)i;
        be[i] = (uint32_t)i + 1;
    }
    check(jb_charspans((const uint8_t*)all.data(), nb, off.data(), nd, bs.data(), be.data(), off.data(), nb, nb, unit, bs.data(),
                       be.data(), units.data()));
    std::vector<std::vector<Token>> out(nd);
    std::vector<uint32_t> at;  // at[u]: the byte of the document at which unit u starts; at[units[d]]: its length
    for (uint32_t d = 0; d < nd; d++) {
        const std::string& doc = docs[d];
        at.assign((size_t)units[d] + 1, (uint32_t)doc.size());
        for (size_t i = 0; i < doc.size(); i++) {
            const size_t g = off[d] + i;
            if (be[g] > bs[g]) at[bs[g]] = (uint32_t)i;
        }
        for (uint64_t k = tok[d]; k < tok[d + 1]; k++) {
            if (cs[k] > ce[k] || ce[k] > units[d]) continue;  // (JB_CHAR_NONE: not from the library's own cuts)
            out[d].push_back(Token{token_at(doc, at[cs[k]], at[ce[k]]), cs[k], ce[k]});
        }
    }
    return out;
}

std::vector<std::string> Tokenizer::CutParallel(const std::string& text, bool hmm, int, bool) {
    return Cut(text, hmm);
}

std::vector<std::vector<std::string>> Tokenizer::CutBatch(const std::vector<std::string>& docs, bool hmm) {
    std::string all;
    std::vector<uint64_t> off(1, 0);
    for (const auto& d : docs) {
        all += d;
        off.push_back(all.size());
    }
    jb_spans sp;
    check(jb_cut_batch(ctx_, (const uint8_t*)all.data(), off.data(), (uint32_t)docs.size(), hmm ? 1 : 0, &sp));
    std::vector<std::vector<std::string>> out(docs.size());
    for (size_t d = 0; d < docs.size(); d++)
        for (uint64_t k = sp.doc_tok[d]; k < sp.doc_tok[d + 1]; k++)
            out[d].push_back(token_at(all, sp.start[k], sp.end[k]));
    jb_spans_free(&sp);
    return out;
}

void Tokenizer::AddWord(const std::string& word, int freq) {
    check(jb_add_word(ctx_, word.data(), word.size(), freq));
}

void Tokenizer::AddWord(const std::string& word, int freq, const std::function<double(double)>& log) {
    int64_t f = freq;
    if (freq < 1) check(jb_suggest_freq(ctx_, word.data(), word.size(), &f));  // (tokenizer.go:373-375)
    const int64_t keys[2] = {f, jb_dict_size(ctx_) + f};
    const double vals[2] = {log((double)keys[0]), log((double)keys[1])};
    check(jb_add_log(ctx_, keys, vals, 2));
    check(jb_add_word(ctx_, word.data(), word.size(), f));
}

void Tokenizer::Save(const std::string& path) { check(jb_save(ctx_, path.c_str())); }

}  // namespace jiebago
