// tokenizer.hpp — C++ mirror of jieba-go's public Tokenizer API
// (/root/reference/tokenizer.go:52-162, 372-379) over libjiebahip.so.
//
// The Go toolchain is absent from this image, so the host side above the C ABI
// is written in C++ (the reference is compiled code); the cgo binding a Go
// maintainer would add instead is jieba-go_amd/go/tokenizer.go.
//
// Same names and argument meaning as the reference.  Where the reference calls
// log.Fatal / panic (constructor load errors, tokenizer.go:397-416,443,452,656,660;
// the cutDAG slice panic), this mirror throws jiebago::Error.
#pragma once
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "jiebahip.h"

namespace jiebago {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

class Tokenizer {
public:
    // NewTokenizer(dictionaryFile) (tokenizer.go:61): dict.txt semantics, HMM from
    // "prob_emit.json" in the working directory (tokenizer.go:654).
    static std::unique_ptr<Tokenizer> NewTokenizer(const std::string& dictionaryFile, int device = 0);
    // NewJiebaTokenizer() (tokenizer.go:69): decodes "prefix_dictionary.gob" from
    // the working directory (newJiebaPrefixDictionary, tokenizer.go:439-458), size
    // 60_101_967 (tokenizer.go:454).
    static std::unique_ptr<Tokenizer> NewJiebaTokenizer(int device = 0);
    // A serialized image written by Save (no parsing or trie build at start).
    static std::unique_ptr<Tokenizer> FromImage(const std::string& path, int device = 0);
    // Full control (paths, semantics, size override, devices).
    static std::unique_ptr<Tokenizer> Open(const jb_config& cfg);

    ~Tokenizer();
    Tokenizer(const Tokenizer&) = delete;
    Tokenizer& operator=(const Tokenizer&) = delete;

    // Cut (tokenizer.go:151)
    std::vector<std::string> Cut(const std::string& text, bool useHmm);
    // Search-engine mode (jieba's cut_for_search; the reference has only Cut): Cut's tokens,
    // each Han token of three or more runes preceded by the dictionary words of two, then
    // three, runes inside it that buildDag has as edges (jb_cut_search in jiebahip.h, with
    // its two differences from Python jieba).
    std::vector<std::string> CutForSearch(const std::string& text, bool useHmm);
    // Full mode (jieba's cut_all; the reference has only Cut): every dictionary word of two or
    // more runes in the text's Han blocks, by start and then by length, overlapping words
    // included, and the single runes that no such word accounts for; non-Han text as Cut cuts
    // it (jb_cut_full in jiebahip.h, with its three differences from Python jieba).
    std::vector<std::string> CutAll(const std::string& text);
    // Token ids (jb_vocab_set / jb_spans_ids in jiebahip.h): attach the caller's vocabulary (a key's
    // id is its index; 1..255 bytes each, no duplicates), replacing any earlier one.
    void SetVocab(const std::vector<std::string>& keys);
    enum class Mode { Cut, Search, Full };
    // Cut / CutForSearch / CutAll (full mode ignores useHmm) with each token's id in the attached
    // vocabulary, JB_ID_UNK when it is not there; looked up on the GPU.
    std::vector<std::string> CutIds(const std::string& text, bool useHmm, std::vector<uint32_t>* ids,
                                    Mode mode = Mode::Cut);
    // Keywords (jieba.analyse.extract_tags; jb_keywords_batch in jiebahip.h, with its differences from
    // jieba's): per document the topK terms of the attached vocabulary by count x weights[id], best
    // first, ties by id; a term whose weight is not > 0 (or whose id is past the table) is no candidate.
    // Counted and ranked on the GPU: no span reaches the host.
    struct Tag {
        uint32_t id;
        float score;
        uint32_t count;
    };
    std::vector<std::vector<Tag>> ExtractTags(const std::vector<std::string>& docs, const std::vector<float>& weights,
                                              uint32_t topK = 20, bool useHmm = true);
    // IDF weights for the attached vocabulary, fitted on a corpus given as batches of documents
    // (jb_df_batch per batch, then jb_idf; both in jiebahip.h): df[id] is the number of documents id
    // occurs in, weights[id] the smoothed IDF float(log((ndocs + 1) / (df + 1)) + 1), or 0 where df is 0,
    // below minDf, above maxDf (JB_DF_NOMAX: no upper bound) or where keep (empty, or one byte per id)
    // is 0.  ExtractTags(docs, fit.weights) afterwards is the whole of TF-IDF.
    struct IdfFit {
        std::vector<float> weights;
        std::vector<uint32_t> df;
        uint64_t ndocs;
    };
    IdfFit FitIdf(const std::vector<std::vector<std::string>>& batches, bool useHmm = true, uint32_t minDf = 1,
                  uint32_t maxDf = JB_DF_NOMAX, const std::vector<uint8_t>& keep = {});
    // Postings (jb_postings_batch in jiebahip.h): the inverted index of a batch under the attached vocabulary.
    // The list of id t is doc / tf[off[t] .. off[t + 1]): the documents that contain t, ascending (docBase + the
    // document's index in docs), each with its term frequency; docLen[d] is document d's token count, unknown
    // tokens included.  Cut, counted and transposed on the GPU: only the index comes back.  With a running
    // docBase the lists of consecutive batches concatenate per id into the lists of the corpus.
    struct Index {
        std::vector<uint64_t> off;  // vocabulary size + 1
        std::vector<uint32_t> doc, tf, docLen;
    };
    Index Postings(const std::vector<std::string>& docs, bool useHmm = true, uint32_t docBase = 0);
    // BM25 search (jb_index_set and jb_search_batch in jiebahip.h).  SetIndex attaches an index (Postings' result
    // for a corpus in one batch, or the batches' lists concatenated per id) to search; it stays on the device
    // with the documents' norms and the ids' weights until the next SetIndex, ClearIndex or the tokenizer's end.
    // Search cuts the queries in plain mode, looks their tokens up in the attached vocabulary and returns per
    // query at most topK documents, best first (score descending, ties by document ascending); a Hit's score is
    // in units of 2^-24 (Score() is the plain value).  Cut, looked up and ranked on the GPU: only the hits come
    // back.
    struct Hit {
        uint32_t doc;
        uint64_t score;
        double Score() const { return (double)score / 16777216.0; }
    };
    void SetIndex(const Index& ix, double k1 = 1.2, double b = 0.75);
    void ClearIndex();
    std::vector<std::vector<Hit>> Search(const std::vector<std::string>& queries, uint32_t topK = 10, bool useHmm = true);
    // TextRank keywords (jieba.analyse.textrank; jb_textrank_batch in jiebahip.h, with the rule and its
    // differences from jieba's): per document the topK words of the attached vocabulary by PageRank over
    // the co-occurrence graph of the kept tokens within `span` positions, `iters` Jacobi rounds, best
    // first, ties by id.  keep holds one byte per id (jieba's part-of-speech, length and stop-word
    // filters; ids past it are not kept).  Needs no weight table.  Ranked on the GPU: no span reaches
    // the host.
    struct Rank {
        uint32_t id;
        float score;
    };
    std::vector<std::vector<Rank>> TextRank(const std::vector<std::string>& docs, const std::vector<uint8_t>& keep,
                                            uint32_t topK = 20, uint32_t span = 5, uint32_t iters = 10,
                                            bool useHmm = true);
    // Joined text (jb_cut_batch_join in jiebahip.h): sep.join(cut(doc)) for every document of a batch, the
    // cut of `mode` (JB_MODE_CUT, JB_MODE_SEARCH, JB_MODE_FULL; full mode ignores useHmm) and the join both
    // on the GPU; only the joined bytes come back.  An invalid byte comes out as U+FFFD; whitespace and
    // non-Han blocks without an alnum byte are absent, as in Cut.  sep holds at most JB_JOIN_MAXSEP bytes.
    std::vector<std::string> CutJoin(const std::vector<std::string>& docs, const std::string& sep = " ",
                                     bool useHmm = true, int mode = JB_MODE_CUT);
    // Token filtering (jb_stopwords_set, jb_cut_batch_filter and jb_batch_filter_set in jiebahip.h).
    // SetStopWords attaches the caller's stop list (1..255 bytes each, no duplicates), replacing any earlier
    // one; it is independent of SetVocab.  CutFiltered is `[w for w in cut(doc) if ...]` for every document of a
    // batch: the cut of `mode` and the filter both on the GPU, by class (rule.drop_classes, JB_TC_* bits), length
    // in runes (rule.min_runes, rule.max_runes; 0: no upper bound) and, with JB_FILTER_STOP in rule.flags, the
    // stop set.  A kept invalid byte comes out as U+FFFD.  SetBatchFilter stores a rule that CutJoin, WordCounts
    // and MinHash filter the cut's tokens by before their own step, until ClearBatchFilter.
    void SetStopWords(const std::vector<std::string>& keys);
    std::vector<std::vector<std::string>> CutFiltered(const std::vector<std::string>& docs,
                                                      const jb_filter_rule& rule = {0, JB_TC_OTHER | JB_TC_INVALID, 0, 0},
                                                      bool useHmm = true, int mode = JB_MODE_CUT);
    void SetBatchFilter(const jb_filter_rule& rule);
    void ClearBatchFilter();
    // jieba's tokenize (jb_cut_batch_charspans in jiebahip.h): per document its tokens with their offsets in
    // the document, in Unicode characters (JB_UNIT_RUNE) or UTF-16 code units (JB_UNIT_UTF16), the cut of
    // `mode` and the conversion both on the GPU; no byte offset reaches the host.  The word is the token's
    // bytes, U+FFFD for an invalid byte, as in Cut; start and end index the document's code points (a Python str, a Go []rune) or its UTF-16 form
    // (a Java String), where an invalid byte counts 1.
    struct Token {
        std::string word;
        uint32_t start, end;
    };
    std::vector<std::vector<Token>> Tokenize(const std::vector<std::string>& docs, bool useHmm = true,
                                             int mode = JB_MODE_CUT, int unit = JB_UNIT_RUNE);
    // Word counts (Counter(jieba.cut(text)); the jb_wc_* calls in jiebahip.h): the distinct tokens of the documents
    // in the cut of `mode` with their exact counts, by count descending and then by bytes, without the words
    // below minCount, the first maxKeys of them (0: all).  The cut and the counting run on the GPU, in a table of
    // nslots slots (a power of two; new words are accepted while fewer than half are taken) and poolBytes for
    // the words over 24 bytes; only the distinct words come back.  Throws Error(JB_ELIMIT) when tokens were
    // dropped for lack of room or two words shared a fingerprint, unless strict is false: the counts are lower
    // bounds then.  SetVocab with the words fits a vocabulary.
    struct WordCount {
        std::string word;
        uint64_t count;
    };
    std::vector<WordCount> WordCounts(const std::vector<std::string>& docs, bool useHmm = true, int mode = JB_MODE_CUT,
                                      uint64_t minCount = 1, uint64_t maxKeys = 0, uint64_t nslots = 1u << 20,
                                      uint64_t poolBytes = 4u << 20, bool strict = true);
    // MinHash signatures (jb_minhash_batch in jiebahip.h): per document K u32 slots over its shingles of n
    // consecutive words of the cut of `mode`, for near-duplicate detection: two documents agree in a slot with
    // the probability of their shingle sets' Jaccard similarity.  The cut and the sketch both run on the GPU;
    // only the signatures come back.  sig holds docs.size() rows of K slots; docN[d] is document d's shingle
    // count, and a document without tokens has 0 there and JB_MH_EMPTY in every slot.
    struct MinHashResult {
        std::vector<uint32_t> sig;   // docs.size() x K
        std::vector<uint32_t> docN;  // docs.size()
    };
    MinHashResult MinHash(const std::vector<std::string>& docs, uint32_t n = 5, uint32_t K = 128, uint64_t seed = 1,
                          bool useHmm = true, int mode = JB_MODE_CUT);
    // Near-duplicate groups (jb_neardup_sig and jb_neardup_labels in jiebahip.h): MinHash as above, then LSH
    // bands of R rows, the bucket join inside the window W and the verification against all K slots on the GPU.
    // label[d] is the least document of d's group: label[d] == d marks the one document of each group to keep.
    // Row j of the CSR (pairOff, pairDoc, pairAgree) lists the earlier documents kept as near-duplicates of j.
    // minAgree == 0 means the integer nearest 0.8 K.
    struct NearDupResult {
        std::vector<uint32_t> label;      // docs.size()
        std::vector<uint64_t> pairOff;    // docs.size() + 1
        std::vector<uint32_t> pairDoc, pairAgree;
        uint64_t stat[JB_ND_NSTAT];
    };
    NearDupResult NearDuplicates(const std::vector<std::string>& docs, uint32_t n = 5, uint32_t K = 128, uint32_t B = 32,
                                 uint32_t R = 4, uint32_t W = 64, uint32_t minAgree = 0, uint64_t seed = 1,
                                 bool useHmm = true, int mode = JB_MODE_CUT);
    // Collocations (jb_colloc_batch and jb_colloc_read in jiebahip.h): how often word a is directly followed by
    // word b over the documents, against how often each occurs alone, counted and scored on the GPU under the
    // attached vocabulary, whose keys (what SetVocab was given) name the pairs: best first, by score, count and ids.
    // scorer is JB_COLLOC_NPMI, JB_COLLOC_RATIO or JB_COLLOC_COUNT; contiguous counts a pair only when the two
    // tokens touch in the text, so that a + b is a substring: the top pairs the dictionary lacks are the words to
    // AddWord.  keep (one byte per key, empty: all) limits the pairs to kept words.  Throws when pairs were
    // dropped for lack of room in the table of nslots slots (a power of two; four times the distinct pairs).
    struct Colloc {
        std::string a, b;
        uint64_t count;
        float score;
    };
    std::vector<Colloc> Collocations(const std::vector<std::string>& docs, const std::vector<std::string>& keys,
                                     int scorer = JB_COLLOC_NPMI, uint64_t minCount = 5, float threshold = 0.5f,
                                     uint64_t topn = 0, bool contiguous = false,
                                     const std::vector<uint8_t>& keep = {}, bool useHmm = true,
                                     uint64_t nslots = 1u << 20);
    // CutParallel (tokenizer.go:81).  Blocks are segmented in parallel on the
    // GPU; numWorkers is accepted for API compatibility.  Output is always in
    // text order (ordered=false in the reference is a block permutation).
    std::vector<std::string> CutParallel(const std::string& text, bool hmm, int numWorkers, bool ordered);
    // Many documents in one device pass (what CutParallel is used for).
    std::vector<std::vector<std::string>> CutBatch(const std::vector<std::string>& docs, bool hmm);
    // AddWord (tokenizer.go:372) without the reference's self-deadlock.  The new
    // weights use the library's restatement of Go's math.Log (jb_go_log).
    void AddWord(const std::string& word, int freq);
    // The same with the caller's logarithm (the Go binding passes math.Log): log(f) of
    // the new frequency and log(size + f) of the new pd.size (addTerm, tokenizer.go:580-585)
    // go to jb_add_log first, so the rebuilt weights use exactly those values.
    void AddWord(const std::string& word, int freq, const std::function<double(double)>& log);
    // Write the current image (AddWord changes included) for FromImage.
    void Save(const std::string& path);

    jb_ctx* handle() { return ctx_; }

private:
    explicit Tokenizer(jb_ctx* c) : ctx_(c) {}
    jb_ctx* ctx_;
};

}  // namespace jiebago
