/*
 * jiebahip.h — C ABI of libjiebahip.so, the MI355X (gfx950) segmentation path
 * behind jieba-go's Tokenizer API.
 *
 * The reference (ericlingit/jieba-go) is a pure-Go package with no FFI; its
 * boundary is its public Go API.  Each entry point below names
 * the reference interface it replaces.  A Go caller binds these through cgo
 * (INTEGRATION.md); the C++ mirror jieba-go_amd/host/tokenizer.hpp and the
 * Python ctypes binding jieba-go_amd/python/jiebahip.py sit on the same calls.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Every function returns JB_OK (0) or a
 *    negative JB_E* code; the library never aborts the process (the reference
 *    calls log.Fatal / panic on load errors, tokenizer.go:397,405,416,443,452,656,660).
 *  - The caller owns every input buffer; nothing is retained past return.
 *  - Outputs returned in jb_spans are owned by the library until jb_spans_free.
 *  - A jb_ctx may be used by several threads at once for cutting (the reference
 *    takes pd.lock.RLock in Cut/CutParallel, tokenizer.go:82-83,152-153);
 *    jb_add_word takes the exclusive lock.
 *  - Token k of the output is the byte range [start[k], end[k]) of the input.
 *    A 1-byte token whose byte is >= 0x80 is an invalid UTF-8 byte, which the
 *    reference emits as "�" (range loop in cutNonZh, tokenizer.go:301-306).
 */
#ifndef JIEBAHIP_H
#define JIEBAHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JB_OK 0
#define JB_EINVAL (-1)  /* bad argument */
#define JB_EIO (-2)     /* file cannot be read (reference: log.Fatal, tokenizer.go:397,443) */
#define JB_EPARSE (-3)  /* dictionary / emission parse error (reference: log.Fatal / panic) */
#define JB_EDEVICE (-4) /* HIP runtime error (no device, launch failure, ...) */
#define JB_ENOMEM (-5)
#define JB_EPANIC (-6)  /* input on which the reference panics (cutDAG slice with tail -1) */
#define JB_ELIMIT (-7)  /* unsupported size (document >= 2 GiB, word > 255 runes) */

typedef struct jb_ctx jb_ctx;
typedef struct jb_image jb_image;

/* Dictionary semantics. */
#define JB_DICT_TXT 0    /* NewTokenizer(dictionaryFile): newPrefixDictionaryFromFile, tokenizer.go:61,389-437
                            (first occurrence wins, size = sum of first occurrences, no prefix entries) */
#define JB_DICT_PREFIX 1 /* dict.txt-format lines read as buildPrefixDictionary does, tokenizer.go:340-366
                            (last value wins, freq-0 prefix entries): the map prefix_dictionary.gob holds */
#define JB_DICT_GOB 2    /* NewJiebaTokenizer(): prefix_dictionary.gob itself, an encoding/gob map[string]int
                            (newJiebaPrefixDictionary, tokenizer.go:69,439-458); size = 60,101,967
                            (tokenizer.go:454) unless size_override > 0 */
#define JB_DICT_IMAGE 3  /* a serialized image written by jb_save / jb_image_save (dictionary, emission
                            table and device arrays; emit_path is ignored): skips parsing and the trie
                            build.  size_override > 0 and different from the saved size rebuilds the weights */
#define JB_JIEBA_SIZE 60101967 /* newJiebaPrefixDictionary's pd.size (tokenizer.go:454) */

typedef struct {
    const char *dict_path;   /* dictionary file in the dict_kind format; NULL: use dict_buf */
    const char *dict_buf;
    size_t dict_len;
    int dict_kind;           /* JB_DICT_TXT or JB_DICT_PREFIX */
    int64_t size_override;   /* > 0 replaces pd.size; NewJiebaTokenizer hard-codes 60_101_967 (tokenizer.go:454) */
    const char *emit_path;   /* prob_emit.json (tokenizer.go:654); NULL: use emit_buf */
    const char *emit_buf;
    size_t emit_len;
    int device;              /* first HIP device ordinal */
    int ndevices;            /* >= 1: documents are sharded over devices device..device+ndevices-1 */
    /* Optional caller-computed logarithms: log_vals[i] is the caller's
     * math.Log(float64(log_keys[i])).  calcDagProba's weights math.Log(tf) - math.Log(pd.size)
     * (tokenizer.go:503,515-519) use these values for the frequencies and the size they
     * cover, and the library's restatement of Go's math.Log (jb_go_log) for the rest, so a
     * Go caller that passes math.Log results gets the reference's weights by construction.
     * The keys a dictionary needs are listed by jb_image_log_keys.  nlog = 0: none. */
    const int64_t *log_keys;
    const double *log_vals;
    size_t nlog;
} jb_config;

typedef struct {
    uint64_t ntokens;
    uint64_t *start;   /* byte offset of each token in the batch */
    uint64_t *end;
    uint64_t *doc_tok; /* ndocs + 1 entries: tokens of document d are [doc_tok[d], doc_tok[d+1]) */
    uint32_t ndocs;
} jb_spans;

/* Replaces NewTokenizer (tokenizer.go:61) and NewJiebaTokenizer (tokenizer.go:69):
 * parse the dictionary and emission table, build the device image and upload it
 * to every configured device. */
int jb_open(const jb_config *cfg, jb_ctx **out);
/* jb_open from an image built by jb_image_build, so the trie is placed once: what the
 * Go binding calls after listing the image's log keys (jb_image_log_keys) and taking
 * math.Log of each (NewTokenizer / NewJiebaTokenizer, tokenizer.go:61-75).  Only
 * cfg->device, cfg->ndevices and the log table (log_keys, log_vals, nlog: the weights
 * are recomputed from them, tokenizer.go:503,515-519) are read.  `img` is consumed on
 * every path, success or not: do not jb_image_free it afterwards. */
int jb_open_image(jb_image *img, const jb_config *cfg, jb_ctx **out);
void jb_close(jb_ctx *ctx);
/* Last error message of the calling thread (never NULL). */
const char *jb_last_error(void);

/* Replaces Tokenizer.Cut (tokenizer.go:151) for one document. */
int jb_cut(jb_ctx *ctx, const uint8_t *text, size_t len, int hmm, jb_spans *out);

/* Replaces Tokenizer.CutParallel (tokenizer.go:81) and batches of Cut calls:
 * ndocs documents concatenated in `text`, document d = [doc_off[d], doc_off[d+1]).
 * Output tokens are in document order (CutParallel with ordered=true; the
 * reference's ordered=false is a block permutation of the same tokens). */
int jb_cut_batch(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm,
                 jb_spans *out);
void jb_spans_free(jb_spans *s);

/* jb_cut_batch into caller-owned arrays (no library allocation; what a Go
 * caller passes as slices): start/end hold up to `cap` tokens, doc_tok ndocs+1
 * entries.  *ntokens receives the token count; when it exceeds cap the call
 * returns JB_ELIMIT with *ntokens set and the caller retries with bigger arrays
 * (a batch of n bytes never has more than n tokens). */
int jb_cut_batch_into(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm,
                      uint64_t *start, uint64_t *end, uint64_t cap, uint64_t *doc_tok, uint64_t *ntokens);

/* jb_cut_batch_into with u32 outputs, offsets relative to the batch's first byte:
 * token k is the byte range [doc_off[0] + start[k], doc_off[0] + end[k]).  Half the
 * output of the u64 form (what a Go caller slices its strings with: the host side of
 * a host batch is bound by writing the spans, 16 bytes per token there, 8 here).  The
 * batch must be under 4 GiB (JB_ELIMIT otherwise; a caller cuts larger ones in parts);
 * JB_ELIMIT with *ntokens set when the arrays are too small, as jb_cut_batch_into. */
int jb_cut_batch_into32(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm,
                        uint32_t *start, uint32_t *end, uint64_t cap, uint64_t *doc_tok, uint64_t *ntokens);

/* Token boundaries as two bitmaps over the batch's bytes instead of spans (2 bits per
 * input byte; 268 MB per GiB instead of 8 bytes per token): bit i of `starts` (word
 * i / 64, bit i % 64) is set when a token begins at byte doc_off[0] + i, bit i of
 * `ends` when a token's last byte is doc_off[0] + i.  Each array holds nwords >=
 * (doc_off[ndocs] - doc_off[0] + 63) / 64 u64 words, and every one of them is written.
 * Tokens never cross a document boundary and never overlap, so start bit k pairs
 * with end bit k in order; a 1-byte token whose byte is >= 0x80 is "�" (as for spans).
 * *ntokens receives the token count.  The host text moves to the device in pieces
 * while earlier pieces are cut and their masks come back (three streams). */
int jb_cut_batch_mask(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm,
                      uint64_t *starts, uint64_t *ends, uint64_t nwords, uint64_t *ntokens);

/* Pinned (page-locked) host memory for batch text: a batch that lies in one such
 * allocation is copied to the device straight from it, without the staging copy
 * that pageable memory needs.  A Go caller builds its CutBatch buffer here (C
 * memory, so cgo's pointer rules allow it).  Free with jb_host_free. */
int jb_host_alloc(size_t n, void **p);
void jb_host_free(void *p);

/* Device-resident form for pipelines and benchmarks: d_text (nbytes, plus 64
 * readable padding bytes; 16-byte aligned) and d_doc_off (ndocs+1 offsets, d_doc_off[0] == 0,
 * d_doc_off[ndocs] == nbytes) are device pointers on ctx's first device; the
 * work is queued on `stream` (a hipStream_t; NULL = default stream) and the
 * call returns without synchronising.  Calls on one ctx may come from several
 * threads and streams: each pipeline waits on the device for the previous one
 * (the workspace is one per device).  Results stay in ctx-owned device memory
 * only until the next call on this ctx, from any thread: *d_start / *d_end (u32
 * token spans), *d_doc_tok (u64[ndocs+1]) and *d_ntok (u64 token count).
 * Concurrent callers use jb_cut_device_into. */
int jb_cut_device(jb_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const uint64_t *d_doc_off,
                  uint32_t ndocs, int hmm, void *stream, uint32_t **d_start, uint32_t **d_end,
                  uint64_t **d_doc_tok, uint64_t **d_ntok);
/* jb_cut_device into caller-owned device arrays, which nothing else writes: d_start /
 * d_end hold cap >= nbytes u32 entries (a batch of n bytes has at most n tokens),
 * d_doc_tok ndocs+1 u64 and *d_ntok the u64 token count, all valid once `stream`
 * reaches the end of this call's work.  Safe from several threads on one ctx. */
int jb_cut_device_into(jb_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const uint64_t *d_doc_off,
                       uint32_t ndocs, int hmm, void *stream, uint32_t *d_start, uint32_t *d_end, uint64_t cap,
                       uint64_t *d_doc_tok, uint64_t *d_ntok);

/* ---- search mode (jieba's cut_for_search; the reference has only Cut) ------
 * The spans of Cut(doc, hmm), expanded.  For each token T = [s, e) of Cut's result, in
 * order, the output holds, all of them byte ranges of the input inside T's document:
 *  - T alone when T's first rune is not Han (a token of a non-Han block);
 *  - for a Han token whose n runes start at bytes p_0 < ... < p_{n-1}, p_n = e:
 *      n > 2: [p_i, p_{i+2}) for i = 0 .. n-2, ascending, where E(i, 2);
 *      n > 3: then [p_i, p_{i+3}) for i = 0 .. n-3, ascending, where E(i, 3);
 *      then T.
 *    E(i, L): buildDag (tokenizer.go:462-497) has the edge of L runes from rune i, that is
 *    termFreq[r_i] is found and not 0 (:468-471), every prefix r_i..r_{i+k}, k < L-1, is
 *    found (:476-478), and termFreq[r_i..r_{i+L-1}] > 0 (:479).
 * Tokens made by the HMM expand like dictionary tokens.  ntokens / *d_ntok and doc_tok
 * describe the expanded list; a token gives at most as many spans as it has bytes, so a
 * batch of n bytes has at most n spans.  Errors (JB_EPANIC included) are those of the plain
 * call.  jb_last_stats keeps reporting the plain counts (tokens = Cut's tokens).
 * Two deliberate differences from Python jieba's cut_for_search:
 *  - a gram that buildDag cannot see is not emitted: one whose first rune has frequency
 *    0, or (JB_DICT_TXT) one with a prefix that is not in the dictionary.  Cut could
 *    never produce that word either;
 *  - non-Han tokens are never expanded: the trie holds only all-Han keys, and the
 *    reference never consults the dictionary for non-Han blocks. */

/* jb_cut in search mode: one document. */
int jb_cut_search(jb_ctx *ctx, const uint8_t *text, size_t len, int hmm, jb_spans *out);
/* jb_cut_batch in search mode (arguments and ownership as jb_cut_batch). */
int jb_cut_batch_search(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm,
                        jb_spans *out);
/* jb_cut_device in search mode (arguments, limits, alignment and lifetime as jb_cut_device):
 * *d_start / *d_end / *d_doc_tok / *d_ntok are the expanded spans, their per-document
 * offsets and their count, in ctx-owned device memory until the next call on this ctx. */
int jb_cut_device_search(jb_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const uint64_t *d_doc_off,
                         uint32_t ndocs, int hmm, void *stream, uint32_t **d_start, uint32_t **d_end,
                         uint64_t **d_doc_tok, uint64_t **d_ntok);
/* jb_cut_device_into in search mode: the expanded spans into caller-owned device arrays of
 * cap >= nbytes u32 entries, d_doc_tok ndocs+1 u64 and *d_ntok the expanded count. */
int jb_cut_device_search_into(jb_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const uint64_t *d_doc_off,
                              uint32_t ndocs, int hmm, void *stream, uint32_t *d_start, uint32_t *d_end,
                              uint64_t cap, uint64_t *d_doc_tok, uint64_t *d_ntok);

/* ---- full mode (jieba's cut_all=True; the reference has only Cut) ------------
 * Every word the dictionary can find in the text, overlapping words included.  There is no
 * hmm argument: full mode never consults the HMM (the plain pipeline runs with hmm = 0).
 * For each splitText block of a document, in text order (tokenizer.go:165-210):
 *  - a non-Han block gives cutNonZh's tokens, exactly as Cut does (the reference never
 *    consults the dictionary there);
 *  - a Han block whose n runes start at bytes p_0 < ... < p_{n-1}, p_n = the block's end:
 *    let D(i) be the set of L such that buildDag (tokenizer.go:462-497) has the edge of L
 *    runes from rune i (1 is always in D(i): a rune that is absent or has count 0 has that
 *    edge alone, :468-471), and M(i) = D(i) \ {1}.  For i = 0 .. n-1 in order:
 *      M(i) not empty: [p_i, p_{i+L}) for each L in M(i), ascending (the one-rune word is
 *        not emitted);
 *      M(i) empty: [p_i, p_{i+1}), unless the nearest earlier rune i' < i of this block with
 *        M(i') not empty has i' + max M(i') > i.  Without such an i' the rune is emitted.
 *        Only the nearest such rune counts, not any rune whose word covers i (jieba's old_j,
 *        the end of the last word emitted).
 *    This is jieba's __cut_all loop restated.
 * The spans are ordered by start byte, then by end, and overlap.  ntokens / *d_ntok and
 * doc_tok describe this list; jb_last_stats keeps reporting the plain counts.  JB_EPANIC
 * cannot arise from the rule itself, but the plain run's errors pass through unchanged.
 * Three deliberate differences from Python jieba's cut_all:
 *  - the DAG is this reference's buildDag, with its gate on the first rune (:468-471) and
 *    its break at an absent prefix (:476-478);
 *  - non-Han text is cut by cutNonZh, not by jieba's re_skip splitting (and re_eng merging);
 *  - the Han class is unicode.Han, not [\u4E00-\u9FD5].
 * Size: a rune gives up to maxlen - 1 spans (maxlen: the longest word, jb_image_info), so a
 * batch of n bytes can give MORE than n spans.  The host calls always return the complete
 * list.  The device calls write the spans whose index is below the arrays' capacity and
 * count the rest: *d_ntok and d_doc_tok always describe the complete list, and
 * jb_device_status returns JB_ELIMIT when the count exceeded the capacity (the caller then
 * repeats the call with arrays of *d_ntok entries).  Counts are kept in 64 bits throughout. */

/* jb_cut in full mode: one document. */
int jb_cut_full(jb_ctx *ctx, const uint8_t *text, size_t len, jb_spans *out);
/* jb_cut_batch in full mode (arguments and ownership as jb_cut_batch). */
int jb_cut_batch_full(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, jb_spans *out);
/* jb_cut_device in full mode (arguments, limits, alignment and lifetime as jb_cut_device).
 * The ctx-owned *d_start / *d_end hold nbytes entries (capacity nbytes) and may be the arrays
 * of jb_cut_device_search: either result is valid until the next call on this ctx. */
int jb_cut_device_full(jb_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const uint64_t *d_doc_off,
                       uint32_t ndocs, void *stream, uint32_t **d_start, uint32_t **d_end, uint64_t **d_doc_tok,
                       uint64_t **d_ntok);
/* jb_cut_device_into in full mode: caller-owned device arrays of any capacity `cap` (u32
 * entries; spans with index >= cap are not written), d_doc_tok ndocs+1 u64, *d_ntok the
 * count of the complete list. */
int jb_cut_device_full_into(jb_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const uint64_t *d_doc_off,
                            uint32_t ndocs, void *stream, uint32_t *d_start, uint32_t *d_end, uint64_t cap,
                            uint64_t *d_doc_tok, uint64_t *d_ntok);

/* ---- token ids (the reference returns strings; a caller's next step numbers them) ------
 * Every span of a span list looked up in a vocabulary of the caller's own, on the device: an
 * embedding row, a term id, a stop-word flag.  The vocabulary is a list of byte strings, each
 * 1..255 bytes of any content; a key's id is its index in the list.  It is not the dictionary:
 * the trie holds only the all-Han keys buildDag can reach, so it cannot answer for "abc",
 * "2024", "，" or a word the HMM made, and a model's vocabulary is not the segmentation
 * dictionary.  The lookup is exact: the key's bytes are compared, not only their hash.
 *
 * The key of a span [s, e) is the bytes text[s..e), with one exception: a 1-byte span whose
 * byte is >= 0x80 (an invalid UTF-8 byte, which the reference emits as "�") is looked up as
 * EF BF BD.  The id is the key's index in the list, or JB_ID_UNK.
 *
 * jb_ids_device: d_start / d_end / d_ntok may be the ctx-owned results of any jb_cut_device*
 * call or the caller's own arrays (of any mode: plain, search, full).  d_text is the text the
 * spans index: nbytes bytes plus 64 readable padding bytes, as for jb_cut_device, 4-byte
 * aligned.  The call writes d_ids[k] for k < min(*d_ntok, cap) and nothing else; *d_ntok is read
 * on the device (in full mode it may exceed cap).  It queues one kernel on `stream` and returns:
 * it does not synchronise, allocate or read anything on the host, and it does not use the
 * per-device workspace, so it is safe from several threads and streams on one ctx (it holds the
 * ctx's shared lock only while queuing).  Queue it on the stream the spans were produced on, or
 * order the two streams yourself.
 * The spans are not trusted: one with start >= end or end > nbytes gets JB_ID_UNK without a
 * single text read (the kernel never reads outside [0, nbytes + 64)), and one longer than the
 * vocabulary's longest key gets JB_ID_UNK without its bytes being read (a 1 MB alnum run is one
 * token).
 *
 * jb_vocab_set builds the table, uploads it to ctx's first device and replaces any earlier one;
 * keys == NULL with nkeys == 0 removes it (keys != NULL with nkeys == 0 attaches an empty
 * vocabulary: every id is JB_ID_UNK).  It takes the exclusive lock and waits for all device work
 * queued earlier on that device before it releases the old table, as jb_add_word does for the
 * image.  On any error the old vocabulary stays attached.  The vocabulary is not part of
 * jb_save, and jb_add_word does not touch it.
 *
 * Errors: JB_EINVAL without a vocabulary attached, for an empty key, for key_off that is not
 * non-decreasing from 0 and for a duplicate key (the message names both indices); JB_ELIMIT for a
 * key over 255 bytes and for nbytes >= 2 GiB.  jb_spans_ids is the convenience path for host
 * spans: it uploads the byte range the spans cover and the spans as u32 to the first device,
 * runs the same kernel and copies the ids back (JB_ELIMIT when that range is 2 GiB or more). */
#define JB_ID_UNK 0xFFFFFFFFu
typedef struct jb_vocab jb_vocab;
/* Host only, no GPU needed (CPU tests): key i is keys[key_off[i] .. key_off[i+1]), key_off has
 * nkeys + 1 entries.  nkeys == 0 is a valid, empty vocabulary. */
int jb_vocab_build(const uint8_t *keys, const uint64_t *key_off, uint32_t nkeys, jb_vocab **out);
void jb_vocab_free(jb_vocab *v);
/* 1 found (*id set), 0 absent (*id = JB_ID_UNK): the device probe, on the host.  The bytes are
 * looked up as they are (the invalid-byte rule above belongs to spans). */
int jb_vocab_lookup(const jb_vocab *v, const uint8_t *tok, size_t len, uint32_t *id);
/* keys, longest key in bytes, slots of the table (a power of two >= 2 * nkeys) */
int jb_vocab_info(const jb_vocab *v, uint32_t *nkeys, uint32_t *maxlen, uint64_t *nslots);
int jb_vocab_set(jb_ctx *ctx, const uint8_t *keys, const uint64_t *key_off, uint32_t nkeys);
int64_t jb_vocab_size(jb_ctx *ctx); /* keys of the attached vocabulary; -1: none attached */
/* ids of a device span list */
int jb_ids_device(jb_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const uint32_t *d_start,
                  const uint32_t *d_end, const uint64_t *d_ntok, uint64_t cap, void *stream, uint32_t *d_ids);
/* ids of a host span list (any jb_spans the library returned for `text`): ids holds
 * spans->ntokens entries. */
int jb_spans_ids(jb_ctx *ctx, const uint8_t *text, const jb_spans *spans, uint32_t *ids);

/* ---- term counts and keywords (jieba.analyse.extract_tags; the reference has only Cut) ------
 * A document's distinct terms with their counts (the document-term matrix, as CSR), and the topk
 * terms of each document by count x weight, on the device: a caller who wants keywords never
 * pays for writing spans or ids back to the host.
 *
 * jb_terms_device.  d_ids is an id list of any mode (jb_ids_device's output or the caller's own)
 * with ids_cap valid entries; d_doc_tok (u64[ndocs + 1]) and d_ntok (u64, read on the device) are
 * those of the jb_cut_device* call whose spans the ids belong to.
 *  - Token k takes part iff k < min(*d_ntok, ids_cap) and d_ids[k] != JB_ID_UNK.  Document d's
 *    tokens are [doc_tok[d], doc_tok[d+1]) clamped to that bound (full mode's list may be longer
 *    than the id array).  doc_tok is non-decreasing.
 *  - Document d's terms are the distinct ids among its tokens, ascending by id, each with its
 *    count: d_term_id / d_term_cnt at [term_off[d], term_off[d+1]).  *d_nterms == term_off[ndocs].
 *  - Capacity, as in full mode: d_term_off (u64[ndocs + 1]) and *d_nterms always describe the
 *    complete list; entries with index >= cap are not written, and nothing else is written.
 *    cap = ids_cap is always enough.  There is no jb_device_status report: the caller checks
 *    *d_nterms <= cap.
 *  - The ids are not trusted: any u32 other than JB_ID_UNK is an id, and no table is indexed by
 *    it.  The call needs no vocabulary.
 *  - d_work is a caller-owned device buffer of nwork >= jb_terms_work_bytes(ids_cap, ndocs) bytes,
 *    8-byte aligned (JB_EINVAL otherwise, with nothing queued): two 8-byte entries per token of
 *    whole sort tiles of JB_TERMS_TILE tokens, plus 32 bytes per tile.  Its contents mean nothing
 *    before or after the call; concurrent calls need buffers of their own.
 *  - The call queues its kernels on `stream` and returns.  It does not synchronise, allocate,
 *    read anything on the host or use the per-device workspace, so it is safe from several
 *    threads and streams on one ctx, exactly like jb_ids_device.  The number of launches depends
 *    on ids_cap alone (4, and 2 per doubling of ids_cap / JB_TERMS_TILE), never on device data.
 *  - Counts are u32: a document has under 2^31 tokens, as batches are under 2 GiB.  JB_ELIMIT for
 *    ids_cap >= 2^32 - JB_TERMS_TILE.
 *
 * jb_keywords_device.  A CSR as above (with the cap it was written with), the caller's per-id
 * weight d_weight (f32[nweights]; IDF is one choice) and topk.
 *  - A term is a candidate iff id < nweights and weight[id] > 0: zero, negative and NaN weights
 *    exclude it, which is how a caller marks stop words and one-rune words.  +Inf is allowed.
 *  - score = (float)cnt * weight[id]: one f32 conversion (round to nearest even) and one f32
 *    multiply, bit-identical to numpy's np.float32(cnt) * w[id].  Products that are subnormal are
 *    outside what is pinned (the device may flush them).
 *  - Row d of d_kw_id / d_kw_score / d_kw_cnt (ndocs x topk each) holds the d_kw_n[d] =
 *    min(topk, candidates) best candidates by score descending, ties by id ascending; the remaining
 *    slots are JB_ID_UNK, 0.0f, 0.  Every slot of every row is written.
 *  - 1 <= topk <= JB_KW_MAXK: JB_EINVAL for 0, JB_ELIMIT above.  jieba's default is 20.
 *  - A CSR that overflowed its arrays (term_off[ndocs] > cap) is never read past cap: documents
 *    whose range passes cap get kw_n = 0.  The caller checks *d_nterms <= cap.
 *  - No vocabulary, allocation or synchronisation, as above: one kernel on `stream`.
 *
 * jb_keywords_batch: host text in, keywords out.  It runs plain Cut (extract_tags uses cut) ->
 * ids -> terms -> keywords on ctx's first device, uploads the text and the weights and copies
 * back only the ndocs x topk records and kw_n (and the token count, which sizes its buffers): no
 * span or id reaches the host.  It needs an
 * attached vocabulary (JB_EINVAL), a batch under 2 GiB (JB_ELIMIT) and doc_off non-decreasing;
 * it allocates and synchronises, like jb_spans_ids, and keeps its device buffers (about 9 bytes per
 * byte of text and 28 per token) for the next call, until jb_close; concurrent calls take turns.  It does not go through the piece /
 * multi-device pipeline of the jb_cut_batch* calls, because pieces may split a document, and it
 * uses one device.  Errors of the cut, JB_EPANIC included, pass through.
 *
 * Deliberate differences from jieba.analyse.extract_tags:
 *  - the vocabulary is closed: unknown tokens are not terms (jieba gives them the median IDF);
 *  - the score is not divided by the document's token total, a per-document constant that leaves
 *    the order unchanged (the caller has doc_tok);
 *  - the length and stop-word filters are the caller's zero weights;
 *  - ties are resolved by id, where jieba's order on ties is arbitrary. */
#define JB_KW_MAXK 64
#define JB_TERMS_TILE 4096
/* Host only, no ctx: non-decreasing in both arguments, never 0. */
size_t jb_terms_work_bytes(uint64_t max_tokens, uint32_t ndocs);
int jb_terms_device(jb_ctx *ctx, const uint32_t *d_ids, uint64_t ids_cap, const uint64_t *d_doc_tok,
                    const uint64_t *d_ntok, uint32_t ndocs, void *stream, uint32_t *d_term_id, uint32_t *d_term_cnt,
                    uint64_t cap, uint64_t *d_term_off, uint64_t *d_nterms, void *d_work, size_t nwork);
int jb_keywords_device(jb_ctx *ctx, const uint32_t *d_term_id, const uint32_t *d_term_cnt, const uint64_t *d_term_off,
                       uint32_t ndocs, uint64_t cap, const float *d_weight, uint32_t nweights, uint32_t topk,
                       void *stream, uint32_t *d_kw_id, float *d_kw_score, uint32_t *d_kw_cnt, uint32_t *d_kw_n);
/* kw_id / kw_score / kw_cnt: ndocs x topk host entries each; kw_n: ndocs. */
int jb_keywords_batch(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm,
                      const float *weights, uint32_t nweights, uint32_t topk, uint32_t *kw_id, float *kw_score,
                      uint32_t *kw_cnt, uint32_t *kw_n);

/* ---- document frequencies and IDF weights (the weight table extract_tags presupposes) ------
 * In how many documents each id occurs, and the IDF weight of each id from those counts, on the
 * device: a caller who cuts their own corpus with their own vocabulary fits the d_weight table of
 * jb_keywords_device here, and the chain "fit on the corpus, then rank every document" never
 * copies a token to the host.
 *
 * jb_df_device adds one batch's document frequencies into d_df (u32[ndf]).  d_term_id, d_nterms and
 * cap are the flat id list of a CSR as jb_terms_device wrote it: a row holds each of its
 * document's ids once, so the document frequency of an id is the number of entries that carry it.
 *  - Entry i takes part iff i < min(*d_nterms, cap) and d_term_id[i] < ndf.  *d_nterms is read on
 *    the device; cap is the capacity the CSR was written with.  An overflowed CSR is never read
 *    past cap: as before, the caller checks *d_nterms <= cap.
 *  - Each such entry does d_df[id] += 1.  Nothing else is written, in particular nothing at or past
 *    d_df[ndf].  The call accumulates: the caller zeroes d_df before the first batch, and counts
 *    that stay within u32 are the caller's bound.
 *  - The ids are not trusted: any u32 is an id, and ids >= ndf are skipped.
 *  - The rows are trusted to hold distinct ids.  A caller's own CSR with an id repeated in a row
 *    counts every entry.
 *  - The call needs no term_off, no vocabulary and no work buffer.
 *  - It queues one kernel on `stream` and returns, exactly like jb_ids_device: it does not
 *    synchronise, allocate, read anything on the host or use the per-device workspace, and it holds
 *    the ctx's shared lock only while queuing, so it is safe from several threads and streams.
 *  - The result is integer sums: identical whatever the order of the adds, and from run to run.
 *  - Errors: JB_EINVAL for a null pointer.  ndf == 0 is valid: nothing is added.
 *
 * jb_idf (host only, no ctx, no GPU) and jb_idf_device compute weight[id] (f32[ndf]) from df[id]
 * (u32[ndf]) by one rule, bit for bit:
 *  - weight[id] = 0.0f when df[id] == 0, when df[id] < min_df, when df[id] > max_df (JB_DF_NOMAX:
 *    no upper bound) or when keep != NULL and keep[id] == 0.  Zero is how jb_keywords_device leaves
 *    out stop words and one-rune words: max_df finds the corpus' own stop words, and keep (u8[ndf])
 *    carries the caller's length filter without a host pass over the weights.
 *  - Otherwise weight[id] = (float)(jb_go_log((double)(ndocs_total + 1) / (double)(df[id] + 1)) + 1.0),
 *    the sums taken in 64 bits: one f64 divide, Go's math.Log as jb_go_log restates it, one f64 add
 *    and one narrowing, round to nearest even.  It is scikit-learn's smoothed IDF.  No clamp is
 *    applied: df[id] > ndocs_total gives what the formula gives, and a weight <= 0 is no candidate
 *    downstream.
 *  - Every one of the ndf weights is written, and nothing else.
 *  - Errors: JB_ELIMIT for ndocs_total >= 2^53, where the conversion to f64 stops being exact;
 *    JB_EINVAL for a null pointer (keep may be NULL; ndf == 0 is valid).
 *  - jb_idf_device queues one kernel on `stream`, with the no-synchronisation contract above.
 *
 * jb_df_batch: host text in, the batch's document frequencies added to the caller's host array
 * df[ndf].  It runs plain Cut -> ids -> terms -> df on ctx's first device through the buffers
 * jb_keywords_batch keeps in the ctx (its ndf device counters are one more buffer that only
 * grows; concurrent calls take turns), copies ndf counters back and adds them to df.  Requirements
 * and errors are jb_keywords_batch's: an attached vocabulary (JB_EINVAL), a batch under 2 GiB
 * (JB_ELIMIT), doc_off non-decreasing, and the cut's errors pass through.  The caller sums ndocs
 * itself: ndocs_total of jb_idf is the number of documents of all batches.
 *
 * Deliberate differences from jieba's idf.txt and TFIDF:
 *  - the vocabulary is closed: there is no median IDF for unknown words;
 *  - the logarithm is Go's restatement (jb_go_log), so that the host rule and the device rule
 *    agree to the bit;
 *  - frequencies count the documents of the caller's batches, whatever "document" means to the
 *    caller (jieba's file was fitted on a corpus of its authors'). */
#define JB_DF_NOMAX 0xFFFFFFFFu
int jb_df_device(jb_ctx *ctx, const uint32_t *d_term_id, const uint64_t *d_nterms, uint64_t cap, uint32_t *d_df,
                 uint32_t ndf, void *stream);
int jb_idf_device(jb_ctx *ctx, const uint32_t *d_df, uint32_t ndf, uint64_t ndocs_total, uint32_t min_df,
                  uint32_t max_df, const uint8_t *d_keep, void *stream, float *d_weight);
/* host only, no ctx, no GPU: the same rule, and the reference the device kernel is pinned to */
int jb_idf(const uint32_t *df, uint32_t ndf, uint64_t ndocs_total, uint32_t min_df, uint32_t max_df,
           const uint8_t *keep, float *weight);
int jb_df_batch(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm, uint32_t *df,
                uint32_t ndf);

/* ---- TextRank keywords (jieba.analyse.textrank; the reference has only Cut) ------------------
 * A document's words ranked by PageRank over their co-occurrence graph, on the device: the second
 * entry point of jieba.analyse, which needs no corpus statistics (no fitted weight table).  Its
 * inputs are those of jb_terms_device and the CSR that call wrote; no token reaches the host.
 *
 * The rule.  jb_textrank (host only, no ctx, no GPU) and jb_textrank_device agree to the bit.
 *  - Id list: token k exists iff k < min(ntok, ids_cap) (the device reads *d_ntok on the device);
 *    document d's tokens are [doc_tok[d], doc_tok[d+1]) clamped to that bound; doc_tok is
 *    non-decreasing.
 *  - CSR of that list, as jb_terms_device wrote it: term_id, term_off (u64[ndocs + 1],
 *    non-decreasing) and the cap it was written with.  Both calls take the rows, they do not derive
 *    them; term_off[ndocs] is the term count, so *d_nterms is not an argument.
 *  - Kept tokens: token k is kept iff id != JB_ID_UNK, id < nkeep, keep[id] != 0 (keep: u8[nkeep])
 *    and the id is found in its document's CSR row, by binary search (rows are ascending).  A
 *    caller's own CSR that lacks the id makes the token not kept; nothing is indexed outside a row.
 *    Tokens that are not kept still occupy their position in the window, which is how jieba counts
 *    words that fail its pairfilter.
 *  - Events: a pair of kept tokens k < j of one document with j - k < span.  Each adds 1 to
 *    W[x_k][x_j] and 1 to W[x_j][x_k]; with x_k == x_j that is 2 in one cell (jieba's addEdge
 *    appends the self edge twice).  out[a] = sum_b W[a][b], kept in 64 bits.  A term is a node iff
 *    out > 0; n is the document's node count.
 *  - Scale: S = 62 - bit_length(n), so n * 2^S <= 2^62; sum ws <= n holds by induction from
 *    ws = 1/n, so no u64 sum below overflows.
 *  - Iteration: Jacobi, in f64, no fused multiply-add.  ws[a] = 1.0 / (double)n; then iters times,
 *    every ws of a round taken from the round before:
 *      r[a]   = (u64) trunc((ws[a] / (double)out[a]) * 2^S)
 *      acc[a] = sum_b W[a][b] * r[b]                              (u64 integer sum)
 *      ws[a]  = (1.0 - 0.85) + 0.85 * ((double)acc[a] * 2^-S)     ((double)acc: to nearest even)
 *    The sum is in integers on purpose: it does not depend on the order of its adds, so the device
 *    uses atomics and is still identical from run to run and identical to jb_textrank.
 *  - Score: mn and mx are the smallest and largest ws over the document's nodes;
 *    score = (float)((ws - mn / 10.0) / (mx - mn / 10.0)), jieba's normalisation.
 *  - Output: row d of kw_id / kw_score (ndocs x topk) holds the kw_n[d] = min(topk, n) best nodes
 *    by the f32 score descending, ties by id ascending; the remaining slots are JB_ID_UNK and 0.0f.
 *    Every slot of every row is written.  A document whose CSR row passes cap gets kw_n = 0, as in
 *    jb_keywords_device.
 *  - Limits: 2 <= span <= JB_TR_MAXSPAN (jieba: 5), 0 <= iters <= JB_TR_MAXITER (jieba: 10; with 0
 *    the ranks are the start values), 1 <= topk <= JB_KW_MAXK: JB_EINVAL below, JB_ELIMIT above, as
 *    the keyword calls.  JB_ELIMIT for ids_cap or cap >= 2^32 - JB_TERMS_TILE; JB_EINVAL for a null
 *    pointer (keep may be NULL when nkeep == 0).
 *
 * jb_textrank_device.  d_work is a caller-owned device buffer of nwork >=
 * jb_textrank_work_bytes(ids_cap, cap, ndocs) bytes, 8-byte aligned (JB_EINVAL otherwise, with
 * nothing queued): 6 bytes per token (its node and the reach of its window inside its document),
 * 28 per term (its document, out, r, acc) and 4 per document (n).  Its contents mean nothing
 * before or after the call; concurrent calls need buffers of their own.  The contract is
 * jb_terms_device's: the call queues its kernels on `stream` and returns; it does not synchronise,
 * allocate, read anything on the host or use the per-device workspace, and it holds the ctx's
 * shared lock only while queuing.  The number of launches is 4 + 2 * iters (2 when ids_cap or cap
 * is 0), never a matter of device data.  Nothing is written outside the outputs and d_work.
 * The push kernel has two forms with identical results (JB_TR_WINDOW, read at jb_open): 1 gathers
 * each token's r once into an LDS tile with a halo of span - 1 and combines a workgroup's adds to
 * one term before the global atomic (the default: 31.7 ms against 64.7 ms for the 139.5M tokens of
 * the 1 GiB corpus with jieba's arguments, beside 6.28 ms for the plain cut step and 4.86 ms for
 * jb_terms_device; profiles/textrank_bench.json); 0 gathers from memory and does one global atomic
 * per token.
 *
 * jb_textrank_batch: host text in, ndocs x topk records and kw_n out.  It runs plain Cut -> ids ->
 * terms -> textrank on ctx's first device through the buffers jb_keywords_batch keeps in the ctx
 * (the work buffer is one more that only grows; concurrent calls take turns).  Requirements and
 * errors are jb_keywords_batch's: an attached vocabulary (JB_EINVAL), a batch under 2 GiB
 * (JB_ELIMIT), doc_off non-decreasing, and the cut's errors pass through.
 *
 * Deliberate differences from jieba.analyse.textrank:
 *  - Jacobi rounds instead of jieba's in-place update in sorted-word order: the ranks are close
 *    (the top 20 were the same 20 words on seeded Zipf documents of 50, 2,000 and 20,000 tokens),
 *    the order is not promised to match;
 *  - the part-of-speech, length and stop-word filters are the caller's keep mask;
 *  - unknown ids are never nodes;
 *  - ties are broken by id;
 *  - fixed-point accumulation with resolution 2^-S: ws differs from plain f64 Jacobi by less than
 *    max(out) * 2^-S / (1 - 0.85). */
#define JB_TR_MAXSPAN 32
#define JB_TR_MAXITER 100
/* Host only, no ctx: non-decreasing in every argument, never 0. */
size_t jb_textrank_work_bytes(uint64_t max_tokens, uint64_t max_terms, uint32_t ndocs);
/* host only, no ctx, no GPU: the rule, and the reference the device kernels are pinned to */
int jb_textrank(const uint32_t *ids, uint64_t ids_cap, const uint64_t *doc_tok, uint64_t ntok, uint32_t ndocs,
                const uint32_t *term_id, const uint64_t *term_off, uint64_t cap, const uint8_t *keep, uint32_t nkeep,
                uint32_t span, uint32_t iters, uint32_t topk, uint32_t *kw_id, float *kw_score, uint32_t *kw_n);
int jb_textrank_device(jb_ctx *ctx, const uint32_t *d_ids, uint64_t ids_cap, const uint64_t *d_doc_tok,
                       const uint64_t *d_ntok, uint32_t ndocs, const uint32_t *d_term_id, const uint64_t *d_term_off,
                       uint64_t cap, const uint8_t *d_keep, uint32_t nkeep, uint32_t span, uint32_t iters,
                       uint32_t topk, void *stream, uint32_t *d_kw_id, float *d_kw_score, uint32_t *d_kw_n,
                       void *d_work, size_t nwork);
/* kw_id / kw_score: ndocs x topk host entries each; kw_n: ndocs. */
int jb_textrank_batch(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm,
                      const uint8_t *keep, uint32_t nkeep, uint32_t span, uint32_t iters, uint32_t topk,
                      uint32_t *kw_id, float *kw_score, uint32_t *kw_n);

/* ---- joined text (" ".join(cut(line)); the reference returns []string) ----------------------
 * The tokens of a span list written out as delimited text, on the device: one contiguous buffer of
 * keys, separators and document terminators, about nbytes + ntokens bytes that can go straight to a
 * file (word2vec / fastText input, an indexer), where a span list is 8 to 16 bytes per token that the
 * host still has to slice.  The output is a gather over a span list, not "the text with separators
 * inserted": search and full mode emit overlapping spans, and one rule serves all three modes.
 *
 * The rule.  jb_join (host only, no ctx, no GPU) and jb_join_device agree to the byte.
 *  - Inputs: text (nbytes bytes; on the device plus 64 readable padding bytes, as for jb_ids_device),
 *    spans start / end (u32) with capacity cap, doc_tok (u64[ndocs + 1], non-decreasing), ntok (the
 *    device reads *d_ntok on the device), sep (seplen bytes) and term (termlen bytes), each of 0 to
 *    JB_JOIN_MAXSEP bytes.
 *  - Token k exists iff k < min(ntok, cap).  Document d's tokens are [doc_tok[d], doc_tok[d+1])
 *    clamped to that bound: the clamps of jb_terms_device, so full mode's over-long list is handled
 *    the same way.  A token before doc_tok[0] or at or past doc_tok[ndocs] belongs to no document.
 *  - The key of span [s, e) follows the jb_ids_device rule: the bytes text[s..e); EF BF BD for a
 *    1-byte span whose byte is >= 0x80 (an invalid UTF-8 byte, the reference's "�").  The spans are
 *    not trusted: s >= e or e > nbytes gives an empty key, and no byte of it is read.  There is no
 *    upper length limit: a 1 MB alnum run is one token and is copied whole.
 *  - Document d's output is key_0 sep key_1 sep ... key_{n-1} term.  The separator stands between
 *    consecutive tokens only; the terminator follows every document, empty ones included (with n = 0
 *    the output is term alone).
 *  - out_doc_off (u64[ndocs + 1], out_doc_off[0] = 0) and nout = out_doc_off[ndocs] always describe
 *    the complete output.  Bytes with index >= out_cap are not written, and nothing else is written,
 *    in particular nothing at or past out[out_cap].  The caller checks nout <= out_cap (as in
 *    jb_terms_device, there is no jb_device_status report).
 *  - All offsets are 64 bits wide: full mode with replacement characters can pass 4 GiB.
 *  - Limits: JB_EINVAL for a null pointer (sep and term may be NULL when their length is 0; start,
 *    end and out when their capacity is 0); JB_ELIMIT for seplen or termlen above JB_JOIN_MAXSEP, for
 *    nbytes >= 2 GiB and for cap >= 2^32 - JB_JOIN_TILE.
 * For spans produced by the library's own cuts, a sep and term that are valid UTF-8 give valid UTF-8
 * output: every token is whole runes, ASCII, or a replaced invalid byte.
 *
 * jb_join_device.  The contract is jb_terms_device's: the call queues its kernels on `stream` and
 * returns; it does not synchronise, allocate, read anything on the host or use the per-device
 * workspace, and it holds the ctx's shared lock only while queuing, so it is safe from several threads
 * and streams on one ctx.  d_start / d_end / d_doc_tok / d_ntok may be the ctx-owned results of any
 * jb_cut_device* call or the caller's own arrays.  sep and term are host pointers and travel as kernel
 * arguments.  d_work is a caller-owned device buffer of nwork >= jb_join_work_bytes(cap, ndocs) bytes,
 * 8-byte aligned (JB_EINVAL otherwise, with nothing queued): 16 bytes per tile of JB_JOIN_TILE tokens,
 * 16 per document and 16 per 256 documents.  Its contents mean nothing before or after the
 * call; concurrent calls need buffers of their own.  The number of launches is 4, whatever cap, ndocs
 * and the device data are: k_join_count (per tile the sum of len(key) + seplen, per document the
 * offset of its first token inside its tile), k_join_scan (tiles and documents, one workgroup, no
 * waits between workgroups), k_join_doc (out_doc_off, *d_nout, every terminator) and k_join_write
 * (the keys and separators).
 * The write kernel has two forms with identical results (JB_JOIN_STAGE, read at jb_open).  0, the
 * plain form (the default): one lane per token, which finds its document by a search over doc_tok and
 * copies its key byte by byte.  1, the staged form: the workgroup assembles a tile's output in LDS,
 * 24 KiB at a time, and streams it out with 16-byte stores aligned to the output address; bytes that
 * do not fill an aligned 16-byte unit (a tile's head and tail, the bytes next to a terminator) are
 * stored one by one, never read-modify-written, and keys of JB_JOIN_LONG bytes or more bypass the
 * staging and are copied by the whole workgroup.  The plain form is the faster one for the 139.5M
 * plain-mode spans of the 1 GiB corpus (3.70 ms against 5.69 ms, beside 6.25 ms for the cut step;
 * profiles/join_bench.json) and ships; the staged form stays selectable.
 *
 * jb_cut_batch_join: host text in, joined text out.  It runs the cut of `mode` (JB_MODE_CUT,
 * JB_MODE_SEARCH, JB_MODE_FULL; hmm is ignored for JB_MODE_FULL), then the join, on ctx's first
 * device through the buffers jb_keywords_batch keeps in the ctx (the output buffer and the work buffer
 * are two more that only grow; concurrent calls take turns), and copies back nout, out_doc_off and the
 * nout bytes only: no span reaches the host.  In full mode, when the span list exceeds the kept span
 * arrays, it grows them and repeats the cut, as the host full-mode call does.  Requirements and errors
 * are jb_keywords_batch's minus the vocabulary: a batch under 2 GiB (JB_ELIMIT), doc_off
 * non-decreasing, and the cut's errors pass through, JB_EPANIC included; JB_EINVAL for an unknown
 * mode.  out->text (out->nbytes bytes) and out->doc_off (out->ndocs + 1) are the library's: release
 * them with jb_joined_free.  The text is page-locked host memory, so that the copy back runs at the
 * link's rate; pinning costs more than the call, so jb_joined_free keeps the largest block it was
 * handed (one per process, until a jb_close) and the next call takes it: release a result before
 * asking for the next one, and only the first call of a size pays for the pinning.
 *
 * Deliberate differences from " ".join(cut(line)) on the reference:
 *  - the separator and the terminator are the caller's, 0 to 8 bytes each;
 *  - whitespace and non-Han blocks without an alnum byte are absent, because the reference drops
 *    them (cutNonZh, tokenizer.go:289-310): the output is not the input with separators added. */
#define JB_JOIN_MAXSEP 8
#define JB_JOIN_TILE 2048 /* tokens per scan tile (one workgroup) */
#define JB_JOIN_LONG 256  /* a key of this many bytes or more takes the cooperative copy path */
#define JB_MODE_CUT 0
#define JB_MODE_SEARCH 1
#define JB_MODE_FULL 2
/* Host only, no ctx: non-decreasing in both arguments, never 0. */
size_t jb_join_work_bytes(uint64_t max_tokens, uint32_t ndocs);
/* host only, no ctx, no GPU: the rule, and the reference the device kernels are pinned to */
int jb_join(const uint8_t *text, uint64_t nbytes, const uint32_t *start, const uint32_t *end, const uint64_t *doc_tok,
            uint64_t ntok, uint64_t cap, uint32_t ndocs, const uint8_t *sep, uint32_t seplen, const uint8_t *term,
            uint32_t termlen, uint8_t *out, uint64_t out_cap, uint64_t *out_doc_off, uint64_t *nout);
int jb_join_device(jb_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const uint32_t *d_start,
                   const uint32_t *d_end, const uint64_t *d_doc_tok, const uint64_t *d_ntok, uint64_t cap,
                   uint32_t ndocs, const uint8_t *sep, uint32_t seplen, const uint8_t *term, uint32_t termlen,
                   void *stream, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_doc_off, uint64_t *d_nout,
                   void *d_work, size_t nwork);
typedef struct {
    uint8_t *text;     /* nbytes bytes: the documents' outputs, one after the other */
    uint64_t nbytes;
    uint64_t *doc_off; /* ndocs + 1: document d's output is text[doc_off[d] .. doc_off[d+1]) */
    uint32_t ndocs;
} jb_joined;
void jb_joined_free(jb_joined *j);
int jb_cut_batch_join(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm, int mode,
                      const uint8_t *sep, uint32_t seplen, const uint8_t *term, uint32_t termlen, jb_joined *out);

/* ---- character offsets (jieba's tokenize(): (word, start, end) in characters) -----------------
 * Every cut returns byte ranges of the UTF-8 input.  A Python caller holds str and slices by code
 * point; Lucene, Elasticsearch, Java, C# and JavaScript index text in UTF-16 code units.  These
 * calls turn a span list of any mode into spans in one of those units, per document, on the device:
 * a prefix count over the text and three lookups per token (the document's start, the span's start and its end).
 *
 * The rule.  jb_charspans (host only, no ctx, no GPU) and jb_charspans_device agree to the bit.
 *  - Runes.  Document d is text[doc_off[d] .. doc_off[d+1]).  It is decoded from its first byte by
 *    Go's utf8.DecodeRune with the document's end as the limit: a sequence cut short by the end of
 *    its document is invalid, and its lead byte is (U+FFFD, 1).  That gives the document's rune
 *    starts, each with a width and a value.
 *  - Units.  units(i) of a rune start i is 1 under JB_UNIT_RUNE; under JB_UNIT_UTF16 it is 2 for a
 *    valid rune >= U+10000 and 1 otherwise.  An invalid byte counts 1, as U+FFFD.
 *  - Position.  pos_d(p), doc_off[d] <= p <= doc_off[d+1], is the sum of units(i) over the rune
 *    starts i of document d with i < p.  A p inside a rune is allowed (a caller's own spans may have
 *    one): the rune that contains it is counted.
 *  - Tokens.  Token k exists iff k < min(ntok, cap), and belongs to document d iff doc_tok[d] <= k <
 *    doc_tok[d+1] (doc_tok u64[ndocs + 1]; the clamps of jb_join).  doc_tok must be non-decreasing for
 *    that; if it is not, every token is still written, some of them as JB_CHAR_NONE.  A token before
 *    doc_tok[0] or at or past doc_tok[ndocs] belongs to no document.
 *  - Per token: cstart[k] = pos_d(start[k]) and cend[k] = pos_d(end[k]) when doc_off[d] <= start[k] <=
 *    end[k] <= doc_off[d+1]; otherwise both are JB_CHAR_NONE (a malformed span, a span that leaves its
 *    document, a token of no document).  The spans, doc_tok and ntok are not trusted: no text byte
 *    outside [0, nbytes + 64) is read, every k < min(ntok, cap) is written in both arrays, and nothing
 *    else is written.
 *  - Per document: doc_units[d] = pos_d(doc_off[d+1]), the document's length in the unit (len(s) in
 *    Python, s.length() in Java), for all ndocs documents.
 *  - Offsets are per document, as jieba's tokenize gives them for one string.
 *  - In place: cstart may be the array start, and cend the array end; each token's two inputs are read
 *    before its two outputs are written.
 *  - Limits: JB_EINVAL for a null pointer (arrays of capacity 0 may be NULL) and for an unknown unit;
 *    the host form also rejects a decreasing doc_off, doc_off[0] != 0 and doc_off[ndocs] != nbytes.
 *    JB_ELIMIT for nbytes >= 2 GiB and for cap >= 2^32 - JB_JOIN_TILE.
 *
 * jb_charspans_device.  The contract is jb_join_device's: the call queues its kernels on `stream` and
 * returns; it does not synchronise, allocate, read anything on the host or use the per-device
 * workspace, and it holds the ctx's shared lock only while queuing.  d_text has nbytes bytes plus 64
 * readable padding bytes and is 4-byte aligned, as for jb_ids_device.  d_doc_off is the array the cut
 * was given and is trusted, as jb_cut_device trusts it.  d_start / d_end / d_doc_tok / d_ntok may be
 * the ctx-owned results of any jb_cut_device* call or the caller's own arrays.  d_work is a
 * caller-owned device buffer of nwork >= jb_charspans_work_bytes(nbytes, ndocs) bytes, 8-byte aligned
 * (JB_EINVAL otherwise, with nothing queued): per tile of JB_CHARSPANS_TILE text bytes 64 words of two
 * bitmaps (16 bytes) and a prefix (4 bytes) each, and 8 bytes of sums, about 0.31 bytes per text byte;
 * today it does not depend on ndocs.  Its contents mean nothing before or after the call; concurrent
 * calls need buffers of their own.  Nothing is written outside the outputs and d_work.
 * The number of launches is 3, whatever nbytes, ndocs, cap and the device data are: k_cs_class (per
 * tile the bitmap of rune starts, under JB_UNIT_UTF16 the bitmap of the starts that count 2, the unit
 * count before each 64-byte word inside the tile and the tile's sum; the document boundaries of a tile
 * come from two searches over d_doc_off), k_cs_scan (the tile sums, one workgroup, no waits between
 * workgroups) and k_cs_lookup (one lane per token: its document by a search over d_doc_tok, then
 * three positions; one lane per document writes doc_units).
 * Measured on the 1 GiB corpus (tools/charspans_bench.py, profiles/charspans_bench.json): the 139.5M
 * plain-mode spans take 2.61 ms in runes and 2.83 ms in UTF-16 units, beside 6.24 ms for the cut step
 * and 3.71 ms for jb_join_device in the same run; search mode's 223.7M spans 3.08 and 3.41 ms, full
 * mode's 320.4M spans 3.53 and 3.96 ms.  k_cs_class, which reads the text, takes 1.60 ms of each and
 * k_cs_scan 0.15 ms; the rest is the lookup, which grows with the span count.
 *
 * jb_cut_batch_charspans: host text in, character spans out, into caller-owned arrays (cstart, cend:
 * cap entries; doc_tok: ndocs + 1; doc_units: ndocs).  It runs the cut of `mode` (JB_MODE_CUT,
 * JB_MODE_SEARCH, JB_MODE_FULL; hmm is ignored for JB_MODE_FULL) and the conversion, in place on the
 * span arrays, on ctx's first device through the buffers jb_keywords_batch keeps in the ctx (the work
 * buffer is one more that only grows; concurrent calls take turns), and copies back the count, the two
 * u32 arrays, doc_tok and doc_units: no byte span reaches the host.  It does not use the multi-device
 * piece pipeline, because pieces may split a document and the offsets are per document.  The cap
 * protocol is jb_cut_batch_into32's: *ntokens is always the complete count, and JB_ELIMIT with
 * *ntokens set says that the arrays are too small (nothing but *ntokens is then written, and the
 * count is compared with cap after the first cut, before anything is grown or repeated).  In full
 * mode, when the span list fits cap but exceeds the kept span arrays, it grows them and repeats the
 * cut.  Other
 * requirements and errors are jb_cut_batch_join's: a batch under 2 GiB (JB_ELIMIT), doc_off
 * non-decreasing, JB_EINVAL for an unknown mode or unit, and the cut's errors pass through, JB_EPANIC
 * included. */
#define JB_UNIT_RUNE 0
#define JB_UNIT_UTF16 1
#define JB_CHAR_NONE 0xFFFFFFFFu
#define JB_CHARSPANS_TILE 4096 /* text bytes per tile (one workgroup) */
/* Host only, no ctx: non-decreasing in both arguments, never 0. */
size_t jb_charspans_work_bytes(uint64_t nbytes, uint32_t ndocs);
/* host only, no ctx, no GPU: the rule, and the reference the device kernels are pinned to */
int jb_charspans(const uint8_t *text, uint64_t nbytes, const uint64_t *doc_off, uint32_t ndocs, const uint32_t *start,
                 const uint32_t *end, const uint64_t *doc_tok, uint64_t ntok, uint64_t cap, int unit, uint32_t *cstart,
                 uint32_t *cend, uint32_t *doc_units);
int jb_charspans_device(jb_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const uint64_t *d_doc_off, uint32_t ndocs,
                        const uint32_t *d_start, const uint32_t *d_end, const uint64_t *d_doc_tok,
                        const uint64_t *d_ntok, uint64_t cap, int unit, void *stream, uint32_t *d_cstart,
                        uint32_t *d_cend, uint32_t *d_doc_units, void *d_work, size_t nwork);
int jb_cut_batch_charspans(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm, int mode,
                           int unit, uint32_t *cstart, uint32_t *cend, uint64_t cap, uint64_t *doc_tok,
                           uint64_t *ntokens, uint32_t *doc_units);

/* ---- word counts and vocabulary fitting: the distinct tokens of a corpus with their counts ----
 *
 * Everything above that numbers tokens needs a vocabulary the caller already has.  These calls make
 * one: distinct token strings with exact global counts are accumulated in a table on the device over
 * any number of batches, in any cut mode, and the much smaller result is read back sorted, ready for
 * jb_vocab_set (Counter(jieba.cut(text)), a min_count vocabulary).
 *
 * The rule.  jb_wc_count (host only, no ctx, no GPU) and the device table agree exactly.
 *  - Tokens.  Token k takes part iff k < min(ntok, cap).
 *  - Key.  A token's key is jb_ids_device's: the bytes text[start .. end); a 1-byte span whose byte is
 *    >= 0x80 is keyed as EF BF BD.
 *  - The spans are not trusted.  A span with start >= end or end > nbytes is bad, a key over 255 bytes
 *    is long; neither is read or counted, each adds to a total of its own (nbad, nlong).
 *  - Counts are u64, exact, independent of the order of the adds and the same from run to run.
 *  - Order.  Keys come by count descending, ties by key bytes ascending (memcmp, a proper prefix
 *    first).  min_count drops the keys below it, max_keys keeps the first max_keys of that order (0: all).
 *  - Accounting.  The counts of all keys before those two filters, plus nbad + nlong + ndropped +
 *    ncollided, are ntokens, the tokens that took part.  The five totals accumulate over the batches.
 *
 * The table is a caller-owned device buffer of jb_wc_table_bytes(nslots, pool_bytes) bytes, 32-byte
 * aligned: nslots (a power of two >= 8; JB_ELIMIT above 2^30) slots of a 64-bit fingerprint, a u64 count
 * and jb_vocab's 32-byte key slot, and pool_bytes (under 4 GiB) for the keys over 24 bytes.  New keys are
 * accepted while fewer than nslots / 2 slots are taken, so size nslots at four times the distinct keys
 * expected.  A token whose key finds no slot, or whose key of over 24 bytes finds no room in the pool,
 * is dropped (ndropped).  Two different keys with one 64-bit fingerprint share a slot: it keeps the key
 * whose first token comes earliest (an earlier batch before a later one), and every token of the other
 * key adds to ncollided and to no count, so a key is never credited with another key's tokens.  With
 * ndropped == 0 and ncollided == 0 the result is complete and exact; otherwise every reported count is
 * a lower bound on the true one.  The accounting holds in both cases.
 *
 * jb_wc_table_bytes and jb_wc_work_bytes are host only, non-decreasing in their arguments and never 0
 * (SIZE_MAX where the size does not fit; a slot count that is not valid is sized as the next valid one).
 *
 * jb_wc_init_device queues the kernel that empties a table (JB_EINVAL for a bad nslots, a null,
 * misaligned or short buffer).
 *
 * jb_wc_add_device adds one batch's spans, of any mode or a caller's own, with jb_terms_device's contract:
 * it queues on `stream` and returns without synchronising, allocating, reading on the host or using
 * the per-device workspace, and takes the shared lock only while queuing.  There are three launches,
 * or none when cap is 0, whatever the data, and no lane ever waits for another.  d_text is 4-byte
 * aligned and readable 64 bytes past nbytes; d_ntok is a device u64; d_work holds
 * jb_wc_work_bytes(cap) bytes (4 per token), 4-byte aligned; d_table is 32-byte aligned and ntable at
 * least jb_wc_table_bytes(8, 0): JB_EINVAL otherwise, with nothing queued.  JB_ELIMIT for nbytes >=
 * 2 GiB or cap >= 2^32 - 256.  No vocabulary is needed.  A buffer that jb_wc_init_device did not
 * fill, or an ntable below what its table needs, is left untouched by the kernels; jb_wc_read then
 * says so.  The count pass has two forms with identical results (JB_WC_COMBINE, read at jb_open): 0
 * is one global atomic per token, 1 (the default) combines a workgroup's adds to a slot in LDS first.
 * JB_WC_HASHBITS (read at jb_open, default 64) keeps only that many low bits of the hash in the
 * fingerprint, so that a test can make keys collide; jb_wc_fp (host only) is the fingerprint of a key
 * of 1 .. 255 bytes at that width (0 for arguments outside that).
 *
 * jb_wc_read synchronises `stream`, copies the table to the host, and sorts and filters there (the
 * distinct keys are orders of magnitude fewer than the tokens).  The table is left unchanged, so
 * reading part-way through is allowed.  JB_EINVAL when the buffer holds no table.  jb_wc_result_free
 * frees the arrays (malloc'd) and zeroes the struct.
 *
 * jb_wc_batch: host text in.  It uploads, cuts in `mode` (JB_MODE_*; hmm is ignored for
 * JB_MODE_FULL) on ctx's first device and adds to the table, through the buffers jb_keywords_batch
 * keeps in the ctx; concurrent calls take turns.  Requirements and errors are jb_keywords_batch's minus
 * the vocabulary, and JB_EINVAL for an unknown mode.  It returns when the batch is in the table.
 *
 * jb_device_alloc / jb_device_free: n bytes of device memory on ctx's first device (256-byte aligned),
 * for a caller that has no binding to the HIP runtime of its own, such as the C++ and Go Tokenizers'
 * WordCounts, to keep a table in.  JB_ENOMEM when the device has no room; jb_device_free waits for the
 * device work that uses the block, and ignores NULL. */
typedef struct jb_wc_result {
    uint8_t *keys;      /* the keys back to back, in the rule's order */
    uint64_t *key_off;  /* nkeys + 1: key i is keys[key_off[i] .. key_off[i+1]) */
    uint64_t *counts;   /* nkeys */
    uint64_t nkeys;
    uint64_t nbad, nlong, ndropped, ncollided, ntokens;
} jb_wc_result;

size_t jb_wc_table_bytes(uint64_t nslots, uint64_t pool_bytes);
size_t jb_wc_work_bytes(uint64_t max_tokens);
uint64_t jb_wc_fp(const uint8_t *key, size_t len, uint32_t bits);
int jb_wc_init_device(jb_ctx *ctx, void *d_table, size_t ntable, uint64_t nslots, uint64_t pool_bytes, void *stream);
int jb_wc_add_device(jb_ctx *ctx, void *d_table, size_t ntable, const uint8_t *d_text, uint64_t nbytes,
                     const uint32_t *d_start, const uint32_t *d_end, const uint64_t *d_ntok, uint64_t cap,
                     void *stream, void *d_work, size_t nwork);
int jb_wc_read(jb_ctx *ctx, const void *d_table, size_t ntable, void *stream, uint64_t min_count, uint64_t max_keys,
               jb_wc_result *out);
void jb_wc_result_free(jb_wc_result *r);
int jb_wc_count(const uint8_t *text, uint64_t nbytes, const uint32_t *start, const uint32_t *end, uint64_t ntok,
                uint64_t cap, uint64_t min_count, uint64_t max_keys, jb_wc_result *out);
int jb_wc_batch(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm, int mode,
                void *d_table, size_t ntable);
int jb_device_alloc(jb_ctx *ctx, size_t n, void **p);
void jb_device_free(jb_ctx *ctx, void *p);

/* ---- MinHash signatures: near-duplicate document sketches ------------------------------------
 *
 * The step that corpus pipelines run right after a cut: shingles of n consecutive words, a MinHash
 * signature of K u32 slots per document, LSH band keys.  Two documents agree in a slot with the
 * probability of their shingle sets' Jaccard similarity.  The signature is computed on the device from
 * the span list the cut left there: no token reaches the host, and ndocs * K * 4 bytes come back.
 *
 * The rule.  jb_minhash (host only, no ctx, no GPU) and jb_minhash_device agree to the bit.  All
 * arithmetic is unsigned and modulo 2^64 unless a width is stated.
 *  - Tokens and documents.  The clamps are jb_join's: token k exists iff k < min(ntok, cap); document
 *    d's tokens are [doc_tok[d], doc_tok[d+1]) clamped to that bound, m_d of them.  A token before
 *    doc_tok[0] or at or past doc_tok[ndocs] belongs to no document.  doc_tok is trusted to be
 *    non-decreasing; if it is not, the affected documents' values are unspecified, but still nothing
 *    outside the outputs and the work buffer is written and no text byte outside [0, nbytes + 64) read.
 *  - Token hash t_k.  The key is jb_ids_device's: the bytes text[s..e); a 1-byte span whose byte is
 *    >= 0x80 is keyed as EF BF BD.  The spans are not trusted: s >= e or e > nbytes gives the empty
 *    key (length 0, no byte read), as in jb_join.  A key longer than 255 bytes is cut to its first 255
 *    bytes (bytes are bytes: the cut may fall inside a rune).  t_k is the vocabulary's hash of the key
 *    (jb_vocab_build's table hash): h = 0x243F6A8885A308D3 ^ (len * 0xFF51AFD7ED558CCD); for every 8-byte
 *    little-endian word w of the key, zero-padded (at least one word, so the empty key mixes one 0):
 *    h = (h ^ w) * 0x9E3779B97F4A7C15, h ^= h >> 32 ("mix"); last h *= 0xD6E8FEB86659FD93, h ^= h >> 32
 *    ("fin").  The first term, with c in place of len, is "init(c)" below.
 *  - Shingles of width n, 1 <= n <= JB_MH_MAXN.  A document with m >= n has the shingles i = 0 .. m - n
 *    over its tokens i .. i + n - 1; one with 0 < m < n has one shingle over all its m tokens; one
 *    with m = 0 has none.  With c the number of tokens folded, the shingle's hash is g = init(c), then
 *    g = mix(g, t) for each token in order, then s = fin(g).  A shingle never crosses a document
 *    boundary.  doc_n[d] (u32) is the document's shingle count: 0, 1 or m - n + 1.
 *  - Hash functions, 1 <= K <= JB_MH_MAXK, from a u64 seed by splitmix64: st += 0x9E3779B97F4A7C15,
 *    z = st, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB,
 *    next = z ^ z >> 31.  From st = seed the values are drawn in the order a_0, b_0, a_1, b_1, ... with
 *    a_j = next() | 1 and b_j = next().  jb_minhash_params (host only) returns them, so that a caller
 *    can sketch a query document elsewhere.
 *  - Signature.  x_i = (uint32_t)s_i, and sig[d * K + j] is the least, over the document's shingles,
 *    of (uint32_t)((a_j * (uint64_t)x_i + b_j) >> 32): multiply-shift hashing.  A document without
 *    shingles has JB_MH_EMPTY in every slot.  Every one of the ndocs * K slots and ndocs counts is
 *    written, and nothing else.
 *  - Band keys.  jb_minhash_bands (host) and jb_minhash_bands_device turn signatures into LSH bucket
 *    keys: B bands of R rows, B * R <= K.  key[d * B + b] (u64) is g = mix(init(R), b), then
 *    g = mix(g, sig[d * K + b * R + r]) for r = 0 .. R - 1, then fin(g).  A document with doc_n[d] == 0
 *    gets JB_MH_NOKEY in every band, so that empty documents never bucket together; a computed key
 *    equal to JB_MH_NOKEY is stored as JB_MH_NOKEY - 1.
 *  - Limits: JB_EINVAL for a null pointer (arrays of capacity 0 may be NULL), for n, K, B or R = 0 and
 *    for B * R > K; JB_ELIMIT for n or K above the maxima, for nbytes >= 2 GiB and for
 *    cap >= 2^32 - JB_MH_TILE.
 *
 * jb_minhash_device.  The contract is jb_join_device's: the call queues its kernels on `stream` and
 * returns; it does not synchronise, allocate, read anything on the host or use the per-device
 * workspace, and it holds the ctx's shared lock only while queuing.  d_text has nbytes bytes plus 64
 * readable padding bytes and is 4-byte aligned, as for jb_ids_device.  d_start / d_end / d_doc_tok /
 * d_ntok may be the ctx-owned results of any jb_cut_device* call, of any mode, or the caller's own.
 * d_work is a caller-owned device buffer of nwork >= jb_minhash_work_bytes(cap, ndocs) bytes, 8-byte
 * aligned (JB_EINVAL otherwise, with nothing queued): 8 bytes per token, the token hashes; today it
 * does not depend on ndocs.  The helper is host only, non-decreasing in both arguments and never 0.
 * The number of launches is 3, whatever the device data are (1, k_mh_init alone, when cap or ndocs is
 * 0): k_mh_init (every slot JB_MH_EMPTY, doc_n from doc_tok alone), k_mh_hash (one lane per token: the
 * key from aligned dwords, t_k into d_work) and k_mh_sig (the minima, by u32 atomicMin; a minimum does
 * not depend on the order, so the bits are the same from run to run).  No lane waits for another.
 * k_mh_sig has two forms with identical bits (JB_MH_FORM, read at jb_open).  0, the plain form: one
 * lane per token finds its document by a search over doc_tok, folds its shingle from d_work and walks
 * the K functions, with an atomicMin only where its value is below what a load of the slot shows.  1,
 * the staged form (the default): one workgroup per tile of JB_MH_TILE tokens loads the tile's hashes
 * and a halo of n - 1 into LDS, folds each shingle once, and every lane owns one hash function for a
 * share of the tile: it keeps a running minimum per run of one document and flushes it with one
 * atomicMin per (tile share, document run, function).
 * Measured on the 1 GiB corpus (tools/minhash_bench.py, profiles/minhash_bench.json; 73,443 documents):
 * the 139.5M plain-mode spans at n = 5, K = 128 take 6.41 ms staged against 344.0 ms plain, beside
 * 6.23 ms for the cut step and 9.08 ms for jb_wc_add_device in the same run (k_mh_hash 0.67 ms, k_mh_sig
 * 5.41 ms); at n = 1, K = 64, 3.90 against 195.7 ms.  Search mode's 223.7M spans: 10.16 and 6.24 ms
 * staged; full mode's 320.4M spans: 14.19 and 8.74 ms.  The two forms' bits were identical in every
 * mode and shape, and those of the plain-mode spans were jb_minhash's over the whole corpus.  The
 * staged form ships.  From pageable host memory jb_minhash_batch takes 35.61 ms for the 1 GiB beside
 * 29.98 ms for jb_cut_batch_into32.
 *
 * jb_minhash_bands_device: one kernel, one lane per (document, band), the same contract.
 *
 * jb_minhash_batch: host text in.  It uploads, cuts in `mode` (JB_MODE_*; hmm is ignored for
 * JB_MODE_FULL) and sketches on ctx's first device, through the buffers jb_keywords_batch keeps in the
 * ctx (one more, for the work buffer and the signatures, that only grows; concurrent calls take
 * turns), and copies back only sig (ndocs * K u32) and doc_n (ndocs u32).  Requirements and errors are
 * jb_wc_batch's; in full mode, when the span list exceeds the kept span arrays, it grows them and
 * repeats the cut.  It does not use the multi-device piece pipeline, because pieces may split a
 * document.
 *
 * Deliberate differences from the usual datasketch recipe:
 *  - 32-bit multiply-shift hashing instead of a hash modulo a Mersenne prime;
 *  - the shingles are runs of jieba words, not character n-grams;
 *  - keys are cut at 255 bytes;
 *  - a document shorter than n words has one shingle over all its words, not none. */
#define JB_MH_MAXN 8
#define JB_MH_MAXK 256
#define JB_MH_TILE 1024 /* tokens per tile of the staged form (one workgroup) */
#define JB_MH_EMPTY 0xFFFFFFFFu
#define JB_MH_NOKEY 0xFFFFFFFFFFFFFFFFull
/* Host only, no ctx: non-decreasing in both arguments, never 0. */
size_t jb_minhash_work_bytes(uint64_t max_tokens, uint32_t ndocs);
/* host only: a[K], b[K] of `seed` */
int jb_minhash_params(uint64_t seed, uint32_t K, uint64_t *a, uint64_t *b);
/* host only, no ctx, no GPU: the rule, and the reference the device kernels are pinned to */
int jb_minhash(const uint8_t *text, uint64_t nbytes, const uint32_t *start, const uint32_t *end, const uint64_t *doc_tok,
               uint64_t ntok, uint64_t cap, uint32_t ndocs, uint32_t n, uint32_t K, uint64_t seed, uint32_t *sig,
               uint32_t *doc_n);
int jb_minhash_bands(const uint32_t *sig, const uint32_t *doc_n, uint32_t ndocs, uint32_t K, uint32_t B, uint32_t R,
                     uint64_t *keys);
int jb_minhash_device(jb_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const uint32_t *d_start,
                      const uint32_t *d_end, const uint64_t *d_doc_tok, const uint64_t *d_ntok, uint64_t cap,
                      uint32_t ndocs, uint32_t n, uint32_t K, uint64_t seed, void *stream, uint32_t *d_sig,
                      uint32_t *d_doc_n, void *d_work, size_t nwork);
int jb_minhash_bands_device(jb_ctx *ctx, const uint32_t *d_sig, const uint32_t *d_doc_n, uint32_t ndocs, uint32_t K,
                            uint32_t B, uint32_t R, void *stream, uint64_t *d_keys);
/* sig: ndocs x K host entries; doc_n: ndocs. */
int jb_minhash_batch(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm, int mode,
                     uint32_t n, uint32_t K, uint64_t seed, uint32_t *sig, uint32_t *doc_n);

/* ---- Token filtering: stop words, classes and lengths ----------------------------------------
 *
 * `[w for w in jieba.cut(s) if w not in stopwords and len(w) > 1]`: a span list of any mode becomes a
 * shorter span list of the same shape (u32 starts and ends, u64 per-document offsets, a count), so that
 * every consumer of a span list (jb_ids_device, jb_join_device, jb_wc_add_device, jb_minhash_device,
 * jb_charspans_device) works on the result unchanged.  No token reaches the host.
 *
 * The rule.  jb_filter (host only, no ctx, no GPU) and jb_filter_device agree exactly, on every output.
 *  - Tokens.  Token k takes part iff k < nt = min(ntok, cap): jb_join's clamps (full mode's list may be
 *    longer than its arrays).
 *  - Key.  jb_ids_device's: the bytes text[s..e); EF BF BD for a 1-byte span whose byte is >= 0x80.
 *  - Bad spans.  The spans are not trusted.  A span with s >= e or e > nbytes is bad: it is never kept
 *    and none of its bytes is read.
 *  - Class.  Every other token has one class, decided from its own bytes only:
 *      JB_TC_INVALID  one byte, and that byte is >= 0x80;
 *      JB_TC_NUM      the first byte is ASCII [0-9A-Za-z], the key has at most 255 bytes, and all of
 *                     them are ASCII digits;
 *      JB_TC_ALNUM    every other key whose first byte is ASCII [0-9A-Za-z]; a key over 255 bytes is
 *                     ALNUM without being scanned (a 1 MB run is one token);
 *      JB_TC_HAN      the first rune is Han (Unicode 13 Script=Han, the cut kernels' class, the
 *                     reference's `zh`, tokenizer.go:21); the rune is decoded by Go's utf8.DecodeRune over
 *                     [s, e), so a sequence cut short by e is (U+FFFD, 1) and not Han;
 *      JB_TC_OTHER    everything else: punctuation, symbols, kana, hangul and other scripts, which the
 *                     reference emits one rune at a time (cutNonZh, tokenizer.go:289-310).  This is a
 *                     deliberate limit: there are no Unicode category tables here.
 *  - Length.  runes(k) is the number of key bytes that are not 10xxxxxx, saturating at 256.  A key
 *    longer than 1024 bytes counts 256 without being read, so no token costs more than 1024 byte reads
 *    (valid UTF-8 has at least 256 runes in 1024 bytes; only a malformed span can tell the difference).
 *    INVALID counts 1.  min_runes and max_runes are at most 255 (JB_ELIMIT above that); max_runes == 0
 *    means no upper bound.  Counting may stop as soon as the answer is decided.
 *  - Stop words.  With JB_FILTER_STOP in the rule's flags a token is a stop word iff its key is found
 *    in the stop set: an exact byte comparison, the vocabulary table's lookup.  A key longer than the
 *    set's longest key is not read for it.
 *  - Decision.  A token gets the first reason that applies, in this order: bad; class (drop_classes has
 *    the class's bit); length (runes < min_runes, or max_runes && runes > max_runes); stop.  With no
 *    reason it is kept.  The stop probe comes last because it costs the most.
 *  - Output.  The kept tokens come in their original order as out_start and out_end (u32).  out_src, a
 *    u32 array that may be NULL, receives the index of each kept token's source token; with it a caller
 *    gathers ids or anything else.  With R(i) the number of kept tokens whose source index is below i,
 *    out_doc_tok[d] = R(min(doc_tok[d], nt)) for d = 0 .. ndocs (u64) and *out_ntok = R(nt).  Entries
 *    with index >= out_cap are not written, and nothing else is written; out_cap = cap is always enough,
 *    and the caller checks *out_ntok <= out_cap, as for jb_terms_device.  Outputs must not alias inputs
 *    or each other: equal pointers return JB_EINVAL.
 *  - Statistics.  stats[5] (u64) is written, not accumulated: ntokens (= nt), nbad, nclass, nlength,
 *    nstop.  ntokens == *out_ntok + nbad + nclass + nlength + nstop always holds.  All values are
 *    integer sums, so they are the same from run to run.
 *  - Errors.  JB_EINVAL: a null pointer (arrays of capacity 0 may be NULL), unknown flag or class bits,
 *    JB_FILTER_STOP without a stop set.  JB_ELIMIT: min_runes or max_runes above 255, nbytes >= 2 GiB,
 *    cap >= 2^32 - JB_FILTER_TILE.
 *
 * The stop set.  jb_stopwords_set(ctx, keys, key_off, nkeys) attaches the caller's stop list, in
 * jb_vocab_set's format and under its contract in every respect: it is built aside and takes the
 * exclusive lock, it waits for queued device work before the old table is released, NULL with 0 keys
 * removes the set, and on any error the old set stays.  It is a second table beside the id vocabulary,
 * with its device copy on the first device; the ids are unused.  It is independent of jb_vocab_set, it
 * is not part of jb_save, and jb_add_word does not touch it.  jb_stopwords_size: the number of keys, or
 * -1 without a set.  The host rule takes a `const jb_vocab *stop` (may be NULL) from jb_vocab_build.
 *
 * jb_filter_device.  The contract is jb_join_device's: the call queues its kernels on `stream` and
 * returns; it does not synchronise, allocate, read anything on the host or use the per-device
 * workspace, and it holds the ctx's shared lock only while queuing.  d_text has nbytes bytes plus 64
 * readable padding bytes and is 4-byte aligned, as for jb_ids_device.  d_work is a caller-owned device
 * buffer of nwork >= jb_filter_work_bytes(cap, ndocs) bytes, 8-byte aligned (JB_EINVAL otherwise, with
 * nothing queued): one bit per token and about 40 bytes per tile of JB_FILTER_TILE tokens.  The helper
 * is host only, non-decreasing in both arguments and never 0.  There are three launches whatever the
 * data; when cap == 0 there is none, only the memsets that zero out_doc_tok, *out_ntok and stats.  No
 * lane waits for another, and there are no global atomics.
 *   k_filt_mark   one lane per token: the key from aligned dwords (jb_ids_device's reads), the decision;
 *                 a wave ballot writes each wave's 64-bit keep word into d_work, and ballots of the four
 *                 reasons give the tile's counts.
 *   k_filt_scan   one workgroup, looping over the tiles: exclusive tile prefixes, the five totals,
 *                 *out_ntok and stats.
 *   k_filt_write  per tile, a kept token's rank is the tile's prefix, plus the popcounts of the tile's
 *                 earlier words, plus the popcount of the lane's own word below the lane; it writes
 *                 out_start, out_end and out_src below out_cap.  ndocs + 1 further lanes compute
 *                 out_doc_tok[d] from the same bitmap and prefixes.
 * Measured on the 1 GiB corpus (tools/filter_bench.py, profiles/filter_bench.json; 73,443 documents) with
 * the rule drop = OTHER | INVALID, min_runes = 2, JB_FILTER_STOP against 1,000 stop keys: the 139.5M
 * plain-mode spans take 2.96 ms (53.5M kept; k_filt_mark 2.49 ms, k_filt_scan 0.14 ms, k_filt_write
 * 0.34 ms), beside 6.26 ms for the cut step, 2.61 ms for jb_charspans_device and 3.73 ms for
 * jb_join_device in the same run; with the class test alone 1.29 ms.  Search mode's 223.7M spans: 4.67
 * and 1.98 ms; full mode's 320.4M spans: 6.78 and 2.80 ms.  The plain-mode outputs were jb_filter's over
 * the whole corpus.  jb_join_device on the filtered list takes 1.78 ms against 3.73 ms.  From pageable
 * host memory jb_cut_batch_join with the batch filter set takes 40.2 ms for the 1 GiB against 51.4 ms
 * without it.
 *
 * jb_cut_batch_filter: host text in, the filtered u32 byte spans (relative to doc_off[0]) out, under
 * jb_cut_batch_into32's cap protocol on the filtered count: *ntokens is always the filtered count, and
 * when it exceeds cap the call returns JB_ELIMIT and nothing but *ntokens and stats is written.
 * It uploads, cuts in `mode` and filters on ctx's first device, through the buffers jb_keywords_batch
 * keeps in the ctx (one more, that only grows; concurrent calls take turns); in full mode, when the
 * span list exceeds the kept span arrays, it grows them and repeats the cut.  stats may be NULL.
 *
 * jb_batch_filter_set(ctx, rule) stores a rule in the ctx (NULL clears it).  While one is set,
 * jb_cut_batch_join, jb_wc_batch and jb_minhash_batch run the filter between their cut and their own
 * step.  With none set, the default, those calls queue exactly the work they queued before this call
 * existed.  jb_cut_batch_charspans and the id-based batch calls (which have weights and keep masks)
 * are deliberately left alone.  A rule with JB_FILTER_STOP needs a stop set at the time of the batch
 * call, which fails with JB_EINVAL otherwise. */
#define JB_TC_HAN 1u
#define JB_TC_ALNUM 2u
#define JB_TC_NUM 4u
#define JB_TC_OTHER 8u
#define JB_TC_INVALID 16u
#define JB_FILTER_STOP 1u
#define JB_FILTER_TILE 2048 /* tokens per tile (one workgroup) */
typedef struct {
    uint32_t flags, drop_classes, min_runes, max_runes;
} jb_filter_rule;
int jb_stopwords_set(jb_ctx *ctx, const uint8_t *keys, const uint64_t *key_off, uint32_t nkeys);
int64_t jb_stopwords_size(jb_ctx *ctx);
/* Host only, no ctx: non-decreasing in both arguments, never 0. */
size_t jb_filter_work_bytes(uint64_t max_tokens, uint32_t ndocs);
/* host only, no ctx, no GPU: the rule, and the reference the device kernels are pinned to */
int jb_filter(const uint8_t *text, uint64_t nbytes, const uint32_t *start, const uint32_t *end, const uint64_t *doc_tok,
              uint64_t ntok, uint64_t cap, uint32_t ndocs, const jb_filter_rule *rule, const jb_vocab *stop,
              uint32_t *out_start, uint32_t *out_end, uint32_t *out_src, uint64_t out_cap, uint64_t *out_doc_tok,
              uint64_t *out_ntok, uint64_t *stats);
int jb_filter_device(jb_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const uint32_t *d_start, const uint32_t *d_end,
                     const uint64_t *d_doc_tok, const uint64_t *d_ntok, uint64_t cap, uint32_t ndocs,
                     const jb_filter_rule *rule, void *stream, uint32_t *d_out_start, uint32_t *d_out_end,
                     uint32_t *d_out_src, uint64_t out_cap, uint64_t *d_out_doc_tok, uint64_t *d_out_ntok,
                     uint64_t *d_stats, void *d_work, size_t nwork);
/* start / end: cap host entries; doc_tok: ndocs + 1; stats: 5 entries or NULL. */
int jb_cut_batch_filter(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm, int mode,
                        const jb_filter_rule *rule, uint32_t *start, uint32_t *end, uint64_t cap, uint64_t *doc_tok,
                        uint64_t *ntokens, uint64_t *stats);
int jb_batch_filter_set(jb_ctx *ctx, const jb_filter_rule *rule);

/* ---- postings (the inverted index; jieba ships a Whoosh ChineseAnalyzer, jieba/analyse/analyzer.py, and
 * leaves the index to Whoosh; the reference has only Cut) -----------------------------------------------
 * The document-term matrix of jb_terms_device by columns: per id, the documents that contain it, ascending,
 * each with its term frequency, on the device.  It replaces copying the CSR to the host and sorting it there
 * (np.argsort(kind="stable") over the flat id list), the last step of an indexer after search-mode cutting,
 * UTF-16 offsets, the token filter and the vocabulary lookup.
 *
 * The rule (jb_postings on host arrays, jb_postings_device on device arrays: one rule, bit for bit).  Inputs:
 * a CSR as jb_terms_device writes it, term_id / term_cnt / term_off (u64[ndocs + 1]) / nterms and the cap it
 * was written with; nids, the index has one list per id below nids; doc_base (u32), added to every document
 * number.  Let n = min(nterms, cap, term_off[ndocs]).
 *  - Entry i takes part iff i < n and term_id[i] < nids.  This is jb_df_device's rule: the ids are not
 *    trusted and no table is indexed by an id >= nids.
 *  - Its document is doc_base + d, where d is the row with term_off[d] <= i < term_off[d + 1].  term_off is
 *    trusted to be non-decreasing from 0; with a caller's own broken offsets the documents are unspecified,
 *    but nothing is written outside the output arrays and nothing is read outside the input arrays.
 *  - Output: the participating entries stably sorted by id, as post_doc (u32) and post_tf (u32, the entry's
 *    term_cnt).  post_off (u64[nids + 1]): the list of id t is [post_off[t], post_off[t + 1]).  *nposts ==
 *    post_off[nids].
 *  - Stability is the whole ordering contract.  Rows come in document order, so every list is ascending by
 *    document; a caller's own CSR that repeats an id in a row keeps those entries in input order.  For a CSR
 *    of jb_terms_device, post_off[t + 1] - post_off[t] is jb_df_device's df[t] for the batch.
 *  - Capacity, as everywhere here: post_off and *nposts always describe the complete result; entries with
 *    index >= pcap are not written, and nothing else is written.  pcap = cap is always enough; the caller
 *    checks *nposts <= pcap.  With doc_base, the lists of consecutive batches concatenate per id into the
 *    lists of the corpus.
 *  - Errors.  JB_EINVAL: a null pointer (arrays of capacity 0 may be NULL), an output that is an input, the
 *    work buffer or another output, or a work buffer that is too small or not 8-byte aligned; nothing is
 *    queued.  JB_ELIMIT: cap >= 2^32 - JB_POSTINGS_TILE, or doc_base + ndocs > 2^32.  nids == 0 is valid:
 *    post_off[0] = 0 and *nposts = 0.
 *
 * jb_postings_device.  The contract is jb_terms_device's: the call queues its kernels on `stream` and
 * returns; it does not synchronise, allocate, read anything on the host or use the per-device workspace, it
 * holds the ctx's shared lock only while queuing, and it needs no vocabulary.  d_work is a caller-owned
 * device buffer of nwork >= jb_postings_work_bytes(cap, nids, ndocs) bytes: 24 bytes per entry of whole
 * tiles of JB_POSTINGS_TILE entries (two key and two payload arrays the passes alternate between) and 1 KiB
 * per tile.  The helper is host only, non-decreasing in every argument and never 0.  The sort is a stable
 * LSD radix sort with key = id (nids for an entry that does not take part, so those sort to the end) and
 * payload = (document, tf), in ceil(bit_width(nids) / 8) passes of 8-bit digits, 1 to 4.  There are three
 * launches per pass and one more, a number that depends on nids alone, never on device data; when cap == 0
 * or nids == 0 there is none, only the memsets that zero post_off and *nposts.  No lane waits for another
 * workgroup, and there are no global atomics.
 *   k_post_hist     per tile, the counts of the 256 digit values (ballot match, one LDS add per group).
 *   k_post_scan     one workgroup per digit value: that value's counters over the tiles become exclusive
 *                   positions, and its total is written.
 *   k_post_scatter  per tile: the 256 totals are scanned again; every entry is written at its digit's
 *                   position for the tile plus its stable rank among the tile's equal digits (a ballot match
 *                   per round of 64, then wave-ordered counters in LDS; jb_postings.hip says why the rank
 *                   follows entry order).  The first pass builds keys and documents from the CSR (a search in
 *                   term_off); the last writes post_doc and post_tf.
 *   k_post_off      one lane per t in 0 .. nids: post_off[t] by binary search in the sorted keys; *nposts.
 * The scatter has two forms, chosen by JB_POSTINGS_FORM at jb_open; their outputs are identical byte for
 * byte.  Form 0 writes each entry straight from its lane to its global position; form 1 first reorders the
 * tile by digit in LDS and writes runs.
 * Measured on the 1 GiB corpus (tools/postings_bench.py, profiles/postings_bench.json; 73,443 documents, the
 * 350,000-key vocabulary: 3 passes, 10 launches): the CSR's 77.3M entries take 3.26 ms in form 0, which ships
 * as the default, and 3.37 ms in form 1 (k_post_hist 0.65 ms, k_post_scan 0.11 ms, k_post_scatter 2.49 ms
 * against 2.59 ms, k_post_off 0.04 ms, each summed over the passes), beside 6.23 ms for the cut step, 4.88 ms
 * for jb_terms_device and 3.22 ms for jb_df_device in the same run.  The two forms' outputs were identical byte
 * for byte and those of jb_postings over the whole corpus (0.41 s on the host).  The path it replaces, the CSR
 * copied to the host (72 ms) and np.argsort(kind="stable") with its gathers there, takes 7.8 s.  From pageable
 * host memory jb_postings_batch takes 100.7 ms for 1 GiB in and 77.3M postings (0.62 GB) out, beside 36.7 ms
 * for jb_df_batch.  The grid covers the tiles of cap, but the tiles past the entry count do nothing, so the
 * cost follows *d_nterms, not cap.
 *
 * jb_postings_batch: host text in, postings out.  It runs plain Cut -> ids -> terms -> postings on ctx's first
 * device through the buffers jb_keywords_batch keeps in the ctx (one more, that only grows; concurrent calls
 * take turns), under jb_cut_batch_into32's cap protocol: *nposts is always the full count, and when it
 * exceeds pcap the call returns JB_ELIMIT with only *nposts and post_off written.  doc_len (u32[ndocs], may
 * be NULL) receives each document's token count, unknown tokens included (BM25's document length).
 * Requirements and errors are jb_df_batch's: an attached vocabulary (JB_EINVAL), a batch under 2 GiB
 * (JB_ELIMIT), doc_off non-decreasing, and the cut's errors pass through.  nids would normally be
 * jb_vocab_size.  Other modes and the token filter stay on the device chain: jb_cut_device_search_into ->
 * jb_filter_device -> jb_ids_device -> jb_terms_device -> jb_postings_device.
 *
 * Deliberate differences from an analyzer-fed index (Whoosh under jieba's ChineseAnalyzer): those of the
 * term counts above, the vocabulary is closed (unknown tokens are in no list), and there are no positions,
 * only term frequencies. */
#define JB_POSTINGS_TILE 4096 /* entries per tile (one workgroup) */
/* Host only, no ctx: non-decreasing in every argument, never 0. */
size_t jb_postings_work_bytes(uint64_t max_terms, uint64_t nids, uint32_t ndocs);
/* host only, no ctx, no GPU: the rule, and the reference the device kernels are pinned to */
int jb_postings(const uint32_t *term_id, const uint32_t *term_cnt, const uint64_t *term_off, uint64_t nterms,
                uint64_t cap, uint32_t ndocs, uint32_t nids, uint32_t doc_base, uint32_t *post_doc, uint32_t *post_tf,
                uint64_t pcap, uint64_t *post_off, uint64_t *nposts);
int jb_postings_device(jb_ctx *ctx, const uint32_t *d_term_id, const uint32_t *d_term_cnt, const uint64_t *d_term_off,
                       const uint64_t *d_nterms, uint64_t cap, uint32_t ndocs, uint32_t nids, uint32_t doc_base,
                       void *stream, uint32_t *d_post_doc, uint32_t *d_post_tf, uint64_t pcap, uint64_t *d_post_off,
                       uint64_t *d_nposts, void *d_work, size_t nwork);
/* post_off: nids + 1 host entries; post_doc / post_tf: pcap; doc_len: ndocs or NULL. */
int jb_postings_batch(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm,
                      uint32_t doc_base, uint64_t pcap, uint64_t *post_off, uint32_t nids, uint32_t *post_doc,
                      uint32_t *post_tf, uint64_t *nposts, uint32_t *doc_len);

/* ---- BM25 search (the query half of the Whoosh use case: Whoosh's default scorer under jieba's
 * ChineseAnalyzer is BM25F; the reference has only Cut) -------------------------------------------------
 * Rank the documents of an index (the postings above, with doc_len) for queries, on the device: cut the query,
 * look up its ids, score and keep the best topk.  It replaces copying the postings to the host and scoring there.
 *
 * The rule, stated once; the host forms and the device forms agree to the bit (the build keeps every f64
 * operation separately rounded).  Parameters: k1 and b are f64, JB_EINVAL unless 0 <= k1 <= 64 and 0 <= b <= 1
 * (NaN is rejected); avgdl is f64, finite and > 0.
 *  - jb_bm25_avgdl (host only): the u64 sum of doc_len divided by ndocs, as f64; JB_EINVAL for ndocs == 0 or a
 *    zero sum.
 *  - jb_bm25_norms(_device): norm[d] = (float)(k1 * ((1.0 - b) + b * ((double)doc_len[d] / avgdl))), each
 *    operation one f64 rounding in that order, then one narrowing; one lane per document.
 *  - jb_bm25_idf(_device): df = min(post_off[t + 1] - post_off[t], ndocs_total), 0 when the offsets decrease;
 *    weight[t] = 0.0f for df == 0, otherwise (float)jb_go_log(1.0 + ((double)(ndocs_total - df) + 0.5) /
 *    ((double)df + 0.5)), Lucene's form, > 0 for every ndocs_total below 2^51 (past that the f64 sum of a list of
 *    every document rounds to 1 and the weight to 0).  JB_ELIMIT for ndocs_total >= 2^53.  One lane per id.
 *  - jb_bm25_search(_device).  Inputs: the index post_doc / post_tf / post_off (u64[nids + 1]) and npost, the
 *    number of valid entries of the two arrays; norm (f32[ndocs]); weight (f32[nweights]); k1; the queries as a
 *    CSR, q_id (u32, q_cap valid entries) and q_off (u64[nq + 1]); topk.
 *     - Query q's entries are [q_off[q], q_off[q + 1]) clamped to q_cap, and only the first JB_BM25_MAXQ of them
 *       are read.  An entry with id t takes part iff t < nids, t < nweights and 0 < weight[t] <= JB_BM25_WMAX
 *       (which excludes NaN and +Inf).  A repeated id counts once per occurrence.  JB_ID_UNK fails the first test
 *       in any real vocabulary; no table is indexed by an id that is not checked.
 *     - The list of t is [post_off[t], post_off[t + 1]) clamped to [0, npost], empty if the offsets decrease.  A
 *       posting takes part iff post_doc < ndocs, post_tf > 0 and norm[post_doc] >= 0 (the norms of jb_bm25_norms
 *       are; a caller's negative or NaN norm drops the document).  Lists are trusted to ascend by document, as
 *       jb_postings* writes them; with a caller's own unsorted lists which postings count is unspecified, but
 *       nothing is read outside the inputs and nothing is written outside the outputs.
 *     - A posting (d, tf) under an entry t contributes, all in f64 with one rounding per operation:
 *       num = (double)tf * (k1 + 1.0); den = (double)tf + (double)norm[d]; x = (double)weight[t] * (num / den);
 *       c = (uint64_t)(x * 16777216.0), truncated.  den >= 1, so c < 2^51 and 1024 entries cannot overflow.
 *     - score[q][d] is the u64 sum of the contributions, in units of 2^-24: an integer, so host and device agree
 *       in any order of adds and from run to run.  A document is a candidate iff its score is > 0.
 *     - Row q of res_doc (u32) and res_score (u64), nq x topk each, holds the res_n[q] = min(topk, candidates)
 *       best candidates, score descending, ties by document ascending; the remaining slots are JB_ID_UNK and 0.
 *       Every slot of every row is written, and nothing else.  1 <= topk <= JB_KW_MAXK: JB_EINVAL for 0,
 *       JB_ELIMIT above.
 *     - JB_EINVAL: a null pointer (arrays of capacity 0 may be NULL), an output that is an input, another output
 *       or the work buffer, a work buffer that is too small or not 8-byte aligned; nothing is queued.  nq == 0,
 *       ndocs == 0 and nids == 0 are valid.
 *
 * jb_bm25_search_device.  The contract is jb_postings_device's: it queues on `stream` and returns; it does not
 * synchronise, allocate or read on the host, it needs no vocabulary, and it holds the ctx's shared lock only
 * while queuing.  The number of launches depends on the arguments alone.  d_work holds nwork >=
 * jb_bm25_work_bytes(nq, ndocs, topk) bytes: per pair of query and document tile (JB_BM25_TILE documents) a
 * count and topk partial records, and the dense rows of form 0 (8 bytes per pair of query and document).  Two
 * forms, chosen by JB_BM25_FORM at jb_open, write identical bytes:
 *   form 1  k_bm25_tile, one workgroup per pair of query and tile: the tile's u64 scores in 64 KiB of LDS, the
 *           part of each entry's list inside the tile by two binary searches, LDS atomics, then the tile's best
 *           topk; k_bm25_merge, one workgroup per query.  No global atomics; no lane waits for another workgroup.
 *   form 0  a memset of the dense rows, k_bm25_scatter (one lane per posting, a global atomicAdd), k_bm25_select
 *           (the same selection per tile), k_bm25_merge.
 * Measured on the 1 GiB corpus's index (tools/bm25_bench.py, profiles/bm25_bench.json; 73,443 documents, 77.3M
 * postings; 1,024 seeded queries of 1 to 8 ids drawn by corpus frequency, 4,593 entries over 141.0M postings,
 * topk 10): form 1 takes 0.96 ms (k_bm25_tile 0.90 ms, k_bm25_merge 0.03 ms) and ships as the default; form 0
 * takes 1.75 ms (k_bm25_scatter 1.23 ms, k_bm25_select 0.42 ms, k_bm25_merge 0.03 ms and the memset), beside
 * 6.00 ms for the cut step and 3.15 ms for jb_postings_device in the same run.  The two forms' rows were
 * identical byte for byte and those of jb_bm25_search on every query (280 ms on the host).  The path it
 * replaces, the postings copied to the host (71 ms) and scored by numpy there, takes 4.4 ms per query (timed on
 * 32 queries: about 4.5 s for all).  From host text jb_search_batch takes 1.66 ms for the 1,024 queries;
 * jb_index_set takes 11 ms.
 *
 * jb_index_set uploads an index (build_index's arrays) to ctx's first device, computes avgdl on the host and
 * the norms and weights on the device with the calls above, and keeps them until the next jb_index_set,
 * jb_index_clear or jb_close, under the ctx's exclusive lock (the jb_vocab_set precedent).  JB_ELIMIT when ndocs
 * or npost is >= 2^32; JB_EINVAL for an index without a token (jb_bm25_avgdl's).  jb_index_info reports ndocs,
 * nids, npost and avgdl (JB_EINVAL with no index).
 * jb_search_batch: host query text in (q_off: u64[nq + 1] byte offsets, as doc_off), records out.  It runs plain
 * Cut -> ids -> jb_bm25_search_device on ctx's first device through the buffers jb_keywords_batch keeps in the
 * ctx (one more, that only grows; concurrent calls take turns); a query's entries are its tokens' ids, unknown
 * tokens included (they do not take part).  Only the nq x topk records and res_n come back.  It needs an
 * attached vocabulary and an attached index whose nids equals the vocabulary's size (JB_EINVAL otherwise); the
 * cut's errors pass through. */
#define JB_BM25_TILE 8192      /* documents per tile (one workgroup per query and tile) */
#define JB_BM25_MAXQ 1024      /* entries of a query that are read */
#define JB_BM25_WMAX 1048576.0f /* 2^20: the largest weight that takes part */
/* Host only, no ctx: non-decreasing in every argument, never 0 (SIZE_MAX when the size overflows). */
size_t jb_bm25_work_bytes(uint32_t nq, uint32_t ndocs, uint32_t topk);
/* host only, no ctx, no GPU: the rule, and the reference the device kernels are pinned to */
int jb_bm25_avgdl(const uint32_t *doc_len, uint32_t ndocs, double *avgdl);
int jb_bm25_norms(const uint32_t *doc_len, uint32_t ndocs, double k1, double b, double avgdl, float *norm);
int jb_bm25_idf(const uint64_t *post_off, uint32_t nids, uint64_t ndocs_total, float *weight);
int jb_bm25_search(const uint32_t *post_doc, const uint32_t *post_tf, const uint64_t *post_off, uint64_t npost,
                   uint32_t nids, const float *norm, uint32_t ndocs, const float *weight, uint32_t nweights, double k1,
                   const uint32_t *q_id, uint64_t q_cap, const uint64_t *q_off, uint32_t nq, uint32_t topk,
                   uint32_t *res_doc, uint64_t *res_score, uint32_t *res_n);
int jb_bm25_norms_device(jb_ctx *ctx, const uint32_t *d_doc_len, uint32_t ndocs, double k1, double b, double avgdl,
                         void *stream, float *d_norm);
int jb_bm25_idf_device(jb_ctx *ctx, const uint64_t *d_post_off, uint32_t nids, uint64_t ndocs_total, void *stream,
                       float *d_weight);
int jb_bm25_search_device(jb_ctx *ctx, const uint32_t *d_post_doc, const uint32_t *d_post_tf, const uint64_t *d_post_off,
                          uint64_t npost, uint32_t nids, const float *d_norm, uint32_t ndocs, const float *d_weight,
                          uint32_t nweights, double k1, const uint32_t *d_q_id, uint64_t q_cap, const uint64_t *d_q_off,
                          uint32_t nq, uint32_t topk, void *stream, uint32_t *d_res_doc, uint64_t *d_res_score,
                          uint32_t *d_res_n, void *d_work, size_t nwork);
/* host arrays in; the index stays on the device */
int jb_index_set(jb_ctx *ctx, const uint64_t *post_off, const uint32_t *post_doc, const uint32_t *post_tf,
                 uint64_t npost, uint32_t nids, const uint32_t *doc_len, uint64_t ndocs, double k1, double b);
int jb_index_clear(jb_ctx *ctx);
int jb_index_info(jb_ctx *ctx, uint64_t *ndocs, uint64_t *nids, uint64_t *npost, double *avgdl);
/* res_doc / res_score: nq * topk host entries; res_n: nq. */
int jb_search_batch(jb_ctx *ctx, const uint8_t *qtext, const uint64_t *q_off, uint32_t nq, int hmm, uint32_t topk,
                    uint32_t *res_doc, uint64_t *res_score, uint32_t *res_n);

/* ---- near-duplicate pairs (the end of the recipe jieba.cut -> word shingles -> MinHash -> LSH bands: join the
 * buckets, verify the candidates, label the groups; the reference has only Cut) ---------------------------
 * Which documents are near-duplicates of which, from the band keys and the signatures of the MinHash calls
 * above, on the device.  It replaces copying the ndocs * B keys and ndocs * K slots to the host, grouping the
 * keys per band, enumerating the pairs of every bucket, dropping the pairs more than one band found and
 * counting agreeing slots there.
 *
 * The rule (jb_neardup on host arrays, jb_neardup_device on device arrays: one rule, bit for bit).  Inputs: key,
 * u64[ndocs * B] row-major (key[d * B + b]) as jb_minhash_bands(_device) writes it, or the caller's own; sig,
 * u32[ndocs * K]; 1 <= B <= JB_MH_MAXK bands; 1 <= K <= JB_MH_MAXK slots; the window 1 <= W <= JB_ND_MAXWIN;
 * 1 <= min_agree <= K.  There is no R: the keys embody it, and B <= K is not required.  Keys and slots are
 * data, never indices: any bit pattern is legal.
 *  - Buckets.  Document d is in bucket (b, key[d * B + b]) of band b unless that key is JB_MH_NOKEY.  The band
 *    is part of the bucket's identity: equal key values in different bands are different buckets.  A bucket's
 *    members are ordered by document number; member d's rank is the number of members below d.
 *  - Candidates.  For i < j let b* be the least band in which both keys are not JB_MH_NOKEY and are equal.  The
 *    pair (i, j) is a candidate iff b* exists and, in that bucket, rank(j) - rank(i) <= W.  A pair is examined
 *    in exactly one band and never reported twice.  A member pairs with at most the W members just below it:
 *    a bucket of m members costs at most m * W, not m^2 / 2, and consecutive members are always candidates,
 *    which keeps a bucket connected for clustering.
 *  - Verification.  agree(i, j) is the number of slots s < K with sig[i * K + s] == sig[j * K + s]: all K
 *    slots, not only the banded ones.  A candidate is kept iff agree >= min_agree; the threshold is an integer
 *    and the rule has no float in it.
 *  - Output: a CSR by the later document.  Row j holds its kept pairs ordered by (b*, i) ascending, as pair_doc
 *    (u32, the earlier document i) and pair_agree (u32); pair_off is u64[ndocs + 1]; *npairs (u64) is the true
 *    count.  Only positions below pcap are written to pair_doc and pair_agree, as with pcap in the postings;
 *    pair_off is always complete.  The order does not depend on how buckets are ordered among themselves.
 *  - Counters, stat (u64[JB_ND_NSTAT]): [JB_ND_NENTRIES] keys that are not JB_MH_NOKEY; [JB_ND_NCAND]
 *    candidates; [JB_ND_NTRUNC] members whose rank is above W.  When ntrunc is 0 the kept pairs are exactly
 *    the set "some band agrees and agree >= min_agree".
 *  - Errors.  JB_EINVAL: a null pointer (arrays of capacity 0 may be NULL), B, K, W or min_agree = 0, an output
 *    that is an input, the work buffer or another output, a work buffer that is too small or not 8-byte
 *    aligned; nothing is queued or written.  JB_ELIMIT: B, K or W above its maximum, min_agree > K,
 *    ndocs * B >= 2^32 - JB_ND_TILE.
 *
 * jb_neardup_labels (host only): label[d] (u32[ndocs]) is the least document of d's connected component over
 * the kept pairs, by a union-find over the CSR; label[d] == d marks the document to keep.  The CSR may be the
 * caller's: an entry >= j in row j is skipped, and offsets are clamped to pcap.
 *
 * jb_neardup_device.  The contract is jb_postings_device's: the call queues its kernels on `stream` and
 * returns; it does not synchronise, allocate or read anything on the host, and it holds the ctx's shared lock
 * only while queuing.  d_work is a caller-owned device buffer of nwork >= jb_neardup_work_bytes(ndocs, B)
 * bytes, 8-byte aligned: 24 bytes per entry of whole tiles of JB_ND_TILE entries (two key and two entry
 * arrays the passes alternate between; after the sort one pair holds the keep masks and the pair counts) and
 * about 1 KiB per tile.  The helper is host only, non-decreasing in both arguments and never 0.  There are 32
 * launches whatever the data are (three memsets and none when ndocs == 0), no lane waits for another workgroup
 * and there are no global atomics; every value is an integer, so the bytes are the same from run to run and
 * equal to jb_neardup's.
 *   k_nd_hist / k_nd_scan / k_nd_scatter   a stable LSD radix sort of the entries (d, b) by (band, key), 8 bits
 *                 per pass, nine passes: the eight key bytes, then the band; the sort of jb_postings_device
 *                 (ballot match, wave-ordered counters in LDS) with a u64 key and the entry as payload.
 *                 JB_MH_NOKEY ends each band.  Stability keeps a bucket's documents ascending.
 *   k_nd_mask     a wave per 64 sorted positions; for a position q whose predecessor has its bucket, lane w < W
 *                 looks at position q - 1 - w: same band and same key (a run is contiguous and ascending, so
 *                 this alone gives the window and the rank), then the first-band test over the two key rows;
 *                 the candidates' signature rows are compared 64 slots at a time.  A u64 keep mask per
 *                 position (hence W <= 64) and its popcount per entry; position q - W - 1 counts ntrunc.
 *   k_nd_tsum / k_nd_base / k_nd_off   the exclusive scan of the counts over the entries into u64 offsets:
 *                 pair_off, *npairs, and the counters' sums into stat.
 *   k_nd_write    for each set bit, highest w first (i ascending), agree again, and the pair at its offset
 *                 when that is below pcap.
 * One form ships (there is no JB_ND_FORM): no second form was written.
 * Measured on the 1 GiB corpus (tools/neardup_bench.py, profiles/neardup_bench.json; 73,443 documents, a seeded
 * tenth replaced before the cut by copies of other documents with 0 to 5 % of their tokens overwritten; n = 5,
 * K = 128, B = 32, R = 4, W = 64, min_agree = 102): the 2.35M entries take 0.70 ms (k_nd_hist 0.13 ms, k_nd_scan
 * 0.06 ms, k_nd_scatter 0.35 ms, k_nd_mask 0.13 ms, k_nd_write 0.07 ms, the scan's three 0.04 ms, each summed over
 * its launches), beside 6.02 ms for the cut step, 5.97 ms for jb_minhash_device and 0.02 ms for
 * jb_minhash_bands_device in the same run; 7,720 candidates, 3,609 pairs, ntrunc 0, 69,881 labels kept.  The
 * outputs were those of jb_neardup over the whole input (476 ms on the host after a 3.9 ms copy; numpy's stable
 * argsort per band, the grouping alone, 125 ms).  4,000,000 synthetic signatures generated on the device (128M
 * entries, a tenth planted copies) take 26.9 ms, of which the sort is 19.4 ms (k_nd_scatter 15.6 ms) and k_nd_mask
 * 6.2 ms; on the first 250,000 of those rows the host rule takes 2.9 s and the device 1.4 ms for the same bytes.
 * From pageable host memory jb_neardup_sig takes 1.90 ms for the corpus's signatures, beside 36.6 ms for
 * jb_minhash_batch.
 *
 * jb_neardup_sig: host signatures in (sig u32[ndocs * K], doc_n u32[ndocs] as jb_minhash_batch returns them).
 * It uploads them, runs jb_minhash_bands_device (B bands of R rows) and jb_neardup_device on ctx's first device
 * through a buffer kept in the ctx that only grows (concurrent calls take turns, as in jb_minhash_batch), and
 * copies the results back under jb_postings_batch's cap protocol: pair_off, *npairs and stat are always
 * complete, and when *npairs exceeds pcap the call returns JB_ELIMIT with only those written.
 *
 * Deliberate differences from the usual LSH join (all pairs of every bucket, every band):
 *  - the window: a member pairs with the W members just below it, not with all of them;
 *  - the first-agreeing-band rule: with a window, a pair beyond the window in its first common band is not
 *    picked up by a later band.  ntrunc tells the caller when that can have happened. */
#define JB_ND_TILE 4096 /* entries per tile (one workgroup) */
#define JB_ND_MAXWIN 64 /* the widest window: a keep mask is one u64 */
#define JB_ND_NSTAT 3
#define JB_ND_NENTRIES 0
#define JB_ND_NCAND 1
#define JB_ND_NTRUNC 2
/* Host only, no ctx: non-decreasing in both arguments, never 0. */
size_t jb_neardup_work_bytes(uint32_t ndocs, uint32_t B);
/* host only, no ctx, no GPU: the rule, and the reference the device kernels are pinned to */
int jb_neardup(const uint64_t *key, const uint32_t *sig, uint32_t ndocs, uint32_t B, uint32_t K, uint32_t W,
               uint32_t min_agree, uint32_t *pair_doc, uint32_t *pair_agree, uint64_t pcap, uint64_t *pair_off,
               uint64_t *npairs, uint64_t *stat);
int jb_neardup_device(jb_ctx *ctx, const uint64_t *d_key, const uint32_t *d_sig, uint32_t ndocs, uint32_t B, uint32_t K,
                      uint32_t W, uint32_t min_agree, uint32_t *d_pair_doc, uint32_t *d_pair_agree, uint64_t pcap,
                      uint64_t *d_pair_off, uint64_t *d_npairs, uint64_t *d_stat, void *d_work, size_t nwork,
                      void *stream);
/* host only: label u32[ndocs] */
int jb_neardup_labels(const uint64_t *pair_off, const uint32_t *pair_doc, uint64_t pcap, uint32_t ndocs,
                      uint32_t *label);
/* pair_off: ndocs + 1 host entries; pair_doc / pair_agree: pcap; stat: JB_ND_NSTAT. */
int jb_neardup_sig(jb_ctx *ctx, const uint32_t *sig, const uint32_t *doc_n, uint32_t ndocs, uint32_t K, uint32_t B,
                   uint32_t R, uint32_t W, uint32_t min_agree, uint32_t *pair_doc, uint32_t *pair_agree, uint64_t pcap,
                   uint64_t *pair_off, uint64_t *npairs, uint64_t *stat);

/* ---- collocations: adjacent-pair counts and new-word scores (gensim's Phrases; the first step of Chinese
 * "new word discovery") -------------------------------------------------------------------------
 *
 * Everything above sees only the words the dictionary knows; a word it lacks comes out in pieces.  jb_add_word
 * changes that, and these calls say what to add: how often token a is directly followed by token b over a
 * corpus, against how often each occurs alone.  The pairs and the corpus-wide token count per id are accumulated
 * on the device over any number of batches, scored there, and only the candidates are read back.
 *
 * The rule.  jb_colloc_count / jb_colloc_score (host only, no ctx, no GPU) and the device agree exactly.
 *  - Inputs: those of jb_textrank_device.  ids (ids_cap valid entries), doc_tok (u64[ndocs + 1], non-decreasing),
 *    ntok, an optional keep (u8[nkeep]), a flag word, and with JB_COLLOC_CONTIG the spans start / end (u32; both
 *    may be NULL without the flag).  Token k exists iff k < min(ntok, ids_cap).  Document d's tokens are
 *    [doc_tok[d], doc_tok[d+1]) clamped to that bound; a token before doc_tok[0], or at or past doc_tok[ndocs],
 *    belongs to no document and takes no part in anything.  The ids are not trusted: any u32 is an id.
 *  - Unigrams.  Every existing token of a document with id < nuni does uni[id] += 1 (uni: u64[nuni], the
 *    caller's), whatever keep and the flags say, so that p(a) is the corpus probability.  N (`known`) is the
 *    number of such tokens, accumulated over the batches.
 *  - Pairs.  (k, k+1) takes part iff both tokens exist and lie in the same document, both ids are < nuni (so
 *    neither is JB_ID_UNK), with nkeep > 0 both ids are < nkeep with keep[id] != 0 (nkeep == 0: keep may be NULL,
 *    every id is kept), and with JB_COLLOC_CONTIG end[k] == start[k+1]: no dropped whitespace, no filtered
 *    token and no overlap lies between them, which makes a+b a substring of the text.  The key is
 *    (uint64_t)a << 32 | b, ordered: (a, b) is not (b, a).  Each pair adds 1 to its key's u64 count.
 *  - Table.  A caller-owned device buffer of jb_colloc_table_bytes(nslots) bytes, 32-byte aligned: a header
 *    with a magic word and the totals, then nslots slots of key and count; nslots is a power of two >= 8
 *    (JB_ELIMIT above 2^30).  New keys are accepted while fewer than nslots / 2 slots are claimed; a pair whose
 *    key finds no slot is dropped.  The totals are u64 and exact: tokens (the tokens that exist), known (N),
 *    pairs, dropped and distinct (the keys claimed).  The sum of the counts plus dropped is pairs, and the sum
 *    of uni is known, always.  A key that is in the table carries its exact count: dropped pairs belong only to
 *    keys that are not in the table.  With dropped == 0 the result is complete, independent of the order of the
 *    adds and the same from run to run.  Which keys survive a full table, and where a key sits, is not
 *    determined and nothing exposes it.
 *  - Score.  For a key's count c, ca = uni[a], cb = uni[b], N, min_count m >= 1 (JB_EINVAL for 0), a float
 *    threshold and a scorer, the pair is no candidate when a or b >= nuni, c < m, ca or cb is 0, c >= N, or any
 *    of c, ca, cb, N is >= 2^53 (the arrays are the caller's and are not trusted).  All arithmetic is f64 with
 *    one rounding per operation and no fused multiply-add; log is jb_go_log.
 *      JB_COLLOC_NPMI   pa = ca/N, pb = cb/N, pab = c/N; s = log(pab / (pa*pb)) / (0.0 - log(pab)): gensim's
 *                       npmi_scorer, in [-1, 1]
 *      JB_COLLOC_RATIO  s = (((double)(c - m) / ca) / cb) * N: Mikolov's score in gensim's operation order
 *      JB_COLLOC_COUNT  s = (double)c: the most frequent pairs, and the way to dump a table
 *    score = (float)s, and the pair is a candidate iff score >= threshold (false for NaN).
 *  - Order of a result: score descending, then count descending, then a ascending, then b ascending.
 *
 * jb_colloc_table_bytes and jb_colloc_work_bytes are host only, non-decreasing in their arguments and never 0
 * (SIZE_MAX where the size does not fit; a slot count that is not valid is sized as the next valid one).
 *
 * jb_colloc_init_device queues the kernels that empty a table and zero d_uni (u64[nuni]).
 *
 * jb_colloc_add_device adds one batch with jb_wc_add_device's and jb_terms_device's contract: it queues on
 * `stream` and returns without synchronising, allocating, reading on the host or using the per-device
 * workspace, and takes the shared lock only while queuing.  Four launches whatever the data (none when ids_cap
 * is 0), and no lane ever waits for another; it writes nothing outside the table, d_uni and
 * d_work.  d_ntok is a device u64; d_work holds jb_colloc_work_bytes(ids_cap, ndocs) bytes, 4-byte aligned;
 * d_table is 32-byte aligned and d_uni 8-byte aligned: JB_EINVAL otherwise, and for unknown flags, with nothing
 * queued.  JB_ELIMIT for ids_cap >= 2^32 - JB_COLLOC_TILE.  A buffer without a valid header is left untouched,
 * and so are d_uni and d_work then.  The count pass has two forms with identical results (JB_COLLOC_COMBINE,
 * read at jb_open): 0 is one global atomic per pair and per unigram, 1 (the default) combines a workgroup's adds
 * in two direct-mapped tables of JB_COLLOC_LDS entries in LDS first, over a share of at least JB_COLLOC_SHARE
 * tiles of JB_COLLOC_TILE tokens; an entry that finds another key's tag goes to memory itself.
 *
 * jb_colloc_score_device is one pass over the slots, queued on `stream`: the candidates go to d_cand_a,
 * d_cand_b (u32), d_cand_cnt (u64) and d_cand_score (f32) of capacity ccap in no promised order; *d_ncand (a
 * device u64) always counts the complete set, entries with index >= ccap are not written, and nothing else is
 * written.  N is read from the table's header on the device.
 *
 * jb_colloc_read synchronises `stream`, runs the score pass into a buffer of its own (growing it and
 * repeating the pass when the candidates outnumber it), copies back only the candidates, sorts them on the
 * host into the order above and keeps the first topn (0: all).  The table is left unchanged.  JB_EINVAL when
 * the buffer holds no table.  jb_colloc_result_free frees the arrays (malloc'd) and zeroes the struct.
 *
 * jb_colloc_count is the rule of the add on host arrays: uni[id] += 1 into the caller's uni, and out holds every
 * pair in the table sorted by key (score = (float)count) with the batch's totals.  nslots (0: no limit, else as
 * above) gives the drop behaviour, with keys accepted in token order.  jb_colloc_score is the score rule over
 * host arrays of n pairs, N given; out holds the candidates in the rule's order, the totals 0.
 *
 * jb_colloc_batch: host text in.  It uploads, runs plain Cut -> ids -> add on ctx's first device through the
 * buffers jb_keywords_batch keeps in the ctx; concurrent calls take turns.  It needs an attached vocabulary
 * (JB_EINVAL), a batch under 2 GiB (JB_ELIMIT) and doc_off non-decreasing; the cut's errors pass through.
 * While a batch filter is set (jb_batch_filter_set) it filters between the cut and the ids, as jb_wc_batch
 * does; with JB_COLLOC_CONTIG a pair across a filtered-out token then does not count, by the rule itself.
 *
 * Deliberate differences from gensim's Phrases:
 *  - JB_COLLOC_RATIO multiplies by N, the corpus's known tokens, where gensim puts the vocabulary's size;
 *  - pairs are ordered and counted per adjacent position, not per sentence with a delimiter set, and no pair
 *    is merged while counting: the next round (add the words, cut again) finds the three-piece words;
 *  - nothing is pruned while counting: a full table drops new keys and says how many pairs that cost.
 *
 * Measured (tools/colloc_bench.py, profiles/colloc_bench.json) on the 1 GiB corpus, 139,547,178 plain-mode ids under
 * the 964,284-key vocabulary its word counts give, 62,835,284 distinct pairs among 139,473,735 in a table of 2^28
 * slots (4.0 GiB, load 0.23; 2^26 slots dropped 31,235,490 pairs): jb_colloc_add_device 16.29 ms in the combining
 * form, the default, against 132.74 ms with one global atomic per add, into a table that holds the pairs already;
 * 225.82 ms against 342.68 ms into an empty one; beside 6.05 ms for the cut step, 1.79 ms for jb_ids_device and
 * 9.19 ms for jb_wc_add_device.  jb_colloc_score_device 1.08 ms for 54,331 candidates (NPMI, min_count 5,
 * threshold 0.5).  Both forms' tables were identical over the whole corpus and equal to jb_colloc_count over its
 * first 64 MiB.  The ids copied to the host take 86 ms and np.unique over the pair keys about 1.7 s. */
#define JB_COLLOC_CONTIG 1u
#define JB_COLLOC_NPMI 0
#define JB_COLLOC_RATIO 1
#define JB_COLLOC_COUNT 2
#define JB_COLLOC_TILE 256   /* tokens per tile */
#define JB_COLLOC_LDS 2048   /* entries of each of the combining form's two LDS tables */
#define JB_COLLOC_SHARE 64   /* the combining form: a workgroup's share is at least this many tiles */
typedef struct jb_colloc_result {
    uint32_t *a, *b;  /* n each: the pair's ids */
    uint64_t *count;  /* n */
    float *score;     /* n */
    uint64_t n;
    uint64_t tokens, known, pairs, dropped, distinct;
} jb_colloc_result;

size_t jb_colloc_table_bytes(uint64_t nslots);
size_t jb_colloc_work_bytes(uint64_t max_tokens, uint32_t ndocs);
int jb_colloc_init_device(jb_ctx *ctx, void *d_table, size_t ntable, uint64_t nslots, uint64_t *d_uni, uint32_t nuni,
                          void *stream);
int jb_colloc_add_device(jb_ctx *ctx, void *d_table, size_t ntable, uint64_t *d_uni, uint32_t nuni,
                         const uint32_t *d_ids, uint64_t ids_cap, const uint64_t *d_doc_tok, const uint64_t *d_ntok,
                         uint32_t ndocs, const uint8_t *d_keep, uint32_t nkeep, uint32_t flags, const uint32_t *d_start,
                         const uint32_t *d_end, void *stream, void *d_work, size_t nwork);
int jb_colloc_score_device(jb_ctx *ctx, const void *d_table, size_t ntable, const uint64_t *d_uni, uint32_t nuni,
                           int scorer, uint64_t min_count, float threshold, uint32_t *d_cand_a, uint32_t *d_cand_b,
                           uint64_t *d_cand_cnt, float *d_cand_score, uint64_t ccap, uint64_t *d_ncand, void *stream);
int jb_colloc_read(jb_ctx *ctx, const void *d_table, size_t ntable, const uint64_t *d_uni, uint32_t nuni, int scorer,
                   uint64_t min_count, float threshold, uint64_t topn, void *stream, jb_colloc_result *out);
void jb_colloc_result_free(jb_colloc_result *r);
int jb_colloc_count(const uint32_t *ids, uint64_t ids_cap, const uint64_t *doc_tok, uint64_t ntok, uint32_t ndocs,
                    const uint8_t *keep, uint32_t nkeep, uint32_t flags, const uint32_t *start, const uint32_t *end,
                    uint64_t nslots, uint64_t *uni, uint32_t nuni, jb_colloc_result *out);
int jb_colloc_score(const uint32_t *a, const uint32_t *b, const uint64_t *count, uint64_t n, const uint64_t *uni,
                    uint32_t nuni, uint64_t N, int scorer, uint64_t min_count, float threshold, uint64_t topn,
                    jb_colloc_result *out);
int jb_colloc_batch(jb_ctx *ctx, const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, int hmm,
                    const uint8_t *keep, uint32_t nkeep, uint32_t flags, void *d_table, size_t ntable, uint64_t *d_uni,
                    uint32_t nuni);

/* Error state of the last jb_cut_device / jb_cut_device_into pipeline on ctx's first
 * device (from any thread): synchronises `stream` (the one that call was queued on) and
 * the pipeline, then returns JB_OK, JB_EPANIC (input on which the reference panics:
 * the spans are not the reference's), JB_EDEVICE (a long-block phase wait gave up,
 * JB_LONG_WAIT_US: the spans are incomplete) or JB_ELIMIT (full mode: the list is longer
 * than the arrays' capacity, the spans past it were not written).  The device calls themselves return
 * before their kernels run, so a caller that must know checks here (a host batch,
 * jb_cut_batch*, returns these codes itself). */
int jb_device_status(jb_ctx *ctx, void *stream);

/* Contiguous byte-balanced ranges of whole documents (the reference's
 * CutParallel deals blocks to goroutines instead, tokenizer.go:81-148), the partition
 * bench.py's one-process-per-GPU runs use (jb_cut_batch itself uses jb_split_points,
 * which may cut inside a document): part k owns documents
 * [cut[k], cut[k+1]), cut has nparts + 1 entries, cut[0] = 0 and
 * cut[nparts] = ndocs.  Host only. */
int jb_shard_bounds(const uint64_t *doc_off, uint32_t ndocs, uint32_t nparts, uint32_t *cut);

/* Byte-balanced split points that may fall inside a document (one
 * large document over several devices): cut has nparts + 1 entries, cut[0] =
 * doc_off[0], cut[nparts] = doc_off[ndocs], and cut[k] is the first document start
 * or Han-run start at or after doc_off[0] + total * k / nparts.  A Han-run start is
 * a byte where a Han rune begins (Go's DecodeRune over the document) and the rune
 * before it is not Han: cutting a document there leaves splitText's blocks
 * (tokenizer.go:165-210) unchanged, and blocks are cut independently
 * (tokenizer.go:158-160), so the parts' tokens are the whole's.  jb_cut_batch
 * shards over its devices with these points.  Host only. */
int jb_split_points(const uint8_t *text, const uint64_t *doc_off, uint32_t ndocs, uint32_t nparts, uint64_t *cut);

/* Replaces Tokenizer.AddWord (tokenizer.go:372; the reference deadlocks there,
 * :376 + :581).  freq < 1 takes suggestFreq's value (tokenizer.go:589-614).
 * Atomic: on any error (JB_ELIMIT for an all-Han word of more than 255 runes -- the
 * trie holds only all-Han keys, so a longer word with a non-Han rune is stored in
 * the dictionary and never walked; JB_EDEVICE, JB_ENOMEM) the dictionary, pd.size
 * and every device's image stay as they were. */
int jb_add_word(jb_ctx *ctx, const char *word, size_t len, int64_t freq);

/* suggestFreq (tokenizer.go:589-614): the frequency AddWord(word, freq < 1) would store. */
int jb_suggest_freq(jb_ctx *ctx, const char *word, size_t len, int64_t *freq);

/* Add caller-computed logarithms (as jb_config.log_keys/log_vals) to ctx's table: they
 * apply from the next image build, i.e. the next jb_add_word.  A Go AddWord passes
 * math.Log of the new frequency and of the new pd.size before calling jb_add_word. */
int jb_add_log(jb_ctx *ctx, const int64_t *keys, const double *vals, size_t n);

/* Dictionary introspection (prefixDictionary.termFreq / size, tokenizer.go:382-383). */
int jb_dict_get(jb_ctx *ctx, const char *word, size_t len, int64_t *freq); /* 1 found, 0 absent */
int64_t jb_dict_size(jb_ctx *ctx);

/* Counters of the last cut on each device of ctx, summed over the devices (a host
 * batch cut in pieces: summed over its pieces).  Synchronises the devices' streams.
 * After a device pipeline (jb_cut_device*) it fills *out and also returns that
 * pipeline's error state, as jb_device_status does.
 * Concurrent small calls (jb_cut of at most 4 KiB) are coalesced into shared k_small
 * batches: after one, the counters are those of the k_small batch that finished last
 * on the device, which may hold other callers' documents beside this caller's. */
typedef struct {
    uint64_t tokens;       /* tokens written */
    uint64_t blocks;       /* splitText blocks, zh and non-zh (tokenizer.go:165-210) */
    uint64_t zh_blocks;    /* of which Han runs (cutZh, tokenizer.go:221) */
    uint64_t long_blocks;  /* zh blocks of >= 8 KiB, cut by the long-block kernel */
    uint64_t viterbi_ties; /* exact stateTransitionRoute ties a == b > minFloat, which the reference
                              resolves in Go's random map order (tokenizer.go:748-753); here the first
                              candidate of stateChange wins */
} jb_stats;
int jb_last_stats(jb_ctx *ctx, jb_stats *out);

/* Per-kernel timing with HIP events on the launch stream (bench / profiling). */
int jb_profile_enable(jb_ctx *ctx, int on);
/* Fills up to cap entries: kernel name, total ms, launches. Synchronises. Returns #entries. */
int jb_profile_read(jb_ctx *ctx, const char **names, double *ms, uint64_t *launches, int cap);
int jb_profile_reset(jb_ctx *ctx);

/* Write ctx's current image (including words added by jb_add_word) to `path`,
 * to be opened later with dict_kind JB_DICT_IMAGE: the fast-start counterpart of
 * the reference shipping prefix_dictionary.gob instead of rebuilding the map
 * from dict.txt (tokenizer.go:439-458 vs :389-437). */
int jb_save(jb_ctx *ctx, const char *path);

/* ---- host-only image access (no GPU needed; used by CPU tests) ---------- */
int jb_image_build(const jb_config *cfg, jb_image **out);
void jb_image_free(jb_image *img);
int jb_image_save(const jb_image *img, const char *path);
/* prefixDictionary view of an image: number of termFreq entries and pd.size. */
int jb_image_dict_info(const jb_image *img, uint64_t *nentries, int64_t *size);
/* Look up a key as the device walk sees it: returns 1 if reachable, with freq and w. */
int jb_image_lookup(const jb_image *img, const char *word, size_t len, int64_t *freq, double *w);
/* nodes stored, hash capacity, pages, max key length in runes, size, -Log(size) */
int jb_image_stats(const jb_image *img, uint64_t *nodes, uint64_t *cap, uint32_t *npages, uint32_t *maxlen,
                   int64_t *size, double *w_absent);
/* emitP[state][string(rune)] as the device sees it (minFloat if absent). */
double jb_image_emit(const jb_image *img, int state, uint32_t rune);
/* The x whose math.Log(float64(x)) the image's weights use (every frequency of a key a
 * Han run can spell, 1 for absent pieces, and pd.size), ascending and distinct: what a
 * caller fills jb_config.log_keys with.  *n receives the count; returns JB_ELIMIT when
 * it exceeds cap (keys may be NULL with cap 0 to ask for the count). */
int jb_image_log_keys(const jb_image *img, int64_t *keys, size_t cap, size_t *n);
/* Go math.Log as used for the weights (src/math/log.go algorithm). */
double jb_go_log(double x);

#ifdef __cplusplus
}
#endif
#endif /* JIEBAHIP_H */
