// Package jiebahip is the drop-in Go front end of the MI355X segmentation path:
// the API of github.com/ericlingit/jieba-go's Tokenizer (tokenizer.go:52-162,
// 372-379) over the C ABI of libjiebahip.so (include/jiebahip.h).
//
// Not built in the development image (no Go toolchain there); see
// INTEGRATION.md for how a maintainer wires it into the reference module.
package jiebahip

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../lib -ljiebahip -Wl,-rpath,${SRCDIR}/../lib
#include <stdlib.h>
#include "jiebahip.h"
*/
import "C"

import (
	"errors"
	"log"
	"math"
	"runtime"
	"sync"
	"unsafe"
)

// JiebaSize is the total count NewJiebaTokenizer uses (tokenizer.go:454).
const JiebaSize = 60101967

// Tokenizer mirrors the reference's Tokenizer: safe for concurrent Cut calls,
// AddWord takes the exclusive lock (tokenizer.go:82-83,152-153,376).
type Tokenizer struct {
	mu  sync.RWMutex
	ctx *C.jb_ctx
}

func lastError() string { return C.GoString(C.jb_last_error()) }

func open(dictPath, emitPath string, kind C.int, size int64) *Tokenizer {
	cd := C.CString(dictPath)
	ce := C.CString(emitPath)
	defer C.free(unsafe.Pointer(cd))
	defer C.free(unsafe.Pointer(ce))
	// cfg is Go memory passed to C by address, so every pointer it holds is C memory
	// (cgo pointer rules: no Go pointer to memory that holds Go pointers).
	var cfg C.jb_config
	cfg.dict_path = cd
	cfg.emit_path = ce
	cfg.dict_kind = kind
	cfg.size_override = C.int64_t(size)
	cfg.device = 0
	cfg.ndevices = 1
	// calcDagProba's weights are math.Log(tf) - math.Log(pd.size) (tokenizer.go:503,
	// 515-519): build the image once, list the values its weights need, take Go's own
	// math.Log of each and open the device context from that image with the table
	// (jb_open_image reweighs it; the trie is not placed again).
	var img *C.jb_image
	if rc := C.jb_image_build(&cfg, &img); rc != C.JB_OK {
		log.Fatal("jiebahip: ", lastError())
	}
	var n C.size_t
	if rc := C.jb_image_log_keys(img, nil, 0, &n); rc != C.JB_OK && rc != C.JB_ELIMIT {
		C.jb_image_free(img)
		log.Fatal("jiebahip: ", lastError())
	}
	cnt := int(n) + 1
	ckeys := (*C.int64_t)(C.malloc(C.size_t(cnt) * C.size_t(unsafe.Sizeof(C.int64_t(0)))))
	cvals := (*C.double)(C.malloc(C.size_t(cnt) * C.size_t(unsafe.Sizeof(C.double(0)))))
	defer C.free(unsafe.Pointer(ckeys))
	defer C.free(unsafe.Pointer(cvals))
	if rc := C.jb_image_log_keys(img, ckeys, n, &n); rc != C.JB_OK {
		C.jb_image_free(img)
		log.Fatal("jiebahip: ", lastError())
	}
	keys := unsafe.Slice(ckeys, cnt)
	vals := unsafe.Slice(cvals, cnt)
	for i := 0; i < int(n); i++ {
		vals[i] = C.double(math.Log(float64(keys[i])))
	}
	cfg.log_keys = ckeys
	cfg.log_vals = cvals
	cfg.nlog = n
	var ctx *C.jb_ctx
	if rc := C.jb_open_image(img, &cfg, &ctx); rc != C.JB_OK { // consumes img
		// the reference stops the process on load errors (tokenizer.go:397,443,656)
		log.Fatal("jiebahip: ", lastError())
	}
	t := &Tokenizer{ctx: ctx}
	runtime.SetFinalizer(t, (*Tokenizer).Close)
	return t
}

// NewTokenizer loads a dict.txt-format dictionary (tokenizer.go:61).
func NewTokenizer(dictionaryFile string) *Tokenizer {
	return open(dictionaryFile, "prob_emit.json", C.JB_DICT_TXT, 0)
}

// NewJiebaTokenizer is the reference's default tokenizer (tokenizer.go:69):
// it decodes prefix_dictionary.gob (tokenizer.go:439-458) with size 60,101,967.
func NewJiebaTokenizer() *Tokenizer {
	return open("prefix_dictionary.gob", "prob_emit.json", C.JB_DICT_GOB, 0)
}

// NewTokenizerFromImage opens an image written by Save: no parsing, no trie build.
func NewTokenizerFromImage(path string) *Tokenizer {
	return open(path, "", C.JB_DICT_IMAGE, 0)
}

// Save writes the current dictionary (AddWord changes included) as an image.
func (t *Tokenizer) Save(path string) error {
	t.mu.RLock()
	defer t.mu.RUnlock()
	cp := C.CString(path)
	defer C.free(unsafe.Pointer(cp))
	if rc := C.jb_save(t.ctx, cp); rc != C.JB_OK {
		return errors.New("jiebahip: " + lastError())
	}
	return nil
}

// Close releases the device context.
func (t *Tokenizer) Close() {
	t.mu.Lock()
	defer t.mu.Unlock()
	if t.ctx != nil {
		C.jb_close(t.ctx)
		t.ctx = nil
	}
}

func spansToTokens(text string, s *C.jb_spans, doc int) []string {
	n := int(s.ntokens)
	starts := unsafe.Slice((*uint64)(unsafe.Pointer(s.start)), n)
	ends := unsafe.Slice((*uint64)(unsafe.Pointer(s.end)), n)
	docTok := unsafe.Slice((*uint64)(unsafe.Pointer(s.doc_tok)), int(s.ndocs)+1)
	a, b := int(docTok[doc]), int(docTok[doc+1])
	out := make([]string, 0, b-a)
	for k := a; k < b; k++ {
		st, en := int(starts[k]), int(ends[k])
		if en-st == 1 && text[st] >= 0x80 {
			out = append(out, "�") // invalid UTF-8 byte (tokenizer.go:301-306)
		} else {
			out = append(out, text[st:en])
		}
	}
	return out
}

// cut32 cuts a batch held in buf (documents [off[d], off[d+1]), off[0] == 0) into u32
// spans (jb_cut_batch_into32) in Go slices: half the bytes the library writes for u64
// spans, which bound a host batch's host side.  A first try has room for one token per
// three bytes; on JB_ELIMIT a second one has the count the library returned.  The slices
// hold no Go pointers, so cgo lets C write them during the call (it keeps none).
func (t *Tokenizer) cut32(buf []byte, off []uint64, hmm C.int) (starts, ends []uint32, docTok []uint64) {
	n := len(off) - 1
	total := int(off[n] - off[0])
	docTok = make([]uint64, n+1)
	capTok := total/3 + 64
	for try := 0; try < 2; try++ {
		starts = make([]uint32, capTok)
		ends = make([]uint32, capTok)
		var nt C.uint64_t
		rc := C.jb_cut_batch_into32(t.ctx, (*C.uint8_t)(unsafe.Pointer(&buf[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
			C.uint32_t(n), hmm, (*C.uint32_t)(unsafe.Pointer(&starts[0])), (*C.uint32_t)(unsafe.Pointer(&ends[0])),
			C.uint64_t(capTok), (*C.uint64_t)(unsafe.Pointer(&docTok[0])), &nt)
		if rc == C.JB_OK {
			return starts[:int(nt)], ends[:int(nt)], docTok
		}
		if rc == C.JB_ELIMIT && int(nt) > capTok {
			capTok = int(nt)
			continue
		}
		// JB_EPANIC: the reference panics on this input (cutDAG slice with tail -1)
		panic("jiebahip: " + lastError())
	}
	panic("jiebahip: " + lastError())
}

// tokens [a, b) of u32 spans over text (offsets from text's first byte) as strings.
func tokens32(text string, starts, ends []uint32, a, b int) []string {
	out := make([]string, 0, b-a)
	for k := a; k < b; k++ {
		st, en := int(starts[k]), int(ends[k])
		if en-st == 1 && text[st] >= 0x80 {
			out = append(out, "�") // invalid UTF-8 byte (tokenizer.go:301-306)
		} else {
			out = append(out, text[st:en])
		}
	}
	return out
}

// Cut segments one text (tokenizer.go:151).  Never returns nil.
func (t *Tokenizer) Cut(text string, useHmm bool) []string {
	t.mu.RLock()
	defer t.mu.RUnlock()
	if len(text) == 0 {
		return []string{}
	}
	b := []byte(text)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	if uint64(len(b)) < 1<<32 { // u32 spans (jb_cut_batch_into32)
		starts, ends, _ := t.cut32(b, []uint64{0, uint64(len(b))}, hmm)
		return tokens32(text, starts, ends, 0, len(starts))
	}
	var s C.jb_spans
	if rc := C.jb_cut(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), C.size_t(len(b)), hmm, &s); rc != C.JB_OK {
		// JB_EPANIC: the reference panics on this input (cutDAG slice with tail -1)
		panic("jiebahip: " + lastError())
	}
	defer C.jb_spans_free(&s)
	return spansToTokens(text, &s, 0)
}

// CutForSearch is search-engine mode (jieba's cut_for_search; the reference has only Cut):
// the tokens of Cut, each Han token of three or more runes preceded by the dictionary
// words of two, then three, runes inside it that buildDag has as edges, in text order
// (jb_cut_batch_search in jiebahip.h, with its two differences from Python jieba: a gram
// buildDag cannot see is not emitted, and non-Han tokens are never expanded).  Never
// returns nil.
func (t *Tokenizer) CutForSearch(text string, useHmm bool) []string {
	t.mu.RLock()
	defer t.mu.RUnlock()
	if len(text) == 0 {
		return []string{}
	}
	b := []byte(text)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	off := []uint64{0, uint64(len(b))}
	var s C.jb_spans
	if rc := C.jb_cut_batch_search(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
		1, hmm, &s); rc != C.JB_OK {
		// JB_EPANIC: the reference panics on this input (cutDAG slice with tail -1)
		panic("jiebahip: " + lastError())
	}
	defer C.jb_spans_free(&s)
	return spansToTokens(text, &s, 0)
}

// CutAll is full mode (jieba's cut_all=True; the reference has only Cut): every dictionary
// word of two or more runes in the text's Han blocks, by start and then by length, overlapping
// words included, and the single runes that no such word accounts for; non-Han text as Cut
// cuts it (jb_cut_batch_full in jiebahip.h, with its three differences from Python jieba: the
// DAG is buildDag's, non-Han text is cutNonZh's, the Han class is unicode.Han).  The HMM is
// never consulted.  With the dictionary 甲 5 / 甲乙 5 / 甲乙丙 0 / 甲乙丙丁 5 / 乙 5 / 乙丙 5 /
// 丙 5 / 丁 5, CutAll("甲乙丙丁戊丁") is 甲乙, 甲乙丙丁, 乙丙, 丁, 戊, 丁 (tests/c_abi_full.c).
// Never returns nil.
func (t *Tokenizer) CutAll(text string) []string {
	t.mu.RLock()
	defer t.mu.RUnlock()
	if len(text) == 0 {
		return []string{}
	}
	b := []byte(text)
	off := []uint64{0, uint64(len(b))}
	var s C.jb_spans
	if rc := C.jb_cut_batch_full(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
		1, &s); rc != C.JB_OK {
		// JB_EPANIC: the reference panics on this input (cutDAG slice with tail -1)
		panic("jiebahip: " + lastError())
	}
	defer C.jb_spans_free(&s)
	return spansToTokens(text, &s, 0)
}

// IDUnknown is the id of a token that is not in the vocabulary (JB_ID_UNK).
const IDUnknown = ^uint32(0)

// SetVocab attaches the caller's vocabulary (jb_vocab_set in jiebahip.h): a key's id is its
// index in keys; keys are 1..255 bytes each and distinct.  It replaces any earlier vocabulary;
// nil removes it, an empty non-nil slice attaches an empty one.  On an error the old one stays.
func (t *Tokenizer) SetVocab(keys []string) error {
	t.mu.Lock()
	defer t.mu.Unlock()
	if keys == nil {
		if rc := C.jb_vocab_set(t.ctx, nil, nil, 0); rc != C.JB_OK {
			return errors.New("jiebahip: " + lastError())
		}
		return nil
	}
	buf := make([]byte, 0, 16)
	off := make([]uint64, len(keys)+1)
	for i, k := range keys {
		buf = append(buf, k...)
		off[i+1] = uint64(len(buf))
	}
	buf = append(buf, 0)
	if rc := C.jb_vocab_set(t.ctx, (*C.uint8_t)(unsafe.Pointer(&buf[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
		C.uint32_t(len(keys))); rc != C.JB_OK {
		return errors.New("jiebahip: " + lastError())
	}
	return nil
}

// CutIds is Cut (mode "cut"), CutForSearch ("search") or CutAll ("full", useHmm ignored) with
// each token's id in the attached vocabulary, looked up on the GPU (jb_spans_ids): IDUnknown
// for a token that is not a key.  With mini_dict.txt and the vocabulary abc, 今天, "�", 一刹那,
// 刹那, 这, 天天, CutIds("abc \xff今天天氣 这一刹那", false, "cut") is abc, �, 今天, 天, 氣, 这,
// 一刹那 with ids 0, 2, 1, unknown, unknown, 5, 3 (tests/c_abi_ids.c).  Never returns nil.
func (t *Tokenizer) CutIds(text string, useHmm bool, mode string) ([]string, []uint32) {
	t.mu.RLock()
	defer t.mu.RUnlock()
	if len(text) == 0 {
		return []string{}, []uint32{}
	}
	b := []byte(text)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	off := []uint64{0, uint64(len(b))}
	tp := (*C.uint8_t)(unsafe.Pointer(&b[0]))
	op := (*C.uint64_t)(unsafe.Pointer(&off[0]))
	var s C.jb_spans
	var rc C.int
	switch mode {
	case "cut":
		rc = C.jb_cut_batch(t.ctx, tp, op, 1, hmm, &s)
	case "search":
		rc = C.jb_cut_batch_search(t.ctx, tp, op, 1, hmm, &s)
	case "full":
		rc = C.jb_cut_batch_full(t.ctx, tp, op, 1, &s)
	default:
		panic("jiebahip: CutIds mode " + mode + ": one of cut, search, full")
	}
	if rc != C.JB_OK {
		// JB_EPANIC: the reference panics on this input (cutDAG slice with tail -1)
		panic("jiebahip: " + lastError())
	}
	defer C.jb_spans_free(&s)
	ids := make([]uint32, int(s.ntokens))
	if len(ids) > 0 {
		if rc := C.jb_spans_ids(t.ctx, tp, &s, (*C.uint32_t)(unsafe.Pointer(&ids[0]))); rc != C.JB_OK {
			panic("jiebahip: " + lastError()) // JB_EINVAL: no vocabulary attached
		}
	}
	return spansToTokens(text, &s, 0), ids
}

// Tag is one keyword of ExtractTags: the term's id in the attached vocabulary, its score
// (count x weight, as float32) and its count in the document.
type Tag struct {
	ID    uint32
	Score float32
	Count uint32
}

// ExtractTags is jieba.analyse.extract_tags over a batch of documents (jb_keywords_batch): per
// document the topK (1..64) terms of the attached vocabulary by count x weights[id], best first,
// ties by id.  A term whose weight is not > 0 (zero, negative, NaN) or whose id is past the table
// is no candidate: that is how stop words and one-rune words are left out.  Cutting (plain Cut),
// lookup, counting and ranking all run on the GPU; only the records come back.  The differences
// from jieba's (closed vocabulary, no division by the token total, ties by id) are listed in
// jiebahip.h.  With mini_dict.txt, the vocabulary abc, 今天, "�", 一刹那, 刹那, 这, 天天 and the
// weights 1, 1.5, 0.5, 2, 1, 0, 1, ExtractTags([]string{"abc abc 今天"}, w, 3, false) is
// {{0, 2, 2}, {1, 1.5, 1}} (tests/c_abi_keywords.c).  Never returns nil.
func (t *Tokenizer) ExtractTags(docs []string, weights []float32, topK int, useHmm bool) [][]Tag {
	t.mu.RLock()
	defer t.mu.RUnlock()
	out := make([][]Tag, len(docs))
	if len(docs) == 0 {
		return out
	}
	if topK < 1 || topK > C.JB_KW_MAXK {
		panic("jiebahip: ExtractTags topK out of range")
	}
	off := make([]uint64, len(docs)+1)
	total := 0
	for i, d := range docs {
		total += len(d)
		off[i+1] = uint64(total)
	}
	b := make([]byte, 0, total+1)
	for _, d := range docs {
		b = append(b, d...)
	}
	b = append(b, 0) // (never an empty slice: its address is passed)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	nrec := len(docs) * topK
	id := make([]uint32, nrec)
	score := make([]float32, nrec)
	cnt := make([]uint32, nrec)
	n := make([]uint32, len(docs))
	var wp *C.float
	if len(weights) > 0 {
		wp = (*C.float)(unsafe.Pointer(&weights[0]))
	}
	rc := C.jb_keywords_batch(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
		C.uint32_t(len(docs)), hmm, wp, C.uint32_t(len(weights)), C.uint32_t(topK),
		(*C.uint32_t)(unsafe.Pointer(&id[0])), (*C.float)(unsafe.Pointer(&score[0])),
		(*C.uint32_t)(unsafe.Pointer(&cnt[0])), (*C.uint32_t)(unsafe.Pointer(&n[0])))
	if rc != C.JB_OK {
		// JB_EINVAL: no vocabulary attached; JB_EPANIC: the reference panics on this input
		panic("jiebahip: " + lastError())
	}
	for d := range docs {
		out[d] = make([]Tag, int(n[d]))
		for r := range out[d] {
			out[d][r] = Tag{id[d*topK+r], score[d*topK+r], cnt[d*topK+r]}
		}
	}
	return out
}

// Rank is one keyword of TextRank: the word's id in the attached vocabulary and its score, which is
// 1 for a document's best word (jieba's normalisation).
type Rank struct {
	Id    uint32
	Score float32
}

// TextRank is jieba.analyse.textrank over a batch of documents: per document the topK words of the
// attached vocabulary (SetVocab) by PageRank over the co-occurrence graph of the kept tokens that
// lie within span positions of each other, after iters Jacobi rounds, best first, ties by id.
// jieba's values are span 5 and 10 rounds.  keep holds one byte per id and carries jieba's
// part-of-speech, length and stop-word filters; ids past it are not kept.  No weight table is
// needed.  Cutting (plain Cut), lookup, counting and ranking all run on the GPU; only the records
// come back.  The rule and its differences from jieba's (Jacobi rounds, closed vocabulary, ties by
// id, fixed-point sums) are in jiebahip.h.  With mini_dict.txt, the vocabulary abc, 今天, "�",
// 一刹那, 刹那, 这, 天天 and keep 1 1 1 1 1 0 1, TextRank([]string{"abc abc 今天"}, keep, 3, 5,
// 10, false) has the two nodes abc and 今天, abc first with score 1 (tests/c_abi_textrank.c).
// Never returns nil.
func (t *Tokenizer) TextRank(docs []string, keep []byte, topK, span, iters int, useHmm bool) [][]Rank {
	t.mu.RLock()
	defer t.mu.RUnlock()
	out := make([][]Rank, len(docs))
	if len(docs) == 0 {
		return out
	}
	if topK < 1 || topK > C.JB_KW_MAXK {
		panic("jiebahip: TextRank topK out of range")
	}
	if span < 2 || span > C.JB_TR_MAXSPAN || iters < 0 || iters > C.JB_TR_MAXITER {
		panic("jiebahip: TextRank span or iters out of range")
	}
	off := make([]uint64, len(docs)+1)
	total := 0
	for i, d := range docs {
		total += len(d)
		off[i+1] = uint64(total)
	}
	b := make([]byte, 0, total+1)
	for _, d := range docs {
		b = append(b, d...)
	}
	b = append(b, 0) // (never an empty slice: its address is passed)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	nrec := len(docs) * topK
	id := make([]uint32, nrec)
	score := make([]float32, nrec)
	n := make([]uint32, len(docs))
	var kp *C.uint8_t
	if len(keep) > 0 {
		kp = (*C.uint8_t)(unsafe.Pointer(&keep[0]))
	}
	rc := C.jb_textrank_batch(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
		C.uint32_t(len(docs)), hmm, kp, C.uint32_t(len(keep)), C.uint32_t(span), C.uint32_t(iters), C.uint32_t(topK),
		(*C.uint32_t)(unsafe.Pointer(&id[0])), (*C.float)(unsafe.Pointer(&score[0])),
		(*C.uint32_t)(unsafe.Pointer(&n[0])))
	if rc != C.JB_OK {
		// JB_EINVAL: no vocabulary attached; JB_EPANIC: the reference panics on this input
		panic("jiebahip: " + lastError())
	}
	for d := range docs {
		out[d] = make([]Rank, int(n[d]))
		for r := range out[d] {
			out[d][r] = Rank{id[d*topK+r], score[d*topK+r]}
		}
	}
	return out
}

// WordCount is one distinct token of a corpus with the number of times it was cut.
type WordCount struct {
	Word  string
	Count uint64
}

// WordCounts counts the distinct tokens of a batch of texts, in the cut of mode (C.JB_MODE_CUT,
// C.JB_MODE_SEARCH, C.JB_MODE_FULL; full mode ignores useHmm): the words by count descending and then by
// bytes, without those below minCount, the first maxKeys of them (0: all).  The cut and the counting both run
// on the GPU, in a table of nslots slots (a power of two; new words are accepted while fewer than half are
// taken) and poolBytes for the words over 24 bytes; only the distinct words come back.  exact is false when
// tokens were dropped for lack of room or two words shared a fingerprint: every count is a lower bound then.
// With mini_dict.txt, WordCounts([]string{"这一刹那 abc abc"}, false, C.JB_MODE_CUT, 1, 0, 1024, 4096) is
// {abc 2} {一刹那 1} {这 1} (tests/c_abi_wc.c).  Never returns nil.
func (t *Tokenizer) WordCounts(texts []string, useHmm bool, mode int, minCount, maxKeys, nslots, poolBytes uint64) (words []WordCount, exact bool) {
	t.mu.RLock()
	defer t.mu.RUnlock()
	words = []WordCount{}
	off := make([]uint64, len(texts)+1)
	total := 0
	for i, d := range texts {
		total += len(d)
		off[i+1] = uint64(total)
	}
	b := make([]byte, 0, total+1)
	for _, d := range texts {
		b = append(b, d...)
	}
	b = append(b, 0) // (never an empty slice: its address is passed)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	ntable := C.jb_wc_table_bytes(C.uint64_t(nslots), C.uint64_t(poolBytes))
	var table unsafe.Pointer
	if C.jb_device_alloc(t.ctx, ntable, &table) != C.JB_OK {
		panic("jiebahip: " + lastError())
	}
	defer C.jb_device_free(t.ctx, table)
	var r C.jb_wc_result
	rc := C.jb_wc_init_device(t.ctx, table, ntable, C.uint64_t(nslots), C.uint64_t(poolBytes), nil)
	if rc == C.JB_OK {
		rc = C.jb_wc_batch(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
			C.uint32_t(len(texts)), hmm, C.int(mode), table, ntable)
	}
	if rc == C.JB_OK {
		rc = C.jb_wc_read(t.ctx, table, ntable, nil, C.uint64_t(minCount), C.uint64_t(maxKeys), &r)
	}
	if rc != C.JB_OK {
		// JB_EINVAL: an unknown mode or a bad nslots; JB_EPANIC: the reference panics on this input
		panic("jiebahip: " + lastError())
	}
	defer C.jb_wc_result_free(&r)
	n := int(r.nkeys)
	koff := unsafe.Slice((*uint64)(unsafe.Pointer(r.key_off)), n+1)
	cnt := unsafe.Slice((*uint64)(unsafe.Pointer(r.counts)), n)
	keys := C.GoBytes(unsafe.Pointer(r.keys), C.int(koff[n]))
	for i := 0; i < n; i++ {
		words = append(words, WordCount{string(keys[koff[i]:koff[i+1]]), cnt[i]})
	}
	return words, r.ndropped == 0 && r.ncollided == 0
}

// MinHash sketches every text of a batch for near-duplicate detection: the cut of mode (C.JB_MODE_CUT,
// C.JB_MODE_SEARCH, C.JB_MODE_FULL; full mode ignores useHmm), shingles of n consecutive words (1 to
// JB_MH_MAXN) and k hash functions (1 to JB_MH_MAXK) of seed, all on the GPU; only the signatures come
// back.  sig[d] holds text d's k slots, docN[d] its shingle count; two texts agree in a slot with the
// probability of their shingle sets' Jaccard similarity.  A text without tokens has docN 0 and
// JB_MH_EMPTY in every slot.  The rule is jiebahip.h's (tests/c_abi_minhash.c).  Never returns nil.
func (t *Tokenizer) MinHash(texts []string, n, k int, seed uint64, useHmm bool, mode int) (sig [][]uint32, docN []uint32) {
	t.mu.RLock()
	defer t.mu.RUnlock()
	sig = make([][]uint32, len(texts))
	docN = make([]uint32, len(texts))
	if len(texts) == 0 {
		return sig, docN
	}
	if n < 1 || n > C.JB_MH_MAXN || k < 1 || k > C.JB_MH_MAXK {
		panic("jiebahip: MinHash n or k out of range")
	}
	off := make([]uint64, len(texts)+1)
	total := 0
	for i, d := range texts {
		total += len(d)
		off[i+1] = uint64(total)
	}
	b := make([]byte, 0, total+1)
	for _, d := range texts {
		b = append(b, d...)
	}
	b = append(b, 0) // (never an empty slice: its address is passed)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	flat := make([]uint32, len(texts)*k)
	rc := C.jb_minhash_batch(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
		C.uint32_t(len(texts)), hmm, C.int(mode), C.uint32_t(n), C.uint32_t(k), C.uint64_t(seed),
		(*C.uint32_t)(unsafe.Pointer(&flat[0])), (*C.uint32_t)(unsafe.Pointer(&docN[0])))
	if rc != C.JB_OK {
		// JB_EINVAL: an unknown mode; JB_EPANIC: the reference panics on this input
		panic("jiebahip: " + lastError())
	}
	for d := range texts {
		sig[d] = flat[d*k : (d+1)*k]
	}
	return sig, docN
}

// NearDuplicates groups the near-duplicates of a batch: MinHash as above, then b LSH bands of r rows, the bucket
// join inside the window w (1 to JB_ND_MAXWIN) and the verification against all k slots on the GPU
// (jb_neardup_sig), and the groups' labels (jb_neardup_labels).  label[d] is the least text of d's group, so
// label[d] == d marks the one text of each group to keep.  minAgree is the least number of equal slots of a kept
// pair; 0 means the integer nearest 0.8 k.  Never returns nil.
func (t *Tokenizer) NearDuplicates(texts []string, n, k, b, r, w, minAgree int, seed uint64, useHmm bool, mode int) (label []uint32) {
	label = make([]uint32, len(texts))
	if len(texts) == 0 {
		return label
	}
	sig, docN := t.MinHash(texts, n, k, seed, useHmm, mode)
	if minAgree == 0 {
		minAgree = (4*k + 2) / 5
		if minAgree < 1 {
			minAgree = 1
		}
	}
	t.mu.RLock()
	defer t.mu.RUnlock()
	flat := sig[0][:len(texts)*k : len(texts)*k] // (MinHash's rows are slices of one array)
	pairOff := make([]uint64, len(texts)+1)
	var stat [C.JB_ND_NSTAT]C.uint64_t
	var np C.uint64_t
	pcap := 4*len(texts) + 1024
	var pairDoc, pairAgree []uint32
	for pass := 0; pass < 2; pass++ {
		pairDoc = make([]uint32, pcap)
		pairAgree = make([]uint32, pcap)
		rc := C.jb_neardup_sig(t.ctx, (*C.uint32_t)(unsafe.Pointer(&flat[0])), (*C.uint32_t)(unsafe.Pointer(&docN[0])),
			C.uint32_t(len(texts)), C.uint32_t(k), C.uint32_t(b), C.uint32_t(r), C.uint32_t(w), C.uint32_t(minAgree),
			(*C.uint32_t)(unsafe.Pointer(&pairDoc[0])), (*C.uint32_t)(unsafe.Pointer(&pairAgree[0])), C.uint64_t(pcap),
			(*C.uint64_t)(unsafe.Pointer(&pairOff[0])), &np, &stat[0])
		if rc == C.JB_ELIMIT && uint64(np) > uint64(pcap) && pass == 0 {
			pcap = int(np) // (the arrays were too small: the count is known now)
			continue
		}
		if rc != C.JB_OK {
			panic("jiebahip: " + lastError())
		}
		break
	}
	if rc := C.jb_neardup_labels((*C.uint64_t)(unsafe.Pointer(&pairOff[0])), (*C.uint32_t)(unsafe.Pointer(&pairDoc[0])),
		np, C.uint32_t(len(texts)), (*C.uint32_t)(unsafe.Pointer(&label[0]))); rc != C.JB_OK {
		panic("jiebahip: " + lastError())
	}
	return label
}

// Colloc is one collocation: word A directly followed by word B, Count times, with its Score.
type Colloc struct {
	A, B  string
	Count uint64
	Score float32
}

// Collocations counts how often word a is directly followed by word b over a batch of texts, against how often
// each occurs alone, and scores the pairs (C.JB_COLLOC_NPMI, C.JB_COLLOC_RATIO, C.JB_COLLOC_COUNT), all on the
// GPU under the attached vocabulary, whose keys (what SetVocab was given) name the pairs: best first, by score,
// count and ids; only the candidates with at least minCount occurrences and a score of at least threshold come
// back, the first topn of them (0: all).  contiguous counts a pair only when the two tokens touch in the text,
// so that A + B is a substring: the top pairs the dictionary lacks are the words to AddWord.  nslots sizes the
// pair table (a power of two; new pairs are accepted while fewer than half are taken); exact is false when
// pairs were dropped for lack of room.  With mini_dict.txt and the vocabulary {abc, 一刹那, 这},
// Collocations([]string{"这一刹那 abc abc"}, keys, C.JB_COLLOC_COUNT, 1, 0, 0, false, false, 1024) is
// {这 一刹那 1} {一刹那 abc 1} {abc abc 1} in the order of the ids (tests/c_abi_colloc.c).  Never returns nil.
func (t *Tokenizer) Collocations(texts []string, keys []string, scorer int, minCount uint64, threshold float32, topn uint64, contiguous, useHmm bool, nslots uint64) (pairs []Colloc, exact bool) {
	t.mu.RLock()
	defer t.mu.RUnlock()
	pairs = []Colloc{}
	nv := int64(C.jb_vocab_size(t.ctx))
	if nv < 0 || nv != int64(len(keys)) {
		panic("jiebahip: Collocations: keys are not the attached vocabulary's (SetVocab)")
	}
	off := make([]uint64, len(texts)+1)
	total := 0
	for i, d := range texts {
		total += len(d)
		off[i+1] = uint64(total)
	}
	b := make([]byte, 0, total+1)
	for _, d := range texts {
		b = append(b, d...)
	}
	b = append(b, 0) // (never an empty slice: its address is passed)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	flags := C.uint32_t(0)
	if contiguous {
		flags = C.JB_COLLOC_CONTIG
	}
	nuni := C.uint32_t(nv)
	ntable := C.jb_colloc_table_bytes(C.uint64_t(nslots))
	var table, uni unsafe.Pointer
	if C.jb_device_alloc(t.ctx, ntable, &table) != C.JB_OK {
		panic("jiebahip: " + lastError())
	}
	defer C.jb_device_free(t.ctx, table)
	if C.jb_device_alloc(t.ctx, C.size_t(nv)*8+8, &uni) != C.JB_OK {
		panic("jiebahip: " + lastError())
	}
	defer C.jb_device_free(t.ctx, uni)
	var r C.jb_colloc_result
	rc := C.jb_colloc_init_device(t.ctx, table, ntable, C.uint64_t(nslots), (*C.uint64_t)(uni), nuni, nil)
	if rc == C.JB_OK {
		rc = C.jb_colloc_batch(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
			C.uint32_t(len(texts)), hmm, nil, 0, flags, table, ntable, (*C.uint64_t)(uni), nuni)
	}
	if rc == C.JB_OK {
		rc = C.jb_colloc_read(t.ctx, table, ntable, (*C.uint64_t)(uni), nuni, C.int(scorer), C.uint64_t(minCount),
			C.float(threshold), C.uint64_t(topn), nil, &r)
	}
	if rc != C.JB_OK {
		// JB_EINVAL: an unknown scorer, minCount 0 or a bad nslots; JB_EPANIC: the reference panics on this input
		panic("jiebahip: " + lastError())
	}
	defer C.jb_colloc_result_free(&r)
	n := int(r.n)
	if n > 0 {
		ia := unsafe.Slice((*uint32)(unsafe.Pointer(r.a)), n)
		ib := unsafe.Slice((*uint32)(unsafe.Pointer(r.b)), n)
		cnt := unsafe.Slice((*uint64)(unsafe.Pointer(r.count)), n)
		sc := unsafe.Slice((*float32)(unsafe.Pointer(r.score)), n)
		for i := 0; i < n; i++ {
			pairs = append(pairs, Colloc{keys[ia[i]], keys[ib[i]], cnt[i], sc[i]})
		}
	}
	return pairs, r.dropped == 0
}

// FilterRule is jb_filter_rule: DropClasses holds C.JB_TC_* bits, MinRunes and MaxRunes (0: no upper bound) are at
// most 255, and Stop drops the tokens found in the stop set (SetStopWords).
type FilterRule struct {
	DropClasses, MinRunes, MaxRunes uint32
	Stop                            bool
}

func (r FilterRule) c() C.jb_filter_rule {
	var f C.jb_filter_rule
	if r.Stop {
		f.flags = C.JB_FILTER_STOP
	}
	f.drop_classes = C.uint32_t(r.DropClasses)
	f.min_runes = C.uint32_t(r.MinRunes)
	f.max_runes = C.uint32_t(r.MaxRunes)
	return f
}

// SetStopWords attaches the caller's stop list (1 to 255 bytes each, no duplicates), replacing any earlier one;
// nil removes it.  It is independent of SetVocab (jb_stopwords_set).
func (t *Tokenizer) SetStopWords(keys []string) error {
	t.mu.Lock()
	defer t.mu.Unlock()
	if keys == nil {
		if rc := C.jb_stopwords_set(t.ctx, nil, nil, 0); rc != C.JB_OK {
			return errors.New("jiebahip: " + lastError())
		}
		return nil
	}
	buf := make([]byte, 0, 16)
	off := make([]uint64, len(keys)+1)
	for i, k := range keys {
		buf = append(buf, k...)
		off[i+1] = uint64(len(buf))
	}
	buf = append(buf, 0)
	if rc := C.jb_stopwords_set(t.ctx, (*C.uint8_t)(unsafe.Pointer(&buf[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
		C.uint32_t(len(keys))); rc != C.JB_OK {
		return errors.New("jiebahip: " + lastError())
	}
	return nil
}

// SetBatchFilter stores a rule that CutJoin, WordCounts and MinHash filter the cut's tokens by before their own
// step; nil clears it (jb_batch_filter_set).
func (t *Tokenizer) SetBatchFilter(rule *FilterRule) error {
	t.mu.Lock()
	defer t.mu.Unlock()
	var rc C.int
	if rule == nil {
		rc = C.jb_batch_filter_set(t.ctx, nil)
	} else {
		f := rule.c()
		rc = C.jb_batch_filter_set(t.ctx, &f)
	}
	if rc != C.JB_OK {
		return errors.New("jiebahip: " + lastError())
	}
	return nil
}

// CutFiltered is Cut (or the cut of mode: C.JB_MODE_CUT, C.JB_MODE_SEARCH, C.JB_MODE_FULL; full mode ignores
// useHmm) for every text of a batch with the tokens the rule drops left out, by class, length in runes and the
// stop set; the cut and the filter both run on the GPU (jb_cut_batch_filter).  A kept invalid byte comes out as
// U+FFFD.  Never returns nil.
func (t *Tokenizer) CutFiltered(texts []string, rule FilterRule, useHmm bool, mode int) [][]string {
	t.mu.RLock()
	defer t.mu.RUnlock()
	out := make([][]string, len(texts))
	if len(texts) == 0 {
		return out
	}
	off := make([]uint64, len(texts)+1)
	total := 0
	for i, d := range texts {
		total += len(d)
		off[i+1] = uint64(total)
	}
	b := make([]byte, 0, total+1)
	for _, d := range texts {
		b = append(b, d...)
	}
	b = append(b, 0) // (never an empty slice: its address is passed)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	f := rule.c()
	tok := make([]uint64, len(texts)+1)
	start := make([]uint32, total+1)
	end := make([]uint32, total+1)
	var n C.uint64_t
	call := func() C.int {
		return C.jb_cut_batch_filter(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
			C.uint32_t(len(texts)), hmm, C.int(mode), &f, (*C.uint32_t)(unsafe.Pointer(&start[0])),
			(*C.uint32_t)(unsafe.Pointer(&end[0])), C.uint64_t(len(start)), (*C.uint64_t)(unsafe.Pointer(&tok[0])), &n, nil)
	}
	rc := call()
	if rc == C.JB_ELIMIT && uint64(n) > uint64(len(start)) { // (full mode: more spans than bytes)
		start = make([]uint32, uint64(n))
		end = make([]uint32, uint64(n))
		rc = call()
	}
	if rc != C.JB_OK {
		// JB_EINVAL: an unknown mode or rule, or Stop without a stop set; JB_EPANIC: the reference panics on this input
		panic("jiebahip: " + lastError())
	}
	for d := range texts {
		out[d] = make([]string, 0, tok[d+1]-tok[d])
		for k := tok[d]; k < tok[d+1]; k++ {
			if end[k]-start[k] == 1 && b[start[k]] >= 0x80 {
				out[d] = append(out[d], "\uFFFD")
			} else {
				out[d] = append(out[d], string(b[start[k]:end[k]]))
			}
		}
	}
	return out
}

// CutJoin is strings.Join(Cut(text), sep) for every text of a batch, with the cut of mode (C.JB_MODE_CUT,
// C.JB_MODE_SEARCH, C.JB_MODE_FULL; full mode ignores useHmm) and the join both on the GPU: only the joined
// bytes come back, no span and no token.  sep holds at most JB_JOIN_MAXSEP (8) bytes.  An invalid byte comes
// out as "�"; whitespace and non-Han blocks without an alnum byte are absent, as in Cut.  With mini_dict.txt,
// CutJoin([]string{"这一刹那", ""}, " ", false, C.JB_MODE_SEARCH) is {"这 一刹 刹那 一刹那", ""}
// (tests/c_abi_join.c).  Never returns nil.
func (t *Tokenizer) CutJoin(texts []string, sep string, useHmm bool, mode int) []string {
	t.mu.RLock()
	defer t.mu.RUnlock()
	out := make([]string, len(texts))
	if len(texts) == 0 {
		return out
	}
	if len(sep) > C.JB_JOIN_MAXSEP {
		panic("jiebahip: CutJoin separator longer than JB_JOIN_MAXSEP")
	}
	off := make([]uint64, len(texts)+1)
	total := 0
	for i, d := range texts {
		total += len(d)
		off[i+1] = uint64(total)
	}
	b := make([]byte, 0, total+1)
	for _, d := range texts {
		b = append(b, d...)
	}
	b = append(b, 0) // (never an empty slice: its address is passed)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	sb := append([]byte(sep), 0)
	var j C.jb_joined
	rc := C.jb_cut_batch_join(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
		C.uint32_t(len(texts)), hmm, C.int(mode), (*C.uint8_t)(unsafe.Pointer(&sb[0])), C.uint32_t(len(sep)), nil, 0, &j)
	if rc != C.JB_OK {
		// JB_EINVAL: an unknown mode; JB_EPANIC: the reference panics on this input
		panic("jiebahip: " + lastError())
	}
	defer C.jb_joined_free(&j)
	joined := C.GoBytes(unsafe.Pointer(j.text), C.int(j.nbytes))
	ooff := unsafe.Slice((*uint64)(unsafe.Pointer(j.doc_off)), len(texts)+1)
	for d := range texts {
		out[d] = string(joined[ooff[d]:ooff[d+1]])
	}
	return out
}

// Token is one entry of Tokenize: the word and its offsets in its text, in the unit asked for.
type Token struct {
	Word       string
	Start, End int
}

// Tokenize is jieba's tokenize for every text of a batch: the tokens of mode (C.JB_MODE_CUT, C.JB_MODE_SEARCH,
// C.JB_MODE_FULL; full mode ignores useHmm) with their offsets in runes (C.JB_UNIT_RUNE: indexes of
// []rune(text)) or in UTF-16 code units (C.JB_UNIT_UTF16: indexes of utf16.Encode([]rune(text))).  The cut and
// the conversion both run on the GPU (jb_cut_batch_charspans); no byte offset comes back.  An invalid byte is
// one rune, as in a range loop over the string, and its word is "�", as in Cut.  Never returns nil.
func (t *Tokenizer) Tokenize(texts []string, useHmm bool, mode, unit int) [][]Token {
	t.mu.RLock()
	defer t.mu.RUnlock()
	out := make([][]Token, len(texts))
	if len(texts) == 0 {
		return out
	}
	off := make([]uint64, len(texts)+1)
	total := 0
	for i, d := range texts {
		total += len(d)
		off[i+1] = uint64(total)
	}
	b := make([]byte, 0, total+1)
	for _, d := range texts {
		b = append(b, d...)
	}
	b = append(b, 0) // (never an empty slice: its address is passed)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	capTok := total/2 + 16
	var cs, ce []uint32
	tok := make([]uint64, len(texts)+1)
	units := make([]uint32, len(texts))
	var n C.uint64_t
	for pass := 0; ; pass++ {
		cs, ce = make([]uint32, capTok), make([]uint32, capTok)
		rc := C.jb_cut_batch_charspans(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
			C.uint32_t(len(texts)), hmm, C.int(mode), C.int(unit), (*C.uint32_t)(unsafe.Pointer(&cs[0])),
			(*C.uint32_t)(unsafe.Pointer(&ce[0])), C.uint64_t(capTok), (*C.uint64_t)(unsafe.Pointer(&tok[0])), &n,
			(*C.uint32_t)(unsafe.Pointer(&units[0])))
		if rc == C.JB_ELIMIT && int(n) > capTok && pass == 0 {
			capTok = int(n) // (the arrays were too small: the count is known now)
			continue
		}
		if rc != C.JB_OK {
			// JB_EINVAL: an unknown mode or unit; JB_EPANIC: the reference panics on this input
			panic("jiebahip: " + lastError())
		}
		break
	}
	for d, text := range texts {
		// at[u]: the byte at which unit u of the text starts (a range loop decodes as utf8.DecodeRune does)
		at := make([]int, int(units[d])+1)
		u := 0
		for i, r := range text {
			at[u] = i
			u++
			if unit == C.JB_UNIT_UTF16 && r >= 0x10000 {
				at[u] = i
				u++
			}
		}
		at[u] = len(text)
		toks := make([]Token, 0, tok[d+1]-tok[d])
		for k := tok[d]; k < tok[d+1]; k++ {
			w := text[at[cs[k]]:at[ce[k]]]
			if len(w) == 1 && w[0] >= 0x80 {
				w = "�" // invalid UTF-8 byte, as in Cut
			}
			toks = append(toks, Token{w, int(cs[k]), int(ce[k])})
		}
		out[d] = toks
	}
	return out
}

// IdfFit is the result of FitIdf: per id of the attached vocabulary its IDF weight and the number
// of documents it occurs in, and the number of documents fitted on.
type IdfFit struct {
	Weights []float32
	Df      []uint32
	Ndocs   uint64
}

// FitIdf fits IDF weights for the attached vocabulary on a corpus given as batches of documents
// (jb_df_batch per batch, then jb_idf).  Weights[id] is the smoothed IDF
// float32(log((Ndocs+1)/(Df[id]+1)) + 1) with the library's restatement of math.Log, or 0 where
// Df[id] is 0, below minDf, above maxDf (0: no upper bound) or where keep (nil, or one byte per
// id) is 0.  Cutting (plain Cut), lookup and counting run on the GPU; per batch only the
// counters come back.  ExtractTags(docs, fit.Weights, ...) afterwards is the whole of TF-IDF.
// With mini_dict.txt, the vocabulary abc, 今天, "�", 一刹那, 刹那, 这, 天天 and the documents
// "abc abc 今天", "abc \xff今天天氣 这一刹那", "这一刹那 今天", "", "刹那 abc", Df is
// {3, 3, 1, 2, 1, 2, 0} (tests/c_abi_df.c).
func (t *Tokenizer) FitIdf(batches [][]string, useHmm bool, minDf, maxDf uint32, keep []byte) IdfFit {
	t.mu.RLock()
	defer t.mu.RUnlock()
	nv := int64(C.jb_vocab_size(t.ctx))
	if nv < 0 {
		panic("jiebahip: FitIdf without a vocabulary (SetVocab)")
	}
	if keep != nil && int64(len(keep)) != nv {
		panic("jiebahip: FitIdf keep holds one byte per id")
	}
	if maxDf == 0 {
		maxDf = C.JB_DF_NOMAX
	}
	fit := IdfFit{Weights: make([]float32, nv), Df: make([]uint32, nv)}
	if nv == 0 {
		for _, docs := range batches {
			fit.Ndocs += uint64(len(docs))
		}
		return fit
	}
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	for _, docs := range batches {
		if len(docs) == 0 {
			continue
		}
		off := make([]uint64, len(docs)+1)
		total := 0
		for i, d := range docs {
			total += len(d)
			off[i+1] = uint64(total)
		}
		b := make([]byte, 0, total+1)
		for _, d := range docs {
			b = append(b, d...)
		}
		b = append(b, 0) // (never an empty slice: its address is passed)
		rc := C.jb_df_batch(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
			C.uint32_t(len(docs)), hmm, (*C.uint32_t)(unsafe.Pointer(&fit.Df[0])), C.uint32_t(nv))
		if rc != C.JB_OK {
			// JB_EPANIC: the reference panics on this input
			panic("jiebahip: " + lastError())
		}
		fit.Ndocs += uint64(len(docs))
	}
	var kp *C.uint8_t
	if keep != nil {
		kp = (*C.uint8_t)(unsafe.Pointer(&keep[0]))
	}
	rc := C.jb_idf((*C.uint32_t)(unsafe.Pointer(&fit.Df[0])), C.uint32_t(nv), C.uint64_t(fit.Ndocs),
		C.uint32_t(minDf), C.uint32_t(maxDf), kp, (*C.float)(unsafe.Pointer(&fit.Weights[0])))
	if rc != C.JB_OK {
		panic("jiebahip: " + lastError())
	}
	return fit
}

// Index is the result of Postings: the inverted index of a batch under the attached vocabulary.  The list
// of id t is Doc / Tf[Off[t]:Off[t+1]]: the documents that contain t, ascending, each with its term
// frequency.  DocLen[d] is document d's token count, unknown tokens included (BM25's document length).
type Index struct {
	Off    []uint64 // vocabulary size + 1
	Doc    []uint32
	Tf     []uint32
	DocLen []uint32
}

// Postings indexes one batch of documents (jb_postings_batch): plain Cut, the vocabulary lookup, the term
// counts and their transposition all run on the GPU, and only the index comes back.  Document numbers are
// docBase + the document's position in docs, so the lists of consecutive batches with a running docBase
// concatenate per id into the lists of the corpus.  With mini_dict.txt, the vocabulary and the documents
// of FitIdf's comment, the list of id 0 (abc) is documents {0, 1, 4} with frequencies {2, 1, 1}.
func (t *Tokenizer) Postings(docs []string, useHmm bool, docBase uint32) Index {
	t.mu.RLock()
	defer t.mu.RUnlock()
	nv := int64(C.jb_vocab_size(t.ctx))
	if nv < 0 {
		panic("jiebahip: Postings without a vocabulary (SetVocab)")
	}
	ix := Index{Off: make([]uint64, nv+1), DocLen: make([]uint32, len(docs))}
	if len(docs) == 0 {
		return ix
	}
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	off := make([]uint64, len(docs)+1)
	total := 0
	for i, d := range docs {
		total += len(d)
		off[i+1] = uint64(total)
	}
	b := make([]byte, 0, total+1)
	for _, d := range docs {
		b = append(b, d...)
	}
	b = append(b, 0) // (never an empty slice: its address is passed)
	// a first guess of one posting per four bytes; the full count comes back with JB_ELIMIT
	pcap := uint64(total/4 + 16)
	var n C.uint64_t
	for pass := 0; ; pass++ {
		ix.Doc = make([]uint32, pcap)
		ix.Tf = make([]uint32, pcap)
		rc := C.jb_postings_batch(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
			C.uint32_t(len(docs)), hmm, C.uint32_t(docBase), C.uint64_t(pcap), (*C.uint64_t)(unsafe.Pointer(&ix.Off[0])),
			C.uint32_t(nv), (*C.uint32_t)(unsafe.Pointer(&ix.Doc[0])), (*C.uint32_t)(unsafe.Pointer(&ix.Tf[0])), &n,
			(*C.uint32_t)(unsafe.Pointer(&ix.DocLen[0])))
		if rc == C.JB_ELIMIT && uint64(n) > pcap && pass == 0 {
			pcap = uint64(n)
			continue
		}
		if rc != C.JB_OK {
			// JB_EPANIC: the reference panics on this input
			panic("jiebahip: " + lastError())
		}
		break
	}
	ix.Doc = ix.Doc[:n]
	ix.Tf = ix.Tf[:n]
	return ix
}

// Hit is one result of Search: a document and its BM25 score in units of 2^-24.
type Hit struct {
	Doc   uint32
	Score uint64
}

// Value is the score as a plain number.
func (h Hit) Value() float64 { return float64(h.Score) / 16777216.0 }

// SetIndex attaches an index to search (jb_index_set): Postings' result for a corpus in one batch, or the
// batches' lists concatenated per id.  The postings, the documents' norms and the ids' BM25 weights stay on
// the device until the next SetIndex, ClearIndex or Close.  Whoosh's defaults are k1 = 1.2, b = 0.75.
func (t *Tokenizer) SetIndex(ix Index, k1, b float64) error {
	t.mu.Lock()
	defer t.mu.Unlock()
	if len(ix.Off) == 0 || len(ix.Doc) != len(ix.Tf) {
		return errors.New("jiebahip: SetIndex: an index without offsets, or Doc and Tf of different lengths")
	}
	var pd, pt, pl *C.uint32_t
	if len(ix.Doc) > 0 {
		pd = (*C.uint32_t)(unsafe.Pointer(&ix.Doc[0]))
		pt = (*C.uint32_t)(unsafe.Pointer(&ix.Tf[0]))
	}
	if len(ix.DocLen) > 0 {
		pl = (*C.uint32_t)(unsafe.Pointer(&ix.DocLen[0]))
	}
	rc := C.jb_index_set(t.ctx, (*C.uint64_t)(unsafe.Pointer(&ix.Off[0])), pd, pt, C.uint64_t(len(ix.Doc)),
		C.uint32_t(len(ix.Off)-1), pl, C.uint64_t(len(ix.DocLen)), C.double(k1), C.double(b))
	if rc != C.JB_OK {
		return errors.New("jiebahip: " + lastError())
	}
	return nil
}

// ClearIndex detaches the index (jb_index_clear).
func (t *Tokenizer) ClearIndex() error {
	t.mu.Lock()
	defer t.mu.Unlock()
	if rc := C.jb_index_clear(t.ctx); rc != C.JB_OK {
		return errors.New("jiebahip: " + lastError())
	}
	return nil
}

// Search ranks the attached index's documents for each query by BM25 (jb_search_batch): the query is cut in
// plain mode and looked up in the attached vocabulary, and at most topK documents come back per query, best
// first (score descending, ties by document ascending).  Cut, looked up and ranked on the GPU.
func (t *Tokenizer) Search(queries []string, topK uint32, useHmm bool) [][]Hit {
	t.mu.RLock()
	defer t.mu.RUnlock()
	out := make([][]Hit, len(queries))
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	off := make([]uint64, len(queries)+1)
	total := 0
	for i, q := range queries {
		total += len(q)
		off[i+1] = uint64(total)
	}
	b := make([]byte, 0, total+1)
	for _, q := range queries {
		b = append(b, q...)
	}
	b = append(b, 0) // (never an empty slice: its address is passed)
	k := int(topK)
	if k == 0 {
		k = 1
	}
	doc := make([]uint32, len(queries)*k+1)
	score := make([]uint64, len(queries)*k+1)
	n := make([]uint32, len(queries)+1)
	rc := C.jb_search_batch(t.ctx, (*C.uint8_t)(unsafe.Pointer(&b[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
		C.uint32_t(len(queries)), hmm, C.uint32_t(topK), (*C.uint32_t)(unsafe.Pointer(&doc[0])),
		(*C.uint64_t)(unsafe.Pointer(&score[0])), (*C.uint32_t)(unsafe.Pointer(&n[0])))
	if rc != C.JB_OK {
		// JB_EPANIC: the reference panics on this input
		panic("jiebahip: " + lastError())
	}
	for q := range queries {
		for r := 0; r < int(n[q]); r++ {
			out[q] = append(out[q], Hit{doc[q*k+r], score[q*k+r]})
		}
	}
	return out
}

// CutParallel (tokenizer.go:81) returns the tokens of Cut in document order.
// The library splits the work itself: the text goes to the device in pieces cut
// at Han-run starts (jb_split_points), and over every device of a multi-device
// context; numWorkers is accepted for API parity.  ordered=false allows any block
// order in the reference; this order is one of them.
func (t *Tokenizer) CutParallel(text string, hmm bool, numWorkers int, ordered bool) []string {
	return t.Cut(text, hmm)
}

// CutBatch segments many documents in one device call (the batched form of Cut).
func (t *Tokenizer) CutBatch(docs []string, useHmm bool) [][]string {
	t.mu.RLock()
	defer t.mu.RUnlock()
	total := 0
	for _, d := range docs {
		total += len(d)
	}
	buf := make([]byte, 0, total+1)
	off := make([]uint64, len(docs)+1)
	for i, d := range docs {
		buf = append(buf, d...)
		off[i+1] = uint64(len(buf))
	}
	buf = append(buf, 0)
	hmm := C.int(0)
	if useHmm {
		hmm = 1
	}
	all := string(buf[:total])
	out := make([][]string, len(docs))
	if uint64(total) < 1<<32 { // u32 spans (jb_cut_batch_into32); tokens share one copy of the batch text
		starts, ends, docTok := t.cut32(buf, off, hmm)
		for i := range docs {
			out[i] = tokens32(all, starts, ends, int(docTok[i]), int(docTok[i+1]))
		}
		return out
	}
	var s C.jb_spans
	if rc := C.jb_cut_batch(t.ctx, (*C.uint8_t)(unsafe.Pointer(&buf[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
		C.uint32_t(len(docs)), hmm, &s); rc != C.JB_OK {
		panic("jiebahip: " + lastError())
	}
	defer C.jb_spans_free(&s)
	for i := range docs {
		out[i] = spansToTokens(all, &s, i)
	}
	return out
}

// AddWord adds or updates a word (tokenizer.go:372).  freq < 1 takes
// suggestFreq's value (tokenizer.go:589-614).  Unlike the reference it does
// not deadlock.
func (t *Tokenizer) AddWord(word string, freq int) {
	t.mu.Lock()
	defer t.mu.Unlock()
	cw := C.CString(word)
	defer C.free(unsafe.Pointer(cw))
	f := C.int64_t(freq)
	if freq < 1 {
		if rc := C.jb_suggest_freq(t.ctx, cw, C.size_t(len(word)), &f); rc != C.JB_OK {
			log.Fatal("jiebahip: ", lastError())
		}
	}
	// Go's math.Log of the new frequency and of the new pd.size for the rebuild
	// (addTerm adds freq to pd.size even when the word was present, tokenizer.go:580-585)
	size := int64(C.jb_dict_size(t.ctx))
	keys := []int64{int64(f), size + int64(f)} // (Go memory without Go pointers: may be passed to C)
	vals := []float64{math.Log(float64(keys[0])), math.Log(float64(keys[1]))}
	if rc := C.jb_add_log(t.ctx, (*C.int64_t)(unsafe.Pointer(&keys[0])), (*C.double)(unsafe.Pointer(&vals[0])), 2); rc != C.JB_OK {
		log.Fatal("jiebahip: ", lastError())
	}
	// atomic: on an error the dictionary and the device image are unchanged
	if rc := C.jb_add_word(t.ctx, cw, C.size_t(len(word)), f); rc != C.JB_OK {
		log.Fatal("jiebahip: ", lastError())
	}
}
