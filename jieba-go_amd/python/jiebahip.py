"""ctypes binding of libjiebahip.so (include/jiebahip.h).

A thin Python view of the same C ABI the Go cgo wrapper binds
(jieba-go_amd/go/tokenizer.go): used by tests/, bench.py and
__graft_entry__.py.  `Tokenizer` mirrors jieba-go's API (tokenizer.go:52-162,
372-379): NewTokenizer / NewJiebaTokenizer / Cut / CutParallel / AddWord.

The library is loaded from jieba-go_amd/lib/ (built in-tree by
`make -C jieba-go_amd`); a missing or unloadable library raises — there is no
CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
# JB_LIB: another in-tree build of the same library (diagnostic variants, e.g. make STAMPS=1 OUT=var/stamps)
LIB_PATH = os.environ.get("JB_LIB") or os.path.join(PKG_DIR, "lib", "libjiebahip.so")

JB_OK, JB_EINVAL, JB_EIO, JB_EPARSE, JB_EDEVICE, JB_ENOMEM, JB_EPANIC, JB_ELIMIT = 0, -1, -2, -3, -4, -5, -6, -7
JB_DICT_TXT, JB_DICT_PREFIX, JB_DICT_GOB, JB_DICT_IMAGE = 0, 1, 2, 3
JIEBA_SIZE = 60_101_967  # tokenizer.go:454
JB_ID_UNK = 0xFFFFFFFF  # the id of a token that is not in the vocabulary
JB_KW_MAXK = 64  # the largest topk of the keyword calls
JB_TERMS_TILE = 4096  # tokens per sort tile of jb_terms_device
JB_DF_NOMAX = 0xFFFFFFFF  # max_df of the idf calls: no upper bound
JB_TR_MAXSPAN = 32  # the largest span of the textrank calls
JB_TR_MAXITER = 100  # the largest iters of the textrank calls
JB_JOIN_MAXSEP = 8  # the longest separator and terminator of the join calls, bytes
JB_JOIN_TILE = 2048  # tokens per scan tile of jb_join_device
JB_JOIN_LONG = 256  # a key of this many bytes or more takes jb_join_device's cooperative copy
JB_MODE_CUT, JB_MODE_SEARCH, JB_MODE_FULL = 0, 1, 2
_MODES = {"cut": JB_MODE_CUT, "search": JB_MODE_SEARCH, "full": JB_MODE_FULL}
JB_UNIT_RUNE, JB_UNIT_UTF16 = 0, 1  # the units of the character-offset calls
JB_CHAR_NONE = 0xFFFFFFFF  # a token without character offsets (malformed, outside its document, of no document)
JB_CHARSPANS_TILE = 4096  # text bytes per tile of jb_charspans_device
_UNITS = {"rune": JB_UNIT_RUNE, "utf16": JB_UNIT_UTF16}
JB_MH_MAXN, JB_MH_MAXK = 8, 256  # the widest shingle (tokens) and the most hash functions of the MinHash calls
JB_MH_TILE = 1024  # tokens per tile of jb_minhash_device's staged form
JB_MH_EMPTY = 0xFFFFFFFF  # every slot of a document without shingles
JB_MH_NOKEY = 0xFFFFFFFFFFFFFFFF  # every band key of a document without shingles
JB_TC_HAN, JB_TC_ALNUM, JB_TC_NUM, JB_TC_OTHER, JB_TC_INVALID = 1, 2, 4, 8, 16  # the token filter's classes
JB_FILTER_STOP = 1  # the filter rule's flag: drop the tokens found in the stop set
JB_FILTER_TILE = 2048  # tokens per tile of jb_filter_device
JB_POSTINGS_TILE = 4096  # entries per tile of jb_postings_device
JB_BM25_TILE = 8192  # documents per tile of jb_bm25_search_device
JB_BM25_MAXQ = 1024  # entries of a query that jb_bm25_search reads
JB_BM25_WMAX = float(1 << 20)  # the largest weight that takes part in a search
JB_BM25_ONE = 1 << 24  # a BM25 score's unit: score / JB_BM25_ONE is the plain value
JB_ND_TILE = 4096  # entries per tile of jb_neardup_device
JB_ND_MAXWIN = 64  # the widest window of the near-duplicate calls
JB_ND_NSTAT = 3  # the near-duplicate calls' counters: entries, candidates, members beyond the window
JB_COLLOC_CONTIG = 1  # the collocation calls' flag: a pair counts only when end[k] == start[k+1]
JB_COLLOC_NPMI, JB_COLLOC_RATIO, JB_COLLOC_COUNT = 0, 1, 2
JB_COLLOC_TILE = 256  # tokens per tile of jb_colloc_add_device
JB_COLLOC_LDS = 2048  # entries of each of the combining count pass's two LDS tables
JB_COLLOC_SHARE = 64  # the combining count pass: a workgroup's share is at least this many tiles
_SCORERS = {"npmi": JB_COLLOC_NPMI, "ratio": JB_COLLOC_RATIO, "count": JB_COLLOC_COUNT}
JB_ND_NENTRIES, JB_ND_NCAND, JB_ND_NTRUNC = 0, 1, 2
_CLASSES = {"han": JB_TC_HAN, "alnum": JB_TC_ALNUM, "num": JB_TC_NUM, "other": JB_TC_OTHER, "invalid": JB_TC_INVALID}
_TOKENIZE_MODES = {"default": JB_MODE_CUT, "search": JB_MODE_SEARCH, "full": JB_MODE_FULL}

# Every symbol include/jiebahip.h declares.
EXPORTS = [
    "jb_open", "jb_close", "jb_last_error", "jb_cut", "jb_cut_batch", "jb_cut_batch_into", "jb_spans_free",
    "jb_cut_device", "jb_cut_device_into", "jb_open_image", "jb_cut_batch_mask", "jb_host_alloc", "jb_host_free",
    "jb_split_points",
    "jb_add_word", "jb_dict_get", "jb_dict_size", "jb_save", "jb_profile_enable", "jb_profile_read",
    "jb_profile_reset", "jb_image_build", "jb_image_free", "jb_image_save", "jb_image_dict_info", "jb_image_lookup",
    "jb_image_stats", "jb_image_emit", "jb_go_log", "jb_shard_bounds", "jb_last_stats",
    "jb_suggest_freq", "jb_add_log", "jb_image_log_keys", "jb_device_status", "jb_cut_batch_into32",
    "jb_cut_search", "jb_cut_batch_search", "jb_cut_device_search", "jb_cut_device_search_into",
    "jb_cut_full", "jb_cut_batch_full", "jb_cut_device_full", "jb_cut_device_full_into",
    "jb_vocab_build", "jb_vocab_free", "jb_vocab_lookup", "jb_vocab_info", "jb_vocab_set", "jb_vocab_size",
    "jb_ids_device", "jb_spans_ids",
    "jb_terms_work_bytes", "jb_terms_device", "jb_keywords_device", "jb_keywords_batch",
    "jb_df_device", "jb_idf_device", "jb_idf", "jb_df_batch",
    "jb_textrank_work_bytes", "jb_textrank", "jb_textrank_device", "jb_textrank_batch",
    "jb_join_work_bytes", "jb_join", "jb_join_device", "jb_joined_free", "jb_cut_batch_join",
    "jb_charspans_work_bytes", "jb_charspans", "jb_charspans_device", "jb_cut_batch_charspans",
    "jb_wc_table_bytes", "jb_wc_work_bytes", "jb_wc_fp", "jb_wc_init_device", "jb_wc_add_device", "jb_wc_read",
    "jb_wc_result_free", "jb_wc_count", "jb_wc_batch", "jb_device_alloc", "jb_device_free",
    "jb_minhash_work_bytes", "jb_minhash_params", "jb_minhash", "jb_minhash_bands", "jb_minhash_device",
    "jb_minhash_bands_device", "jb_minhash_batch",
    "jb_stopwords_set", "jb_stopwords_size", "jb_filter_work_bytes", "jb_filter", "jb_filter_device",
    "jb_cut_batch_filter", "jb_batch_filter_set",
    "jb_postings_work_bytes", "jb_postings", "jb_postings_device", "jb_postings_batch",
    "jb_bm25_work_bytes", "jb_bm25_avgdl", "jb_bm25_norms", "jb_bm25_idf", "jb_bm25_search", "jb_bm25_norms_device",
    "jb_bm25_idf_device", "jb_bm25_search_device", "jb_index_set", "jb_index_clear", "jb_index_info", "jb_search_batch",
    "jb_neardup_work_bytes", "jb_neardup", "jb_neardup_device", "jb_neardup_labels", "jb_neardup_sig",
    "jb_colloc_table_bytes", "jb_colloc_work_bytes", "jb_colloc_init_device", "jb_colloc_add_device",
    "jb_colloc_score_device", "jb_colloc_read", "jb_colloc_result_free", "jb_colloc_count", "jb_colloc_score",
    "jb_colloc_batch",
]


class JbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class jb_config(C.Structure):
    _fields_ = [
        ("dict_path", C.c_char_p), ("dict_buf", C.c_char_p), ("dict_len", C.c_size_t), ("dict_kind", C.c_int),
        ("size_override", C.c_int64), ("emit_path", C.c_char_p), ("emit_buf", C.c_char_p), ("emit_len", C.c_size_t),
        ("device", C.c_int), ("ndevices", C.c_int),
        ("log_keys", C.POINTER(C.c_int64)), ("log_vals", C.POINTER(C.c_double)), ("nlog", C.c_size_t),
    ]


class jb_stats(C.Structure):
    _fields_ = [("tokens", C.c_uint64), ("blocks", C.c_uint64), ("zh_blocks", C.c_uint64),
                ("long_blocks", C.c_uint64), ("viterbi_ties", C.c_uint64)]


class jb_joined(C.Structure):
    _fields_ = [("text", C.POINTER(C.c_uint8)), ("nbytes", C.c_uint64), ("doc_off", C.POINTER(C.c_uint64)),
                ("ndocs", C.c_uint32)]


class _Joined:
    """Owner of a jb_joined: jb_joined_free when the last array over its text goes away."""

    def __init__(self):
        self.j = jb_joined()

    def __del__(self):
        if _lib is not None:
            _lib.jb_joined_free(C.byref(self.j))


class jb_wc_result(C.Structure):
    _fields_ = [("keys", C.POINTER(C.c_uint8)), ("key_off", C.POINTER(C.c_uint64)), ("counts", C.POINTER(C.c_uint64)),
                ("nkeys", C.c_uint64), ("nbad", C.c_uint64), ("nlong", C.c_uint64), ("ndropped", C.c_uint64),
                ("ncollided", C.c_uint64), ("ntokens", C.c_uint64)]


class WcResult:
    """A word-count result: keys (a list of bytes, by count descending, then by bytes), counts (uint64, one per
    key) and the five totals of the rule (bad, long, dropped, collided, tokens)."""

    def __init__(self, r):
        n = r.nkeys
        off = np.ctypeslib.as_array(r.key_off, (n + 1,)).tolist()
        raw = bytes(np.ctypeslib.as_array(r.keys, (max(off[n], 1),))[:off[n]])
        self.keys = [raw[off[i]:off[i + 1]] for i in range(n)]
        self.counts = np.ctypeslib.as_array(r.counts, (max(n, 1),))[:n].copy()
        self.bad, self.long, self.dropped, self.collided, self.tokens = (
            r.nbad, r.nlong, r.ndropped, r.ncollided, r.ntokens)

    def __repr__(self):
        return (f"WcResult({len(self.keys)} keys, tokens={self.tokens}, bad={self.bad}, long={self.long}, "
                f"dropped={self.dropped}, collided={self.collided})")


class jb_colloc_result(C.Structure):
    _fields_ = [("a", C.POINTER(C.c_uint32)), ("b", C.POINTER(C.c_uint32)), ("count", C.POINTER(C.c_uint64)),
                ("score", C.POINTER(C.c_float)), ("n", C.c_uint64), ("tokens", C.c_uint64), ("known", C.c_uint64),
                ("pairs", C.c_uint64), ("dropped", C.c_uint64), ("distinct", C.c_uint64)]


class CollocResult:
    """A collocation result: a, b (uint32 ids), count (uint64) and score (float32), one entry per pair in the
    rule's order, and the five totals (tokens, known, pairs, dropped, distinct)."""

    def __init__(self, r):
        n = r.n
        self.a = np.ctypeslib.as_array(r.a, (max(n, 1),))[:n].copy()
        self.b = np.ctypeslib.as_array(r.b, (max(n, 1),))[:n].copy()
        self.count = np.ctypeslib.as_array(r.count, (max(n, 1),))[:n].copy()
        self.score = np.ctypeslib.as_array(r.score, (max(n, 1),))[:n].copy()
        self.tokens, self.known, self.pairs, self.dropped, self.distinct = (
            r.tokens, r.known, r.pairs, r.dropped, r.distinct)

    def totals(self):
        return (self.tokens, self.known, self.pairs, self.dropped, self.distinct)

    def __len__(self):
        return len(self.a)

    def __repr__(self):
        return (f"CollocResult({len(self.a)} pairs, tokens={self.tokens}, known={self.known}, pairs={self.pairs}, "
                f"dropped={self.dropped}, distinct={self.distinct})")


def _scorer(scorer):
    if isinstance(scorer, str):
        if scorer not in _SCORERS:
            raise ValueError(f"scorer {scorer!r}: one of 'npmi', 'ratio', 'count'")
        return _SCORERS[scorer]
    return int(scorer)


class jb_filter_rule(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("drop_classes", C.c_uint32), ("min_runes", C.c_uint32),
                ("max_runes", C.c_uint32)]


def filter_rule(drop=(), min_runes=0, max_runes=0, stop=False):
    """A jb_filter_rule: `drop` is a JB_TC_* mask or an iterable of class names ("han", "alnum", "num", "other",
    "invalid"); min_runes / max_runes bound a token's length in runes (max_runes 0: no upper bound); stop drops
    the tokens found in the stop set."""
    if isinstance(drop, jb_filter_rule):
        return drop
    if isinstance(drop, str):
        drop = (drop,)
    if not isinstance(drop, int):
        m = 0
        for c in drop:
            if c not in _CLASSES:
                raise ValueError(f"class {c!r}: one of {sorted(_CLASSES)}")
            m |= _CLASSES[c]
        drop = m
    return jb_filter_rule(JB_FILTER_STOP if stop else 0, drop, min_runes, max_runes)


class jb_spans(C.Structure):
    _fields_ = [
        ("ntokens", C.c_uint64), ("start", C.POINTER(C.c_uint64)), ("end", C.POINTER(C.c_uint64)),
        ("doc_tok", C.POINTER(C.c_uint64)), ("ndocs", C.c_uint32),
    ]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise JbError(JB_EIO, f"{LIB_PATH} not built: run `make -C jieba-go_amd` (no CPU fallback exists)")
        # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7
        # (ROCm 7.0) under torch/lib.  Loading torch first makes the dynamic
        # linker bind libjiebahip.so's libamdhip64.so.7 dependency to that same
        # runtime, so torch tensors and this library share device pointers,
        # streams and one HSA context.  (Loading the system ROCm 7.2 runtime and
        # torch's side by side in one process left torch with "No HIP GPUs are
        # available".)  Outside Python (Go / C++ callers) the system runtime is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, cp = C.c_void_p, C.c_char_p
        L.jb_open.argtypes = [C.POINTER(jb_config), C.POINTER(vp)]
        L.jb_close.argtypes = [vp]
        L.jb_close.restype = None
        L.jb_last_error.restype = cp
        L.jb_cut.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(jb_spans)]
        L.jb_cut_batch.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, C.POINTER(jb_spans)]
        L.jb_cut_batch_into.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, vp, C.c_uint64, vp,
                                        C.POINTER(C.c_uint64)]
        L.jb_cut_search.argtypes = L.jb_cut.argtypes
        L.jb_cut_batch_search.argtypes = L.jb_cut_batch.argtypes
        L.jb_cut_full.argtypes = [vp, vp, C.c_size_t, C.POINTER(jb_spans)]  # (no hmm argument)
        L.jb_cut_batch_full.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(jb_spans)]
        L.jb_spans_free.argtypes = [C.POINTER(jb_spans)]
        L.jb_spans_free.restype = None
        L.jb_cut_device.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, vp, C.POINTER(vp), C.POINTER(vp),
                                    C.POINTER(vp), C.POINTER(vp)]
        L.jb_cut_device_into.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, vp, vp, vp, C.c_uint64, vp,
                                         vp]
        L.jb_cut_device_search.argtypes = L.jb_cut_device.argtypes
        L.jb_cut_device_search_into.argtypes = L.jb_cut_device_into.argtypes
        L.jb_cut_device_full.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.POINTER(vp), C.POINTER(vp),
                                         C.POINTER(vp), C.POINTER(vp)]
        L.jb_cut_device_full_into.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp]
        L.jb_open_image.argtypes = [vp, C.POINTER(jb_config), C.POINTER(vp)]
        L.jb_cut_batch_mask.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.jb_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
        L.jb_host_free.argtypes = [vp]
        L.jb_host_free.restype = None
        L.jb_add_word.argtypes = [vp, cp, C.c_size_t, C.c_int64]
        L.jb_dict_get.argtypes = [vp, cp, C.c_size_t, C.POINTER(C.c_int64)]
        L.jb_dict_size.argtypes = [vp]
        L.jb_dict_size.restype = C.c_int64
        L.jb_save.argtypes = [vp, cp]
        L.jb_image_save.argtypes = [vp, cp]
        L.jb_image_dict_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]
        L.jb_profile_enable.argtypes = [vp, C.c_int]
        L.jb_profile_reset.argtypes = [vp]
        L.jb_profile_read.argtypes = [vp, C.POINTER(cp), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        L.jb_image_build.argtypes = [C.POINTER(jb_config), C.POINTER(vp)]
        L.jb_image_free.argtypes = [vp]
        L.jb_image_free.restype = None
        L.jb_image_lookup.argtypes = [vp, cp, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        L.jb_image_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        L.jb_image_emit.argtypes = [vp, C.c_int, C.c_uint32]
        L.jb_image_emit.restype = C.c_double
        L.jb_go_log.argtypes = [C.c_double]
        L.jb_go_log.restype = C.c_double
        L.jb_shard_bounds.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
        L.jb_split_points.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp]
        L.jb_image_log_keys.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.jb_suggest_freq.argtypes = [vp, cp, C.c_size_t, C.POINTER(C.c_int64)]
        L.jb_add_log.argtypes = [vp, vp, vp, C.c_size_t]
        L.jb_last_stats.argtypes = [vp, C.POINTER(jb_stats)]
        L.jb_device_status.argtypes = [vp, vp]
        L.jb_cut_batch_into32.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, vp, C.c_uint64, vp,
                                          C.POINTER(C.c_uint64)]
        L.jb_vocab_build.argtypes = [vp, vp, C.c_uint32, C.POINTER(vp)]
        L.jb_vocab_free.argtypes = [vp]
        L.jb_vocab_free.restype = None
        L.jb_vocab_lookup.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_uint32)]
        L.jb_vocab_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        L.jb_vocab_set.argtypes = [vp, vp, vp, C.c_uint32]
        L.jb_vocab_size.argtypes = [vp]
        L.jb_vocab_size.restype = C.c_int64
        L.jb_ids_device.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp]
        L.jb_spans_ids.argtypes = [vp, vp, C.POINTER(jb_spans), vp]
        L.jb_terms_work_bytes.argtypes = [C.c_uint64, C.c_uint32]
        L.jb_terms_work_bytes.restype = C.c_size_t
        L.jb_terms_device.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp, vp,
                                      C.c_size_t]
        L.jb_keywords_device.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint64, vp, C.c_uint32, C.c_uint32, vp, vp,
                                         vp, vp, vp]
        L.jb_keywords_batch.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
        L.jb_df_device.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint32, vp]
        L.jb_idf_device.argtypes = [vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.jb_idf.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp]
        L.jb_df_batch.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, C.c_uint32]
        L.jb_textrank_work_bytes.restype = C.c_size_t
        L.jb_textrank_work_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        L.jb_textrank.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32,
                                  C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.jb_textrank_device.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32,
                                         C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.c_size_t]
        L.jb_textrank_batch.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_uint32, vp, vp, vp]
        L.jb_join_work_bytes.restype = C.c_size_t
        L.jb_join_work_bytes.argtypes = [C.c_uint64, C.c_uint32]
        L.jb_join.argtypes = [vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp,
                              C.c_uint32, vp, C.c_uint64, vp, C.POINTER(C.c_uint64)]
        L.jb_join_device.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp,
                                     C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, C.c_size_t]
        L.jb_joined_free.argtypes = [C.POINTER(jb_joined)]
        L.jb_joined_free.restype = None
        L.jb_cut_batch_join.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, C.c_int, vp, C.c_uint32, vp, C.c_uint32,
                                        C.POINTER(jb_joined)]
        L.jb_charspans_work_bytes.restype = C.c_size_t
        L.jb_charspans_work_bytes.argtypes = [C.c_uint64, C.c_uint32]
        L.jb_charspans.argtypes = [vp, C.c_uint64, vp, C.c_uint32, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_int, vp, vp,
                                   vp]
        L.jb_charspans_device.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint64, C.c_int, vp,
                                          vp, vp, vp, vp, C.c_size_t]
        L.jb_cut_batch_charspans.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, vp, C.c_uint64, vp,
                                             C.POINTER(C.c_uint64), vp]
        L.jb_wc_table_bytes.restype = C.c_size_t
        L.jb_wc_table_bytes.argtypes = [C.c_uint64, C.c_uint64]
        L.jb_wc_work_bytes.restype = C.c_size_t
        L.jb_wc_work_bytes.argtypes = [C.c_uint64]
        L.jb_wc_fp.restype = C.c_uint64
        L.jb_wc_fp.argtypes = [vp, C.c_size_t, C.c_uint32]
        L.jb_wc_init_device.argtypes = [vp, vp, C.c_size_t, C.c_uint64, C.c_uint64, vp]
        L.jb_wc_add_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp, C.c_size_t]
        L.jb_wc_read.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint64, C.c_uint64, C.POINTER(jb_wc_result)]
        L.jb_wc_result_free.argtypes = [C.POINTER(jb_wc_result)]
        L.jb_wc_result_free.restype = None
        L.jb_wc_count.argtypes = [vp, C.c_uint64, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                  C.POINTER(jb_wc_result)]
        L.jb_wc_batch.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, C.c_int, vp, C.c_size_t]
        L.jb_minhash_work_bytes.restype = C.c_size_t
        L.jb_minhash_work_bytes.argtypes = [C.c_uint64, C.c_uint32]
        L.jb_minhash_params.argtypes = [C.c_uint64, C.c_uint32, vp, vp]
        L.jb_minhash.argtypes = [vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.c_uint64, vp, vp]
        L.jb_minhash_bands.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp]
        L.jb_minhash_device.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.c_uint64, vp, vp, vp, vp, C.c_size_t]
        L.jb_minhash_bands_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
        L.jb_minhash_batch.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, vp,
                                       vp]
        L.jb_stopwords_set.argtypes = [vp, vp, vp, C.c_uint32]
        L.jb_stopwords_size.restype = C.c_int64
        L.jb_stopwords_size.argtypes = [vp]
        L.jb_filter_work_bytes.restype = C.c_size_t
        L.jb_filter_work_bytes.argtypes = [C.c_uint64, C.c_uint32]
        L.jb_filter.argtypes = [vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp,
                                C.c_uint64, vp, vp, vp]
        L.jb_filter_device.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp,
                                       C.c_uint64, vp, vp, vp, vp, C.c_size_t]
        L.jb_cut_batch_filter.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, C.c_int, vp, vp, vp, C.c_uint64, vp, vp, vp]
        L.jb_batch_filter_set.argtypes = [vp, vp]
        L.jb_postings_work_bytes.restype = C.c_size_t
        L.jb_postings_work_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        L.jb_postings.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp,
                                  C.c_uint64, vp, vp]
        L.jb_postings_device.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp,
                                         C.c_uint64, vp, vp, vp, C.c_size_t]
        L.jb_postings_batch.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint64, vp, C.c_uint32, vp, vp,
                                        vp, vp]
        L.jb_bm25_work_bytes.restype = C.c_size_t
        L.jb_bm25_work_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        L.jb_bm25_avgdl.argtypes = [vp, C.c_uint32, C.POINTER(C.c_double)]
        L.jb_bm25_norms.argtypes = [vp, C.c_uint32, C.c_double, C.c_double, C.c_double, vp]
        L.jb_bm25_idf.argtypes = [vp, C.c_uint32, C.c_uint64, vp]
        L.jb_bm25_search.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.c_double, vp,
                                     C.c_uint64, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.jb_bm25_norms_device.argtypes = [vp, vp, C.c_uint32, C.c_double, C.c_double, C.c_double, vp, vp]
        L.jb_bm25_idf_device.argtypes = [vp, vp, C.c_uint32, C.c_uint64, vp, vp]
        L.jb_bm25_search_device.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32,
                                            C.c_double, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp,
                                            C.c_size_t]
        L.jb_index_set.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, C.c_double, C.c_double]
        L.jb_index_clear.argtypes = [vp]
        L.jb_index_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_double)]
        L.jb_search_batch.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp]
        L.jb_neardup_work_bytes.restype = C.c_size_t
        L.jb_neardup_work_bytes.argtypes = [C.c_uint32, C.c_uint32]
        L.jb_neardup.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64,
                                 vp, vp, vp]
        L.jb_neardup_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp,
                                        C.c_uint64, vp, vp, vp, vp, C.c_size_t, vp]
        L.jb_neardup_labels.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp]
        L.jb_neardup_sig.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     vp, vp, C.c_uint64, vp, vp, vp]
        L.jb_colloc_table_bytes.restype = C.c_size_t
        L.jb_colloc_table_bytes.argtypes = [C.c_uint64]
        L.jb_colloc_work_bytes.restype = C.c_size_t
        L.jb_colloc_work_bytes.argtypes = [C.c_uint64, C.c_uint32]
        L.jb_colloc_init_device.argtypes = [vp, vp, C.c_size_t, C.c_uint64, vp, C.c_uint32, vp]
        L.jb_colloc_add_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint32, vp,
                                           C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_size_t]
        L.jb_colloc_score_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_int, C.c_uint64, C.c_float, vp, vp,
                                             vp, vp, C.c_uint64, vp, vp]
        L.jb_colloc_read.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_int, C.c_uint64, C.c_float, C.c_uint64, vp,
                                     C.POINTER(jb_colloc_result)]
        L.jb_colloc_result_free.argtypes = [C.POINTER(jb_colloc_result)]
        L.jb_colloc_result_free.restype = None
        L.jb_colloc_count.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp,
                                      C.c_uint64, vp, C.c_uint32, C.POINTER(jb_colloc_result)]
        L.jb_colloc_score.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_int, C.c_uint64, C.c_float,
                                      C.c_uint64, C.POINTER(jb_colloc_result)]
        L.jb_colloc_batch.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp,
                                      C.c_uint32]
        L.jb_device_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.jb_device_free.argtypes = [vp, vp]
        L.jb_device_free.restype = None
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        raise JbError(rc, lib().jb_last_error().decode("utf-8", "replace"))
    return rc


def _b(s):
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


def make_config(dict_path=None, emit_path=None, dict_bytes=None, emit_bytes=None, kind=JB_DICT_TXT,
                size_override=0, device=0, ndevices=1, logs=None):
    """logs: optional {x: math.Log(float64(x))} the caller computed (jb_config.log_keys/log_vals)."""
    cfg = jb_config()
    keep = []
    if logs:
        ks = np.ascontiguousarray(list(logs.keys()), np.int64)
        vs = np.ascontiguousarray([logs[k] for k in logs.keys()], np.float64)
        keep += [ks, vs]
        cfg.log_keys = ks.ctypes.data_as(C.POINTER(C.c_int64))
        cfg.log_vals = vs.ctypes.data_as(C.POINTER(C.c_double))
        cfg.nlog = len(ks)
    if dict_path is not None:
        cfg.dict_path = os.fsencode(dict_path)
    else:
        d = _b(dict_bytes or b"")
        keep.append(d)
        cfg.dict_buf, cfg.dict_len = d, len(d)
    if emit_path is not None:
        cfg.emit_path = os.fsencode(emit_path)
    else:
        e = _b(emit_bytes or b"{}")
        keep.append(e)
        cfg.emit_buf, cfg.emit_len = e, len(e)
    cfg.dict_kind = kind
    cfg.size_override = size_override
    cfg.device = device
    cfg.ndevices = ndevices
    cfg._keep = keep
    return cfg


def spans_to_tokens(text, starts, ends):
    """(start, end) byte spans -> Go strings; an invalid UTF-8 byte becomes "�"."""
    t = _b(text)
    out = []
    for a, b in zip(starts, ends):
        if b - a == 1 and t[a] >= 0x80:
            out.append("�")
        else:
            out.append(t[a:b].decode("utf-8"))
    return out


class Image:
    """Host-only device image (no GPU needed): loader + table builder."""

    def __init__(self, cfg):
        h = C.c_void_p()
        _check(lib().jb_image_build(C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib().jb_image_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lookup(self, word):
        w = _b(word)
        f, x = C.c_int64(), C.c_double()
        r = _check(lib().jb_image_lookup(self.h, w, len(w), C.byref(f), C.byref(x)))
        return (f.value, x.value) if r else None

    def stats(self):
        n, cap, sz = C.c_uint64(), C.c_uint64(), C.c_int64()
        npg, ml = C.c_uint32(), C.c_uint32()
        wa = C.c_double()
        _check(lib().jb_image_stats(self.h, C.byref(n), C.byref(cap), C.byref(npg), C.byref(ml), C.byref(sz),
                                    C.byref(wa)))
        return dict(nodes=n.value, cap=cap.value, npages=npg.value, maxlen=ml.value, size=sz.value,
                    w_absent=wa.value)

    def emit(self, state, ch):
        return lib().jb_image_emit(self.h, "BMES".index(state), ord(ch))

    def save(self, path):
        _check(lib().jb_image_save(self.h, os.fsencode(path)))

    def log_keys(self):
        """jb_image_log_keys: the x whose math.Log the weights use."""
        n = C.c_size_t()
        lib().jb_image_log_keys(self.h, None, 0, C.byref(n))
        out = np.zeros(max(n.value, 1), np.int64)
        _check(lib().jb_image_log_keys(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def dict_info(self):
        n, sz = C.c_uint64(), C.c_int64()
        _check(lib().jb_image_dict_info(self.h, C.byref(n), C.byref(sz)))
        return n.value, sz.value


def pack_keys(keys):
    """A list of str / bytes keys -> (bytes uint8, key_off uint64[nkeys + 1]) as jb_vocab_build takes them."""
    ks = [_b(k) for k in keys]
    off = np.zeros(len(ks) + 1, np.uint64)
    if ks:
        off[1:] = np.cumsum([len(k) for k in ks], dtype=np.uint64)
    buf = np.frombuffer(b"".join(ks) + b"\0", np.uint8)  # (never an empty array: its pointer is passed)
    return buf, off


class Vocab:
    """Host-only vocabulary table (no GPU needed): the builder and the device probe on the host.
    `keys` is a list of str / bytes, or a (bytes, key_off) pair; a key's id is its index."""

    def __init__(self, keys=None, packed=None):
        buf, off = packed if packed is not None else pack_keys(keys)
        buf = np.ascontiguousarray(buf, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        h = C.c_void_p()
        _check(lib().jb_vocab_build(buf.ctypes.data, off.ctypes.data, len(off) - 1, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib().jb_vocab_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lookup(self, tok):
        """The key's id, or None."""
        t = _b(tok)
        i = C.c_uint32()
        return i.value if _check(lib().jb_vocab_lookup(self.h, t, len(t), C.byref(i))) else None

    def info(self):
        n, ml, ns = C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(lib().jb_vocab_info(self.h, C.byref(n), C.byref(ml), C.byref(ns)))
        return dict(nkeys=n.value, maxlen=ml.value, nslots=ns.value)


class Tokenizer:
    """jieba-go Tokenizer over the MI355X path."""

    _vocab_keys = None  # the attached vocabulary's keys by id (set_vocab)

    def __init__(self, cfg):
        h = C.c_void_p()
        _check(lib().jb_open(C.byref(cfg), C.byref(h)))
        self.h = h

    @classmethod
    def from_image(cls, image, device=0, ndevices=1, logs=None):
        """jb_open_image: a ctx from an Image built by jb_image_build (the trie is placed
        once), optionally reweighed with the caller's {x: math.Log(x)}.  Consumes `image`."""
        cfg = make_config(dict_bytes=b"", device=device, ndevices=ndevices, logs=logs)
        h, img = C.c_void_p(), image.h
        image.h = None  # jb_open_image owns it from here, success or not
        _check(lib().jb_open_image(img, C.byref(cfg), C.byref(h)))
        self = cls.__new__(cls)
        self.h = h
        return self

    @classmethod
    def NewTokenizer(cls, dictionaryFile, emit_path="prob_emit.json", device=0):
        """tokenizer.go:61 — dict.txt semantics."""
        return cls(make_config(dict_path=dictionaryFile, emit_path=emit_path, kind=JB_DICT_TXT, device=device))

    @classmethod
    def NewJiebaTokenizer(cls, dict_path="prefix_dictionary.gob", emit_path="prob_emit.json", device=0):
        """tokenizer.go:69 — decodes prefix_dictionary.gob (tokenizer.go:439-458), size 60,101,967.
        A path ending in .txt is read with buildPrefixDictionary semantics instead (the map the gob holds)."""
        if str(dict_path).endswith(".txt"):
            return cls(make_config(dict_path=dict_path, emit_path=emit_path, kind=JB_DICT_PREFIX,
                                   size_override=JIEBA_SIZE, device=device))
        return cls(make_config(dict_path=dict_path, emit_path=emit_path, kind=JB_DICT_GOB, device=device))

    @classmethod
    def FromImage(cls, image_path, device=0, ndevices=1):
        """Open a serialized image written by save() (no parsing, no trie build)."""
        return cls(make_config(dict_path=image_path, kind=JB_DICT_IMAGE, device=device, ndevices=ndevices))

    def save(self, path):
        """Write the current image (including AddWord changes) for FromImage."""
        _check(lib().jb_save(self.h, os.fsencode(path)))

    def close(self):
        if self.h:
            lib().jb_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- cutting ---------------------------------------------------------
    def cut_spans(self, text, hmm, _fn="jb_cut"):
        t = _b(text)
        sp = jb_spans()
        _check(getattr(lib(), _fn)(self.h, t, len(t), int(hmm), C.byref(sp)))
        try:
            n = sp.ntokens
            s = np.ctypeslib.as_array(sp.start, (max(n, 1),))[:n].copy()
            e = np.ctypeslib.as_array(sp.end, (max(n, 1),))[:n].copy()
        finally:
            lib().jb_spans_free(C.byref(sp))
        return s, e

    def Cut(self, text, useHmm):
        """Tokenizer.Cut (tokenizer.go:151)."""
        s, e = self.cut_spans(text, useHmm)
        return spans_to_tokens(text, s.tolist(), e.tolist())

    def cut_search_spans(self, text, hmm):
        """jb_cut_search: the spans of Cut, each Han token of three or more runes preceded by
        the dictionary words of two, then three, runes inside it (overlapping spans)."""
        return self.cut_spans(text, hmm, "jb_cut_search")

    def CutForSearch(self, text, useHmm):
        """Search-engine mode (jieba's cut_for_search on this reference's DAG, jiebahip.h)."""
        s, e = self.cut_search_spans(text, useHmm)
        return spans_to_tokens(text, s.tolist(), e.tolist())

    def cut_full_spans(self, text):
        """jb_cut_full: every dictionary word of two or more runes in the text's Han blocks, by
        start then length, and the single runes no such word accounts for (overlapping spans)."""
        t = _b(text)
        sp = jb_spans()
        _check(lib().jb_cut_full(self.h, t, len(t), C.byref(sp)))
        try:
            n = sp.ntokens
            s = np.ctypeslib.as_array(sp.start, (max(n, 1),))[:n].copy()
            e = np.ctypeslib.as_array(sp.end, (max(n, 1),))[:n].copy()
        finally:
            lib().jb_spans_free(C.byref(sp))
        return s, e

    def CutAll(self, text):
        """Full mode (jieba's cut_all=True on this reference's DAG, jiebahip.h)."""
        s, e = self.cut_full_spans(text)
        return spans_to_tokens(text, s.tolist(), e.tolist())

    def CutParallel(self, text, hmm, numWorkers=1, ordered=True):
        """Tokenizer.CutParallel (tokenizer.go:81): always in text order."""
        return self.Cut(text, hmm)

    def cut_batch(self, buf, doc_off, hmm, _fn="jb_cut_batch"):
        """Host batch -> (starts u64, ends u64, doc_tok u64[ndocs+1])."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        nd = len(doc_off) - 1
        sp = jb_spans()
        _check(getattr(lib(), _fn)(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, int(hmm), C.byref(sp)))
        try:
            n = sp.ntokens
            s = np.ctypeslib.as_array(sp.start, (max(n, 1),))[:n].copy()
            e = np.ctypeslib.as_array(sp.end, (max(n, 1),))[:n].copy()
            d = np.ctypeslib.as_array(sp.doc_tok, (nd + 1,)).copy()
        finally:
            lib().jb_spans_free(C.byref(sp))
        return s, e, d

    def cut_batch_search(self, buf, doc_off, hmm):
        """jb_cut_batch_search: cut_batch in search mode; doc_tok indexes the expanded spans."""
        return self.cut_batch(buf, doc_off, hmm, "jb_cut_batch_search")

    def cut_batch_full(self, buf, doc_off):
        """jb_cut_batch_full: cut_batch in full mode; doc_tok indexes the full-mode spans, which
        may outnumber the bytes."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        nd = len(doc_off) - 1
        sp = jb_spans()
        _check(lib().jb_cut_batch_full(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, C.byref(sp)))
        try:
            n = sp.ntokens
            s = np.ctypeslib.as_array(sp.start, (max(n, 1),))[:n].copy()
            e = np.ctypeslib.as_array(sp.end, (max(n, 1),))[:n].copy()
            d = np.ctypeslib.as_array(sp.doc_tok, (nd + 1,)).copy()
        finally:
            lib().jb_spans_free(C.byref(sp))
        return s, e, d

    def cut_batch_into(self, buf, doc_off, hmm, out=None):
        """Host batch into caller-owned arrays (jb_cut_batch_into).  `out` =
        (starts u64, ends u64, doc_tok u64[ndocs+1]) to reuse; grown when too
        small.  Returns (starts[:n], ends[:n], doc_tok, out)."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        nd = len(doc_off) - 1
        if out is None or len(out[2]) != nd + 1:
            cap = max(1024, int(doc_off[-1] - doc_off[0]) // 2)
            out = (np.empty(cap, np.uint64), np.empty(cap, np.uint64), np.empty(nd + 1, np.uint64))
        n = C.c_uint64()
        for _ in range(2):
            rc = lib().jb_cut_batch_into(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, int(hmm),
                                         out[0].ctypes.data, out[1].ctypes.data, len(out[0]), out[2].ctypes.data,
                                         C.byref(n))
            if rc == JB_ELIMIT and n.value > len(out[0]):
                out = (np.empty(n.value, np.uint64), np.empty(n.value, np.uint64), out[2])
                continue
            _check(rc)
            break
        k = n.value
        return out[0][:k], out[1][:k], out[2], out

    def cut_batch_into32(self, buf, doc_off, hmm, out=None):
        """jb_cut_batch_into32: u32 spans relative to doc_off[0] in caller-owned arrays.
        `out` = (starts u32, ends u32, doc_tok u64[ndocs+1]) to reuse; grown when too
        small.  Returns (starts[:n], ends[:n], doc_tok, out)."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        nd = len(doc_off) - 1
        if out is None or len(out[2]) != nd + 1:
            cap = max(1024, int(doc_off[-1] - doc_off[0]) // 2)
            out = (np.empty(cap, np.uint32), np.empty(cap, np.uint32), np.empty(nd + 1, np.uint64))
        n = C.c_uint64()
        for _ in range(2):
            rc = lib().jb_cut_batch_into32(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, int(hmm),
                                           out[0].ctypes.data, out[1].ctypes.data, len(out[0]), out[2].ctypes.data,
                                           C.byref(n))
            if rc == JB_ELIMIT and n.value > len(out[0]):
                out = (np.empty(n.value, np.uint32), np.empty(n.value, np.uint32), out[2])
                continue
            _check(rc)
            break
        k = n.value
        return out[0][:k], out[1][:k], out[2], out

    def cut_batch_mask(self, buf, doc_off, hmm, out=None):
        """jb_cut_batch_mask: (starts u64 words, ends u64 words, ntokens); `out` = the
        two arrays to reuse."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)  # (a HostBuffer's .array stays where it is)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        nd = len(doc_off) - 1
        nw = (int(doc_off[-1] - doc_off[0]) + 63) // 64 if nd else 0
        if out is None or len(out[0]) < nw:
            out = (np.empty(max(nw, 1), np.uint64), np.empty(max(nw, 1), np.uint64))
        n = C.c_uint64()
        _check(lib().jb_cut_batch_mask(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, int(hmm), out[0].ctypes.data,
                                       out[1].ctypes.data, len(out[0]), C.byref(n)))
        return out[0][:nw], out[1][:nw], n.value

    def cut_device(self, d_text_ptr, nbytes, d_doc_off_ptr, ndocs, hmm, stream_ptr=0, _fn="jb_cut_device"):
        """Device-resident cut; returns device pointers (start, end, doc_tok, ntok)."""
        a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(getattr(lib(), _fn)(self.h, C.c_void_p(d_text_ptr), nbytes, C.c_void_p(d_doc_off_ptr), ndocs,
                                   int(hmm), C.c_void_p(stream_ptr), C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def cut_device_search(self, d_text_ptr, nbytes, d_doc_off_ptr, ndocs, hmm, stream_ptr=0):
        """jb_cut_device_search: cut_device in search mode (the expanded spans)."""
        return self.cut_device(d_text_ptr, nbytes, d_doc_off_ptr, ndocs, hmm, stream_ptr, "jb_cut_device_search")

    def cut_device_search_into(self, d_text_ptr, nbytes, d_doc_off_ptr, ndocs, hmm, d_start, d_end, cap, d_doc_tok,
                               d_ntok, stream_ptr=0):
        """jb_cut_device_search_into: the expanded spans into caller-owned device arrays."""
        self.cut_device_into(d_text_ptr, nbytes, d_doc_off_ptr, ndocs, hmm, d_start, d_end, cap, d_doc_tok, d_ntok,
                             stream_ptr, "jb_cut_device_search_into")

    def cut_device_full(self, d_text_ptr, nbytes, d_doc_off_ptr, ndocs, stream_ptr=0):
        """jb_cut_device_full: cut_device in full mode.  The ctx-owned arrays hold nbytes spans; the
        count and doc_tok describe the complete list (device_status reports JB_ELIMIT when it is longer)."""
        a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().jb_cut_device_full(self.h, C.c_void_p(d_text_ptr), nbytes, C.c_void_p(d_doc_off_ptr), ndocs,
                                        C.c_void_p(stream_ptr), C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def cut_device_full_into(self, d_text_ptr, nbytes, d_doc_off_ptr, ndocs, d_start, d_end, cap, d_doc_tok, d_ntok,
                             stream_ptr=0):
        """jb_cut_device_full_into: the full-mode spans into caller-owned device arrays of any
        capacity; spans past it are counted, not written."""
        _check(lib().jb_cut_device_full_into(self.h, C.c_void_p(d_text_ptr), nbytes, C.c_void_p(d_doc_off_ptr), ndocs,
                                             C.c_void_p(stream_ptr), C.c_void_p(d_start), C.c_void_p(d_end), cap,
                                             C.c_void_p(d_doc_tok), C.c_void_p(d_ntok)))

    def cut_device_into(self, d_text_ptr, nbytes, d_doc_off_ptr, ndocs, hmm, d_start, d_end, cap, d_doc_tok, d_ntok,
                        stream_ptr=0, _fn="jb_cut_device_into"):
        """jb_cut_device_into: caller-owned device outputs (raw pointers)."""
        _check(getattr(lib(), _fn)(self.h, C.c_void_p(d_text_ptr), nbytes, C.c_void_p(d_doc_off_ptr), ndocs,
                                        int(hmm), C.c_void_p(stream_ptr), C.c_void_p(d_start), C.c_void_p(d_end),
                                        cap, C.c_void_p(d_doc_tok), C.c_void_p(d_ntok)))

    # -- token ids -------------------------------------------------------
    def set_vocab(self, keys, packed=None):
        """jb_vocab_set: attach a vocabulary (a list of str / bytes; a key's id is its index), replacing
        any earlier one.  None removes it; an empty list attaches an empty vocabulary."""
        if keys is None and packed is None:
            _check(lib().jb_vocab_set(self.h, None, None, 0))
            self._vocab_keys = None
            return
        buf, off = packed if packed is not None else pack_keys(keys)
        buf = np.ascontiguousarray(buf, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        _check(lib().jb_vocab_set(self.h, buf.ctypes.data, off.ctypes.data, len(off) - 1))
        # (the keys by id, for the calls that name ids: collocations, find_new_words)
        raw = bytes(buf[:int(off[-1])])
        self._vocab_keys = [raw[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]

    @property
    def vocab_size(self):
        """Keys of the attached vocabulary; -1 when none is attached."""
        return lib().jb_vocab_size(self.h)

    def spans_ids(self, text, starts, ends):
        """jb_spans_ids: the ids (uint32, JB_ID_UNK when absent) of host spans of `text` (str, bytes or
        a uint8 array)."""
        t = np.ascontiguousarray(text, np.uint8) if isinstance(text, np.ndarray) else np.frombuffer(
            _b(text) + b"\0", np.uint8)
        s = np.ascontiguousarray(starts, np.uint64)
        e = np.ascontiguousarray(ends, np.uint64)
        sp = jb_spans()
        sp.ntokens = len(s)
        sp.start = s.ctypes.data_as(C.POINTER(C.c_uint64))
        sp.end = e.ctypes.data_as(C.POINTER(C.c_uint64))
        ids = np.empty(len(s), np.uint32)
        _check(lib().jb_spans_ids(self.h, t.ctypes.data, C.byref(sp), ids.ctypes.data))
        return ids

    def ids_device(self, d_text_ptr, nbytes, d_start, d_end, d_ntok, cap, d_ids, stream_ptr=0):
        """jb_ids_device over raw device pointers: d_ids[k] for k < min(*d_ntok, cap); queued on the stream."""
        _check(lib().jb_ids_device(self.h, C.c_void_p(d_text_ptr), nbytes, C.c_void_p(d_start), C.c_void_p(d_end),
                                   C.c_void_p(d_ntok), cap, C.c_void_p(stream_ptr), C.c_void_p(d_ids)))

    def CutIds(self, text, useHmm, mode="cut"):
        """Cut / CutForSearch / CutAll (mode "cut", "search", "full"; full mode ignores useHmm) and the
        tokens' ids in the attached vocabulary: (tokens, ids uint32)."""
        if mode == "cut":
            s, e = self.cut_spans(text, useHmm)
        elif mode == "search":
            s, e = self.cut_search_spans(text, useHmm)
        elif mode == "full":
            s, e = self.cut_full_spans(text)
        else:
            raise ValueError(f"mode {mode!r}: one of 'cut', 'search', 'full'")
        return spans_to_tokens(text, s.tolist(), e.tolist()), self.spans_ids(text, s, e)

    # -- term counts and keywords ----------------------------------------
    def terms_device(self, d_ids, ids_cap, d_doc_tok, d_ntok, ndocs, d_term_id, d_term_cnt, cap, d_term_off, d_nterms,
                     d_work, nwork, stream_ptr=0):
        """jb_terms_device over raw device pointers: the CSR of per-document (id, count), ids ascending;
        entries with index >= cap are not written.  d_work: terms_work_bytes(ids_cap, ndocs) bytes."""
        _check(lib().jb_terms_device(self.h, C.c_void_p(d_ids), ids_cap, C.c_void_p(d_doc_tok), C.c_void_p(d_ntok),
                                     ndocs, C.c_void_p(stream_ptr), C.c_void_p(d_term_id), C.c_void_p(d_term_cnt), cap,
                                     C.c_void_p(d_term_off), C.c_void_p(d_nterms), C.c_void_p(d_work), nwork))

    def keywords_device(self, d_term_id, d_term_cnt, d_term_off, ndocs, cap, d_weight, nweights, topk, d_kw_id,
                        d_kw_score, d_kw_cnt, d_kw_n, stream_ptr=0):
        """jb_keywords_device over raw device pointers: per document the topk terms by count x weight."""
        _check(lib().jb_keywords_device(self.h, C.c_void_p(d_term_id), C.c_void_p(d_term_cnt), C.c_void_p(d_term_off),
                                        ndocs, cap, C.c_void_p(d_weight), nweights, topk, C.c_void_p(stream_ptr),
                                        C.c_void_p(d_kw_id), C.c_void_p(d_kw_score), C.c_void_p(d_kw_cnt),
                                        C.c_void_p(d_kw_n)))

    def keywords_batch(self, buf, doc_off, hmm, weights, topk=20):
        """jb_keywords_batch: host batch -> (kw_id u32[ndocs, topk], kw_score f32, kw_cnt u32, kw_n u32[ndocs])."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        nd = len(doc_off) - 1
        rows = max(nd, 1) * max(int(topk), 1)
        ki, ks, kc = np.empty(rows, np.uint32), np.empty(rows, np.float32), np.empty(rows, np.uint32)
        kn = np.empty(max(nd, 1), np.uint32)
        _check(lib().jb_keywords_batch(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, int(hmm),
                                       w.ctypes.data if len(w) else None, len(w), topk, ki.ctypes.data, ks.ctypes.data,
                                       kc.ctypes.data, kn.ctypes.data))
        shape = (nd, int(topk))
        return ki[:nd * topk].reshape(shape), ks[:nd * topk].reshape(shape), kc[:nd * topk].reshape(shape), kn[:nd]

    def extract_tags(self, texts, weights, topK=20, hmm=True, keys=None):
        """jieba.analyse.extract_tags over a list of documents (str / bytes), with the attached vocabulary
        and the caller's per-id weights: per document a list of (key, score, count), best first.  `key`
        is the term's id, or keys[id] when the vocabulary's key list is passed.  The differences from
        jieba's (closed vocabulary, no division by the token total, ties by id) are in jiebahip.h."""
        docs = [_b(t) for t in texts]
        off = np.zeros(len(docs) + 1, np.uint64)
        if docs:
            off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
        buf = np.frombuffer(b"".join(docs) + b"\0", np.uint8)
        ki, ks, kc, kn = self.keywords_batch(buf, off, hmm, weights, topK)
        return [[(int(ki[d, r]) if keys is None else keys[int(ki[d, r])], float(ks[d, r]), int(kc[d, r]))
                 for r in range(int(kn[d]))] for d in range(len(docs))]

    # -- document frequencies and IDF weights ------------------------------
    def df_device(self, d_term_id, d_nterms, cap, d_df, ndf, stream_ptr=0):
        """jb_df_device over raw device pointers: d_df[id] += 1 for every entry i < min(*d_nterms, cap) of the
        CSR's flat id list whose id is < ndf; queued on the stream."""
        _check(lib().jb_df_device(self.h, C.c_void_p(d_term_id), C.c_void_p(d_nterms), cap, C.c_void_p(d_df), ndf,
                                  C.c_void_p(stream_ptr)))

    def idf_device(self, d_df, ndf, ndocs, d_weight, min_df=1, max_df=None, d_keep=0, stream_ptr=0):
        """jb_idf_device over raw device pointers: d_weight[id] for every id < ndf, by the rule of idf()."""
        _check(lib().jb_idf_device(self.h, C.c_void_p(d_df), ndf, ndocs, min_df, JB_DF_NOMAX if max_df is None else max_df,
                                   C.c_void_p(d_keep), C.c_void_p(stream_ptr), C.c_void_p(d_weight)))

    def df_batch(self, buf, doc_off, hmm, df):
        """jb_df_batch: the host batch's document frequencies, added in place to df (a contiguous uint32
        array indexed by id); returns df."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        if not (isinstance(df, np.ndarray) and df.dtype == np.uint32 and df.flags.c_contiguous and df.flags.writeable):
            raise ValueError("df: a writeable contiguous uint32 array")
        _check(lib().jb_df_batch(self.h, buf.ctypes.data, doc_off.ctypes.data, len(doc_off) - 1, int(hmm),
                                 df.ctypes.data if len(df) else None, len(df)))
        return df

    def fit_idf(self, batches, hmm=True, min_df=1, max_df=None, keep=None):
        """Fit IDF weights for the attached vocabulary on a corpus given as an iterable of batches, each a
        list of documents (str / bytes): (weights f32[vocab_size], df u32[vocab_size], ndocs).
        extract_tags(texts, weights) afterwards is the whole of TF-IDF."""
        nv = self.vocab_size
        if nv < 0:
            raise JbError(JB_EINVAL, "fit_idf: no vocabulary attached (set_vocab)")
        df = np.zeros(nv, np.uint32)
        ndocs = 0
        for batch in batches:
            docs = [_b(t) for t in batch]
            if not docs:
                continue
            off = np.zeros(len(docs) + 1, np.uint64)
            off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
            self.df_batch(np.frombuffer(b"".join(docs) + b"\0", np.uint8), off, hmm, df)
            ndocs += len(docs)
        return idf(df, ndocs, min_df, max_df, keep), df, ndocs

    # -- TextRank keywords ----------------------------------------------------
    def textrank_device(self, d_ids, ids_cap, d_doc_tok, d_ntok, ndocs, d_term_id, d_term_off, cap, d_keep, nkeep,
                        d_kw_id, d_kw_score, d_kw_n, d_work, nwork, span=5, iters=10, topk=20, stream_ptr=0):
        """jb_textrank_device over raw device pointers: per document the topk nodes of its co-occurrence graph
        by PageRank.  d_work: textrank_work_bytes(ids_cap, cap, ndocs) bytes."""
        _check(lib().jb_textrank_device(self.h, C.c_void_p(d_ids), ids_cap, C.c_void_p(d_doc_tok), C.c_void_p(d_ntok),
                                        ndocs, C.c_void_p(d_term_id), C.c_void_p(d_term_off), cap, C.c_void_p(d_keep),
                                        nkeep, span, iters, topk, C.c_void_p(stream_ptr), C.c_void_p(d_kw_id),
                                        C.c_void_p(d_kw_score), C.c_void_p(d_kw_n), C.c_void_p(d_work), nwork))

    def textrank_batch(self, buf, doc_off, hmm, keep, span=5, iters=10, topk=20):
        """jb_textrank_batch: host batch -> (kw_id u32[ndocs, topk], kw_score f32, kw_n u32[ndocs])."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        k = np.ascontiguousarray(keep, dtype=np.uint8)
        nd = len(doc_off) - 1
        rows = max(nd, 1) * max(int(topk), 1)
        ki, ks, kn = np.empty(rows, np.uint32), np.empty(rows, np.float32), np.empty(max(nd, 1), np.uint32)
        _check(lib().jb_textrank_batch(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, int(hmm),
                                       k.ctypes.data if len(k) else None, len(k), span, iters, topk, ki.ctypes.data,
                                       ks.ctypes.data, kn.ctypes.data))
        shape = (nd, int(topk))
        return ki[:nd * topk].reshape(shape), ks[:nd * topk].reshape(shape), kn[:nd]

    def textrank(self, texts, keep, topK=20, span=5, iters=10, hmm=True, keys=None):
        """jieba.analyse.textrank over a list of documents (str / bytes), with the attached vocabulary and
        the caller's keep mask (one byte per id: jieba's part-of-speech, length and stop-word filters): per
        document a list of (key, score), best first.  `key` is the term's id, or keys[id] when the
        vocabulary's key list is passed.  The differences from jieba's (Jacobi rounds, closed vocabulary,
        ties by id, fixed-point sums) are in jiebahip.h."""
        docs = [_b(t) for t in texts]
        off = np.zeros(len(docs) + 1, np.uint64)
        if docs:
            off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
        buf = np.frombuffer(b"".join(docs) + b"\0", np.uint8)
        ki, ks, kn = self.textrank_batch(buf, off, hmm, keep, span, iters, topK)
        return [[(int(ki[d, r]) if keys is None else keys[int(ki[d, r])], float(ks[d, r])) for r in range(int(kn[d]))]
                for d in range(len(docs))]

    # -- joined text -------------------------------------------------------
    def join_device(self, d_text_ptr, nbytes, d_start, d_end, d_doc_tok, d_ntok, cap, ndocs, sep, term, d_out, out_cap,
                    d_out_doc_off, d_nout, d_work, nwork, stream_ptr=0):
        """jb_join_device over raw device pointers: per document its keys joined by sep and ended by term (host
        bytes, up to JB_JOIN_MAXSEP each) into d_out below out_cap; d_out_doc_off (u64[ndocs + 1]) and *d_nout
        describe the complete output.  d_work: join_work_bytes(cap, ndocs) bytes."""
        sep, term = _b(sep), _b(term)
        _check(lib().jb_join_device(self.h, C.c_void_p(d_text_ptr), nbytes, C.c_void_p(d_start), C.c_void_p(d_end),
                                    C.c_void_p(d_doc_tok), C.c_void_p(d_ntok), cap, ndocs, sep, len(sep), term,
                                    len(term), C.c_void_p(stream_ptr), C.c_void_p(d_out), out_cap,
                                    C.c_void_p(d_out_doc_off), C.c_void_p(d_nout), C.c_void_p(d_work), nwork))

    def cut_batch_join(self, buf, doc_off, hmm, mode="cut", sep=b" ", term=b"\n"):
        """jb_cut_batch_join: host batch -> (joined text uint8[nout], out_doc_off u64[ndocs + 1]); mode "cut",
        "search" or "full" (or a JB_MODE_* value; full mode ignores hmm)."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        nd = len(doc_off) - 1
        sep, term = _b(sep), _b(term)
        if isinstance(mode, str):
            if mode not in _MODES:
                raise ValueError(f"mode {mode!r}: one of 'cut', 'search', 'full'")
            mode = _MODES[mode]
        j = _Joined()
        _check(lib().jb_cut_batch_join(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, int(hmm), int(mode), sep,
                                       len(sep), term, len(term), C.byref(j.j)))
        off = np.ctypeslib.as_array(j.j.doc_off, (nd + 1,)).copy()
        if j.j.nbytes == 0:
            return np.empty(0, np.uint8), off
        # the library's buffer itself, not a copy: the array keeps `j` alive, and `j` frees the buffer
        j.__array_interface__ = {"shape": (j.j.nbytes,), "typestr": "|u1", "version": 3,
                                 "data": (C.cast(j.j.text, C.c_void_p).value, False)}
        return np.asarray(j), off

    def cut_join(self, texts, sep=" ", term="", hmm=True, mode="cut"):
        """sep.join(cut(text)) + term for every text (str / bytes) in one batch: a list of str, one per text."""
        if not texts:
            return []
        docs = [_b(t) for t in texts]
        buf = np.frombuffer(b"".join(docs) + b"\0", np.uint8)
        off = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
        out, ooff = self.cut_batch_join(buf, off, hmm, mode, sep, term)
        raw = out.tobytes()
        return [raw[int(ooff[d]):int(ooff[d + 1])].decode("utf-8") for d in range(len(docs))]

    # -- character offsets -------------------------------------------------
    def charspans_device(self, d_text_ptr, nbytes, d_doc_off, ndocs, d_start, d_end, d_doc_tok, d_ntok, cap, unit,
                         d_cstart, d_cend, d_doc_units, d_work, nwork, stream_ptr=0):
        """jb_charspans_device over raw device pointers: the byte spans of the tokens below min(*d_ntok, cap) as
        spans in runes or UTF-16 code units per document (unit "rune", "utf16" or a JB_UNIT_* value) into
        d_cstart / d_cend (they may be d_start / d_end), and each document's length into d_doc_units.
        d_work: charspans_work_bytes(nbytes, ndocs) bytes."""
        _check(lib().jb_charspans_device(self.h, C.c_void_p(d_text_ptr), nbytes, C.c_void_p(d_doc_off), ndocs,
                                         C.c_void_p(d_start), C.c_void_p(d_end), C.c_void_p(d_doc_tok),
                                         C.c_void_p(d_ntok), cap, _unit(unit), C.c_void_p(stream_ptr),
                                         C.c_void_p(d_cstart), C.c_void_p(d_cend), C.c_void_p(d_doc_units),
                                         C.c_void_p(d_work), nwork))

    def cut_batch_charspans(self, buf, doc_off, hmm, mode="cut", unit="rune", out=None):
        """jb_cut_batch_charspans: host batch -> (cstart[:n], cend[:n], doc_tok, doc_units, out), the tokens of
        `mode` ("cut", "search", "full" or a JB_MODE_* value) as per-document spans in `unit`.  `out` = (cstart
        u32, cend u32, doc_tok u64[ndocs + 1], doc_units u32[ndocs]) to reuse; the span arrays are grown when
        too small."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        nd = len(doc_off) - 1
        if isinstance(mode, str):
            if mode not in _MODES:
                raise ValueError(f"mode {mode!r}: one of 'cut', 'search', 'full'")
            mode = _MODES[mode]
        unit = _unit(unit)
        if out is None or len(out[2]) != nd + 1:
            cap = max(1024, int(doc_off[-1] - doc_off[0]) // 2)
            out = (np.empty(cap, np.uint32), np.empty(cap, np.uint32), np.empty(nd + 1, np.uint64),
                   np.empty(max(nd, 1), np.uint32))
        n = C.c_uint64()
        for _ in range(2):
            rc = lib().jb_cut_batch_charspans(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, int(hmm), int(mode), unit,
                                              out[0].ctypes.data, out[1].ctypes.data, len(out[0]), out[2].ctypes.data,
                                              C.byref(n), out[3].ctypes.data)
            if rc == JB_ELIMIT and n.value > len(out[0]):
                out = (np.empty(n.value, np.uint32), np.empty(n.value, np.uint32), out[2], out[3])
                continue
            _check(rc)
            break
        k = n.value
        return out[0][:k], out[1][:k], out[2], out[3][:nd], out

    def tokenize(self, texts, mode="default", hmm=True, unit="rune"):
        """jieba's tokenize for every text (str) of a batch: a list of [(word, start, end)] per text, with start
        and end in Unicode characters (unit "rune": word == text[start:end], taken from the str itself) or in
        UTF-16 code units (unit "utf16": the word is cut from the text's UTF-16 form).  mode "default", "search"
        or "full" (which ignores hmm).  The cut and the conversion run on the GPU; no byte offset is decoded
        here.  A str with a lone surrogate has no UTF-8 form and raises UnicodeEncodeError."""
        if mode not in _TOKENIZE_MODES:
            raise ValueError(f"mode {mode!r}: one of 'default', 'search', 'full'")
        unit = _unit(unit)
        if not texts:
            return []
        docs = [t.encode("utf-8") for t in texts]
        buf = np.frombuffer(b"".join(docs) + b"\0", np.uint8)
        off = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
        cs, ce, dtok, _, _ = self.cut_batch_charspans(buf, off, hmm, _TOKENIZE_MODES[mode], unit)
        cs, ce, dtok = cs.tolist(), ce.tolist(), dtok.tolist()
        out = []
        for d, t in enumerate(texts):
            if unit == JB_UNIT_UTF16:
                u = t.encode("utf-16-le")
                out.append([(u[2 * cs[k]:2 * ce[k]].decode("utf-16-le"), cs[k], ce[k])
                            for k in range(dtok[d], dtok[d + 1])])
            else:
                out.append([(t[cs[k]:ce[k]], cs[k], ce[k]) for k in range(dtok[d], dtok[d + 1])])
        return out

    # -- word counts and vocabulary fitting --------------------------------
    def wc_init_device(self, d_table, ntable, nslots, pool_bytes, stream_ptr=0):
        """jb_wc_init_device: an empty word-count table of nslots slots (a power of two >= 8) and pool_bytes of
        pool in the device buffer d_table (ntable >= wc_table_bytes(nslots, pool_bytes) bytes, 32-byte aligned)."""
        _check(lib().jb_wc_init_device(self.h, C.c_void_p(d_table), ntable, nslots, pool_bytes, C.c_void_p(stream_ptr)))

    def wc_add_device(self, d_table, ntable, d_text_ptr, nbytes, d_start, d_end, d_ntok, cap, d_work, nwork,
                      stream_ptr=0):
        """jb_wc_add_device over raw device pointers: the tokens k < min(*d_ntok, cap) of a span list of any mode
        added to the table; queued on the stream.  d_work: wc_work_bytes(cap) bytes."""
        _check(lib().jb_wc_add_device(self.h, C.c_void_p(d_table), ntable, C.c_void_p(d_text_ptr), nbytes,
                                      C.c_void_p(d_start), C.c_void_p(d_end), C.c_void_p(d_ntok), cap,
                                      C.c_void_p(stream_ptr), C.c_void_p(d_work), nwork))

    def wc_read(self, d_table, ntable, min_count=1, max_keys=0, stream_ptr=0):
        """jb_wc_read: synchronise the stream and read the table back sorted: a WcResult.  The table stays as it is."""
        r = jb_wc_result()
        _check(lib().jb_wc_read(self.h, C.c_void_p(d_table), ntable, C.c_void_p(stream_ptr), min_count, max_keys,
                                C.byref(r)))
        try:
            return WcResult(r)
        finally:
            lib().jb_wc_result_free(C.byref(r))

    def wc_batch(self, buf, doc_off, hmm, d_table, ntable, mode="cut"):
        """jb_wc_batch: a host batch cut in `mode` ("cut", "search", "full" or a JB_MODE_* value; full mode
        ignores hmm) and added to the table."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        if isinstance(mode, str):
            if mode not in _MODES:
                raise ValueError(f"mode {mode!r}: one of 'cut', 'search', 'full'")
            mode = _MODES[mode]
        _check(lib().jb_wc_batch(self.h, buf.ctypes.data, doc_off.ctypes.data, len(doc_off) - 1, int(hmm), int(mode),
                                 C.c_void_p(d_table), ntable))

    def word_counts(self, batches, mode="cut", hmm=True, min_count=1, max_keys=0, nslots=1 << 22,
                    pool_bytes=16 << 20, strict=True):
        """Counter(cut(text)) over a corpus given as an iterable of batches, each a list of documents (str /
        bytes): (keys, counts), the distinct tokens as bytes by count descending, then by bytes, with their
        uint64 counts.  The counting runs on the GPU in a table of nslots slots (new keys are accepted while
        fewer than half are taken) and pool_bytes for keys over 24 bytes.  When tokens were dropped for lack of
        room or two keys shared a fingerprint, the counts are lower bounds: JbError, unless strict is False."""
        r = self._word_counts(batches, mode, hmm, min_count, max_keys, nslots, pool_bytes, strict)
        return r.keys, r.counts

    def _word_counts(self, batches, mode, hmm, min_count, max_keys, nslots, pool_bytes, strict):
        ntable = wc_table_bytes(nslots, pool_bytes)
        d_table = C.c_void_p()
        _check(lib().jb_device_alloc(self.h, ntable, C.byref(d_table)))
        try:
            self.wc_init_device(d_table.value, ntable, nslots, pool_bytes)
            for batch in batches:
                docs = [_b(t) for t in batch]
                if not docs:
                    continue
                off = np.zeros(len(docs) + 1, np.uint64)
                off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
                self.wc_batch(np.frombuffer(b"".join(docs) + b"\0", np.uint8), off, hmm, d_table.value, ntable, mode)
            r = self.wc_read(d_table.value, ntable, min_count, max_keys)
        finally:
            lib().jb_device_free(self.h, d_table)
        if strict and (r.dropped or r.collided):
            raise JbError(JB_ELIMIT, f"word_counts: {r.dropped} tokens dropped for lack of room and {r.collided} in "
                                     f"fingerprint collisions: the counts are lower bounds (raise nslots / "
                                     f"pool_bytes, or pass strict=False)")
        return r

    def fit_vocab(self, batches, mode="cut", hmm=True, min_count=1, max_keys=0, nslots=1 << 22, pool_bytes=16 << 20,
                  strict=True):
        """word_counts, then set_vocab with the keys (a key's id is its rank): (keys, counts).  Afterwards ids,
        terms, IDF and keywords run on the corpus with no token string having reached the host."""
        keys, counts = self.word_counts(batches, mode, hmm, min_count, max_keys, nslots, pool_bytes, strict)
        self.set_vocab(keys)
        return keys, counts

    # -- MinHash signatures ------------------------------------------------
    def minhash_device(self, d_text_ptr, nbytes, d_start, d_end, d_doc_tok, d_ntok, cap, ndocs, n, K, seed, d_sig,
                       d_doc_n, d_work, nwork, stream_ptr=0):
        """jb_minhash_device over raw device pointers: per document the K-slot MinHash signature of its shingles
        of n tokens (u32[ndocs, K] into d_sig) and its shingle count (u32[ndocs] into d_doc_n), from a span
        list of any mode; queued on the stream.  d_work: minhash_work_bytes(cap, ndocs) bytes."""
        _check(lib().jb_minhash_device(self.h, C.c_void_p(d_text_ptr), nbytes, C.c_void_p(d_start), C.c_void_p(d_end),
                                       C.c_void_p(d_doc_tok), C.c_void_p(d_ntok), cap, ndocs, n, K, seed,
                                       C.c_void_p(stream_ptr), C.c_void_p(d_sig), C.c_void_p(d_doc_n),
                                       C.c_void_p(d_work), nwork))

    def minhash_bands_device(self, d_sig, d_doc_n, ndocs, K, B, R, d_keys, stream_ptr=0):
        """jb_minhash_bands_device over raw device pointers: the LSH keys of B bands of R rows (u64[ndocs, B] into
        d_keys) of the signatures at d_sig; queued on the stream."""
        _check(lib().jb_minhash_bands_device(self.h, C.c_void_p(d_sig), C.c_void_p(d_doc_n), ndocs, K, B, R,
                                             C.c_void_p(stream_ptr), C.c_void_p(d_keys)))

    def minhash_batch(self, buf, doc_off, hmm, n=5, K=128, seed=1, mode="cut"):
        """jb_minhash_batch: host batch -> (sig uint32[ndocs, K], doc_n uint32[ndocs]); mode "cut", "search" or
        "full" (or a JB_MODE_* value; full mode ignores hmm)."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        nd = len(doc_off) - 1
        if isinstance(mode, str):
            if mode not in _MODES:
                raise ValueError(f"mode {mode!r}: one of 'cut', 'search', 'full'")
            mode = _MODES[mode]
        sig = np.empty((nd, max(int(K), 0)), np.uint32)
        doc_n = np.empty(nd, np.uint32)
        _check(lib().jb_minhash_batch(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, int(hmm), int(mode), n, K, seed,
                                      sig.ctypes.data if sig.size else None, doc_n.ctypes.data if nd else None))
        return sig, doc_n

    def minhash(self, texts, n=5, K=128, seed=1, mode="cut", hmm=True):
        """The MinHash signatures of a batch of texts (str / bytes), cut in `mode` and sketched on the GPU over
        shingles of n consecutive words: (sig uint32[ndocs, K], doc_n uint32[ndocs]).  The share of equal slots
        of two rows estimates the Jaccard similarity of the two documents' shingle sets; a document without
        tokens has doc_n 0 and JB_MH_EMPTY in every slot.  The rule is jiebahip.h's."""
        docs = [_b(t) for t in texts]
        off = np.zeros(len(docs) + 1, np.uint64)
        if docs:
            off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
        return self.minhash_batch(np.frombuffer(b"".join(docs) + b"\0", np.uint8), off, hmm, n, K, seed, mode)

    # -- token filtering ---------------------------------------------------
    def set_stop_words(self, keys, packed=None):
        """jb_stopwords_set: attach a stop set (a list of str / bytes), replacing any earlier one.  None removes
        it; an empty list attaches an empty set."""
        if keys is None and packed is None:
            _check(lib().jb_stopwords_set(self.h, None, None, 0))
            return
        buf, off = packed if packed is not None else pack_keys(keys)
        buf = np.ascontiguousarray(buf, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        _check(lib().jb_stopwords_set(self.h, buf.ctypes.data, off.ctypes.data, len(off) - 1))

    @property
    def stop_words_size(self):
        """Keys of the attached stop set; -1 when none is attached."""
        return lib().jb_stopwords_size(self.h)

    def filter_device(self, d_text_ptr, nbytes, d_start, d_end, d_doc_tok, d_ntok, cap, ndocs, rule, d_out_start,
                      d_out_end, d_out_src, out_cap, d_out_doc_tok, d_out_ntok, d_stats, d_work, nwork, stream_ptr=0):
        """jb_filter_device over raw device pointers: the tokens of a span list of any mode that `rule` (a
        jb_filter_rule, see filter_rule) keeps, in order, as a span list of the same shape (u32 starts / ends and,
        when d_out_src is not 0, source indices at ranks below out_cap; u64 doc_tok[ndocs + 1]; a u64 count; 5 u64
        statistics); queued on the stream.  d_work: filter_work_bytes(cap, ndocs) bytes."""
        _check(lib().jb_filter_device(self.h, C.c_void_p(d_text_ptr), nbytes, C.c_void_p(d_start), C.c_void_p(d_end),
                                      C.c_void_p(d_doc_tok), C.c_void_p(d_ntok), cap, ndocs,
                                      C.byref(rule) if rule is not None else None, C.c_void_p(stream_ptr),
                                      C.c_void_p(d_out_start), C.c_void_p(d_out_end), C.c_void_p(d_out_src), out_cap,
                                      C.c_void_p(d_out_doc_tok), C.c_void_p(d_out_ntok), C.c_void_p(d_stats),
                                      C.c_void_p(d_work), nwork))

    def cut_batch_filter(self, buf, doc_off, hmm, rule, mode="cut", out=None):
        """jb_cut_batch_filter: host batch -> (start[:n], end[:n], doc_tok, stats, out), the tokens of `mode`
        ("cut", "search", "full" or a JB_MODE_* value) that `rule` keeps, as u32 byte spans relative to
        doc_off[0].  stats: uint64[5] (ntokens, nbad, nclass, nlength, nstop).  `out` = (start u32, end u32,
        doc_tok u64[ndocs + 1]) to reuse; the span arrays are grown when too small."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        nd = len(doc_off) - 1
        if isinstance(mode, str):
            if mode not in _MODES:
                raise ValueError(f"mode {mode!r}: one of 'cut', 'search', 'full'")
            mode = _MODES[mode]
        if out is None or len(out[2]) != nd + 1:
            cap = max(1024, int(doc_off[-1] - doc_off[0]) // 2)
            out = (np.empty(cap, np.uint32), np.empty(cap, np.uint32), np.empty(nd + 1, np.uint64))
        n = C.c_uint64()
        stats = np.zeros(5, np.uint64)
        for _ in range(2):
            rc = lib().jb_cut_batch_filter(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, int(hmm), int(mode),
                                           C.byref(rule) if rule is not None else None, out[0].ctypes.data,
                                           out[1].ctypes.data, len(out[0]), out[2].ctypes.data, C.byref(n),
                                           stats.ctypes.data)
            if rc == JB_ELIMIT and n.value > len(out[0]):
                out = (np.empty(n.value, np.uint32), np.empty(n.value, np.uint32), out[2])
                continue
            _check(rc)
            break
        k = n.value
        return out[0][:k], out[1][:k], out[2], stats, out

    def set_batch_filter(self, drop=(), min_runes=0, max_runes=0, stop=False):
        """jb_batch_filter_set: while set, cut_batch_join / cut_join, wc_batch / word_counts / fit_vocab and
        minhash_batch / minhash filter the cut's tokens by this rule (see filter_rule) before their own step."""
        r = filter_rule(drop, min_runes, max_runes, stop)
        _check(lib().jb_batch_filter_set(self.h, C.byref(r)))

    def clear_batch_filter(self):
        """jb_batch_filter_set(NULL): the host-batch calls see every token of the cut again."""
        _check(lib().jb_batch_filter_set(self.h, None))

    def cut_filtered(self, texts, drop=("other", "invalid"), min_runes=0, max_runes=0, stop=False, mode="cut", hmm=True):
        """`[w for w in cut(text) if ...]` for every text (str / bytes) of a batch: a list of token lists, cut in
        `mode` and filtered on the GPU by class, length in runes and the stop set (set_stop_words).  An invalid
        byte that is kept comes back as U+FFFD."""
        docs = [_b(t) for t in texts]
        if not docs:
            return []
        all_ = b"".join(docs)
        off = np.zeros(len(docs) + 1, np.uint64)
        off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
        s, e, dtok, _, _ = self.cut_batch_filter(np.frombuffer(all_ + b"\0", np.uint8), off, hmm,
                                                 filter_rule(drop, min_runes, max_runes, stop), mode)
        s, e, dtok = s.tolist(), e.tolist(), dtok.tolist()
        return [[all_[s[k]:e[k]].decode("utf-8", "replace") for k in range(dtok[d], dtok[d + 1])]
                for d in range(len(docs))]

    # -- postings (the inverted index) ------------------------------------------
    def postings_device(self, d_term_id, d_term_cnt, d_term_off, d_nterms, cap, ndocs, nids, doc_base, d_post_doc,
                        d_post_tf, pcap, d_post_off, d_nposts, d_work, nwork, stream_ptr=0):
        """jb_postings_device over raw device pointers: the CSR of terms_device by columns.  The entries
        i < min(*d_nterms, cap, term_off[ndocs]) with id < nids, stably sorted by id, as u32 documents (doc_base +
        row) and term frequencies at positions below pcap, u64 post_off[nids + 1] and a u64 count; queued on the
        stream.  d_work: postings_work_bytes(cap, nids, ndocs) bytes."""
        _check(lib().jb_postings_device(self.h, C.c_void_p(d_term_id), C.c_void_p(d_term_cnt), C.c_void_p(d_term_off),
                                        C.c_void_p(d_nterms), cap, ndocs, nids, doc_base, C.c_void_p(stream_ptr),
                                        C.c_void_p(d_post_doc), C.c_void_p(d_post_tf), pcap, C.c_void_p(d_post_off),
                                        C.c_void_p(d_nposts), C.c_void_p(d_work), nwork))

    def postings_batch(self, buf, doc_off, hmm, doc_base=0, nids=None, pcap=None):
        """jb_postings_batch: host batch -> (post_off u64[nids + 1], post_doc u32[n], post_tf u32[n], doc_len
        u32[ndocs]) of the plain cut's terms under the attached vocabulary; document numbers start at doc_base.
        nids defaults to vocab_size.  With `pcap` given the arrays hold that many entries and a longer result
        raises JbError(JB_ELIMIT); otherwise they are grown to the count the first call reports."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        nd = len(doc_off) - 1
        if nids is None:
            nids = max(self.vocab_size, 0)
        cap = max(1024, int(doc_off[-1] - doc_off[0]) // 4) if pcap is None else pcap
        post_off = np.zeros(nids + 1, np.uint64)
        doc_len = np.zeros(nd, np.uint32)
        n = C.c_uint64()
        p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        for _ in range(2):
            pd, pt = np.empty(cap, np.uint32), np.empty(cap, np.uint32)
            rc = lib().jb_postings_batch(self.h, buf.ctypes.data, doc_off.ctypes.data, nd, int(hmm), doc_base, cap,
                                         post_off.ctypes.data, nids, p(pd), p(pt), C.byref(n), p(doc_len))
            if rc == JB_ELIMIT and n.value > cap and pcap is None:
                cap = n.value
                continue
            _check(rc)
            break
        return post_off, pd[:n.value], pt[:n.value], doc_len

    def build_index(self, batches, hmm=True):
        """Index a corpus given as an iterable of batches, each a list of documents (str / bytes), under the
        attached vocabulary: (post_off u64[vocab_size + 1], post_doc u32, post_tf u32, doc_len u32[ndocs], ndocs).
        The list of id t is post_doc / post_tf[post_off[t]:post_off[t + 1]], ascending by document number
        (documents are numbered in the order they come); doc_len is each document's token count."""
        nv = self.vocab_size
        if nv < 0:
            raise JbError(JB_EINVAL, "build_index: no vocabulary attached (set_vocab)")
        parts, lens, ndocs = [], [], 0
        for batch in batches:
            docs = [_b(t) for t in batch]
            if not docs:
                continue
            off = np.zeros(len(docs) + 1, np.uint64)
            off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
            po, pd, pt, dl = self.postings_batch(np.frombuffer(b"".join(docs) + b"\0", np.uint8), off, hmm, ndocs, nv)
            parts.append((po, pd, pt))
            lens.append(dl)
            ndocs += len(docs)
        post_off = np.zeros(nv + 1, np.uint64)
        for po, _, _ in parts:
            post_off += po
        total = int(post_off[nv])
        post_doc, post_tf = np.empty(total, np.uint32), np.empty(total, np.uint32)
        # batch b's list of id t goes behind the lists of id t of the batches before it
        at = post_off[:-1].astype(np.int64)
        for po, pd, pt in parts:
            n = np.diff(po.astype(np.int64))
            if len(pd):
                dst = np.repeat(at - po[:-1].astype(np.int64), n) + np.arange(len(pd), dtype=np.int64)
                post_doc[dst] = pd
                post_tf[dst] = pt
            at += n
        doc_len = np.concatenate(lens) if lens else np.zeros(0, np.uint32)
        return post_off, post_doc, post_tf, doc_len, ndocs

    # -- BM25 search over the index ------------------------------------------
    def bm25_norms_device(self, d_doc_len, ndocs, k1, b, avgdl, d_norm, stream_ptr=0):
        """jb_bm25_norms_device over raw device pointers: f32 norm[d] from u32 doc_len[d]; queued on the stream."""
        _check(lib().jb_bm25_norms_device(self.h, C.c_void_p(d_doc_len), ndocs, k1, b, avgdl, C.c_void_p(stream_ptr),
                                          C.c_void_p(d_norm)))

    def bm25_idf_device(self, d_post_off, nids, ndocs_total, d_weight, stream_ptr=0):
        """jb_bm25_idf_device over raw device pointers: f32 weight[t] from the lists' lengths; queued on the stream."""
        _check(lib().jb_bm25_idf_device(self.h, C.c_void_p(d_post_off), nids, ndocs_total, C.c_void_p(stream_ptr),
                                        C.c_void_p(d_weight)))

    def bm25_search_device(self, d_post_doc, d_post_tf, d_post_off, npost, nids, d_norm, ndocs, d_weight, nweights, k1,
                           d_q_id, q_cap, d_q_off, nq, topk, d_res_doc, d_res_score, d_res_n, d_work, nwork,
                           stream_ptr=0):
        """jb_bm25_search_device over raw device pointers: per query of the CSR (u32 q_id, u64 q_off[nq + 1]) the
        topk best documents of the index as u32 res_doc / u64 res_score [nq, topk] (units of 2^-24) and u32
        res_n[nq]; queued on the stream.  d_work: bm25_work_bytes(nq, ndocs, topk) bytes."""
        _check(lib().jb_bm25_search_device(self.h, C.c_void_p(d_post_doc), C.c_void_p(d_post_tf), C.c_void_p(d_post_off),
                                           npost, nids, C.c_void_p(d_norm), ndocs, C.c_void_p(d_weight), nweights, k1,
                                           C.c_void_p(d_q_id), q_cap, C.c_void_p(d_q_off), nq, topk,
                                           C.c_void_p(stream_ptr), C.c_void_p(d_res_doc), C.c_void_p(d_res_score),
                                           C.c_void_p(d_res_n), C.c_void_p(d_work), nwork))

    def set_index(self, post_off, post_doc, post_tf, doc_len, ndocs=None, k1=1.2, b=0.75):
        """jb_index_set: attach an index to search, replacing any earlier one: build_index's tuple unchanged
        (tk.set_index(*tk.build_index(batches))).  The postings, the documents' norms and the ids' BM25 weights
        stay on the device."""
        po = np.ascontiguousarray(post_off, np.uint64)
        pd = np.ascontiguousarray(post_doc, np.uint32)
        pt = np.ascontiguousarray(post_tf, np.uint32)
        dl = np.ascontiguousarray(doc_len, np.uint32)
        if ndocs is not None and ndocs != len(dl):
            raise ValueError(f"set_index: ndocs = {ndocs}, doc_len has {len(dl)} entries")
        if len(pd) != len(pt):
            raise ValueError("set_index: post_doc and post_tf differ in length")
        p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        _check(lib().jb_index_set(self.h, po.ctypes.data, p(pd), p(pt), len(pd), len(po) - 1, p(dl), len(dl), k1, b))

    def clear_index(self):
        """jb_index_clear: detach the index."""
        _check(lib().jb_index_clear(self.h))

    def index_info(self):
        """jb_index_info: (ndocs, nids, npost, avgdl) of the attached index."""
        nd, ni, npo, av = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        _check(lib().jb_index_info(self.h, C.byref(nd), C.byref(ni), C.byref(npo), C.byref(av)))
        return nd.value, ni.value, npo.value, av.value

    def search_batch(self, buf, q_off, hmm, topk=10):
        """jb_search_batch: host query text -> (res_doc u32[nq, topk], res_score u64[nq, topk], res_n u32[nq])."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        nq = len(q_off) - 1
        rows = max(nq, 1) * max(int(topk), 1)
        rd, rs, rn = np.empty(rows, np.uint32), np.empty(rows, np.uint64), np.empty(max(nq, 1), np.uint32)
        _check(lib().jb_search_batch(self.h, buf.ctypes.data, q_off.ctypes.data, nq, int(hmm), topk, rd.ctypes.data,
                                     rs.ctypes.data, rn.ctypes.data))
        shape = (nq, int(topk))
        return rd[:nq * topk].reshape(shape), rs[:nq * topk].reshape(shape), rn[:nq]

    def search(self, queries, topk=10, hmm=True):
        """Rank the attached index's documents for each query (str / bytes) by BM25: per query a list of
        (document, score), best first, at most topk.  The query is cut in plain mode and looked up in the
        attached vocabulary; unknown tokens do not count."""
        qs = [_b(t) for t in queries]
        off = np.zeros(len(qs) + 1, np.uint64)
        if qs:
            off[1:] = np.cumsum([len(q) for q in qs], dtype=np.uint64)
        rd, rs, rn = self.search_batch(np.frombuffer(b"".join(qs) + b"\0", np.uint8), off, hmm, topk)
        return [[(int(rd[q, r]), int(rs[q, r]) / JB_BM25_ONE) for r in range(int(rn[q]))] for q in range(len(qs))]

    # -- near-duplicate pairs ----------------------------------------------------
    def neardup_device(self, d_key, d_sig, ndocs, B, K, W, min_agree, d_pair_doc, d_pair_agree, pcap, d_pair_off,
                       d_npairs, d_stat, d_work, nwork, stream_ptr=0):
        """jb_neardup_device over raw device pointers: the band keys (u64[ndocs, B]) joined per bucket inside the
        window W and verified against the signatures (u32[ndocs, K]): the kept pairs as a CSR by the later document
        (u32 earlier documents and agree counts at positions below pcap, u64 pair_off[ndocs + 1], a u64 count and
        u64 stat[JB_ND_NSTAT]); queued on the stream.  d_work: neardup_work_bytes(ndocs, B) bytes."""
        _check(lib().jb_neardup_device(self.h, C.c_void_p(d_key), C.c_void_p(d_sig), ndocs, B, K, W, min_agree,
                                       C.c_void_p(d_pair_doc), C.c_void_p(d_pair_agree), pcap, C.c_void_p(d_pair_off),
                                       C.c_void_p(d_npairs), C.c_void_p(d_stat), C.c_void_p(d_work), nwork,
                                       C.c_void_p(stream_ptr)))

    def near_duplicates(self, sig, doc_n, B, R, W=64, min_agree=None, pcap=None):
        """jb_neardup_sig: host signatures (uint32[ndocs, K]) and shingle counts -> (pair_off u64[ndocs + 1],
        pair_doc u32[n], pair_agree u32[n], stat u64[JB_ND_NSTAT]): row j lists the earlier documents i kept as
        near-duplicates of j.  min_agree defaults to the integer nearest 0.8 K.  With `pcap` given the arrays hold
        that many pairs and a longer result raises JbError(JB_ELIMIT); otherwise they are grown to the count the
        first call reports."""
        sig = np.ascontiguousarray(sig, np.uint32)
        doc_n = np.ascontiguousarray(doc_n, np.uint32)
        nd, K = sig.shape
        if min_agree is None:
            min_agree = _default_agree(K)
        cap = max(1024, 4 * nd) if pcap is None else pcap
        pair_off = np.zeros(nd + 1, np.uint64)
        stat = np.zeros(JB_ND_NSTAT, np.uint64)
        n = C.c_uint64()
        p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        for _ in range(2):
            pd, pa = np.empty(cap, np.uint32), np.empty(cap, np.uint32)
            rc = lib().jb_neardup_sig(self.h, p(sig), p(doc_n), nd, K, B, R, W, min_agree, p(pd), p(pa), cap,
                                      pair_off.ctypes.data, C.byref(n), stat.ctypes.data)
            if rc == JB_ELIMIT and n.value > cap and pcap is None:
                cap = n.value
                continue
            _check(rc)
            break
        return pair_off, pd[:n.value], pa[:n.value], stat

    def dedup(self, texts, n=5, K=128, B=32, R=4, W=64, min_agree=None, seed=1, mode="cut", hmm=True):
        """Near-duplicate groups of a batch of texts (str / bytes): cut, MinHash over shingles of n words, LSH
        bands and the bucket join on the GPU, then the groups' labels.  Returns (label uint32[ndocs], keep
        bool[ndocs]): label[d] is the least document of d's group and keep[d] = (label[d] == d) marks the one
        document of each group to keep.  min_agree defaults to the integer nearest 0.8 K."""
        sig, doc_n = self.minhash(texts, n, K, seed, mode, hmm)
        pair_off, pair_doc, _, _ = self.near_duplicates(sig, doc_n, B, R, W, min_agree)
        label = neardup_labels(pair_off, pair_doc)
        return label, label == np.arange(len(label), dtype=np.uint32)

    # -- collocations: adjacent-pair counts and new-word scores ---------------
    def colloc_init_device(self, d_table, ntable, nslots, d_uni, nuni, stream_ptr=0):
        """jb_colloc_init_device: an empty pair table of nslots slots (a power of two >= 8) in the device buffer
        d_table (ntable >= colloc_table_bytes(nslots) bytes, 32-byte aligned), and d_uni (u64[nuni]) zeroed."""
        _check(lib().jb_colloc_init_device(self.h, C.c_void_p(d_table), ntable, nslots, C.c_void_p(d_uni), nuni,
                                           C.c_void_p(stream_ptr)))

    def colloc_add_device(self, d_table, ntable, d_uni, nuni, d_ids, ids_cap, d_doc_tok, d_ntok, ndocs, d_keep, nkeep,
                          flags, d_start, d_end, d_work, nwork, stream_ptr=0):
        """jb_colloc_add_device over raw device pointers: the unigrams and adjacent pairs of the tokens
        k < min(*d_ntok, ids_cap) added to d_uni and the table; queued on the stream.  d_work:
        colloc_work_bytes(ids_cap, ndocs) bytes."""
        _check(lib().jb_colloc_add_device(self.h, C.c_void_p(d_table), ntable, C.c_void_p(d_uni), nuni,
                                          C.c_void_p(d_ids), ids_cap, C.c_void_p(d_doc_tok), C.c_void_p(d_ntok), ndocs,
                                          C.c_void_p(d_keep), nkeep, flags, C.c_void_p(d_start), C.c_void_p(d_end),
                                          C.c_void_p(stream_ptr), C.c_void_p(d_work), nwork))

    def colloc_score_device(self, d_table, ntable, d_uni, nuni, scorer, min_count, threshold, d_cand_a, d_cand_b,
                            d_cand_cnt, d_cand_score, ccap, d_ncand, stream_ptr=0):
        """jb_colloc_score_device over raw device pointers: the table's candidates under a scorer ("npmi", "ratio",
        "count" or a JB_COLLOC_* value) into arrays of capacity ccap, *d_ncand the complete count; queued."""
        _check(lib().jb_colloc_score_device(self.h, C.c_void_p(d_table), ntable, C.c_void_p(d_uni), nuni,
                                            _scorer(scorer), min_count, threshold, C.c_void_p(d_cand_a),
                                            C.c_void_p(d_cand_b), C.c_void_p(d_cand_cnt), C.c_void_p(d_cand_score), ccap,
                                            C.c_void_p(d_ncand), C.c_void_p(stream_ptr)))

    def colloc_read(self, d_table, ntable, d_uni, nuni, scorer="npmi", min_count=5, threshold=0.5, topn=0,
                    stream_ptr=0):
        """jb_colloc_read: synchronise the stream, score on the device and read the candidates back sorted: a
        CollocResult.  The table stays as it is."""
        r = jb_colloc_result()
        _check(lib().jb_colloc_read(self.h, C.c_void_p(d_table), ntable, C.c_void_p(d_uni), nuni, _scorer(scorer),
                                    min_count, threshold, topn, C.c_void_p(stream_ptr), C.byref(r)))
        try:
            return CollocResult(r)
        finally:
            lib().jb_colloc_result_free(C.byref(r))

    def colloc_batch(self, buf, doc_off, hmm, d_table, ntable, d_uni, nuni, keep=None, flags=0):
        """jb_colloc_batch: a host batch cut in plain mode, numbered by the attached vocabulary and added to the
        table and d_uni; the batch filter applies when one is set."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        keep = np.zeros(0, np.uint8) if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
        _check(lib().jb_colloc_batch(self.h, buf.ctypes.data, doc_off.ctypes.data, len(doc_off) - 1, int(hmm),
                                     keep.ctypes.data if len(keep) else None, len(keep), flags, C.c_void_p(d_table),
                                     ntable, C.c_void_p(d_uni), nuni))

    def _collocations(self, batches, scorer, min_count, threshold, topn, contiguous, keep, hmm, nslots):
        nuni = self.vocab_size
        if nuni <= 0:
            raise JbError(JB_EINVAL, "collocations: no vocabulary attached (set_vocab, fit_vocab)")
        ntable = colloc_table_bytes(nslots)
        d_table, d_uni = C.c_void_p(), C.c_void_p()
        _check(lib().jb_device_alloc(self.h, ntable, C.byref(d_table)))
        try:
            _check(lib().jb_device_alloc(self.h, nuni * 8, C.byref(d_uni)))
            self.colloc_init_device(d_table.value, ntable, nslots, d_uni.value, nuni)
            for batch in batches:
                docs = [_b(t) for t in batch]
                if not docs:
                    continue
                off = np.zeros(len(docs) + 1, np.uint64)
                off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
                self.colloc_batch(np.frombuffer(b"".join(docs) + b"\0", np.uint8), off, hmm, d_table.value, ntable,
                                  d_uni.value, nuni, keep, JB_COLLOC_CONTIG if contiguous else 0)
            r = self.colloc_read(d_table.value, ntable, d_uni.value, nuni, scorer, min_count, threshold, topn)
        finally:
            lib().jb_device_free(self.h, d_uni)
            lib().jb_device_free(self.h, d_table)
        if r.dropped:
            raise JbError(JB_ELIMIT, f"collocations: {r.dropped} pairs dropped for lack of room: pairs are missing "
                                     f"(raise nslots)")
        return r

    def collocations(self, batches, scorer="npmi", min_count=5, threshold=0.5, topn=0, contiguous=False, keep=None,
                     hmm=True, nslots=1 << 24):
        """The collocations of a corpus given as an iterable of batches, each a list of documents (str / bytes):
        a list of (key_a, key_b, count, score), best first, the keys (bytes) those of the attached vocabulary
        (set_vocab, fit_vocab), counted and scored on the GPU.  contiguous counts a pair only when the two tokens
        touch in the text; keep (u8 per id) limits the pairs to kept ids; nslots sizes the pair table (new pairs
        are accepted while fewer than half are taken).  JbError when pairs were dropped for lack of room."""
        r = self._collocations(batches, scorer, min_count, threshold, topn, contiguous, keep, hmm, nslots)
        keys = self._vocab_keys
        return [(keys[int(a)], keys[int(b)], int(c), float(s)) for a, b, c, s in zip(r.a, r.b, r.count, r.score)]

    def find_new_words(self, batches, scorer="npmi", min_count=5, threshold=0.5, topn=0, hmm=False, nslots=1 << 24):
        """collocations with contiguous=True over the vocabulary keys whose every rune is Han: the concatenations
        a+b (str) the dictionary lacks (dict_get absent or 0), best first, ready for AddWord.  hmm is off by
        default: the HMM itself glues runs of single runes, which hides the pairs this looks for."""
        keep = np.array([1 if is_han_key(k) else 0 for k in self._vocab_keys or []], np.uint8)
        out, seen = [], set()
        for a, b, _, _ in self.collocations(batches, scorer, min_count, threshold, 0, True, keep, hmm, nslots):
            w = (a + b).decode("utf-8")
            if w in seen or self.dict_get(w):
                continue
            seen.add(w)
            out.append(w)
            if topn and len(out) == topn:
                break
        return out

    def device_status(self, stream_ptr=0):
        """jb_device_status: raises JbError when the last device pipeline hit an error."""
        _check(lib().jb_device_status(self.h, C.c_void_p(stream_ptr)))

    def last_stats(self):
        """Counters of the last pipeline run (jb_last_stats); synchronises."""
        st = jb_stats()
        _check(lib().jb_last_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in jb_stats._fields_}

    def last_ties(self):
        return self.last_stats()["viterbi_ties"]

    # -- dictionary ------------------------------------------------------
    def AddWord(self, word, freq):
        """Tokenizer.AddWord (tokenizer.go:372) without the reference's deadlock."""
        w = _b(word)
        _check(lib().jb_add_word(self.h, w, len(w), freq))

    def suggest_freq(self, word):
        """suggestFreq (tokenizer.go:589-614)."""
        w = _b(word)
        f = C.c_int64()
        _check(lib().jb_suggest_freq(self.h, w, len(w), C.byref(f)))
        return f.value

    def add_log(self, logs):
        """jb_add_log: caller-computed {x: math.Log(float64(x))} for the next image build."""
        ks = np.ascontiguousarray(list(logs.keys()), np.int64)
        vs = np.ascontiguousarray([logs[k] for k in logs.keys()], np.float64)
        _check(lib().jb_add_log(self.h, ks.ctypes.data, vs.ctypes.data, len(ks)))

    def dict_get(self, word):
        w = _b(word)
        f = C.c_int64()
        return f.value if _check(lib().jb_dict_get(self.h, w, len(w), C.byref(f))) else None

    @property
    def size(self):
        return lib().jb_dict_size(self.h)

    # -- profiling -------------------------------------------------------
    def profile(self, on=True):
        _check(lib().jb_profile_enable(self.h, int(on)))

    def profile_reset(self):
        _check(lib().jb_profile_reset(self.h))

    def profile_read(self):
        cap = 128  # (more than the library's kernels: 63)
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        n = (C.c_uint64 * cap)()
        k = _check(lib().jb_profile_read(self.h, names, ms, n, cap))
        return {names[i].decode(): (ms[i], n[i]) for i in range(k)}


class HostBuffer:
    """jb_host_alloc'd pinned memory as a numpy uint8 array (`.array`); batches cut
    from that array skip the library's staging copy."""

    def __init__(self, n):
        p = C.c_void_p()
        _check(lib().jb_host_alloc(n, C.byref(p)))
        self.p = p
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(n, 1)).from_address(p.value))[:n]

    def free(self):
        if self.p:
            self.array = None
            lib().jb_host_free(self.p)
            self.p = None


def mask_to_spans(ms, me, nbytes, base=0):
    """Boundary masks -> (starts, ends) byte spans (start bit k pairs with end bit k)."""
    nw = (nbytes + 63) // 64
    sb = np.unpackbits(np.asarray(ms[:nw]).view(np.uint8), bitorder="little")[:nbytes]
    eb = np.unpackbits(np.asarray(me[:nw]).view(np.uint8), bitorder="little")[:nbytes]
    return (np.flatnonzero(sb).astype(np.uint64) + np.uint64(base),
            np.flatnonzero(eb).astype(np.uint64) + np.uint64(base + 1))


_hip = None


def dev_to_host(ptr, nbytes, dtype):
    """Copy nbytes of device memory at a raw pointer into a numpy array."""
    global _hip
    if _hip is None:
        lib()
        _hip = C.CDLL("libamdhip64.so.7")  # the runtime libjiebahip.so is bound to
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype)
    if nbytes:
        rc = _hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2)  # hipMemcpyDeviceToHost
        if rc != 0:
            raise JbError(JB_EDEVICE, f"hipMemcpy failed: {rc}")
    return out


def loaded_runtime():
    """Paths of the HIP runtime and of libjiebahip.so mapped into this process."""
    out = set()
    try:
        with open("/proc/self/maps") as f:
            for l in f:
                if "libamdhip64" in l or "libjiebahip" in l:
                    out.add(l.split()[-1])
    except OSError:
        pass
    return sorted(out)


def shard_bounds(doc_off, nparts):
    """jb_shard_bounds: the document ranges jb_cut_batch gives each device."""
    doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
    cut = np.zeros(nparts + 1, np.uint32)
    _check(lib().jb_shard_bounds(doc_off.ctypes.data, len(doc_off) - 1, nparts, cut.ctypes.data))
    return [int(x) for x in cut]


def split_points(buf, doc_off, nparts):
    """jb_split_points: byte cuts at document starts or Han-run starts."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
    cut = np.zeros(nparts + 1, np.uint64)
    _check(lib().jb_split_points(buf.ctypes.data, doc_off.ctypes.data, len(doc_off) - 1, nparts, cut.ctypes.data))
    return [int(x) for x in cut]


def terms_work_bytes(max_tokens, ndocs):
    """jb_terms_work_bytes: bytes of the work buffer jb_terms_device needs (host only)."""
    return lib().jb_terms_work_bytes(max_tokens, ndocs)


def go_log(x):
    return lib().jb_go_log(float(x))


def idf(df, ndocs, min_df=1, max_df=None, keep=None):
    """jb_idf (host only): weights f32[len(df)] from document frequencies: 0 where df is 0, below min_df,
    above max_df (None: no upper bound) or where keep[id] == 0; else the smoothed IDF
    float32(go_log((ndocs + 1) / (df + 1)) + 1)."""
    df = np.ascontiguousarray(df, dtype=np.uint32)
    w = np.empty(len(df), np.float32)
    k = None
    if keep is not None:
        k = np.ascontiguousarray(keep, dtype=np.uint8)
        if len(k) != len(df):
            raise ValueError("keep: one entry per id")
    _check(lib().jb_idf(df.ctypes.data if len(df) else None, len(df), ndocs, min_df,
                        JB_DF_NOMAX if max_df is None else max_df, k.ctypes.data if k is not None and len(k) else None,
                        w.ctypes.data if len(w) else None))
    return w


def join_work_bytes(max_tokens, ndocs):
    """jb_join_work_bytes: bytes of the work buffer jb_join_device needs (host only)."""
    return lib().jb_join_work_bytes(max_tokens, ndocs)


def join(text, starts, ends, doc_tok, sep=b" ", term=b"\n", ntok=None, cap=None, nbytes=None, out_cap=None):
    """jb_join (host only): the joined-text rule of jiebahip.h on host arrays (text bytes or a uint8 array, u32
    spans, u64 doc_tok).  Returns (out uint8[out_cap], out_doc_off u64[ndocs + 1], nout); without out_cap the
    output array holds exactly the nout bytes."""
    t = np.ascontiguousarray(text, np.uint8) if isinstance(text, np.ndarray) else np.frombuffer(_b(text), np.uint8)
    s = np.ascontiguousarray(starts, np.uint32)
    e = np.ascontiguousarray(ends, np.uint32)
    d = np.ascontiguousarray(doc_tok, np.uint64)
    sep, term = _b(sep), _b(term)
    nd = len(d) - 1
    cap = len(s) if cap is None else cap
    ntok = len(s) if ntok is None else ntok
    nbytes = len(t) if nbytes is None else nbytes
    off = np.empty(nd + 1, np.uint64)
    n = C.c_uint64()

    def call(out, ocap):
        _check(lib().jb_join(t.ctypes.data if len(t) else None, nbytes, s.ctypes.data if len(s) else None,
                             e.ctypes.data if len(e) else None, d.ctypes.data, ntok, cap, nd, sep, len(sep), term,
                             len(term), out.ctypes.data if ocap else None, ocap, off.ctypes.data, C.byref(n)))
    if out_cap is None:
        call(np.empty(1, np.uint8), 0)
        out_cap = n.value
    out = np.empty(max(out_cap, 1), np.uint8)
    call(out, out_cap)
    return out[:out_cap], off, n.value


def wc_table_bytes(nslots, pool_bytes):
    """jb_wc_table_bytes: bytes of a word-count table of nslots slots and pool_bytes of pool (host only)."""
    return lib().jb_wc_table_bytes(nslots, pool_bytes)


def wc_work_bytes(max_tokens):
    """jb_wc_work_bytes: bytes of the work buffer jb_wc_add_device needs (host only)."""
    return lib().jb_wc_work_bytes(max_tokens)


def wc_fp(key, bits=64):
    """jb_wc_fp (host only): the fingerprint of a key (1 .. 255 bytes) that keeps the hash's low `bits` bits."""
    k = _b(key)
    return lib().jb_wc_fp(k, len(k), bits)


def wc_count(text, starts, ends, ntok=None, cap=None, nbytes=None, min_count=1, max_keys=0):
    """jb_wc_count (host only): the word-count rule of jiebahip.h on host arrays (text bytes or a uint8 array,
    u32 spans): a WcResult."""
    t = np.ascontiguousarray(text, np.uint8) if isinstance(text, np.ndarray) else np.frombuffer(_b(text), np.uint8)
    s = np.ascontiguousarray(starts, np.uint32)
    e = np.ascontiguousarray(ends, np.uint32)
    cap = len(s) if cap is None else cap
    ntok = len(s) if ntok is None else ntok
    nbytes = len(t) if nbytes is None else nbytes
    r = jb_wc_result()
    _check(lib().jb_wc_count(t.ctypes.data if len(t) else None, nbytes, s.ctypes.data if len(s) else None,
                             e.ctypes.data if len(e) else None, ntok, cap, min_count, max_keys, C.byref(r)))
    try:
        return WcResult(r)
    finally:
        lib().jb_wc_result_free(C.byref(r))


def minhash_work_bytes(max_tokens, ndocs):
    """jb_minhash_work_bytes: bytes of the work buffer jb_minhash_device needs (host only)."""
    return lib().jb_minhash_work_bytes(max_tokens, ndocs)


def minhash_params(seed, K):
    """jb_minhash_params (host only): (a uint64[K], b uint64[K]), the K hash functions of `seed`."""
    a, b = np.empty(max(int(K), 0), np.uint64), np.empty(max(int(K), 0), np.uint64)
    _check(lib().jb_minhash_params(seed, K, a.ctypes.data if len(a) else None, b.ctypes.data if len(b) else None))
    return a, b


def minhash(text, starts, ends, doc_tok, n=5, K=128, seed=1, ntok=None, cap=None, nbytes=None):
    """jb_minhash (host only): the MinHash rule of jiebahip.h on host arrays (text bytes or a uint8 array, u32
    spans, u64 doc_tok): (sig uint32[ndocs, K], doc_n uint32[ndocs])."""
    t = np.ascontiguousarray(text, np.uint8) if isinstance(text, np.ndarray) else np.frombuffer(_b(text), np.uint8)
    s = np.ascontiguousarray(starts, np.uint32)
    e = np.ascontiguousarray(ends, np.uint32)
    d = np.ascontiguousarray(doc_tok, np.uint64)
    nd = len(d) - 1
    cap = len(s) if cap is None else cap
    ntok = len(s) if ntok is None else ntok
    nbytes = len(t) if nbytes is None else nbytes
    sig = np.empty((nd, max(int(K), 0)), np.uint32)
    doc_n = np.empty(nd, np.uint32)
    p = lambda a: a.ctypes.data if a.size else None
    _check(lib().jb_minhash(p(t), nbytes, p(s), p(e), d.ctypes.data, ntok, cap, nd, n, K, seed, p(sig), p(doc_n)))
    return sig, doc_n


def minhash_bands(sig, doc_n, B, R):
    """jb_minhash_bands (host only): the LSH keys (uint64[ndocs, B]) of B bands of R rows of the signatures
    sig (uint32[ndocs, K]); doc_n (uint32[ndocs]) marks the documents without shingles, which get JB_MH_NOKEY."""
    sig = np.ascontiguousarray(sig, np.uint32)
    doc_n = np.ascontiguousarray(doc_n, np.uint32)
    nd, K = sig.shape
    keys = np.empty((nd, max(int(B), 0)), np.uint64)
    p = lambda a: a.ctypes.data if a.size else None
    _check(lib().jb_minhash_bands(p(sig), p(doc_n), nd, K, B, R, p(keys)))
    return keys


def filter_work_bytes(max_tokens, ndocs):
    """jb_filter_work_bytes: bytes of the work buffer jb_filter_device needs (host only)."""
    return lib().jb_filter_work_bytes(max_tokens, ndocs)


def filter_spans(text, starts, ends, doc_tok, rule=None, stop=None, ntok=None, cap=None, nbytes=None, out_cap=None,
                 src=True):
    """jb_filter (host only): the filter rule of jiebahip.h on host arrays (text bytes or a uint8 array, u32 spans,
    u64 doc_tok).  `rule` is a jb_filter_rule (see filter_rule; None keeps every good span), `stop` a Vocab or
    None.  Returns (out_start, out_end, out_src or None, out_doc_tok, out_ntok, stats uint64[5]); the arrays have
    out_cap entries (default cap), of which min(out_ntok, out_cap) are written."""
    t = np.ascontiguousarray(text, np.uint8) if isinstance(text, np.ndarray) else np.frombuffer(_b(text), np.uint8)
    s = np.ascontiguousarray(starts, np.uint32)
    e = np.ascontiguousarray(ends, np.uint32)
    d = np.ascontiguousarray(doc_tok, np.uint64)
    nd = len(d) - 1
    cap = len(s) if cap is None else cap
    ntok = len(s) if ntok is None else ntok
    nbytes = len(t) if nbytes is None else nbytes
    out_cap = cap if out_cap is None else out_cap
    rule = filter_rule() if rule is None else rule
    os_, oe = np.zeros(out_cap, np.uint32), np.zeros(out_cap, np.uint32)
    osrc = np.zeros(out_cap, np.uint32) if src else None
    odt = np.zeros(nd + 1, np.uint64)
    n = C.c_uint64()
    stats = np.zeros(5, np.uint64)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    _check(lib().jb_filter(p(t), nbytes, p(s), p(e), d.ctypes.data, ntok, cap, nd, C.byref(rule),
                           stop.h if stop is not None else None, p(os_), p(oe), p(osrc), out_cap, odt.ctypes.data,
                           C.byref(n), stats.ctypes.data))
    return os_, oe, osrc, odt, n.value, stats


def postings_work_bytes(max_terms, nids, ndocs):
    """jb_postings_work_bytes: bytes of the work buffer jb_postings_device needs (host only)."""
    return lib().jb_postings_work_bytes(max_terms, nids, ndocs)


def postings(term_id, term_cnt, term_off, nids, doc_base=0, nterms=None, cap=None, pcap=None):
    """jb_postings (host only): the postings rule of jiebahip.h on host arrays (a CSR: u32 ids and counts, u64
    term_off[ndocs + 1]).  Returns (post_doc, post_tf, post_off u64[nids + 1], nposts); the arrays have pcap
    entries (default cap), of which min(nposts, pcap) are written."""
    ti = np.ascontiguousarray(term_id, np.uint32)
    tc = np.ascontiguousarray(term_cnt, np.uint32)
    to = np.ascontiguousarray(term_off, np.uint64)
    nd = len(to) - 1
    cap = len(ti) if cap is None else cap
    nterms = len(ti) if nterms is None else nterms
    pcap = cap if pcap is None else pcap
    pd, pt = np.zeros(pcap, np.uint32), np.zeros(pcap, np.uint32)
    po = np.zeros(nids + 1, np.uint64)
    n = C.c_uint64()
    p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    _check(lib().jb_postings(p(ti), p(tc), to.ctypes.data, nterms, cap, nd, nids, doc_base, p(pd), p(pt), pcap,
                             po.ctypes.data, C.byref(n)))
    return pd, pt, po, n.value


def _default_agree(K):
    """The integer nearest 0.8 K, at least 1: the near-duplicate calls' default threshold."""
    return max(1, (4 * int(K) + 2) // 5)


def neardup_work_bytes(ndocs, B):
    """jb_neardup_work_bytes: bytes of the work buffer jb_neardup_device needs (host only)."""
    return lib().jb_neardup_work_bytes(ndocs, B)


def neardup(key, sig, W=64, min_agree=None, pcap=None):
    """jb_neardup (host only): the near-duplicate rule of jiebahip.h on host arrays (band keys uint64[ndocs, B],
    signatures uint32[ndocs, K]).  Returns (pair_doc, pair_agree, pair_off u64[ndocs + 1], npairs, stat
    u64[JB_ND_NSTAT]); without `pcap` the arrays hold exactly the npairs pairs, with it they have pcap entries,
    of which min(npairs, pcap) are written.  min_agree defaults to the integer nearest 0.8 K."""
    key = np.ascontiguousarray(key, np.uint64)
    sig = np.ascontiguousarray(sig, np.uint32)
    (nd, B), K = key.shape, sig.shape[1]
    if sig.shape[0] != nd:
        raise ValueError("neardup: key and sig have different numbers of rows")
    if min_agree is None:
        min_agree = _default_agree(K)
    po, st, n = np.zeros(nd + 1, np.uint64), np.zeros(JB_ND_NSTAT, np.uint64), C.c_uint64()
    p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    for cap in ((0, None) if pcap is None else (pcap,)):
        cap = n.value if cap is None else cap
        pd, pa = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        _check(lib().jb_neardup(p(key), p(sig), nd, B, K, W, min_agree, p(pd), p(pa), cap, po.ctypes.data, C.byref(n),
                                st.ctypes.data))
    return pd, pa, po, n.value, st


def neardup_labels(pair_off, pair_doc, pcap=None):
    """jb_neardup_labels (host only): label uint32[ndocs], the least document of each document's connected
    component over the pairs of the CSR (pair_off u64[ndocs + 1], pair_doc u32); pcap defaults to len(pair_doc)."""
    po = np.ascontiguousarray(pair_off, np.uint64)
    pd = np.ascontiguousarray(pair_doc, np.uint32)
    nd = len(po) - 1
    label = np.zeros(nd, np.uint32)
    _check(lib().jb_neardup_labels(po.ctypes.data, pd.ctypes.data if pd.size else None, len(pd) if pcap is None else pcap,
                                   nd, label.ctypes.data if nd else None))
    return label


def bm25_work_bytes(nq, ndocs, topk):
    """jb_bm25_work_bytes: bytes of the work buffer jb_bm25_search_device needs (host only)."""
    return lib().jb_bm25_work_bytes(nq, ndocs, topk)


def bm25_avgdl(doc_len):
    """jb_bm25_avgdl (host only): the mean of u32 doc_len as a float."""
    dl = np.ascontiguousarray(doc_len, np.uint32)
    av = C.c_double()
    _check(lib().jb_bm25_avgdl(dl.ctypes.data if dl.size else None, len(dl), C.byref(av)))
    return av.value


def bm25_norms(doc_len, k1, b, avgdl):
    """jb_bm25_norms (host only): f32 norm[d] = k1 * ((1 - b) + b * doc_len[d] / avgdl)."""
    dl = np.ascontiguousarray(doc_len, np.uint32)
    out = np.zeros(len(dl), np.float32)
    p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    _check(lib().jb_bm25_norms(p(dl), len(dl), k1, b, avgdl, p(out)))
    return out


def bm25_idf(post_off, ndocs_total):
    """jb_bm25_idf (host only): f32 weight[t] = go_log(1 + (N - df + 0.5) / (df + 0.5)) from the lists' lengths."""
    po = np.ascontiguousarray(post_off, np.uint64)
    out = np.zeros(len(po) - 1, np.float32)
    _check(lib().jb_bm25_idf(po.ctypes.data, len(po) - 1, ndocs_total, out.ctypes.data if out.size else None))
    return out


def bm25_search(post_doc, post_tf, post_off, norm, weight, k1, q_id, q_off, topk=10, npost=None, nids=None, ndocs=None,
                nweights=None, q_cap=None):
    """jb_bm25_search (host only): the search rule of jiebahip.h on host arrays.  Returns (res_doc u32[nq, topk],
    res_score u64[nq, topk] in units of 2^-24, res_n u32[nq])."""
    pd = np.ascontiguousarray(post_doc, np.uint32)
    pt = np.ascontiguousarray(post_tf, np.uint32)
    po = np.ascontiguousarray(post_off, np.uint64)
    nm = np.ascontiguousarray(norm, np.float32)
    wt = np.ascontiguousarray(weight, np.float32)
    qi = np.ascontiguousarray(q_id, np.uint32)
    qo = np.ascontiguousarray(q_off, np.uint64)
    npost = min(len(pd), len(pt)) if npost is None else npost
    nids = len(po) - 1 if nids is None else nids
    ndocs = len(nm) if ndocs is None else ndocs
    nweights = len(wt) if nweights is None else nweights
    q_cap = len(qi) if q_cap is None else q_cap
    nq = len(qo) - 1
    rows = max(nq, 1) * max(int(topk), 1)
    rd, rs, rn = np.zeros(rows, np.uint32), np.zeros(rows, np.uint64), np.zeros(max(nq, 1), np.uint32)
    p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    _check(lib().jb_bm25_search(p(pd), p(pt), po.ctypes.data, npost, nids, p(nm), ndocs, p(wt), nweights, k1, p(qi), q_cap,
                                qo.ctypes.data, nq, topk, rd.ctypes.data, rs.ctypes.data, rn.ctypes.data))
    shape = (nq, int(topk))
    return rd[:nq * topk].reshape(shape), rs[:nq * topk].reshape(shape), rn[:nq]


def _unit(unit):
    if isinstance(unit, str):
        if unit not in _UNITS:
            raise ValueError(f"unit {unit!r}: one of 'rune', 'utf16'")
        return _UNITS[unit]
    return int(unit)


def charspans_work_bytes(nbytes, ndocs):
    """jb_charspans_work_bytes: bytes of the work buffer jb_charspans_device needs (host only)."""
    return lib().jb_charspans_work_bytes(nbytes, ndocs)


def charspans(text, doc_off, starts, ends, doc_tok, unit="rune", ntok=None, cap=None, nbytes=None, inplace=False):
    """jb_charspans (host only): the character-offset rule of jiebahip.h on host arrays (text bytes or a uint8
    array, u64 doc_off, u32 spans, u64 doc_tok).  Returns (cstart u32[cap], cend u32[cap], doc_units
    u32[ndocs]); entries at or past min(ntok, cap) are left as JB_CHAR_NONE - 1 (0xFFFFFFFE), which the rule
    never writes.  inplace: the outputs are the (copied) span arrays themselves."""
    t = np.ascontiguousarray(text, np.uint8) if isinstance(text, np.ndarray) else np.frombuffer(_b(text), np.uint8)
    o = np.ascontiguousarray(doc_off, np.uint64)
    s = np.array(starts, np.uint32)
    e = np.array(ends, np.uint32)
    d = np.ascontiguousarray(doc_tok, np.uint64)
    nd = len(o) - 1
    cap = len(s) if cap is None else cap
    ntok = len(s) if ntok is None else ntok
    if inplace:
        cs, ce = s, e
    else:
        cs, ce = np.full(len(s), 0xFFFFFFFE, np.uint32), np.full(len(e), 0xFFFFFFFE, np.uint32)
    units = np.zeros(nd, np.uint32)
    p = lambda a: a.ctypes.data if len(a) else None
    nbytes = len(t) if nbytes is None else nbytes
    _check(lib().jb_charspans(p(t), nbytes, o.ctypes.data, nd, p(s), p(e), d.ctypes.data, ntok, cap, _unit(unit),
                              p(cs), p(ce), p(units)))
    return cs, ce, units


def textrank_work_bytes(max_tokens, max_terms, ndocs):
    """jb_textrank_work_bytes: bytes of the work buffer jb_textrank_device needs (host only)."""
    return lib().jb_textrank_work_bytes(max_tokens, max_terms, ndocs)


def textrank(ids, doc_tok, term_id, term_off, keep, span=5, iters=10, topk=20, ntok=None, ids_cap=None, cap=None):
    """jb_textrank (host only): the TextRank rule of jiebahip.h on host arrays, with the CSR rows of
    jb_terms_device (term_id, term_off) taken from the caller -> (kw_id u32[ndocs, topk], kw_score f32,
    kw_n u32[ndocs]).  ntok, ids_cap and cap default to the arrays' lengths."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    doc_tok = np.ascontiguousarray(doc_tok, dtype=np.uint64)
    term_id = np.ascontiguousarray(term_id, dtype=np.uint32)
    term_off = np.ascontiguousarray(term_off, dtype=np.uint64)
    k = np.ascontiguousarray(keep, dtype=np.uint8)
    nd = len(doc_tok) - 1
    if len(term_off) != nd + 1:
        raise ValueError("term_off: one entry per document and one more")
    ids_cap = len(ids) if ids_cap is None else ids_cap
    cap = len(term_id) if cap is None else cap
    if ids_cap > len(ids) or cap > len(term_id):
        raise ValueError("ids_cap / cap: at most the arrays' lengths")
    rows = max(nd, 1) * max(int(topk), 1)
    ki, ks, kn = np.empty(rows, np.uint32), np.empty(rows, np.float32), np.empty(max(nd, 1), np.uint32)
    _check(lib().jb_textrank(ids.ctypes.data if len(ids) else None, ids_cap, doc_tok.ctypes.data,
                             len(ids) if ntok is None else ntok, nd, term_id.ctypes.data if len(term_id) else None,
                             term_off.ctypes.data, cap, k.ctypes.data if len(k) else None, len(k), span, iters, topk,
                             ki.ctypes.data, ks.ctypes.data, kn.ctypes.data))
    shape = (nd, int(topk))
    return ki[:nd * topk].reshape(shape), ks[:nd * topk].reshape(shape), kn[:nd]


def is_han_key(key):
    """Is every rune of the key Han, by the class test jb_filter uses (jb_is_han's ranges)?"""
    try:
        t = _b(key).decode("utf-8")
    except UnicodeDecodeError:
        return False
    return len(t) > 0 and all(_is_han(ord(ch)) for ch in t)


# jb_is_han's ranges (jb_common.h: Unicode 13.0.0 Script=Han), the test jb_filter's class JB_TC_HAN uses
_HAN_RANGES = ((0x2E80, 0x2E99), (0x2E9B, 0x2EF3), (0x2F00, 0x2FD5), (0x3005, 0x3005), (0x3007, 0x3007),
               (0x3021, 0x3029), (0x3038, 0x303B), (0x3400, 0x4DBF), (0x4E00, 0x9FFC), (0xF900, 0xFA6D),
               (0xFA70, 0xFAD9), (0x16FF0, 0x16FF1), (0x20000, 0x2A6DD), (0x2A700, 0x2B734), (0x2B740, 0x2B81D),
               (0x2B820, 0x2CEA1), (0x2CEB0, 0x2EBE0), (0x2F800, 0x2FA1D), (0x30000, 0x3134A))


def _is_han(r):
    return any(lo <= r <= hi for lo, hi in _HAN_RANGES)


def colloc_table_bytes(nslots):
    """jb_colloc_table_bytes: the bytes of a pair table of nslots slots."""
    return lib().jb_colloc_table_bytes(nslots)


def colloc_work_bytes(max_tokens, ndocs):
    """jb_colloc_work_bytes: the bytes of jb_colloc_add_device's work buffer."""
    return lib().jb_colloc_work_bytes(max_tokens, ndocs)


def colloc_count(ids, doc_tok, uni, keep=None, flags=0, starts=None, ends=None, ntok=None, ids_cap=None, nslots=0):
    """jb_colloc_count, the rule of the add on host arrays (no GPU): uni (uint64, modified in place) gets the
    unigrams, and a CollocResult holds every pair in the table sorted by key with the batch's totals."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    doc_tok = np.ascontiguousarray(doc_tok, dtype=np.uint64)
    assert uni.dtype == np.uint64 and uni.flags.c_contiguous
    keep = np.zeros(0, np.uint8) if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    ids_cap = len(ids) if ids_cap is None else ids_cap
    ntok = ids_cap if ntok is None else ntok
    st = None if starts is None else np.ascontiguousarray(starts, dtype=np.uint32)
    en = None if ends is None else np.ascontiguousarray(ends, dtype=np.uint32)
    r = jb_colloc_result()
    _check(lib().jb_colloc_count(ids.ctypes.data if len(ids) else None, ids_cap, doc_tok.ctypes.data, ntok,
                                 len(doc_tok) - 1, keep.ctypes.data if len(keep) else None, len(keep), flags,
                                 None if st is None else st.ctypes.data, None if en is None else en.ctypes.data, nslots,
                                 uni.ctypes.data if len(uni) else None, len(uni), C.byref(r)))
    try:
        return CollocResult(r)
    finally:
        lib().jb_colloc_result_free(C.byref(r))


def colloc_score(a, b, count, uni, N, scorer="npmi", min_count=5, threshold=0.5, topn=0, nuni=None):
    """jb_colloc_score, the score rule on host arrays (no GPU): the candidates in the rule's order."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    uni = np.ascontiguousarray(uni, dtype=np.uint64)
    nuni = len(uni) if nuni is None else nuni
    r = jb_colloc_result()
    _check(lib().jb_colloc_score(a.ctypes.data if len(a) else None, b.ctypes.data if len(a) else None,
                                 count.ctypes.data if len(a) else None, len(a), uni.ctypes.data if len(uni) else None, nuni,
                                 N, _scorer(scorer), min_count, threshold, topn, C.byref(r)))
    try:
        return CollocResult(r)
    finally:
        lib().jb_colloc_result_free(C.byref(r))
