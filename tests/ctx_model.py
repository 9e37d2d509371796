"""A shadow model of one long-lived tokenizer, and a generator of call sequences: a helper, not a test.

Model answers every call of a sequence from the references the suite already trusts (Oracle.cut_batch,
search_ref, full_ref, vocab_ref, terms_ref, df_ref, textrank_ref, join_ref, charspans_ref, wc_ref) and keeps
what a jb_ctx keeps between calls: the dictionary (an Oracle that add_word changes), the vocabulary (a Python
dict) with its keep mask and weights, and the token count jb_last_stats owes the caller; and what a caller
keeps beside it, the word-count table (a Counter that only grows).  It never calls the code under test; the
one thing it takes from libjiebahip.so is Go's logarithm (jiebahip.go_log, a host function), through bm25_ref
and colloc_ref as the per-feature tests do, so the index and collocation-score cases need the built library.

gen_ops(seed, nsteps) draws a sequence of plain tuples (see OPS); make_batch turns a tuple's batch
specification into text.  coverage(ops) says which of the transitions between calls a sequence contains;
test_ctx_model.py pins the seeds that test_gpu_sequences.py runs to the ones that contain them all.
gen_ops2 / coverage2 / SEEDS2 are the same over OPS2, which adds the calls of joined text, character offsets
and word counts; gen_ops' own output is pinned by a digest in test_ctx_model.py.
gen_ops3 / coverage3 / SEEDS3 do the same over OPS3: MinHash, the caller's filter, postings, BM25 search,
near-duplicate pairs and collocations (minhash_ref, filter_ref, postings_ref, bm25_ref, neardup_ref, colloc_ref
over the model's spans), with the three pieces of state that came with them: the stop set, the ctx's batch
filter (FILTERED says which calls honour it) and the attached index; and a second caller-owned table, the
collocation counts.  gen_ops2's output is pinned by a digest too.
"""
import collections
import random
import re

from collections import Counter

import numpy as np

import bm25_ref as BR
import charspans_ref as CR
import colloc_ref as CLR
import df_ref as DR
import filter_ref as FR
import full_ref as F
import join_ref as JR
import minhash_ref as MR
import neardup_ref as NR
import oracle as O
import postings_ref as PR
import search_ref as R
import synth
import terms_ref as TR
import textrank_ref as KR
import vocab_ref as V
import wc_ref as W

UNK = V.UNK
MODES = ("plain", "search", "full")
ROUTES = ("host", "device", "device_into")
CLASSES = ("tiny", "small", "grow", "manydocs", "empty", "offset")
OPS = ("cut", "add_word", "set_vocab", "ids", "keywords_batch", "df_batch", "textrank_batch", "last_stats")
BATCH_OPS = ("keywords_batch", "df_batch", "textrank_batch")
SMALL_MAX = 4096  # k_small's limit in bytes (and in documents)
WORK_MIN_BYTES, WORK_MIN_DOCS = 4096, 1024  # ensure_work's floor
MAX_BYTES = 400 << 10
VOCAB_SOURCE = ("small", 1700, 40 << 10)  # the batch whose tokens the vocabularies are drawn from
# The sequences test_gpu_sequences.py runs: gen_ops(seed, NSTEPS).  test_ctx_model.py holds every seed to
# covered(): swap one for a seed that misses a transition and that test fails.
SEEDS = (6, 24, 38)
NSTEPS = 40
# The second op set: the calls of joined text, character offsets and word counts among the older ones.
NEW_BATCH_OPS = ("join_batch", "charspans_batch", "wc_batch")
ALL_BATCH_OPS = BATCH_OPS + NEW_BATCH_OPS
OPS2 = OPS + NEW_BATCH_OPS + ("join", "charspans", "wc_read")
UNITS = {"rune": CR.RUNE, "utf16": CR.UTF16}
LIB_MODE = {"plain": "cut", "search": "search", "full": "full"}  # the binding's names of MODES
SEEDS2 = (1308, 1931, 3045)  # gen_ops2(seed, NSTEPS2); held to covered2() by test_ctx_model.py
NSTEPS2 = 60
# The word-count table of a sequence (one for all its wc_batch calls); test_ctx_model.py asserts from the
# model that no sequence fills a quarter of the slots or half of the pool.
WC_NSLOTS, WC_POOL = 1 << 18, 1 << 20
# The collocation table of a sequence or a script, under the same cap: no more than a quarter of the slots are
# taken (new pairs are accepted while fewer than half are), asserted from the model in test_ctx_model.py.
COLLOC_NSLOTS = 1 << 18
# Which *_batch kinds run the ctx's batch filter (jb_batch_filter_set) between their cut and their own step.
# test_ctx_model.py derives the same table from the FrontOpts of every entry point of jb_batch.cpp.
FILTERED = {"join_batch": True, "wc_batch": True, "minhash_batch": True, "colloc_batch": True,
            "charspans_batch": False, "filter_batch": False, "keywords_batch": False, "df_batch": False,
            "textrank_batch": False, "postings_batch": False, "search_batch": False}
ENTRY_POINTS = {"join_batch": "jb_cut_batch_join", "wc_batch": "jb_wc_batch", "minhash_batch": "jb_minhash_batch",
                "colloc_batch": "jb_colloc_batch", "charspans_batch": "jb_cut_batch_charspans",
                "filter_batch": "jb_cut_batch_filter", "keywords_batch": "jb_keywords_batch", "df_batch": "jb_df_batch",
                "textrank_batch": "jb_textrank_batch", "postings_batch": "jb_postings_batch",
                "search_batch": "jb_search_batch"}
SCORERS = {"npmi": CLR.NPMI, "ratio": CLR.RATIO, "count": CLR.COUNT}
CLASS_BITS = {"han": FR.HAN, "alnum": FR.ALNUM, "num": FR.NUM, "other": FR.OTHER, "invalid": FR.INVALID}


class ModelError(Exception):
    """The model's JB_EINVAL."""


class Rule(collections.namedtuple("Rule", "drop min_runes max_runes stop")):
    """A filter rule: drop is a mask of filter_ref's class bits."""


def rule(drop=(), min_runes=0, max_runes=0, stop=False):
    m = 0
    for c in drop:
        m |= CLASS_BITS[c]
    return Rule(m, min_runes, max_runes, bool(stop))


# The rules the sequences use, by number: as a caller's rule (filter_batch) and as the ctx's batch filter; the last
# two ask for the stop set.
RULES = (rule(("other", "invalid"), 2), rule(("alnum", "num", "other"), 0, 2), rule(("other",), 0, 0, True),
         rule(("invalid",), 0, 2, True))

Index = collections.namedtuple("Index", "post_off post_doc post_tf doc_len nids vversion k1 b norm weight",
                               defaults=(None, None, None, None))


# ---- batches ---------------------------------------------------------------------------------------------
class Batch:
    """A batch as the host calls take it: buf (64 zero bytes behind the text), doc_off (which may start
    inside buf), and the specification it was made from."""

    def __init__(self, spec, buf, off):
        self.spec = spec
        self.off = np.ascontiguousarray(off, np.uint64)
        end = int(self.off[-1])
        b = np.zeros(end + 64, np.uint8)
        b[:end] = np.asarray(buf, np.uint8)[:end]
        self.buf = b
        self.nbytes = end - int(self.off[0])
        self.ndocs = len(self.off) - 1

    def rel(self):
        """(text, doc_off) with doc_off[0] == 0, as the device calls take them."""
        a = int(self.off[0])
        return self.buf[a:], self.off - np.uint64(a)


def from_texts(spec, texts):
    buf, off = R.batch_of(texts)
    return Batch(spec, buf, off)


def _trim(off, limit):
    """The longest prefix of whole documents of at most `limit` bytes (at least one document)."""
    n = max(1, int(np.searchsorted(np.asarray(off, np.uint64), limit, side="right")) - 1)
    return off[:n + 1]


DUP_SENTENCES = 10


def dup_plan(a, b):
    """Per document of the dups batch (a, b): ("new", None, None), ("copy", source, None) or ("near", source,
    the sentence replaced); a source is an earlier new document."""
    assert 4 <= b <= 64
    rng = random.Random(a)
    plan, news = [], []
    for k in range(b):
        if k < 2 or k % 2 == 0:
            news.append(k)
            plan.append(("new", None, None))
        elif k % 4 == 1:
            plan.append(("copy", rng.choice(news), None))
        else:
            plan.append(("near", rng.choice(news), rng.randrange(DUP_SENTENCES)))
    return plan


def make_batch(s, spec):
    """spec = (class, a, b) -> Batch, from the synthetic generator s (synth.Synth):
    tiny      b sentences from document a: at most 4,096 bytes, k_small's route for a plain host call
    small     documents from a, at most b bytes (6 to 60 KiB)
    grow      documents from a, at most b bytes (up to 400 KiB)
    large     as grow: the large batch of a *_batch call
    manydocs  b documents of one or two runes, cut from the sentences at a
    empty     b empty documents
    offset    as small, from sentences, and starting at document 3 of its buffer
    dups      b documents (at most 64) of DUP_SENTENCES sentences each, from the sentences at a: about half are
              new; of the rest, in turn, one is an exact copy of an earlier document and one a copy with one
              sentence replaced by a new one (dup_plan says which)
    queries   as tiny (b <= 8; more sentences give a batch over 4,096 bytes), with an empty document and one of
              ASCII words behind the sentences: queries for search_batch, of which some find documents and
              some find none"""
    cls, a, b = spec
    if cls == "queries":
        buf, off, _ = s.corpus(synth.KIND_SENTENCES, a, max_docs=b)
        o = [int(x) for x in (_trim(off, SMALL_MAX - 64) if b <= 8 else off)]
        return from_texts(spec, [bytes(buf[o[k]:o[k + 1]]) for k in range(len(o) - 1)] + [b"", b"zzz 2999 qqq"])
    if cls == "dups":
        buf, off, _ = s.corpus(synth.KIND_SENTENCES, a, max_docs=(b + 1) * DUP_SENTENCES)
        o = [int(x) for x in off]
        sent = [bytes(buf[o[k]:o[k + 1]]) for k in range(len(o) - 1)]
        assert len(sent) == (b + 1) * DUP_SENTENCES
        docs, fresh = [], iter(sent)
        for kind, src, pos in dup_plan(a, b):
            if kind == "new":
                docs.append([next(fresh) for _ in range(DUP_SENTENCES)])
            elif kind == "copy":
                docs.append(list(docs[src]))
            else:
                docs.append(docs[src][:pos] + [next(fresh)] + docs[src][pos + 1:])
        return from_texts(spec, [b"".join(d) for d in docs])
    if cls == "tiny":
        buf, off, _ = s.corpus(synth.KIND_SENTENCES, a, max_docs=b)
        return Batch(spec, buf, _trim(off, SMALL_MAX))
    if cls in ("small", "grow", "large"):
        buf, off, _ = s.corpus(synth.KIND_DOCS, a, target_bytes=b)
        return Batch(spec, buf, _trim(off, b))
    if cls == "offset":
        buf, off, _ = s.corpus(synth.KIND_SENTENCES, a, target_bytes=b)
        return Batch(spec, buf, _trim(off, b)[3:])
    if cls == "manydocs":
        buf, off, _ = s.corpus(synth.KIND_SENTENCES, a, target_bytes=8 * b)
        runes = bytes(buf[:int(off[-1])]).decode("utf-8", "ignore")
        rng = random.Random(a)
        docs, p = [], 0
        while len(docs) < b:
            n = rng.randint(1, 2)
            docs.append(runes[p:p + n])
            p += n
        assert p <= len(runes)
        return from_texts(spec, docs)
    if cls == "empty":
        return Batch(spec, np.zeros(0, np.uint8), np.zeros(b + 1, np.uint64))
    raise ValueError(spec)


# ---- the model ---------------------------------------------------------------------------------------------
class Model:
    def __init__(self, dict_bytes, emit_bytes, kind=0, size_override=0, source=None):
        """source: the Batch the vocabularies and the words to add are drawn from (vocab_keys, pick_word)."""
        self.o = O.Oracle(dict_bytes, emit_bytes, kind, size_override)
        self.version = 0  # of the dictionary
        self.vversion = 0  # of the vocabulary
        self.vocab = None
        self.keys = None
        self.keep = None
        self.weights = None
        self.last_tokens = None  # what jb_last_stats()["tokens"] must be; None before the first cut
        self.source = source
        self._fresh()
        self._cache = {}
        self._pool = None
        self.wc = Counter()  # the word-count table: wc_ref's keys, only ever added to
        self.wc_bad = self.wc_long = self.wc_tokens = 0
        self.stop, self.sversion = None, 0  # the stop set: a frozenset of byte keys, or None
        self.bfilter, self.fversion = None, 0  # the batch filter: a Rule, or None
        self.index, self.iversion = None, 0  # the attached index (build_index, set_index) and how many there were
        self.cl = None  # the collocation table (colloc_init)
        self.events = []  # ("filtered", spec, rule, tokens, kept) of every use of a rule: test_ctx_model.py reads it

    def _fresh(self):
        self.grams = R.Grams(self.o)
        self.blocks = F.Blocks(self.o)

    # -- the dictionary
    def suggest(self, word):
        """suggestFreq (tokenizer.go:589-614): -> (frequency, the pieces of Cut(word, false))."""
        pieces = self.o.cut(word, False)
        dsize = float(self.o.size)
        if dsize < 1.0:
            dsize = 1.0
        f = 1.0
        for p in pieces:
            v = self.o.get(p)
            f *= float(v if v is not None else 1) / dsize
        return max(int(f * dsize) + 1, self.o.get(word) or 1), pieces

    def add_word(self, word, freq):
        """AddWord (tokenizer.go:372-379, 580-585) -> the frequency stored.  With freq < 1 the library cuts
        the word to suggest one: that cut is the ctx's last one."""
        if freq < 1:
            freq, pieces = self.suggest(word)
            self.last_tokens = len(pieces)
        self.o.add_term(word, freq)
        self.version += 1
        self._fresh()  # (both cache dictionary lookups)
        return freq

    def reachable(self, word):
        """Whether buildDag can reach `word` once it is a key with a positive frequency: every proper prefix
        is a key (tokenizer.go:475-478; AddWord adds none), and the first rune passes the gate (:468-471)."""
        return (self.o.get(word[0]) or 0) > 0 and all(self.o.get(word[:k]) is not None for k in range(2, len(word)))

    def is_edge(self, word):
        """Whether build_dag of the word alone has the edge over all of it."""
        return len(word) in self.o.build_dag(word).get(0, [])

    def pick_word(self, k, batch=None):
        """The k-th pair of adjacent Han runes of the batch (default: the source batch) that is reachable and
        not a key, as test_graph_replay_after_add_word picks its word."""
        b = batch or self.source
        text = bytes(b.buf[int(b.off[0]):int(b.off[-1])]).decode("utf-8", "replace")
        seen = []
        for m in re.finditer("(?=([一-龥]{2}))", text):
            w = m.group(1)
            if w not in seen and self.o.get(w) is None and self.reachable(w):
                seen.append(w)
                if len(seen) > k:
                    return w
        raise ValueError(f"fewer than {k + 1} candidate words")

    # -- the vocabulary
    def vocab_keys(self, vid):
        """Vocabulary number vid: a seeded part of the source batch's tokens, in a seeded order.  An even vid
        takes 60 % of the tokens of at most six bytes; an odd one a quarter of all of them, and one key
        longer than any token: fewer keys and a longer longest key, among them tokens that occur."""
        if self._pool is None:
            s, e, _ = self.o.cut_batch(self.source.buf, self.source.off, True)
            data = bytes(self.source.buf)
            self._pool = sorted({V.span_key(data, a, b) for a, b in zip(s.tolist(), e.tolist())})
        rng = random.Random(1000 + vid)
        keys = [k for k in self._pool if rng.random() < (0.25 if vid & 1 else 0.6) and (vid & 1 or len(k) <= 6)]
        rng.shuffle(keys)
        if vid & 1:
            keys.append(("長" * (12 + vid)).encode())
        return keys

    def stop_keys(self, sid):
        """Stop set number sid: 40 of the source batch's most frequent tokens, every second one from the sid-th
        on, so that the sets of two neighbouring numbers share no key."""
        s, e, _ = self.o.cut_batch(self.source.buf, self.source.off, True)
        data = bytes(self.source.buf)
        c = Counter(V.span_key(data, a, b) for a, b in zip(s.tolist(), e.tolist()))
        return [k for k, _ in sorted(c.items(), key=lambda kv: (-kv[1], kv[0]))][sid % 2::2][:40]

    def set_vocab(self, keys):
        self.keys = list(keys)
        self.vocab = V.key_dict(self.keys)
        self.vversion += 1
        rng = np.random.default_rng(len(self.keys))
        self.keep = np.array([len(k.decode("utf-8", "replace")) >= 2 for k in self.keys], np.uint8)
        w = rng.random(len(self.keys)).astype(np.float32) * np.float32(8.0)
        w[rng.random(len(self.keys)) < 0.1] = 0.0
        self.weights = w

    # -- cuts
    def cut(self, batch, mode, hmm, count=True):
        """(starts u64, ends u64, doc_tok u64) of the batch in the mode, offsets into batch.buf."""
        hmm = bool(hmm) and mode != "full"
        key = (batch.spec, mode, hmm, self.version)
        if key not in self._cache:
            if mode == "full":
                self._cache[key] = F.expected(self.o, batch.buf, batch.off, self.blocks)
            else:
                pk = (batch.spec, "plain", hmm, self.version)
                if pk not in self._cache:
                    s, e, d = self.o.cut_batch(batch.buf, batch.off, hmm, nthreads=8)
                    self._cache[pk] = (s.astype(np.uint64), e.astype(np.uint64), d)
                if mode == "search":
                    self._cache[key] = R.expand(self.o, batch.buf, *self._cache[pk], self.grams)
        if count:  # (search and full mode report the plain counts)
            self.last_tokens = len(self.cut(batch, "plain", hmm, count=False)[0])
        return self._cache[key]

    def ids(self, text, starts, ends, nbytes):
        return V.expect_ids(self.vocab, bytes(text), [int(x) for x in starts], [int(x) for x in ends], nbytes)

    # -- the *_batch calls: plain Cut -> ids -> terms, then the call's own step
    def chain(self, batch, hmm):
        key = (batch.spec, "chain", bool(hmm), self.version, self.vversion)
        if key not in self._cache:
            s, e, d = self.cut(batch, "plain", hmm, count=False)
            ids = self.ids(batch.buf, s, e, int(batch.off[-1]))
            self._cache[key] = (ids, d, TR.terms(ids, d, len(ids), max(len(ids), 1)))
        self.last_tokens = len(self._cache[key][0])
        return self._cache[key]

    def keywords(self, batch, hmm, topk):
        _, _, csr = self.chain(batch, hmm)
        return TR.keywords(csr, self.weights, topk)

    def df(self, batch, hmm, ndf):
        _, _, (tid, _, _) = self.chain(batch, hmm)
        return DR.df(tid, len(tid), max(len(tid), 1), ndf)

    def textrank(self, batch, hmm, span=5, iters=10, topk=20):
        key = (batch.spec, "textrank", bool(hmm), self.version, self.vversion, span, iters, topk)
        ids, d, (tid, _, toff) = self.chain(batch, hmm)
        if key not in self._cache:
            self._cache[key] = KR.textrank(ids, d, tid, toff, self.keep, span, iters, topk)
        return self._cache[key]

    # -- joined text, character offsets, word counts: join_ref, charspans_ref and wc_ref over the model's spans
    def join(self, batch, mode, hmm, sep, term):
        """jb_cut_batch_join -> (the output's bytes, out_doc_off as a list)."""
        hmm = bool(hmm) and mode != "full"
        s, e, d = self.spans("join_batch", batch, mode, hmm)
        key = (batch.spec, "join", mode, hmm, self.version, sep, term, self.fkey("join_batch"))
        if key not in self._cache:
            self._cache[key] = JR.join_ref(batch.buf[:int(batch.off[-1])], s, e, d, sep, term)
        return self._cache[key]

    def charspans(self, batch, mode, hmm, unit):
        """jb_cut_batch_charspans -> (cstart, cend, doc_tok, doc_units)."""
        hmm = bool(hmm) and mode != "full"
        s, e, d = self.cut(batch, mode, hmm)
        key = (batch.spec, "charspans", mode, hmm, self.version, unit)
        if key not in self._cache:
            cs, ce, un = CR.charspans_ref(batch.buf[:int(batch.off[-1])], batch.off, s, e, d, UNITS[unit])
            self._cache[key] = (np.array(cs, np.uint32), np.array(ce, np.uint32), d, np.array(un, np.uint32))
        return self._cache[key]

    def wc_add(self, text, starts, ends, ntok=None, cap=None, nbytes=None):
        """jb_wc_add_device: the spans' keys into the table."""
        r = W.wc_ref(text, starts, ends, ntok, cap, nbytes)
        self.wc.update(r.all)
        self.wc_bad += r.bad
        self.wc_long += r.long
        self.wc_tokens += r.tokens

    def wc_batch(self, batch, mode, hmm):
        """jb_wc_batch: the batch's tokens in the mode into the table, with the dictionary as it is now."""
        s, e, _ = self.spans("wc_batch", batch, mode, hmm)
        self.wc_add(batch.buf[:int(batch.off[-1])], s, e)

    def wc_result(self):
        """What jb_wc_read owes the caller: a wc_ref.Ref of the whole table, in the rule's order."""
        items = W.order(self.wc)
        return W.Ref([k for k, _ in items], [v for _, v in items], self.wc_bad, self.wc_long, self.wc_tokens, dict(self.wc))

    def wc_size(self):
        """(distinct keys, their bytes together): what the table has to hold."""
        return len(self.wc), sum(len(k) for k in self.wc)

    # -- the stop set and the batch filter
    def set_stop(self, keys):
        """jb_stopwords_set: a list of byte keys, or None for no stop set."""
        self.stop = None if keys is None else frozenset(keys)
        self.sversion += 1

    def set_filter(self, rule):
        """jb_batch_filter_set: a Rule, or None to clear.  A second rule replaces the first."""
        self.bfilter = rule
        self.fversion += 1

    def fkey(self, kind):
        """The part of a cache key that follows the batch filter, for a call of `kind`."""
        if not (FILTERED[kind] and self.bfilter is not None):
            return None
        return (self.bfilter, self.sversion if self.bfilter.stop else None)

    def filtered(self, batch, mode, hmm, rule):
        """filter_ref over the model's spans of the batch -> (starts u64, ends u64, doc_tok u64, stats list).
        A rule that asks for a stop set while there is none is the library's JB_EINVAL, raised by the filter
        step after the cut has run (jb_batch.cpp:151, batch_filter_step -> jb_filter_device's check,
        jb_capi.cpp:1418): jb_last_stats follows the cut."""
        hmm = bool(hmm) and mode != "full"
        s, e, d = self.cut(batch, mode, hmm)
        if rule.stop and self.stop is None:
            raise ModelError("JB_FILTER_STOP without a stop set")
        key = (batch.spec, "filtered", mode, hmm, self.version, rule, self.sversion if rule.stop else None)
        if key not in self._cache:
            end = int(batch.off[-1])
            fs, fe, _, fd, _, stats = FR.filter_ref(batch.buf[:end], s, e, d, FR.STOP if rule.stop else 0, rule.drop,
                                                    rule.min_runes, rule.max_runes, self.stop or (), nbytes=end)
            self._cache[key] = (np.array(fs, np.uint64), np.array(fe, np.uint64), np.array(fd, np.uint64), stats)
        self.events.append(("filtered", batch.spec, rule, self._cache[key][3][0], len(self._cache[key][0])))
        return self._cache[key]

    def spans(self, kind, batch, mode, hmm):
        """The span list a *_batch call of `kind` works on: the cut's, or what the batch filter keeps of it
        when one is set and the call honours it (FILTERED)."""
        if FILTERED[kind] and self.bfilter is not None:
            return self.filtered(batch, mode, hmm, self.bfilter)[:3]
        return self.cut(batch, mode, hmm)

    # -- MinHash, the caller's filter, postings, search, near-duplicates, collocations
    def minhash(self, batch, mode, hmm, n, K, seed):
        """jb_minhash_batch -> (sig u32[ndocs, K], doc_n u32[ndocs])."""
        hmm = bool(hmm) and mode != "full"
        s, e, d = self.spans("minhash_batch", batch, mode, hmm)
        key = (batch.spec, "minhash", mode, hmm, self.version, n, K, seed, self.fkey("minhash_batch"))
        if key not in self._cache:
            end = int(batch.off[-1])
            self._cache[key] = MR.minhash_ref(batch.buf[:end], s, e, d, n, K, seed, nbytes=end)
        return self._cache[key]

    def filter_batch(self, batch, mode, hmm, rule):
        """jb_cut_batch_filter with the caller's rule -> (start u32, end u32, doc_tok u64, stats u64[5]), the
        spans relative to doc_off[0].  The ctx's batch filter plays no part.  Without the stop set the rule asks
        for, the call is refused before it cuts (batch_device, jb_batch.cpp:62): jb_last_stats stays."""
        if rule.stop and self.stop is None:
            raise ModelError("JB_FILTER_STOP without a stop set")
        fs, fe, fd, stats = self.filtered(batch, mode, hmm, rule)
        base = np.uint64(int(batch.off[0]))
        return (fs - base).astype(np.uint32), (fe - base).astype(np.uint32), fd, np.array(stats, np.uint64)

    def need_vocab(self):
        if self.vocab is None:
            raise ModelError("no vocabulary attached")  # (batch_device: before the cut)

    def postings(self, batch, hmm, doc_base=0):
        """jb_postings_batch with nids = the vocabulary's key count -> (post_off u64[nids + 1], post_doc u32,
        post_tf u32, doc_len u32[ndocs])."""
        self.need_vocab()
        _, d, (tid, tcnt, toff) = self.chain(batch, hmm)
        key = (batch.spec, "postings", bool(hmm), self.version, self.vversion, doc_base)
        if key not in self._cache:
            pd, pt, po = PR.postings(tid, tcnt, toff, nids=len(self.keys), doc_base=doc_base)
            self._cache[key] = (po, pd, pt, np.diff(d.astype(np.int64)).astype(np.uint32))
        return self._cache[key]

    def build_index(self, batches, hmm):
        """The index of one or two batches under the vocabulary as it is now: each batch's postings with doc_base
        advancing, the lists of an id one behind the other.  -> an Index, not attached yet."""
        nids, base = len(self.keys), 0
        ids, docs, tfs, lens = [], [], [], []
        for b in batches:
            po, pd, pt, dl = self.postings(b, hmm, base)
            ids.append(np.repeat(np.arange(nids, dtype=np.int64), np.diff(po.astype(np.int64))))
            docs.append(pd)
            tfs.append(pt)
            lens.append(dl)
            base += b.ndocs
        ids, docs, tfs = np.concatenate(ids), np.concatenate(docs), np.concatenate(tfs)
        order = np.lexsort((docs, ids))  # (by id, then by document: a document is in one batch only)
        po = np.searchsorted(ids[order], np.arange(nids + 1, dtype=np.int64), side="left").astype(np.uint64)
        return Index(po, docs[order].astype(np.uint32), tfs[order].astype(np.uint32), np.concatenate(lens), nids,
                     self.vversion)

    def set_index(self, ix, k1=1.2, b=0.75):
        """jb_index_set: the index with its norms and weights by bm25_ref.  None detaches (jb_index_clear)."""
        if ix is not None:
            avg = BR.avgdl(ix.doc_len)
            ix = ix._replace(k1=k1, b=b, norm=BR.norms(ix.doc_len, k1, b, avg), weight=BR.idf(ix.post_off, len(ix.doc_len)))
        self.index = ix
        self.iversion += 1

    def search(self, batch, hmm, topk):
        """jb_search_batch -> (res_doc u32[nq, topk], res_score u64[nq, topk], res_n u32[nq]) over the attached
        index and the ids of the plain cut under the dictionary and the vocabulary as they are now.  The three
        refusals come before the cut (jb_batch.cpp:697-704): jb_last_stats stays."""
        ix = self.index
        if self.vocab is None or ix is None or ix.nids != len(self.keys):
            raise ModelError("no vocabulary, no index, or an index of another id count")
        ids, d, _ = self.chain(batch, hmm)
        key = (batch.spec, "search", bool(hmm), self.version, self.vversion, topk, self.iversion)
        if key not in self._cache:
            nd = len(ix.doc_len)
            self._cache[key] = BR.search(ix.post_doc, ix.post_tf, ix.post_off, len(ix.post_doc), ix.nids, ix.norm, nd,
                                         ix.weight, ix.nids, ix.k1, ids, max(len(ids), 1), d, topk)
        return self._cache[key]

    def neardup(self, sig, doc_n, B, R, W, min_agree):
        """jb_neardup_sig -> (pair_off u64[ndocs + 1], pair_doc u32, pair_agree u32, stat u64[3])."""
        pd, pa, po, stat = NR.neardup(MR.bands_ref(sig, doc_n, B, R), sig, W, min_agree)
        return po, pd, pa, stat

    def colloc_init(self):
        """jb_colloc_init_device with nuni = the vocabulary's key count: an empty table tied to this vocabulary."""
        self.need_vocab()
        self.cl = dict(table={}, uni=[0] * len(self.keys), nuni=len(self.keys), vversion=self.vversion,
                       tokens=0, known=0, pairs=0)

    def colloc_batch(self, batch, hmm, keep=None, contig=False):
        """jb_colloc_batch: plain-mode ids, after the batch filter when one is set, into the table."""
        self.need_vocab()
        cl = self.cl
        assert cl["vversion"] == self.vversion  # (the driver re-initialises its table on set_vocab)
        s, e, d = self.spans("colloc_batch", batch, "plain", hmm)
        ids = self.ids(batch.buf, s, e, int(batch.off[-1]))
        _, _, tot = CLR.count(ids, d, cl["nuni"], keep, CLR.CONTIG if contig else 0, s, e, uni=cl["uni"], table=cl["table"])
        for k in ("tokens", "known", "pairs"):
            cl[k] += tot[k]

    def colloc_result(self, scorer, min_count, threshold, topn=0):
        """What jb_colloc_read owes: ([(a, b, count, f32 score)] in the rule's order, (tokens, known, pairs, dropped,
        distinct))."""
        cl = self.cl
        rows = CLR.score([(a, b, c) for (a, b), c in cl["table"].items()], cl["uni"], cl["nuni"], cl["known"],
                         SCORERS[scorer], min_count, threshold, topn)
        return rows, (cl["tokens"], cl["known"], cl["pairs"], 0, len(cl["table"]))


# ---- the op generator ---------------------------------------------------------------------------------------
def gen_ops2(seed, nsteps):
    """gen_ops over OPS2: the same deck with three of each of the six new kinds in it:
    ("join_batch", mode, hmm, spec, sep, term)           sep, term of join_ref.SEPS
    ("join", sep, term)                                  jb_join_device on the last device cut's spans
    ("charspans_batch", mode, hmm, spec, unit, reuse)    unit of UNITS; reuse: into the previous call's span arrays
    ("charspans", unit, inplace)                         jb_charspans_device on the last device cut's spans
    ("wc_batch", mode, hmm, spec), ("wc_read",)          one table per sequence
    The six *_batch kinds alternate together between a batch over 4,096 bytes and one under."""
    return gen_ops(seed, nsteps, OPS2)


def spec_at(op):
    """The batch specification of a cut or a *_batch op."""
    return op[4] if op[0] == "cut" else op[3] if op[0] in NEW_BATCH_OPS else op[2]


def gen_ops(seed, nsteps, op_set=OPS, per_kind=3, min_cuts=14):
    """nsteps plain tuples:
    ("cut", mode, hmm, route, spec)           mode of MODES, route of ROUTES, spec for make_batch
    ("add_word", k, freq)                     Model.pick_word(k); three of them
    ("set_vocab", vid)                        Model.vocab_keys(vid)
    ("ids", route)                            the ids of the last cut's spans ("host": jb_spans_ids)
    ("keywords_batch", hmm, spec, topk), ("df_batch", hmm, spec), ("textrank_batch", hmm, spec, span, iters, topk)
    ("last_stats",)
    A "grow" batch is larger than any batch before it in the sequence; a cut may repeat the batch of an
    earlier device cut."""
    rng = random.Random(seed)
    ops, dev_specs = [], []
    top = 0  # an upper bound of the bytes of every batch so far
    nadd = nvid = 0
    doc0 = 100 * (seed % 97)

    def spec_of(cls):
        nonlocal top, doc0
        doc0 += 7
        if cls == "tiny":
            sp, hi = (cls, doc0, rng.randint(1, 8)), SMALL_MAX
        elif cls == "small":
            b = rng.randint(34 << 10, 60 << 10)  # (a document is at most 28 KiB: at least 6 KiB stay)
            sp, hi = (cls, doc0, b), b
        elif cls == "large":
            b = rng.randint(100 << 10, 160 << 10)
            sp, hi = (cls, doc0, b), b
        elif cls == "grow":
            lo = max(top, 64 << 10) + (30 << 10)  # (the trim drops less than one document)
            if lo + (8 << 10) > MAX_BYTES:
                return spec_of("small")
            b = rng.randint(lo, min(lo + (60 << 10), MAX_BYTES))
            sp, hi = (cls, doc0, b), b
        elif cls == "manydocs":
            n = rng.randint(1100, 1600)
            sp, hi = (cls, doc0, n), 8 * n
        elif cls == "empty":
            sp, hi = (cls, 0, rng.randint(1, 7)), 0
        else:
            b = rng.randint(8 << 10, 30 << 10)
            sp, hi = ("offset", doc0, b), b
        top = max(top, hi)
        return sp

    # The deck: three of every kind but "cut", cuts for the rest, shuffled; the cuts' classes and the *_batch
    # calls' sizes come from decks of their own, so that every class and both orders of size occur.
    kinds = [k for k in op_set if k != "cut"] * per_kind
    assert nsteps >= len(kinds) + min_cuts >= len(kinds) + 2 * len(CLASSES)
    kinds += ["cut"] * (nsteps - len(kinds))
    rng.shuffle(kinds)
    ncut = kinds.count("cut")
    cut_cls = list(CLASSES) * 2 + rng.choices(CLASSES, (4, 3, 1, 1, 1, 2), k=ncut - 2 * len(CLASSES))
    rng.shuffle(cut_cls)
    big = rng.random() < 0.5  # the *_batch calls alternate between a batch over 4,096 bytes and one under
    forced = None  # after one add_word: a tiny plain host cut, then the other two modes
    if op_set is not OPS:  # (decks of the new kinds' flags; the first set draws nothing here)
        reuse, inplace = [False, True, True], [True, True, False]
        rng.shuffle(reuse)
        rng.shuffle(inplace)
    for kind in kinds:
        if kind == "add_word":
            ops.append((kind, nadd, (10_000_000, 0, 777)[nadd % 3]))
            if nadd == seed % 3:
                forced = [("plain", "host", "tiny"), ("search", None, None), ("full", None, None)]
                rng.shuffle(forced)
            nadd += 1
        elif kind == "cut":
            mode, hmm, route, cls = rng.choice(MODES), rng.random() < 0.5, rng.choice(ROUTES), cut_cls.pop()
            if forced:
                fm, fr, fc = forced.pop()
                mode, route, cls = fm, fr or route, fc or cls
            after_grow = any(op[0] == "cut" for op in ops) and [op for op in ops if op[0] == "cut"][-1][4][0] == "grow"
            if dev_specs and not (forced is not None and mode == "plain" and route == "host") and \
                    rng.random() < (0.8 if after_grow else 0.15):
                sp, route = rng.choice(dev_specs), rng.choice(ROUTES[1:])
            else:
                sp = spec_of(cls)
            if route != "host" and sp not in dev_specs and sp[0] != "grow":
                dev_specs.append(sp)
            ops.append((kind, mode, hmm and mode != "full", route, sp))
        elif kind in ALL_BATCH_OPS:
            sp = spec_of(rng.choice(("small", "large", "large", "offset")) if big else rng.choice(("tiny", "tiny", "empty")))
            big = not big
            hmm = rng.random() < 0.5
            if kind == "keywords_batch":
                ops.append((kind, hmm, sp, rng.choice((1, 5, 20))))
            elif kind == "df_batch":
                ops.append((kind, hmm, sp))
            elif kind == "textrank_batch":
                ops.append((kind, hmm, sp, rng.choice((2, 5)), rng.choice((3, 10)), rng.choice((5, 20))))
            else:
                mode = rng.choice(MODES)
                hmm = hmm and mode != "full"
                if kind == "join_batch":
                    ops.append((kind, mode, hmm, sp, rng.choice(JR.SEPS), rng.choice(JR.SEPS)))
                elif kind == "charspans_batch":
                    ops.append((kind, mode, hmm, sp, rng.choice(sorted(UNITS)), reuse.pop()))
                else:
                    ops.append((kind, mode, hmm, sp))
        elif kind == "join":
            ops.append((kind, rng.choice(JR.SEPS), rng.choice(JR.SEPS)))
        elif kind == "charspans":
            ops.append((kind, rng.choice(sorted(UNITS)), inplace.pop()))  # (the decks hold three: per_kind <= 3)
        elif kind == "ids":
            ops.append((kind, rng.choice(("host", "device"))))
        elif kind == "set_vocab":
            nvid += 1
            ops.append((kind, nvid))
        else:
            ops.append((kind,))
    return ops


def _large(cls):
    return cls in ("small", "large", "grow", "offset", "manydocs")


# ---- the third op set: MinHash, the caller's filter, postings, search, near-duplicates and collocations ----------
NEWEST_BATCH_OPS = ("minhash_batch", "filter_batch", "postings_batch", "search_batch", "colloc_batch")
ALL_BATCH_OPS3 = ALL_BATCH_OPS + NEWEST_BATCH_OPS
OPS3 = OPS2 + NEWEST_BATCH_OPS + ("colloc_read", "neardup", "set_stop", "set_filter", "clear_filter", "build_index",
                                  "clear_index")
FILTERED_OPS = tuple(k for k in ALL_BATCH_OPS3 if FILTERED[k])
FULL_OPS = ("minhash_batch", "wc_batch", "join_batch")  # the kinds that take a mode and honour it in the front's regrow
HANDOVER_OPS = ("postings_batch", "search_batch", "colloc_batch")  # the kinds that cut kArTokens up as ids and terms
QUERIES_LARGE = (380, 560)  # sentences of a large query batch, and
DUPS_LARGE = (40, 56)  # documents of a dups batch of gen_ops3: 24 to 48 KiB each (test_ctx_model.py)
NBASE3 = 25  # gen_ops3's share of older ops: one of every kind of OPS2 and twelve cuts
NSTEPS3 = 95  # gen_ops3 makes exactly this many: NBASE3 older ops and the 70 of its five runs
SEEDS3 = (7, 11, 17)  # gen_ops3(seed, NSTEPS3); held to covered3() and to the conditions on their inputs by test_ctx_model.py


def spec_at3(op):
    """The batch specification of a cut or a *_batch op of OPS3."""
    return op[3] if op[0] in ("minhash_batch", "filter_batch") else op[2] if op[0] in NEWEST_BATCH_OPS else spec_at(op)


def large3(spec):
    return _large(spec[0]) or spec[0] == "dups" or (spec[0] == "queries" and spec[2] > 8)


def gen_ops3(seed, nsteps):
    """A sequence over OPS3: gen_ops2's kinds, once each, among twelve cuts (gen_ops with per_kind 1), merged in a
    seeded order with five runs of the newest kinds, each run in its own order:
    ("minhash_batch", mode, hmm, spec, n, K), ("filter_batch", mode, hmm, spec, rule), ("postings_batch", hmm, spec),
    ("search_batch", hmm, spec, topk), ("colloc_batch", hmm, spec, keep, contig), ("colloc_read", scorer),
    ("neardup", B, R, min_agree)    on the signatures of the last minhash_batch, as Driver keeps them
    ("set_stop", sid)               Model.stop_keys(sid)
    ("set_filter", rule), ("clear_filter",)    rule: a number of RULES
    ("build_index", spec, spec or None, k1, b), ("clear_index",)
    The runs: two chains that alternate a newest kind with an older *_batch kind and a batch over 4,096 bytes with one
    under; a full-mode call before each of HANDOVER_OPS; the batch filter's life; the index's and the collocation
    table's around an add_word and a set_vocab; two near-duplicate joins.  Where the older ops fall between them
    is the seed's: coverage3 says what a sequence still contains."""
    assert nsteps > NBASE3
    base = gen_ops(seed, NBASE3, OPS2, per_kind=1, min_cuts=12)
    rng = random.Random(seed ^ 0x5EED3)
    doc0 = [20_000 + 100 * (seed % 89)]

    def spec_of(big, kind=None):
        doc0[0] += 7
        if kind == "search_batch":
            return ("queries", doc0[0], rng.randint(QUERIES_LARGE[0], QUERIES_LARGE[1]) if big else rng.randint(2, 6))
        if big:  # (24 to 48 KiB: sentences, of which the trim drops less than one and `offset` the first three)
            return ("offset", doc0[0], rng.randint(26 << 10, 48 << 10))
        return rng.choice((("tiny", doc0[0], rng.randint(1, 8)), ("tiny", doc0[0], rng.randint(1, 8)), ("empty", 0, rng.randint(1, 7))))

    def op(kind, big, mode=None, spec=None, rules=(0, 1)):
        sp = spec or spec_of(big, kind)
        mode = mode or rng.choice(MODES)
        hmm = rng.random() < 0.5
        mh = hmm and mode != "full"
        if kind == "keywords_batch":
            return (kind, hmm, sp, rng.choice((1, 5, 20)))
        if kind == "df_batch":
            return (kind, hmm, sp)
        if kind == "textrank_batch":
            return (kind, hmm, sp, rng.choice((2, 5)), rng.choice((3, 10)), rng.choice((5, 20)))
        if kind == "join_batch":
            return (kind, mode, mh, sp, rng.choice(JR.SEPS), rng.choice(JR.SEPS))
        if kind == "charspans_batch":
            return (kind, mode, mh, sp, rng.choice(sorted(UNITS)), False)
        if kind == "wc_batch":
            return (kind, mode, mh, sp)
        if kind == "minhash_batch":
            return (kind, mode, mh, sp, rng.choice((1, 3, 5)), rng.choice((16, 64, 128)))
        if kind == "filter_batch":
            return (kind, mode, mh, sp, rng.choice(rules))
        if kind == "postings_batch":
            return (kind, hmm, sp)
        if kind == "search_batch":
            return (kind, hmm, sp, rng.choice((1, 10, 64)))
        if kind == "colloc_batch":
            return (kind, hmm, sp, rng.random() < 0.5, rng.random() < 0.5)
        raise ValueError(kind)

    def chain(big):
        new, old = list(NEWEST_BATCH_OPS) + [rng.choice(NEWEST_BATCH_OPS)], list(ALL_BATCH_OPS)
        rng.shuffle(new)
        rng.shuffle(old)
        out = []
        for a, b in zip(new, old):
            out += [op(a, big), op(b, not big)]
        return out

    def shuffled(kinds):
        kinds = list(kinds)
        rng.shuffle(kinds)
        return kinds

    runs = [chain(True), chain(False)]
    runs.append([o for after in shuffled(HANDOVER_OPS) for o in (op(rng.choice(FULL_OPS), rng.random() < 0.5, "full"),
                                                                 op(after, rng.random() < 0.5))])
    stop_rule, big = rng.choice((2, 3)), rng.random() < 0.5
    life = [("set_stop", 0), ("set_filter", rng.choice((0, 1)))]
    for k in shuffled(ALL_BATCH_OPS3):
        big = not big
        life.append(op(k, big))
    life += [("set_filter", stop_rule), op(rng.choice(FILTERED_OPS), True), ("set_stop", 1), op(rng.choice(FILTERED_OPS), True),
             ("clear_filter",)]
    life += [op(k, rng.random() < 0.5) for k in shuffled(FILTERED_OPS)]
    runs.append(life)
    runs.append([("build_index", spec_of(True), rng.choice((None, spec_of(True))), 1.2, 0.75), op("search_batch", False),
                 op("colloc_batch", True), ("add_word", 5, 10_000_000), op("search_batch", True), op("colloc_batch", False),
                 ("colloc_read", rng.choice(sorted(SCORERS))), ("set_vocab", 7), op("search_batch", False),
                 ("clear_index",), op("search_batch", False),
                 ("build_index", spec_of(True), None, rng.choice((1.2, 2.0)), rng.choice((0.75, 0.0))),
                 op("search_batch", False), ("colloc_read", "count")])
    doc0[0] += 7
    agree = lambda K: rng.choice((K // 2, (4 * K + 2) // 5))  # noqa: E731
    runs.append([op("minhash_batch", True, "plain", ("dups", doc0[0], rng.randint(DUPS_LARGE[0], DUPS_LARGE[1]))), ("neardup", 32, 4, agree(128)),
                 op("minhash_batch", False, None, spec_of(False)), ("neardup", 8, 2, agree(16))])
    runs[-1][0] = runs[-1][0][:4] + (5, 128)
    runs[-1][2] = runs[-1][2][:4] + (3, 16)
    rng.shuffle(runs)
    new = [o for r in runs for o in r]
    assert len(base) + len(new) == nsteps, (len(base), len(new))
    # the merge: every order of the two lists that keeps each one's own is as likely as another
    take = [True] * len(base) + [False] * len(new)
    rng.shuffle(take)
    a, b = iter(base), iter(new)
    return [next(a) if t else next(b) for t in take]


def coverage3(ops):
    """What a sequence over OPS3 contains: {name: count or truth}, every value truthy for a seed to be used."""
    out = {"kinds": {k: sum(1 for op in ops if op[0] == k) for k in OPS3}}
    batch = [op for op in ops if op[0] in ALL_BATCH_OPS3]
    # sizes and neighbours among the *_batch calls, which share kArText and kArTokens
    for k in NEWEST_BATCH_OPS:
        out[k + ":large_then_tiny"] = out[k + ":tiny_then_large"] = out[k + ":after_older"] = False
    for k in ALL_BATCH_OPS:
        out[k + ":after_newest"] = False
    for k in HANDOVER_OPS:
        out["full_mode_then:" + k] = False
    for p, op in zip(batch, batch[1:]):
        k, big, was = op[0], large3(spec_at3(op)), large3(spec_at3(p))
        if k in NEWEST_BATCH_OPS:
            if big != was:
                out[k + (":tiny_then_large" if big else ":large_then_tiny")] = True
            if p[0] in ALL_BATCH_OPS:
                out[k + ":after_older"] = True
        elif p[0] in NEWEST_BATCH_OPS:
            out[k + ":after_newest"] = True
        if k in HANDOVER_OPS and p[0] in FULL_OPS and p[1] == "full":
            out["full_mode_then:" + k] = True
    # the batch filter: every kind while one is set, the filtered kinds again after the clear, a rule replaced,
    # and under a stop-using rule a set_stop of other keys between two filtered calls
    during, after, flt, cleared, sid, stop_state = set(), set(), None, False, None, 0
    out["filter_replaced"] = out["stop_set_replaced_under_a_rule"] = False
    for op in ops:
        k = op[0]
        if k == "set_filter":
            out["filter_replaced"] |= flt is not None
            flt, stop_state = op[1], 0
        elif k == "clear_filter":
            cleared, flt, stop_state = cleared or flt is not None, None, 0
        elif k == "set_stop":
            if stop_state == 1 and op[1] != sid:
                stop_state = 2
            sid = op[1]
        elif k in ALL_BATCH_OPS3:
            if flt is not None:
                during.add(k)
                if FILTERED[k] and RULES[flt].stop and sid is not None:
                    out["stop_set_replaced_under_a_rule"] |= stop_state == 2
                    stop_state = max(stop_state, 1)
            elif cleared:
                after.add(k)
    out["every_kind_under_a_filter"] = during >= set(ALL_BATCH_OPS3)
    out["filtered_kinds_after_the_clear"] = after >= set(FILTERED_OPS)
    # the index: a search on each side of an add_word with the index kept; a set_vocab under an attached index, a
    # search (refused), a build_index, a search (answered)
    out["search_around_add"] = out["vocab_replaced_under_an_index"] = False
    valid, around, replaced = False, 0, 0
    for op in ops:
        k = op[0]
        if k == "build_index":
            valid, around, replaced = True, 0, 2 if replaced == 2 else 0
        elif k == "clear_index":
            valid, around, replaced = False, 0, 2 if replaced == 2 else 0
        elif k == "set_vocab":
            replaced, around, valid = 1 if valid else 0, 0, False
        elif k == "add_word" and around == 1:
            around = 2
        elif k == "search_batch":
            if valid and around in (0, 2):
                out["search_around_add"] |= around == 2
                around = 1 if around == 0 else around
            if replaced == 1 and not valid:
                replaced = 2
            elif replaced == 2 and valid:
                out["vocab_replaced_under_an_index"] = True
    # the collocation table on both sides of an add_word, read after both (a set_vocab starts a new table)
    out["colloc_around_add"] = False
    state = 0
    for op in ops:
        if op[0] == "colloc_batch" and state in (0, 2):
            state += 1
        elif op[0] == "add_word" and state == 1:
            state = 2
        elif op[0] == "set_vocab":
            state = 0
        elif op[0] == "colloc_read" and state == 3:
            out["colloc_around_add"] = True
    # a near-duplicate join on the signatures of a dups batch, and one on a batch without planted copies
    out["neardup_with_copies"] = out["neardup_without"] = False
    last = None
    for op in ops:
        if op[0] == "minhash_batch":
            last = op[3][0] == "dups"
        elif op[0] == "neardup" and last is not None:
            out["neardup_with_copies" if last else "neardup_without"] = True
    return out


def covered3(ops):
    c = coverage3(ops)
    return all(v >= 1 for v in c["kinds"].values()) and all(v for k, v in c.items() if k != "kinds")


def coverage(ops):
    """What a sequence contains: {name: count or truth}.  Every value must be truthy (and the counts at
    least as large as test_ctx_model.py asks) for a seed to be used."""
    kinds = {k: sum(1 for op in ops if op[0] == k) for k in OPS}
    classes = {c: 0 for c in CLASSES}
    for op in ops:
        if op[0] == "cut":
            classes[op[4][0]] += 1
        elif op[0] in BATCH_OPS and op[2][0] in classes:
            classes[op[2][0]] += 1
    out = {"kinds": kinds, "classes": classes}
    # an add_word followed by each of the three modes before the next add_word
    out["add_then_every_mode"] = False
    out["tiny_plain_host_after_add"] = False
    seen, after = set(), False
    for op in ops:
        if op[0] == "add_word":
            seen, after = set(), True
        elif op[0] == "cut" and after:
            seen.add(op[1])
            if op[1] == "plain" and op[3] == "host" and op[4][0] == "tiny":
                out["tiny_plain_host_after_add"] = True
            if len(seen) == 3:
                out["add_then_every_mode"] = True
    # a grow followed by a repeat of an earlier device batch
    out["grow_then_repeat"] = False
    dev, before, grown = set(), set(), set()
    for op in ops:
        if op[0] != "cut":
            continue
        sp, route = op[4], op[3]
        if route != "host" and sp in before:
            out["grow_then_repeat"] = True
        if sp[0] == "grow" and sp not in grown:  # (its first cut is the one that grows the workspace)
            grown.add(sp)
            before = set(dev)
        if route != "host":
            dev.add(sp)
    # each *_batch call on a tiny batch right after a large one, and on a large one right after a tiny one
    # (among the *_batch calls, which share the arenas)
    prev = None
    for k in BATCH_OPS:
        out[k + ":large_then_tiny"] = out[k + ":tiny_then_large"] = False
    for op in ops:
        if op[0] not in BATCH_OPS:
            continue
        big = _large(op[2][0])
        if prev is not None and prev != big:
            out[op[0] + (":tiny_then_large" if big else ":large_then_tiny")] = True
        prev = big
    return out


def dev_state(ops):
    """Per op, what Driver holds as the last device cut when the op runs: None, or the route of that cut.
    A device cut stays the last one until another call cuts (a host cut, a *_batch call) or AddWord
    replaces the image; ids, join, charspans, set_vocab, wc_read and last_stats leave it."""
    out, cur = [], None
    for op in ops:
        out.append(cur)
        if op[0] == "cut":
            cur = op[3] if op[3] != "host" else None
        elif op[0] in ALL_BATCH_OPS or op[0] == "add_word":
            cur = None
    return out


def coverage2(ops):
    """coverage() of a sequence over OPS2, with the conditions of the new kinds."""
    old = coverage([op for op in ops if op[0] in OPS])
    out = {k: v for k, v in old.items() if ":" not in k}
    out["kinds"] = {k: sum(1 for op in ops if op[0] == k) for k in OPS2}
    for op in ops:
        if op[0] in NEW_BATCH_OPS and op[3][0] in out["classes"]:
            out["classes"][op[3][0]] += 1
    # the six *_batch kinds share the arenas: each on both transitions of size among all of them, each new
    # kind directly after an older one and each older one directly after a new one
    for k in ALL_BATCH_OPS:
        out[k + ":large_then_tiny"] = out[k + ":tiny_then_large"] = False
        out[k + (":after_old" if k in NEW_BATCH_OPS else ":after_new")] = False
    prev = None
    for op in ops:
        if op[0] not in ALL_BATCH_OPS:
            continue
        big, new = _large(spec_at(op)[0]), op[0] in NEW_BATCH_OPS
        if prev is not None:
            if prev[0] != big:
                out[op[0] + (":tiny_then_large" if big else ":large_then_tiny")] = True
            if prev[1] != new:
                out[op[0] + (":after_old" if new else ":after_new")] = True
        prev = (big, new)
    # a wc_batch on each side of an add_word, with a wc_read after both
    out["wc_around_add"] = False
    state = 0  # 1: a wc_batch, 2: then an add_word, 3: then a wc_batch
    for op in ops:
        if op[0] == "wc_batch" and state in (0, 2):
            state += 1
        elif op[0] == "add_word" and state == 1:
            state = 2
        elif op[0] == "wc_read" and state == 3:
            out["wc_around_add"] = True
    # an in-place charspans on the ctx-owned arrays of a device cut (Driver repeats that cut afterwards)
    out["charspans_inplace_on_ctx_arrays"] = any(
        op[0] == "charspans" and op[2] and st == "device" for op, st in zip(ops, dev_state(ops)))
    # a charspans_batch with reuse whose span arrays are too small: those of a call on at most 4,096 bytes
    # (at most 4,096 entries, grown or not), handed to a large batch (over 64 KiB: more tokens than that)
    out["charspans_reuse_too_small"] = False
    cap_small = False  # whether the kept arrays are known to have at most 4,096 entries
    for op in ops:
        if op[0] != "charspans_batch":
            continue
        small = op[3][0] in ("tiny", "empty") and op[1] != "full"
        if not op[5]:
            cap_small = small
        elif cap_small and op[3][0] == "large":
            out["charspans_reuse_too_small"], cap_small = True, False
        else:
            cap_small = cap_small and small
    return out


def covered2(ops, min_kind=3, min_class=2):
    c = coverage2(ops)
    return (all(v >= min_kind for v in c["kinds"].values()) and all(v >= min_class for v in c["classes"].values()) and
            all(v for k, v in c.items() if k not in ("kinds", "classes")))


def covered(ops, min_kind=3, min_class=2):
    c = coverage(ops)
    return (all(v >= min_kind for v in c["kinds"].values()) and all(v >= min_class for v in c["classes"].values()) and
            all(v for k, v in c.items() if k not in ("kinds", "classes")))
