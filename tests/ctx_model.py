"""A shadow model of one long-lived tokenizer, and a generator of call sequences: a helper, not a test.

Model answers every call of a sequence from the references the suite already trusts (Oracle.cut_batch,
search_ref, full_ref, vocab_ref, terms_ref, df_ref, textrank_ref, join_ref, charspans_ref, wc_ref) and keeps
what a jb_ctx keeps between calls: the dictionary (an Oracle that add_word changes), the vocabulary (a Python
dict) with its keep mask and weights, and the token count jb_last_stats owes the caller; and what a caller
keeps beside it, the word-count table (a Counter that only grows).  It never calls the library.

gen_ops(seed, nsteps) draws a sequence of plain tuples (see OPS); make_batch turns a tuple's batch
specification into text.  coverage(ops) says which of the transitions between calls a sequence contains;
test_ctx_model.py pins the seeds that test_gpu_sequences.py runs to the ones that contain them all.
gen_ops2 / coverage2 / SEEDS2 are the same over OPS2, which adds the calls of joined text, character offsets
and word counts; gen_ops' own output is pinned by a digest in test_ctx_model.py.
"""
import random
import re

from collections import Counter

import numpy as np

import charspans_ref as CR
import df_ref as DR
import full_ref as F
import join_ref as JR
import oracle as O
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


def make_batch(s, spec):
    """spec = (class, a, b) -> Batch, from the synthetic generator s (synth.Synth):
    tiny      b sentences from document a: at most 4,096 bytes, k_small's route for a plain host call
    small     documents from a, at most b bytes (6 to 60 KiB)
    grow      documents from a, at most b bytes (up to 400 KiB)
    large     as grow: the large batch of a *_batch call
    manydocs  b documents of one or two runes, cut from the sentences at a
    empty     b empty documents
    offset    as small, from sentences, and starting at document 3 of its buffer"""
    cls, a, b = spec
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
        s, e, d = self.cut(batch, mode, hmm)
        key = (batch.spec, "join", mode, hmm, self.version, sep, term)
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
        s, e, _ = self.cut(batch, mode, hmm)
        self.wc_add(batch.buf[:int(batch.off[-1])], s, e)

    def wc_result(self):
        """What jb_wc_read owes the caller: a wc_ref.Ref of the whole table, in the rule's order."""
        items = W.order(self.wc)
        return W.Ref([k for k, _ in items], [v for _, v in items], self.wc_bad, self.wc_long, self.wc_tokens, dict(self.wc))

    def wc_size(self):
        """(distinct keys, their bytes together): what the table has to hold."""
        return len(self.wc), sum(len(k) for k in self.wc)


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


def gen_ops(seed, nsteps, op_set=OPS):
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
    kinds = [k for k in op_set if k != "cut"] * 3
    assert nsteps >= len(kinds) + 14
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
            ops.append((kind, rng.choice(sorted(UNITS)), inplace.pop()))
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
