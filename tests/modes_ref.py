"""Large expected outputs for the search-, full- and id-mode tests from small ones: a helper, not a test.

Documents are cut independently, so a batch that repeats a base list of documents r times has the
base's expected spans shifted by the base's byte length, and its doc_tok shifted by the base's span
count (replicate; test_modes_ref.py checks it against the references computed directly).  A Part is a
base list of documents with its references (oracle.cut_batch, search_ref, full_ref), computed once;
a Batch is Parts, each repeated, laid end to end.  Nothing here calls the library under test.
"""
import numpy as np

import full_ref as F
import search_ref as R


def replicate(want, base_bytes, r):
    """(starts, ends, doc_tok) of a base of base_bytes bytes -> those of the base repeated r times."""
    s, e, d = (np.asarray(x, np.uint64) for x in want)
    n = len(s)
    assert int(d[-1]) == n
    sh = (np.arange(r, dtype=np.uint64) * np.uint64(base_bytes))[:, None]
    sn = (np.arange(r, dtype=np.uint64) * np.uint64(n))[:, None]
    return ((s[None, :] + sh).ravel(), (e[None, :] + sh).ravel(),
            np.concatenate([(d[None, :-1] + sn).ravel(), np.array([r * n], np.uint64)]))


def replicate_ids(ids, r):
    """The ids of a base's spans -> those of the base repeated r times (a token's id is its bytes')."""
    return np.tile(np.asarray(ids, np.uint32), r)


def join(parts):
    """[((starts, ends, doc_tok), nbytes)] of lists of documents -> those of the lists laid end to end."""
    ss, es, ds = [], [], []
    b = n = 0
    for (s, e, d), nb in parts:
        ss.append(np.asarray(s, np.uint64) + np.uint64(b))
        es.append(np.asarray(e, np.uint64) + np.uint64(b))
        ds.append(np.asarray(d, np.uint64)[:-1] + np.uint64(n))
        b += int(nb)
        n += len(s)
    ds.append(np.array([n], np.uint64))
    return np.concatenate(ss), np.concatenate(es), np.concatenate(ds)


class Part:
    """Documents (texts, or (buf, doc_off) with doc_off[0] == 0) and their expected outputs, cached."""

    def __init__(self, o, texts=None, buf=None, off=None, grams=None, blocks=None):
        if texts is not None:
            buf, off = R.batch_of(texts)
        self.o = o
        self.off = np.asarray(off, np.uint64)
        assert int(self.off[0]) == 0
        self.nbytes = int(self.off[-1])
        self.buf = np.ascontiguousarray(np.asarray(buf, np.uint8)[:self.nbytes])
        self.ndocs = len(self.off) - 1
        self.grams = grams
        self.blocks = blocks
        self._c = {}

    def _padded(self):
        return np.concatenate([self.buf, np.zeros(64, np.uint8)])

    def want(self, mode, hmm=False):
        """mode: 'cut', 'search' or 'full' (full mode ignores hmm)."""
        key = (mode, bool(hmm) and mode != "full")
        if key not in self._c:
            buf = self._padded()
            if mode == "full":
                self._c[key] = F.expected(self.o, buf, self.off, self.blocks)
            else:
                if ("cut", key[1]) not in self._c:
                    self._c[("cut", key[1])] = self.o.cut_batch(buf, self.off, key[1], nthreads=8)
                if mode == "search":
                    self._c[key] = R.expand(self.o, buf, *self._c[("cut", key[1])], self.grams)
        return self._c[key]

    def ntok(self, hmm=False):
        return len(self.want("cut", hmm)[0])

    def han_tokens(self, hmm=False):
        """Plain tokens that start with a Han rune."""
        if ("han", bool(hmm)) not in self._c:
            self._c[("han", bool(hmm))] = self._han_tokens(hmm)
        return self._c[("han", bool(hmm))]

    def _han_tokens(self, hmm):
        s = self.want("cut", hmm)[0].astype(np.int64)
        lead = self.buf[s]
        n = 0
        data = self.buf.tobytes()
        for p in s[lead >= 0xE0].tolist():
            try:
                n += R.is_han(ord(data[p:p + (4 if data[p] >= 0xF0 else 3)].decode("utf-8")))
            except (UnicodeDecodeError, TypeError):
                pass
        return n


def filler_part(o, units):
    """One document of `units` times "x ": `units` plain tokens ("x"; cutNonZh drops the space), each
    copied by both modes."""
    p = Part(o, texts=["x " * units])
    assert p.ntok(False) == units == p.ntok(True) and len(p.want("full")[0]) == units
    return p


class Batch:
    """[(Part, repeats)] laid end to end: the text, doc_off and every mode's expected output."""

    def __init__(self, items):
        self.items = [(p, r) for p, r in items if r > 0]
        self.nbytes = sum(p.nbytes * r for p, r in self.items)
        self.buf = np.concatenate([np.tile(p.buf, r) for p, r in self.items] + [np.zeros(64, np.uint8)])
        offs, b = [], 0
        for p, r in self.items:
            sh = (np.arange(r, dtype=np.uint64) * np.uint64(p.nbytes))[:, None]
            offs.append((p.off[None, :-1] + sh).ravel() + np.uint64(b))
            b += p.nbytes * r
        self.off = np.concatenate(offs + [np.array([b], np.uint64)])
        self.ndocs = len(self.off) - 1

    def want(self, mode, hmm=False):
        return join([(replicate(p.want(mode, hmm), p.nbytes, r), p.nbytes * r) for p, r in self.items])

    def ntok(self, hmm=False):
        return sum(p.ntok(hmm) * r for p, r in self.items)

    def han_tokens(self, hmm=False):
        return sum(p.han_tokens(hmm) * r for p, r in self.items)


def prefix_docs(part, ndocs):
    """The first ndocs documents of a Part as a Part of its own (references computed afresh)."""
    return Part(part.o, buf=part.buf, off=part.off[:ndocs + 1], grams=part.grams, blocks=part.blocks)


def exact_batch(o, corpus, target, hmm, share, fill_doc=4096):
    """A Batch of exactly `target` plain tokens (hmm as given): "x " filler first, then `corpus` (a Part)
    repeated to about `share` of the tokens; a corpus larger than that is cut down to its first documents."""
    per = corpus.ntok(hmm)
    wantc = int(target * share)
    if per > wantc:
        d = corpus.want("cut", hmm)[2].astype(np.int64)
        nd = int(np.searchsorted(d, wantc, side="right")) - 1
        if nd >= 1:
            corpus = prefix_docs(corpus, nd)
        else:  # (the first document alone is too long: the largest single document that fits the target)
            cnt = np.diff(d)
            j = int(np.argmax(np.where(cnt <= target, cnt, -1)))
            assert 0 < cnt[j] <= target, (target, cnt.tolist())
            a, b = int(corpus.off[j]), int(corpus.off[j + 1])
            corpus = Part(corpus.o, texts=[corpus.buf[a:b].tobytes()], grams=corpus.grams, blocks=corpus.blocks)
        per = corpus.ntok(hmm)
    r = max(1, wantc // per)
    rest = target - r * per
    assert rest >= 0, (target, per, r)
    items = []
    if rest >= fill_doc:
        items.append((filler_part(o, fill_doc), rest // fill_doc))
    if rest % fill_doc:
        items.append((filler_part(o, rest % fill_doc), 1))
    items.append((corpus, r))
    b = Batch(items)
    assert b.ntok(hmm) == target
    return b


def pieces(doc_off, piece_bytes):
    """plan_pieces' greedy rule (jb_plan.cpp): pieces of whole documents of at most piece_bytes bytes (a longer document
    is a piece of its own) -> [(first document, one past the last)]."""
    off = [int(x) for x in doc_off]
    out, a, n = [], 0, len(off) - 1
    while a < n:
        b = a + 1
        while b < n and off[b + 1] - off[a] <= piece_bytes:
            b += 1
        out.append((a, b))
        a = b
    return out


def long_blocks_recipe():
    """The dictionary and texts of test_long_blocks_many (test_gpu_parity.py), restated: several long blocks
    in one batch, words of 65 to 200 runes whose every prefix is a key, and a rune that starts up to 20 words.
    Returns (dictionary text, texts)."""
    import random
    rng = random.Random(5)
    pool = [chr(c) for c in range(0x4E00, 0x4E00 + 300)]
    lines = [f"{'丁' * k} {10 + k}" for k in range(1, 21)]
    longw = []
    for _ in range(30):
        w = "".join(rng.choice(pool) for _ in range(rng.randint(65, 200)))
        longw.append(w)
        lines += [f"{w[:k]} {rng.randint(1, 3) if k < len(w) else 10 ** 6}" for k in range(1, len(w) + 1)]
    a = "".join(rng.choice(longw) for _ in range(40))
    b = "丁" * 3000
    c = "".join(rng.choice([rng.choice(longw), "丁" * rng.randint(1, 30),
                            "".join(rng.choice(pool) for _ in range(rng.randint(1, 40)))]) for _ in range(300))
    texts = [a + "x" + c, b, c + "。" + a, "短文本，中文", b[:2800] + a[:3000], "丁乙" * 1500]
    return "\n".join(lines) + "\n", texts
