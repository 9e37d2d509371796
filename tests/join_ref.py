"""The joined-text rule of jiebahip.h (jb_join, jb_join_device) stated independently in Python, from spans:
per document sep.join(keys) + term.  Used by every join test; the seeded span lists the host and the GPU
tests share live here too."""
import numpy as np

REPL = b"\xef\xbf\xbd"


def key(text, nbytes, s, e):
    """The key of span [s, e): its bytes, U+FFFD for one invalid byte, nothing for a malformed span."""
    if s >= e or e > nbytes:
        return b""
    if e - s == 1 and text[s] >= 0x80:
        return REPL
    return bytes(text[s:e])


def join_ref(text, starts, ends, doc_tok, sep=b" ", term=b"\n", ntok=None, cap=None, nbytes=None):
    """(output bytes, out_doc_off as a list of ndocs + 1 ints) of the complete output."""
    text = bytes(text)
    nbytes = len(text) if nbytes is None else nbytes
    cap = len(starts) if cap is None else cap
    ntok = len(starts) if ntok is None else ntok
    n = min(ntok, cap)
    s, e = [int(x) for x in starts[:n]], [int(x) for x in ends[:n]]
    docs, off = [], [0]
    for d in range(len(doc_tok) - 1):
        a, b = min(int(doc_tok[d]), n), min(int(doc_tok[d + 1]), n)
        docs.append(sep.join(key(text, nbytes, s[k], e[k]) for k in range(a, b)) + term)
        off.append(off[-1] + len(docs[-1]))
    return b"".join(docs), off


class Case:
    """One input of the join calls; .want() is join_ref's answer."""

    def __init__(self, name, text, starts, ends, doc_tok, sep=b" ", term=b"\n", ntok=None, cap=None, nbytes=None):
        self.name, self.text = name, bytes(text)
        self.starts, self.ends = np.asarray(starts, np.uint32), np.asarray(ends, np.uint32)
        self.doc_tok = np.asarray(doc_tok, np.uint64)
        self.sep, self.term = sep, term
        self.ntok = len(self.starts) if ntok is None else ntok
        self.cap = len(self.starts) if cap is None else cap
        self.nbytes = len(self.text) if nbytes is None else nbytes
        self._want = None

    def want(self):
        if self._want is None:
            self._want = join_ref(self.text, self.starts, self.ends, self.doc_tok, self.sep, self.term, self.ntok,
                                  self.cap, self.nbytes)
        return self._want

    def __repr__(self):
        return f"<{self.name}: {len(self.starts)} spans, {len(self.doc_tok) - 1} documents>"


SEPS = [b"", b" ", b"\xe3\x80\x80", b"<-sep8->"]  # 0, 1, 3 and 8 bytes


def from_keys(name, docs, sep=b" ", term=b"\n", lead=b""):
    """A case from documents given as lists of keys (bytes): the text is `lead` and then the keys one after
    the other, so the spans are adjacent and in order."""
    text, s, e, d = bytearray(lead), [], [], [0]
    for doc in docs:
        for k in doc:
            s.append(len(text))
            text += k
            e.append(len(text))
        d.append(len(s))
    return Case(name, text, s, e, d, sep, term)


def random_case(seed, ntokens=None, max_docs=12):
    """A seeded span list over a text with invalid bytes: ordered, overlapping and malformed spans, empty
    documents first, last and in a row, and on some seeds ntok > cap and doc_tok running past ntok."""
    rng = np.random.default_rng(seed)
    nbytes = int(rng.integers(1, 400))
    text = rng.integers(0x20, 0x7F, nbytes).astype(np.uint8)
    bad = rng.random(nbytes) < 0.15
    text[bad] = rng.integers(0x80, 0x100, int(bad.sum())).astype(np.uint8)
    n = int(rng.integers(0, 300)) if ntokens is None else ntokens
    s = rng.integers(0, nbytes, n).astype(np.int64)
    ln = rng.choice([1, 1, 2, 3, 7, 30], n)
    e = np.minimum(s + ln, nbytes)
    kind = rng.random(n)
    e = np.where(kind < 0.05, s, e)                   # empty
    e = np.where((kind >= 0.05) & (kind < 0.08), np.maximum(s - 1, 0), e)  # reversed
    e = np.where((kind >= 0.08) & (kind < 0.11), nbytes + 1 + ln, e)   # past the text
    s = np.where((kind >= 0.11) & (kind < 0.13), 0xFFFFFFF0, s)        # far outside
    ndocs = int(rng.integers(1, max_docs + 1))
    cuts = np.sort(rng.integers(0, n + 1, ndocs - 1)) if ndocs > 1 else np.zeros(0, np.int64)
    if ndocs > 3 and rng.random() < 0.5:
        cuts[:2] = 0      # empty documents first
        cuts[-1] = n      # and last
    doc_tok = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    ntok, cap = n, n
    mode = seed % 4
    if mode == 1 and n:  # full mode's over-long list: the count exceeds the arrays
        cap = int(rng.integers(0, n + 1))
        ntok = n + int(rng.integers(0, 50))
        doc_tok = np.minimum(doc_tok * 2, ntok).astype(np.uint64)
    elif mode == 2 and n:  # doc_tok runs past ntok
        ntok = int(rng.integers(0, n + 1))
    sep = SEPS[int(rng.integers(0, 4))]
    term = [b"", b"\n", b"\r\n!", b"<-term8>"][int(rng.integers(0, 4))]
    c = Case(f"random-{seed}", text.tobytes(), s[:cap] if cap < n else s, e[:cap] if cap < n else e, doc_tok, sep, term,
             ntok=ntok, cap=cap)
    return c


def out_caps(nout):
    return sorted({0, 1, max(nout - 1, 0), nout, nout + 5})
