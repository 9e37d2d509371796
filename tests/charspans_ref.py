"""The character-offset rule of jiebahip.h (jb_charspans, jb_charspans_device) stated independently in Python
over codepoint_cases.runes, the model of Go's utf8.DecodeRune that shares no code with the library.  Used by
every charspans test; the case builders the host and the GPU tests share live here too.  A helper, not a
test."""
import numpy as np

import codepoint_cases as CC

NONE = 0xFFFFFFFF
RUNE, UTF16 = 0, 1
W = 64  # text bytes per bitmap word of the device pass


def units_of(rune, width, unit):
    """A rune start's units: an invalid byte is (U+FFFD, 1) and counts 1."""
    return 2 if unit == UTF16 and width > 1 and rune >= 0x10000 else 1


def doc_positions(doc, unit):
    """pos_d(p) for p in 0..len(doc): the units of the rune starts before p; a p inside a rune counts it."""
    pos, acc = [0] * (len(doc) + 1), 0
    for a, b, r in CC.runes(doc):
        pos[a] = acc
        acc += units_of(r, b - a, unit)
        for p in range(a + 1, b):
            pos[p] = acc
    pos[len(doc)] = acc
    return pos


def charspans_ref(text, doc_off, starts, ends, doc_tok, unit, ntok=None, cap=None):
    """(cstart, cend, doc_units) as lists; cstart / cend have min(ntok, cap) entries."""
    text = bytes(text)
    cap = len(starts) if cap is None else cap
    ntok = len(starts) if ntok is None else ntok
    n = min(ntok, cap)
    off = [int(x) for x in doc_off]
    tok = [int(x) for x in doc_tok]
    cs, ce, units = [NONE] * n, [NONE] * n, []
    for d in range(len(off) - 1):
        so, eo = off[d], off[d + 1]
        pos = doc_positions(text[so:eo], unit)
        units.append(pos[-1])
        for k in range(min(tok[d], n), min(tok[d + 1], n)):
            s, e = int(starts[k]), int(ends[k])
            if so <= s <= e <= eo:
                cs[k], ce[k] = pos[s - so], pos[e - so]
    return cs, ce, units


class Case:
    """One input of the charspans calls; .want(unit) is charspans_ref's answer."""

    def __init__(self, name, text, doc_off, starts, ends, doc_tok, ntok=None, cap=None):
        self.name, self.text = name, bytes(text)
        self.doc_off = np.asarray(doc_off, np.uint64)
        self.starts, self.ends = np.asarray(starts, np.uint32), np.asarray(ends, np.uint32)
        self.doc_tok = np.asarray(doc_tok, np.uint64)
        self.ntok = len(self.starts) if ntok is None else ntok
        self.cap = len(self.starts) if cap is None else cap
        self.nbytes = len(self.text)
        assert int(self.doc_off[-1]) == self.nbytes and len(self.doc_tok) == len(self.doc_off)
        self._want = {}

    def want(self, unit):
        if unit not in self._want:
            self._want[unit] = charspans_ref(self.text, self.doc_off, self.starts, self.ends, self.doc_tok, unit,
                                             self.ntok, self.cap)
        return self._want[unit]

    def __repr__(self):
        return f"<{self.name}: {self.nbytes} bytes, {len(self.starts)} spans, {len(self.doc_off) - 1} documents>"


def rune_spans(docs):
    """(text, doc_off, starts, ends, doc_tok) with one span per rune of every document."""
    text, off, s, e, tok = b"".join(docs), [0], [], [], [0]
    for doc in docs:
        base = off[-1]
        for a, b, _ in CC.runes(doc):
            s.append(base + a)
            e.append(base + b)
        off.append(base + len(doc))
        tok.append(len(s))
    return text, off, s, e, tok


def from_docs(name, docs, every_byte=False):
    """A case with one span per rune of each document (documents are bytes), and with every_byte also a span
    [p, q) for every byte p of a document and q = p, p + 1 and the document's end: positions inside runes."""
    text, off, s, e, tok = rune_spans(docs)
    if every_byte:
        s, e, tok = [], [], [0]
        for d in range(len(docs)):
            for p in range(off[d], off[d + 1] + 1):
                for q in sorted({p, min(p + 1, off[d + 1]), off[d + 1]}):
                    s.append(p)
                    e.append(q)
            tok.append(len(s))
    return Case(name, text, off, s, e, tok)


def from_batch(name, buf, off):
    """A case over a codepoint_cases corpus (buf, off): one span per rune of the model's decode."""
    return from_docs(name, CC.docs_of(buf, off))


def valid_rune_spans(buf, off):
    """(starts, ends, doc_tok) of one span per rune of a corpus that is valid UTF-8 throughout, by numpy: there
    a rune starts at every byte that is no continuation byte and ends where the next one starts."""
    n = int(off[-1])
    b = np.asarray(buf, np.uint8)[:n]
    s = np.flatnonzero((b & 0xC0) != 0x80).astype(np.uint32)
    e = np.concatenate([s[1:], np.array([n], np.uint32)]).astype(np.uint32)
    return s, e, np.searchsorted(s, np.asarray(off, np.uint64)).astype(np.uint64)


# ---- pieces the edge cases are built from ---------------------------------------------------------------------
R2, R3, R4 = "é".encode(), "中".encode(), "𠀀".encode()  # widths 2, 3 and 4 (the last counts 2 in UTF-16)
EMOJI = "😀".encode()
TRUNCATED = (b"\xc3", b"\xe4\xb8", b"\xf0\xa0\x80")  # leads whose sequence the document's end cuts short
MALFORMED = (b"\xc0\x80", b"\xe0\x80\x80", b"\xf0\x80\x80\x80", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf4\x90\x80\x80",
             b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80", b"\xfe", b"\xff", b"\x80", b"\xbf\xbf\xbf\xbf", b"\xe4\xb8\x41",
             b"\xf0\xa0\x80\x41", b"\xc3\xc3\xa9")


def filler(n, seed=0):
    """n bytes of valid UTF-8 of mixed widths (padded with ASCII to the exact length)."""
    rng = np.random.default_rng(seed)
    parts, left = [], n
    pool = (b"a", b"Z", R2, R3, R3, R4, EMOJI)
    while left > 0:
        p = pool[int(rng.integers(0, len(pool)))]
        if len(p) > left:
            p = b"x" * left
        parts.append(p)
        left -= len(p)
    return b"".join(parts)


def at_offset(edge, rune, k):
    """A one-document text in which byte k of `rune` is the byte at offset `edge`."""
    head = edge - k
    assert head >= 0
    return filler(head, edge + k) + rune + filler(37, k)


def boundary_docs(edge, delta, trunc, ncont):
    """Two documents whose boundary lies at offset edge + delta: the first ends in the truncated lead `trunc`,
    the second begins with ncont continuation bytes."""
    cut = edge + delta
    assert cut >= len(trunc)
    first = filler(cut - len(trunc), cut) + trunc
    second = b"\x80\xbf\x80"[:ncont] + filler(41, ncont)
    return [first, second]


def random_case(seed, nbytes=None, max_docs=9):
    """A seeded text of valid runes, malformed sequences and truncated leads, cut into documents at random bytes
    (inside runes too), with ordered, malformed and out-of-document spans, empty documents, and on some seeds
    ntok > cap, ntok < the list and doc_tok running past the count."""
    rng = np.random.default_rng(seed)
    nbytes = int(rng.integers(0, 400)) if nbytes is None else nbytes
    pool = (b"a", b" ", R2, R3, R4, EMOJI) + MALFORMED + TRUNCATED
    parts, left = [], nbytes
    while left > 0:
        p = pool[int(rng.integers(0, len(pool)))][:left]
        parts.append(p)
        left -= len(p)
    text = b"".join(parts)
    ndocs = int(rng.integers(1, max_docs + 1))
    cuts = np.sort(rng.integers(0, nbytes + 1, ndocs - 1)) if ndocs > 1 else np.zeros(0, np.int64)
    if ndocs > 3 and rng.random() < 0.5:
        cuts[:2] = 0          # empty documents first
        cuts[-1] = nbytes     # and last
    off = np.concatenate([[0], cuts, [nbytes]]).astype(np.int64)
    s, e, tok = [], [], [0]
    for d in range(ndocs):
        so, eo = int(off[d]), int(off[d + 1])
        for _ in range(int(rng.integers(0, 12))):
            a = int(rng.integers(so, eo + 1))
            b = int(rng.integers(a, min(eo, a + 9) + 1))
            kind = rng.random()
            if kind < 0.05:
                a, b = b, a - 1 if a else 0       # reversed (or equal)
            elif kind < 0.10:
                b = eo + 1 + int(rng.integers(0, 5))    # past the document
            elif kind < 0.15:
                a = so - 1 - int(rng.integers(0, 5)) if so else 0xFFFFFFF0  # before it, or far outside
            elif kind < 0.18:
                a, b = 0xFFFFFFF0, 0xFFFFFFFF
            s.append(a & 0xFFFFFFFF)
            e.append(b & 0xFFFFFFFF)
        tok.append(len(s))
    n = len(s)
    tok = np.asarray(tok, np.uint64)
    ntok, cap = n, n
    mode = seed % 4
    if mode == 1 and n:    # the count exceeds the arrays (full mode's over-long list)
        cap = int(rng.integers(0, n + 1))
        ntok = n + int(rng.integers(0, 50))
        tok = np.minimum(tok * 2, ntok).astype(np.uint64)
    elif mode == 2 and n:  # doc_tok runs past the count
        ntok = int(rng.integers(0, n + 1))
    elif mode == 3 and n:  # tokens before doc_tok[0] and after doc_tok[ndocs]
        tok = np.clip(tok.astype(np.int64) + 2, 0, max(n - 2, 2)).astype(np.uint64)
    return Case(f"random-{seed}", text, off, s[:cap], e[:cap], tok, ntok=ntok, cap=cap)
