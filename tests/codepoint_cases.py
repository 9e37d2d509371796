"""Code-point and malformed-sequence corpora, and an independent model of the rune rules: a helper, not a test.

Every token boundary starts from three questions about a rune: is it Go-valid UTF-8, is it \\p{Han}, is it
unicode.IsSpace.  The model below answers them from Python's own strict UTF-8 decoder and from tables
written here; it shares no code with the oracle or with jb_common.h.  The corpora put every Unicode scalar
value, every byte class of malformed input, truncation at document ends and the tile-end lookahead through
the cut paths.  Each corpus function returns (buf, off): the documents concatenated (with zero bytes after
them) and their offsets.  Nothing here needs a GPU or the library.
"""
import bisect
import json
import random

import numpy as np

TILE = 4096

# ---- the model ------------------------------------------------------------------------------------------
# Unicode 13.0.0 Script=Han (Go 1.18 unicode.Han), the 19 ranges
HAN = [(0x2E80, 0x2E99), (0x2E9B, 0x2EF3), (0x2F00, 0x2FD5), (0x3005, 0x3005), (0x3007, 0x3007),
       (0x3021, 0x3029), (0x3038, 0x303B), (0x3400, 0x4DBF), (0x4E00, 0x9FFC), (0xF900, 0xFA6D),
       (0xFA70, 0xFAD9), (0x16FF0, 0x16FF1), (0x20000, 0x2A6DD), (0x2A700, 0x2B734), (0x2B740, 0x2B81D),
       (0x2B820, 0x2CEA1), (0x2CEB0, 0x2EBE0), (0x2F800, 0x2FA1D), (0x30000, 0x3134A)]
_HAN_LO = [a for a, _ in HAN]
# Go's unicode.IsSpace: White_Space
SPACE = frozenset([9, 10, 11, 12, 13, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
                  + list(range(0x2000, 0x200B)))
ALNUM = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz")


def is_han(r):
    k = bisect.bisect_right(_HAN_LO, r) - 1
    return k >= 0 and r <= HAN[k][1]


def is_space(r):
    return r in SPACE


def decode(b, i=0):
    """Go's utf8.DecodeRune at b[i:] -> (rune, width): the width comes from the lead byte, Python's strict
    decoder says whether those bytes are one valid rune; anything else is (U+FFFD, 1)."""
    b0 = b[i]
    if b0 < 0x80:
        return b0, 1
    if b0 >= 0xC0:
        n = 2 if b0 < 0xE0 else (3 if b0 < 0xF0 else 4)
        s = bytes(b[i:i + n])
        if len(s) == n:
            try:
                return ord(s.decode("utf-8")), n
            except UnicodeDecodeError:
                pass
    return 0xFFFD, 1


def runes(doc):
    """[(start, end, rune)] of a document's bytes (decoded with a cache on the four bytes at hand)."""
    out, i, n = [], 0, len(doc)
    cache = _DEC
    while i < n:
        k = doc[i:i + 4]
        v = cache.get(k)
        if v is None:
            v = cache[k] = decode(k)
        out.append((i, i + v[1], v[0]))
        i += v[1]
    return out


_DEC = {}


def split_blocks(doc):
    """splitText with the zh regex: [(start, end, is Han)] of the maximal Han runs and what lies between."""
    out = []
    for a, b, r in runes(doc):
        h = is_han(r)
        if out and out[-1][2] == h:
            out[-1][1] = b
        else:
            out.append([a, b, h])
    return [tuple(x) for x in out]


def cut_nonzh(doc, a=0, b=None):
    """cutNonZh on doc[a:b]: no token without a [0-9A-Za-z] byte; else alnum runs whole, every other
    rune alone, spaces dropped.  -> [(start, end)]"""
    b = len(doc) if b is None else b
    blk = doc[a:b]
    if not any(c in ALNUM for c in blk):
        return []
    out = []
    run = None
    for s, e, r in runes(blk):
        if r < 0x80 and r in ALNUM:
            if run is None:
                run = s
            continue
        if run is not None:
            out.append((a + run, a + s))
            run = None
        if r not in SPACE:
            out.append((a + s, a + e))
    if run is not None:
        out.append((a + run, b))
    return out


def cut_singles(doc, blocks=None):
    """Cut without the HMM under a dictionary that has no word of two or more runes in the text: every
    Han rune is a token, non-Han blocks go through cutNonZh.  -> [(start, end)]"""
    out = []
    for a, b, h in (split_blocks(doc) if blocks is None else blocks):
        if h:
            out += [(a + s, a + e) for s, e, _ in runes(doc[a:b])]
        else:
            out += cut_nonzh(doc, a, b)
    return out


# ---- helpers ----------------------------------------------------------------------------------------------
def batch_of(docs):
    bs = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in docs]
    off = np.zeros(len(bs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs) + b"\0" * 64, np.uint8), off


def docs_of(buf, off):
    data = bytes(np.asarray(buf, np.uint8)[:int(off[-1])])
    o = [int(x) for x in off]
    return [data[a:b] for a, b in zip(o[:-1], o[1:])]


def concat(parts):
    """[(buf, off)] laid end to end -> (buf, off)."""
    bufs, offs, base = [], [np.zeros(1, np.uint64)], 0
    for buf, off in parts:
        n = int(off[-1])
        bufs.append(np.asarray(buf, np.uint8)[:n])
        offs.append(np.asarray(off[1:], np.uint64) + np.uint64(base))
        base += n
    return np.concatenate(bufs + [np.zeros(64, np.uint8)]), np.concatenate(offs)


def one_document(buf, off):
    return buf, np.array([0, int(off[-1])], np.uint64)


def small_batches(buf, off, limit=4096, max_docs=4096):
    """Consecutive documents in batches of at most `limit` bytes and `max_docs` documents (a longer
    document is a batch of its own): [(first document, one past the last)]."""
    o = np.asarray(off, np.int64)
    out, a, n = [], 0, len(o) - 1
    while a < n:
        b = int(np.searchsorted(o, o[a] + limit, side="right")) - 1
        b = max(a + 1, min(b, a + max_docs, n))
        out.append((a, b))
        a = b
    return out


def encode_np(cps):
    """UTF-8 of code points that all have the same width -> (n, width) uint8."""
    c = np.asarray(cps, np.uint32)
    hi = int(c.max())
    if hi < 0x80:
        return c[:, None].astype(np.uint8)
    if hi < 0x800:
        cols = [0xC0 | (c >> 6), 0x80 | (c & 63)]
    elif hi < 0x10000:
        cols = [0xE0 | (c >> 12), 0x80 | ((c >> 6) & 63), 0x80 | (c & 63)]
    else:
        cols = [0xF0 | (c >> 18), 0x80 | ((c >> 12) & 63), 0x80 | ((c >> 6) & 63), 0x80 | (c & 63)]
    return np.stack(cols, axis=1).astype(np.uint8)


def width_of(c):
    return 1 if c < 0x80 else (2 if c < 0x800 else (3 if c < 0x10000 else 4))


def _width_groups(cps):
    """Ascending code points -> [(width, the code points of that width)], in order."""
    c = np.asarray(cps, np.uint32)
    w = np.where(c < 0x80, 1, np.where(c < 0x800, 2, np.where(c < 0x10000, 3, 4)))
    assert bool(np.all(np.diff(w) >= 0))
    return [(k, c[w == k]) for k in (1, 2, 3, 4) if bool(np.any(w == k))]


# ---- S: one document per scalar value ---------------------------------------------------------------------
def all_scalars():
    return np.concatenate([np.arange(0, 0xD800, dtype=np.uint32), np.arange(0xE000, 0x110000, dtype=np.uint32)])


def sprime_scalars():
    """U+0080..U+323FF, and of planes 4..16 the first and last 256 code points and every 257th between."""
    parts = [np.arange(0x80, 0xD800, dtype=np.uint32), np.arange(0xE000, 0x32400, dtype=np.uint32)]
    for p in range(4, 17):
        base = p << 16
        parts += [np.arange(base, base + 256, dtype=np.uint32),
                  np.arange(base + 256, base + 0x10000 - 256, 257, dtype=np.uint32),
                  np.arange(base + 0x10000 - 256, base + 0x10000, dtype=np.uint32)]
    return np.concatenate(parts)


S_HEAD, S_MID, S_TAIL = "，".encode(), "，中a".encode(), b"b"


def scalar_docs(cps, shift=0):
    """The document "，" + c + "，中a" + c + "b" of every code point c (ascending), after one document of
    `shift` bytes of "x".  13, 15, 17 or 19 bytes by c's width."""
    bufs, lens = [], []
    if shift:
        bufs.append(np.full(shift, ord("x"), np.uint8))
        lens.append(np.array([shift], np.uint64))
    for w, c in _width_groups(cps):
        enc = encode_np(c)
        n = len(c)
        rows = np.concatenate([np.tile(np.frombuffer(S_HEAD, np.uint8), (n, 1)), enc,
                               np.tile(np.frombuffer(S_MID, np.uint8), (n, 1)), enc,
                               np.tile(np.frombuffer(S_TAIL, np.uint8), (n, 1))], axis=1)
        assert rows.shape[1] == 11 + 2 * w
        bufs.append(rows.ravel())
        lens.append(np.full(n, rows.shape[1], np.uint64))
    off = np.zeros(sum(len(x) for x in lens) + 1, np.uint64)
    np.cumsum(np.concatenate(lens), out=off[1:])
    return np.concatenate(bufs + [np.zeros(64, np.uint8)]), off


def corpus_S(shift=0):
    return scalar_docs(all_scalars(), shift)


def corpus_Sprime(shift=0):
    return scalar_docs(sprime_scalars(), shift)


def scalar_token_counts(cps):
    """Tokens of each scalar document whatever the dictionary and the HMM setting: a Han c is a block
    of its own twice (，|c|，|中|a|c|b: 5 tokens, the blocks of "，" alone have no alnum); a space is
    dropped from "a" c "b" (中, a, b: 3); any other c above U+007F is a token there (中, a, c, b: 4).
    ASCII c (an alnum c joins "a" and "b", and gives the first block an alnum) goes through the model."""
    c = np.asarray(cps, np.uint32)
    han = np.zeros(len(c), bool)
    for lo, hi in HAN:
        han |= (c >= lo) & (c <= hi)
    sp = np.isin(c, np.array(sorted(SPACE), np.uint32))
    out = np.where(han, 5, np.where(sp, 3, 4)).astype(np.int64)
    for k in np.flatnonzero(c < 0x80).tolist():
        ch = bytes([int(c[k])])
        out[k] = len(cut_singles(S_HEAD + ch + S_MID + ch + S_TAIL))
    return out


# ---- D: dense documents -------------------------------------------------------------------------------------
def corpus_D(per=24):
    """"a" + 24 consecutive scalars of S' + "b"."""
    cps = sprime_scalars().tolist()
    return batch_of(["a" + "".join(map(chr, cps[i:i + per])) + "b" for i in range(0, len(cps), per)])


# ---- M: malformed sequences -----------------------------------------------------------------------------
M_R = (0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xE4, 0xFF)
M_PAIRS = ((0x80, 0x80), (0xBF, 0xBF), (0x80, 0x41), (0x41, 0x80))


def malformed_seqs():
    """(235904, 4) uint8: b0 in C0..FF, any b1, (b2, b3) of four pairs; then b0 in 80..FF with b1, b2, b3
    each of M_R.  Overlong forms, surrogates, values past U+10FFFF and valid runes are all among them."""
    b0, b1, p = np.meshgrid(np.arange(0xC0, 0x100), np.arange(0x100), np.arange(4), indexing="ij")
    pairs = np.array(M_PAIRS, np.uint8)
    a = np.stack([b0.ravel(), b1.ravel(), pairs[p.ravel(), 0], pairs[p.ravel(), 1]], axis=1)
    r = np.array(M_R)
    g = np.meshgrid(np.arange(0x80, 0x100), r, r, r, indexing="ij")
    b = np.stack([x.ravel() for x in g], axis=1)
    return np.concatenate([a, b]).astype(np.uint8)


def corpus_M():
    """"中" + s + "文a" + s + "，" of every malformed sequence s."""
    s = malformed_seqs()
    n = len(s)

    def col(t):
        return np.tile(np.frombuffer(t.encode(), np.uint8), (n, 1))
    rows = np.concatenate([col("中"), s, col("文a"), s, col("，")], axis=1)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(rows.shape[1])
    return np.concatenate([rows.ravel(), np.zeros(64, np.uint8)]), off


# ---- T: truncation at a document end --------------------------------------------------------------------
T_RUNES = ([0xE9, 0x3A9, 0x85, 0xA0, 0x7FF, 0x80,                         # width 2 (none is Han)
            0x3000, 0xFFFD, 0x20AC, 0x800, 0xFFFF, 0x2028, 0x3042, 0xD7FF, 0xE000,  # width 3, not Han
            0x4E2D, 0x6587, 0x3005, 0x3007, 0xF900,                       # width 3, Han
            0x1F600, 0x10000, 0x10FFFF, 0x16FEF, 0x1FFFF,                 # width 4, not Han
            0x20001, 0x2A700, 0x30000, 0x2F800]                           # width 4, Han
           + [0x2E80, 0x2E99, 0x3400, 0x4DBF, 0x4E00, 0x9FFC]             # first and last of three ranges
           + [0x16FF0, 0x16FF1, 0x20000, 0x2A6DD, 0x3134A])


def corpus_T():
    """For each encoding s and each k in 1..len(s)-1: "a" + s[:k], then s[k:] + "b"."""
    docs = []
    for r in T_RUNES:
        s = chr(r).encode("utf-8")
        for k in range(1, len(s)):
            docs += [b"a" + s[:k], s[k:] + b"b"]
    return batch_of(docs)


# ---- L: lookahead at a tile end -----------------------------------------------------------------------------
def overlong4(r):
    """The 4-byte overlong form of a BMP value."""
    return bytes([0xF0, 0x80 | (r >> 12), 0x80 | ((r >> 6) & 0x3F), 0x80 | (r & 0x3F)])


L_SECOND = ["一", "㐀", "𠀀", "鿼", "〇"]  # second runes of the two- and three-rune words (URO, Ext-A, 4-byte, ...)
L_VALID = ["一", "文", "𠀀"]             # tails after which the edges must appear
L_TAILS = ([overlong4(r) for r in (0x4E00, 0x3400, 0x9FFC, 0x3007)]
           + [b"\xf5\x84\xb8\x80", b"\xf4\x90\x80\x80", b"\xe0\x84\xb8", b"\xed\xa0\x80", b"\xe4\xb8", b"\xf0\xa0\x80"]
           + [t.encode() for t in L_VALID] + [b"", "，".encode()])
L_ENDS = (4094, 4095, 4096, 4097, 4098)
L_RUN = 40


def dict_L():
    lines = ["丁 5", "文 5", "丁文 100000"]
    for x in L_SECOND:
        lines += [f"{x} 5", f"丁{x} 100000", f"丁{x}丁 200000"]
    return "\n".join(lines) + "\n"


def corpus_L():
    """Documents of ASCII filler, "，", 40 x 丁 and the tail s + "丁丁文", laid out so that the last 丁 of
    the run ends at each offset of L_ENDS against a 4 KiB tile, once with the document starting in the
    run's tile and once in the tile before; documents of "y" bytes fill the gaps.  The first documents
    put their runs in the first three tiles of the batch.
    Returns (buf, off, cases): cases[k] = (document index, tail, byte offset of the end of the run)."""
    run = ("，" + "丁" * L_RUN).encode()
    docs, cases, pos = [], [], 0
    k = 0
    for tail in L_TAILS:
        for before in (False, True):
            for e in L_ENDS:
                tp = pos // TILE
                if before:  # the document starts late in tile t - 1
                    t = (tp if pos % TILE <= 3900 else tp + 1) + 1
                    start = max(pos, (t - 1) * TILE + 3000 + 7 * (k % 5))
                else:       # the document starts in tile t, the run's
                    t = tp if pos % TILE <= 3500 else tp + 1
                    start = max(pos, t * TILE + 11 * (k % 7))
                end = t * TILE + e  # the absolute end of the run (e >= 4096: in the next tile)
                if start > pos:
                    docs.append(b"y" * (start - pos))
                fill = end - len(run) - start
                assert fill >= 0
                doc = b"f" * fill + run + tail + "丁丁文".encode()
                cases.append((len(docs), tail, end))
                docs.append(doc)
                pos = start + len(doc)
                k += 1
    buf, off = batch_of(docs)
    return buf, off, cases


# ---- E: a dictionary and texts over the rare Han ranges ---------------------------------------------------
def pool_E(seed=19):
    rng = random.Random(seed)
    pool = []
    for lo, hi in HAN:
        pool += [lo, hi] + [rng.randint(lo, hi) for _ in range(20)]
    pool += [rng.randint(0x4E00, 0x9FA5) for _ in range(50)]
    return [chr(c) for c in dict.fromkeys(pool)]


def neighbours_E():
    """The code points just outside each end of each Han range (not Han, not surrogates)."""
    out = []
    for lo, hi in HAN:
        out += [c for c in (lo - 1, hi + 1) if not is_han(c)]
    return [chr(c) for c in dict.fromkeys(out)]


def files_E(outdir, seed=23, nwords=3000):
    """dict.txt and prob_emit.json in outdir (the formats of synth.Synth.write_files): about nwords words
    of 1..4 pool runes with seeded frequencies, every proper prefix a key; emission rows of all four
    states for every pool rune.  Returns (dict path, emit path, words)."""
    import os
    rng = random.Random(seed)
    pool = pool_E()
    words = {}
    for ch in pool:
        words[ch] = rng.randint(1, 5000)
    while len(words) < nwords:
        w = "".join(rng.choice(pool) for _ in range(rng.choice((2, 2, 2, 3, 3, 4))))
        for k in range(2, len(w)):
            words.setdefault(w[:k], rng.choice((0, rng.randint(1, 2000))))
        words.setdefault(w, rng.randint(1, 200000))
    dp, ep = os.path.join(outdir, "dict.txt"), os.path.join(outdir, "prob_emit.json")
    with open(dp, "w", encoding="utf-8") as f:
        f.write("".join(f"{w} {c} n\n" for w, c in words.items()))
    emit = {st: {ch: -rng.uniform(2.0, 12.0) for ch in pool} for st in "BEMS"}
    with open(ep, "w", encoding="utf-8") as f:
        json.dump(emit, f, ensure_ascii=False)
    return dp, ep, words


def corpus_E(words, seed=29, ndocs=300):
    """300 seeded documents of 0..400 pieces (pool words, single pool runes, the outside neighbour of each
    range end, "a1", "，", U+3000, three malformed strings), and all of them again as one document."""
    rng = random.Random(seed)
    pool, nb = pool_E(), neighbours_E()
    multi = [w for w in words if len(w) > 1]
    bad = [overlong4(0x4E00), b"\xed\xa0\x80", b"\xf4\x90\x80\x80"]
    docs = []
    for _ in range(ndocs):
        parts = []
        for _ in range(rng.randint(0, 400)):
            r = rng.random()
            if r < 0.55:
                parts.append(rng.choice(multi).encode())
            elif r < 0.75:
                parts.append(rng.choice(pool).encode())
            elif r < 0.85:
                parts.append(rng.choice(nb).encode())
            elif r < 0.97:
                parts.append(rng.choice(("a1", "，", "　")).encode())
            else:
                parts.append(rng.choice(bad))
        docs.append(b"".join(parts))
    docs.append(b"".join(docs))
    return batch_of(docs)
