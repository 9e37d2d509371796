"""Expected search-mode output (jb_cut_*_search) from the oracle: a helper, not a test.

The rules are those of include/jiebahip.h: for each token T of Cut(doc, hmm), in order,
a non-Han token gives T alone; a Han token of n runes gives its 2-rune grams (n > 2) and
then its 3-rune grams (n > 3) that buildDag has as edges, each in text order, then T.
The edges are restated here from the dictionary alone (Oracle.get): the gate on the
first rune (tokenizer.go:468-471), the break at the first absent prefix (:476-478) and
the frequency test (:479).  Pure Python on the CPU.
"""
import numpy as np

# Unicode 13.0.0 Script=Han = Go 1.18 unicode.Han: the ranges of jb_is_han (jb_common.h)
HAN_RANGES = (
    (0x2E80, 0x2E99), (0x2E9B, 0x2EF3), (0x2F00, 0x2FD5), (0x3005, 0x3005), (0x3007, 0x3007), (0x3021, 0x3029),
    (0x3038, 0x303B), (0x3400, 0x4DBF), (0x4E00, 0x9FFC), (0xF900, 0xFA6D), (0xFA70, 0xFAD9), (0x16FF0, 0x16FF1),
    (0x20000, 0x2A6DD), (0x2A700, 0x2B734), (0x2B740, 0x2B81D), (0x2B820, 0x2CEA1), (0x2CEB0, 0x2EBE0),
    (0x2F800, 0x2FA1D), (0x30000, 0x3134A),
)


def is_han(r):
    return any(lo <= r <= hi for lo, hi in HAN_RANGES)


class Grams:
    """E(i, L) of the rules above, with the dictionary lookups cached."""

    def __init__(self, oracle):
        self.o = oracle
        self.cache = {}

    def get(self, key):
        v = self.cache.get(key, self)
        if v is self:
            v = self.cache[key] = self.o.get(key)
        return v

    def edge(self, runes, i, L):
        f = self.get(runes[i])
        if f is None or f == 0:  # :468-471
            return False
        for k in range(1, L - 1):  # :476-478 (the prefix of one rune is the gate's)
            if self.get(runes[i:i + k + 1]) is None:
                return False
        g = self.get(runes[i:i + L])
        return g is not None and g > 0  # :479

    def of_token(self, tok):
        """tok: the token's bytes -> [(from, to)] byte offsets inside it, grams only, in output order."""
        try:
            runes = tok.decode("utf-8")
        except UnicodeDecodeError:
            return []
        n = len(runes)
        if n < 3 or not is_han(ord(runes[0])):
            return []
        p = [0]
        for ch in runes:
            p.append(p[-1] + len(ch.encode("utf-8")))
        out = [(p[i], p[i + 2]) for i in range(n - 1) if self.edge(runes, i, 2)]
        if n > 3:
            out += [(p[i], p[i + 3]) for i in range(n - 2) if self.edge(runes, i, 3)]
        return out


def expand(oracle, buf, starts, ends, doc_tok, grams=None):
    """The plain spans (starts, ends, doc_tok) of `buf` -> the search-mode (starts, ends, doc_tok)."""
    g = grams or Grams(oracle)
    data = bytes(np.asarray(buf, np.uint8))
    s = np.asarray(starts, np.int64)
    e = np.asarray(ends, np.int64)
    cnt = np.ones(len(s), np.int64)
    extra = {}
    for i in np.flatnonzero(e - s >= 9).tolist():  # (three runes are at least nine bytes)
        a = int(s[i])
        if data[a] < 0x80:
            continue
        gr = g.of_token(data[a:int(e[i])])
        if gr:
            extra[i] = gr
            cnt[i] += len(gr)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    xs = np.zeros(int(first[-1]), np.uint64)
    xe = np.zeros(int(first[-1]), np.uint64)
    last = first[1:] - 1
    xs[last] = s
    xe[last] = e
    for i, gr in extra.items():
        k, a = int(first[i]), int(s[i])
        for j, (x, y) in enumerate(gr):
            xs[k + j] = a + x
            xe[k + j] = a + y
    xd = first[np.asarray(doc_tok, np.int64)].astype(np.uint64)
    return xs, xe, xd


def expected(oracle, buf, doc_off, hmm, nthreads=8, grams=None):
    """(starts, ends, doc_tok) of the search-mode cut of a batch, from oracle.cut_batch's spans."""
    s, e, d = oracle.cut_batch(buf, doc_off, hmm, nthreads=nthreads)
    return expand(oracle, buf, s, e, d, grams)


def expected_text(oracle, text, hmm):
    """The search-mode tokens of one document, as strings."""
    import oracle as O
    b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    off = np.array([0, len(b)], np.uint64)
    s, e, _ = expected(oracle, np.frombuffer(b + b"\0" * 16, np.uint8), off, hmm, nthreads=1)
    return O.spans_to_tokens(b, s.astype(np.int64), e.astype(np.int64))


# The hand-checked examples: (dictionary text or None for tests/golden/mini_dict.txt, [(text, expected tokens)])
EXAMPLES = [
    ("甲 10\n甲乙 20\n甲乙丙 30\n甲乙丙丁 40\n乙 0\n乙丙 50\n丙 5\n丙丁 60\n丁 7\n", [
        ("甲乙丙丁", ["甲乙", "丙丁", "甲乙丙", "甲乙丙丁"]),  # 乙丙: 乙 has frequency 0; 乙丙丁 is absent
        ("甲乙丙", ["甲乙", "甲乙丙"]),  # n = 3: no 3-gram pass
        ("x甲乙丙丁y 甲乙丙丁丁", ["x", "甲乙", "丙丁", "甲乙丙", "甲乙丙丁", "y", "甲乙", "丙丁", "甲乙丙", "甲乙丙丁",
                           "丁"]),
    ]),
    (None, [
        ("这一刹那的", ["这", "一刹", "刹那", "一刹那", "的"]),
        ("abcd 1234", ["abcd", "1234"]),
    ]),
    ("𠀀 10\n𠀀𠀁 20\n𠀀𠀁中 30\n𠀀𠀁中𪜀 40\n𠀁 3\n𠀁中 9\n中 50\n中𪜀 8\n𪜀 4\n", [  # 4-byte Han runes
        ("a𠀀𠀁中𪜀𠀀𠀁中", ["a", "𠀀𠀁", "𠀁中", "中𪜀", "𠀀𠀁中", "𠀀𠀁中𪜀", "𠀀𠀁", "𠀁中", "𠀀𠀁中"]),
    ]),
]
# every record is zero: the dictionary's size is -73, so DevImage::plainw == 0
PLAINW0_DICT = "甲 5\n甲乙 3\n甲乙丙 4\n甲乙丙丁 6\n乙 2\n乙丙 1\n丙 2\n丙丁 3\n丁 1\n戊 -100\n"


def overflow_recipe(nfill=3000, seed=11):
    """The nested-chain dictionary and texts of test_record_overflow_paths (test_gpu_parity.py), restated:
    runes with more than 4 edges and edges longer than 8 runes.  Returns (dictionary text, texts)."""
    import random
    rng = random.Random(seed)
    pool = [chr(c) for c in range(0x4E00, 0x4E00 + 600)]
    lines, seqs = [], []
    f = 7
    for _ in range(40):  # nested chains: every prefix of a 6..24-rune string is a word
        s = "".join(rng.choice(pool) for _ in range(rng.randint(6, 24)))
        seqs.append(s)
        for k in range(1, len(s) + 1):
            if rng.random() < 0.8:
                f += rng.randint(1, 5)
                lines.append(f"{s[:k]} {f}")
    fill = []
    for i in range(nfill):
        w = rng.choice(pool) + rng.choice(pool) + (rng.choice(pool) if i % 3 == 0 else "")
        fill.append(w)
        lines.append(f"{w} {1000 + 3 * i}")
    texts = []
    for _ in range(400):
        parts = []
        for _ in range(rng.randint(1, 12)):
            r = rng.random()
            if r < 0.35:
                s = rng.choice(seqs)
                parts.append(s[: rng.randint(1, len(s))])
            elif r < 0.7:
                parts.append(rng.choice(fill))
            elif r < 0.9:
                parts.append("".join(rng.choice(pool) for _ in range(rng.randint(1, 6))))
            else:
                parts.append(rng.choice(["，", "。", " ab12 ", "\n"]))
        texts.append("".join(parts))
    texts.append("".join(seqs))  # one block through every chain
    texts.append("".join(seqs) * 6)  # the same as a long block
    return "\n".join(lines) + "\n", texts


def batch_of(texts):
    bs = [t.encode("utf-8") if isinstance(t, str) else t for t in texts]
    off = np.zeros(len(bs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs) + b"\0" * 16, np.uint8), off
