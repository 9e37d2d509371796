"""Expected full-mode output (jb_cut_*_full) from the oracle alone: a helper, not a test.

The rules are those of include/jiebahip.h.  Each document is split by the oracle's splitText;
a non-Han block gives the oracle's cutNonZh tokens; a Han block gives what jieba's __cut_all
loop gives on Oracle.build_dag's DAG of the block, run here literally (literal_block), with its
old_j variable.  closed_block restates the same output by the header's closed rule (the nearest
earlier rune that has words); test_full_host.py checks the two against each other, and the
kernels follow the closed rule, so the literal loop is an independent check of them.
Pure Python on the CPU.
"""
import numpy as np

import oracle as O


def literal_block(dag, n):
    """jieba's __cut_all loop over a block of n runes.  dag: {i: [exclusive end, ...]} as buildDag
    returns it (jieba's DAG holds inclusive ends, hence the - 1).  -> [(i, exclusive end)]."""
    out = []
    old_j = -1
    for k in range(n):
        L = [e - 1 for e in dag.get(k, [])]
        if len(L) == 1 and k > old_j:
            out.append((k, L[0] + 1))
            old_j = L[0]
        else:
            for j in L:
                if j > k:
                    out.append((k, j + 1))
                    old_j = j
    return out


def closed_block(dag, n):
    """The header's rule: M(i) = D(i) minus {1}; a rune with M = {} is emitted alone unless the nearest
    earlier rune i' with M(i') != {} has i' + max M(i') > i."""
    out = []
    M = [sorted(e - i for e in dag.get(i, []) if e - i > 1) for i in range(n)]
    for i in range(n):
        if M[i]:
            out += [(i, i + L) for L in M[i]]
            continue
        near = next((j for j in range(i - 1, -1, -1) if M[j]), None)
        if near is None or near + max(M[near]) <= i:
            out.append((i, i + 1))
    return out


class Blocks:
    """The spans of a block, relative to it, with the oracle's answers cached per block text."""

    def __init__(self, oracle, rule=literal_block):
        self.o = oracle
        self.rule = rule
        self.han = {}
        self.non = {}
        self.stats = {"han_spans": 0, "multi": 0, "dropped": 0, "zero_like": 0}

    def of_han(self, blk):
        v = self.han.get(blk)
        if v is None:
            runes = blk.decode("utf-8")
            p = [0]
            for ch in runes:
                p.append(p[-1] + len(ch.encode("utf-8")))
            dag = self.o.build_dag(blk)
            sp = self.rule(dag, len(runes))
            v = self.han[blk] = [(p[i], p[j]) for i, j in sp]
            single = {i for i, j in sp if j == i + 1}
            self.stats["dropped"] += sum(1 for i in range(len(runes))
                                         if i not in single and all(e - i <= 1 for e in dag.get(i, [])))
            self.stats["zero_like"] += sum(1 for i in range(len(runes))
                                           if len(dag.get(i, [])) > 4 or max(dag.get(i, [i + 1])) - i > 8)
        self.stats["han_spans"] += len(v)
        self.stats["multi"] += sum(1 for a, b in v if b - a > 4)
        return v

    def of_non(self, blk):
        v = self.non.get(blk)
        if v is None:
            s = np.zeros(len(blk) + 1, np.uint32)
            e = np.zeros(len(blk) + 1, np.uint32)
            n = O.lib().or_cut_nonzh(blk, len(blk), s.ctypes.data, e.ctypes.data, len(blk) + 1)
            v = self.non[blk] = list(zip(s[:n].tolist(), e[:n].tolist()))
        return v


def expected(oracle, buf, doc_off, blocks=None):
    """(starts u64, ends u64, doc_tok u64) of the full-mode cut of a batch."""
    bl = blocks or Blocks(oracle)
    data = bytes(np.asarray(buf, np.uint8))
    off = [int(x) for x in doc_off]
    xs, xe, xd = [], [], [0]
    for a, b in zip(off[:-1], off[1:]):
        base = a
        for blk, han in (O.split_text(data[a:b]) if b > a else []):
            for x, y in (bl.of_han(blk) if han else bl.of_non(blk)):
                xs.append(base + x)
                xe.append(base + y)
            base += len(blk)
        assert base == b
        xd.append(len(xs))
    return np.array(xs, np.uint64), np.array(xe, np.uint64), np.array(xd, np.uint64)


def expected_text(oracle, text, blocks=None):
    """The full-mode tokens of one document, as strings."""
    b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    s, e, _ = expected(oracle, np.frombuffer(b + b"\0" * 16, np.uint8), [0, len(b)], blocks)
    return O.spans_to_tokens(b, s.astype(np.int64), e.astype(np.int64))


# The hand-worked examples of the header's rule: (dictionary text, [(text, expected tokens)])
DICT_A = "甲 10\n甲乙 20\n甲乙丙 30\n甲乙丙丁 40\n乙 0\n乙丙 50\n丙 5\n丙丁 60\n丁 7\n"  # (search_ref.EXAMPLES[0])
DICT_B = "甲 5\n甲乙 5\n甲乙丙 0\n甲乙丙丁 5\n乙 5\n乙丙 5\n丙 5\n丁 5\n"
EXAMPLES = [
    (DICT_A, [
        ("甲乙丙丁", ["甲乙", "甲乙丙", "甲乙丙丁", "丙丁"]),  # 乙 has frequency 0: no 乙丙; 乙 and 丁 are covered
        ("x甲乙丙丁y 丁甲", ["x", "甲乙", "甲乙丙", "甲乙丙丁", "丙丁", "y", "丁", "甲"]),  # (cutNonZh drops the space)
    ]),
    (DICT_B, [
        # the first 丁 is emitted although 甲乙丙丁 covers it: the nearest rune with words is 乙, and 乙丙
        # ends before it; 丙 is dropped
        ("甲乙丙丁戊丁", ["甲乙", "甲乙丙丁", "乙丙", "丁", "戊", "丁"]),
    ]),
    ("𠀀 10\n𠀀𠀁 20\n𠀀𠀁中 30\n𠀀𠀁中𪜀 40\n𠀁 3\n𠀁中 9\n中 50\n中𪜀 8\n𪜀 4\n", [  # 4-byte Han runes
        ("a𠀀𠀁中𪜀𠀀𠀁中", ["a", "𠀀𠀁", "𠀀𠀁中", "𠀀𠀁中𪜀", "𠀁中", "中𪜀", "𠀀𠀁", "𠀀𠀁中", "𠀁中"]),
    ]),
]


def chain_dict(n=12, rune="甲"):
    """rune, rune x 2, ..., rune x n, all with positive frequencies: a text of that rune alone gives
    nearly n - 1 spans per rune, more spans than bytes."""
    return "".join(f"{rune * k} {100 + k}\n" for k in range(1, n + 1))
