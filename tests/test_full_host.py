"""CPU: full mode's expected output (tests/full_ref.py) against the hand-worked examples, the
literal jieba loop against the header's closed rule, and the library's new entry points.  No kernel
is launched here."""
import ctypes as C
import random

import numpy as np
import pytest

import full_ref as F
import jiebahip as J
import oracle as O
import synth

KINDS = [(J.JB_DICT_TXT, 0), (J.JB_DICT_PREFIX, J.JIEBA_SIZE)]


def _emit(mini_paths):
    with open(mini_paths[1], "rb") as f:
        return f.read()


@pytest.mark.parametrize("kind,size", KINDS)
def test_hand_worked_examples(mini_paths, kind, size):
    for dict_text, cases in F.EXAMPLES:
        o = O.Oracle(dict_text, _emit(mini_paths), kind, size)
        for rule in (F.literal_block, F.closed_block):
            for text, want in cases:
                assert F.expected_text(o, text, F.Blocks(o, rule)) == want, (text, kind, rule.__name__)
        o.close()


def test_literal_loop_equals_closed_rule_on_random_dags():
    rng = random.Random(5)
    nd = 0
    for _ in range(3000):
        n = rng.randint(1, 14)
        dag = {}
        for i in range(n):
            ends = {i + 1} if rng.random() < 0.8 else set()  # (buildDag may leave out the one-rune edge)
            for L in range(2, n - i + 1):
                if rng.random() < 0.25:
                    ends.add(i + L)
            dag[i] = sorted(ends) or [i + 1]
        a, b = F.literal_block(dag, n), F.closed_block(dag, n)
        assert a == b, dag
        nd += len(a)
    assert nd > 10000


@pytest.mark.parametrize("kind,size", KINDS)
def test_literal_loop_equals_closed_rule_on_texts(syn_small, kind, size):
    """Random corpus texts and texts of 4-byte Han runes, both dictionary kinds."""
    dp, ep, s = syn_small
    o = O.Oracle.from_files(dp, ep, kind, size)
    buf, off, _ = s.corpus(synth.KIND_DOCS, 1000, target_bytes=64 << 10)
    lit, clo = F.Blocks(o, F.literal_block), F.Blocks(o, F.closed_block)
    a, b = F.expected(o, buf, off, lit), F.expected(o, buf, off, clo)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert len(a[0]) > 5000 and lit.stats["multi"] > 1000 and lit.stats["dropped"] > 100, lit.stats
    assert int(a[2][-1]) == len(a[0]) and np.all(np.diff(a[0].astype(np.int64)) >= 0)  # by start
    o.close()
    o = O.Oracle(F.EXAMPLES[2][0], _emit((None, ep)), kind, size)
    rng = random.Random(9)
    for _ in range(200):
        t = "".join(rng.choice("𠀀𠀁中𪜀a，") for _ in range(rng.randint(0, 30)))
        assert F.expected_text(o, t, F.Blocks(o, F.literal_block)) == F.expected_text(
            o, t, F.Blocks(o, F.closed_block)), t
    o.close()


def test_expansion_dictionary_gives_more_spans_than_bytes(mini_paths):
    o = O.Oracle(F.chain_dict(12), _emit(mini_paths), 0, 0)
    text = "甲" * 200
    toks = F.expected_text(o, text)
    assert len(toks) == sum(min(11, 199 - i) for i in range(200)) and len(toks) > 3 * 200
    assert toks[:11] == ["甲" * k for k in range(2, 13)] and toks[-1] == "甲甲"
    o.close()


def test_library_exports_full_entry_points():
    """The four new symbols exist and refuse a null context before any device work."""
    L = J.lib()
    sp = J.jb_spans()
    off = (C.c_uint64 * 2)(0, 0)
    a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.jb_cut_full(None, b"", 0, C.byref(sp)) == J.JB_EINVAL
    assert L.jb_cut_batch_full(None, b"", off, 1, C.byref(sp)) == J.JB_EINVAL
    assert L.jb_cut_device_full(None, None, 0, None, 0, None, C.byref(a), C.byref(b), C.byref(c),
                                C.byref(d)) == J.JB_EINVAL
    assert L.jb_cut_device_full_into(None, None, 0, None, 0, None, None, None, 0, None, None) == J.JB_EINVAL
    for name in ("jb_cut_full", "jb_cut_batch_full", "jb_cut_device_full", "jb_cut_device_full_into"):
        assert name in J.EXPORTS
