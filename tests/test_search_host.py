"""CPU: search mode's expected output (tests/search_ref.py) against the hand-checked examples and
against buildDag itself, and the library's new entry points.  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest

import jiebahip as J
import oracle as O
import search_ref as R
import synth

KINDS = [(J.JB_DICT_TXT, 0), (J.JB_DICT_PREFIX, J.JIEBA_SIZE)]


@pytest.mark.parametrize("hmm", [False, True])
@pytest.mark.parametrize("kind,size", KINDS)
def test_hand_checked_examples(mini_paths, kind, size, hmm):
    with open(mini_paths[1], "rb") as f:
        emit = f.read()
    with open(mini_paths[0], "rb") as f:
        mini = f.read()
    for dict_text, cases in R.EXAMPLES:
        o = O.Oracle(mini if dict_text is None else dict_text, emit, kind, size)
        for text, want in cases:
            assert R.expected_text(o, text, hmm) == want, (text, kind, hmm)
        o.close()


@pytest.mark.parametrize("kind,size", KINDS)
def test_grams_are_build_dag_edges(syn_small, kind, size):
    """Every Han token of the corpus: the helper's grams are buildDag's edges of 2 and (n > 3) 3 runes."""
    dp, ep, s = syn_small
    o = O.Oracle.from_files(dp, ep, kind, size)
    buf, off, _ = s.corpus(synth.KIND_DOCS, 1000, target_bytes=256 << 10)
    data = bytes(buf)
    g = R.Grams(o)
    seen, ngr = set(), 0
    for hmm in (False, True):
        ps, pe, _ = o.cut_batch(buf, off, hmm, nthreads=8)
        for a, b in zip(ps.tolist(), pe.tolist()):
            tok = data[a:b]
            if tok in seen or tok[0] < 0x80:
                continue
            seen.add(tok)
            try:
                runes = tok.decode("utf-8")
            except UnicodeDecodeError:
                continue
            if not R.is_han(ord(runes[0])):
                continue
            n = len(runes)
            dag = o.build_dag(tok)
            p = [0]
            for ch in runes:
                p.append(p[-1] + len(ch.encode("utf-8")))
            want = [(p[i], p[i + 2]) for i in range(n - 1) if n > 2 and i + 2 in dag[i]]
            want += [(p[i], p[i + 3]) for i in range(n - 2) if n > 3 and i + 3 in dag[i]]
            assert g.of_token(tok) == want, runes
            ngr += len(want)
    assert ngr > 1000
    o.close()


def test_library_exports_search_entry_points():
    """The four new symbols exist and refuse a null context before any device work."""
    L = J.lib()
    sp = J.jb_spans()
    off = (C.c_uint64 * 2)(0, 0)
    a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.jb_cut_search(None, b"", 0, 0, C.byref(sp)) == J.JB_EINVAL
    assert L.jb_cut_batch_search(None, b"", off, 1, 0, C.byref(sp)) == J.JB_EINVAL
    assert L.jb_cut_device_search(None, None, 0, None, 0, 0, None, C.byref(a), C.byref(b), C.byref(c),
                                  C.byref(d)) == J.JB_EINVAL
    assert L.jb_cut_device_search_into(None, None, 0, None, 0, 0, None, None, None, 0, None, None) == J.JB_EINVAL
