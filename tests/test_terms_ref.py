"""CPU: the numpy reference of the term-count and keyword calls (terms_ref.py) against small cases
worked out by hand."""
import numpy as np

import terms_ref as TR

U = TR.UNK


def _f32(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def test_terms_by_hand():
    #      doc 0        doc 1 (empty)  doc 2        doc 3 (all unknown)  doc 4 (cut by the bound)
    ids = [5, 3, 5, U,                 0, 0xFFFFFFFE, 0,  U, U,          7, 7, 9]
    doc_tok = [0, 4, 4, 7, 9, 12]
    tid, tcnt, off = TR.terms(ids, doc_tok, 12, 12)
    assert tid.tolist() == [3, 5, 0, 0xFFFFFFFE, 7, 9] and tcnt.tolist() == [1, 2, 2, 1, 2, 1]
    assert off.tolist() == [0, 2, 2, 4, 4, 6] and tid.dtype == np.uint32 and off.dtype == np.uint64
    # the bound: min(ntok, ids_cap) = 10 drops the last 7 and the 9; 8 leaves document 4 empty
    for ntok, cap in ((10, 12), (12, 10), (10, 10)):
        tid, tcnt, off = TR.terms(ids, doc_tok, ntok, cap)
        assert tid.tolist() == [3, 5, 0, 0xFFFFFFFE, 7] and tcnt.tolist() == [1, 2, 2, 1, 1]
        assert off.tolist() == [0, 2, 2, 4, 4, 5]
    tid, tcnt, off = TR.terms(ids, doc_tok, 8, 12)
    assert off.tolist() == [0, 2, 2, 4, 4, 4] and len(tid) == 4
    tid, tcnt, off = TR.terms(ids, doc_tok, 0, 12)
    assert off.tolist() == [0] * 6 and len(tid) == 0 and len(tcnt) == 0
    # a token list that runs past the documents: the tokens after doc_tok[ndocs] belong to nobody
    tid, tcnt, off = TR.terms([1, 1, 2], [0, 2], 3, 3)
    assert tid.tolist() == [1] and tcnt.tolist() == [2] and off.tolist() == [0, 1]


def test_keywords_by_hand():
    # ids               0    1    2     3    4     5       6    7
    w = np.array([1.0, 2.0, 0.0, -1.0, np.nan, np.inf, 0.5, 1.0], np.float32)
    tid = np.array([0, 1, 2, 3, 4, 6, 7, 9,     5, 6,      2, 3, 4, 8], np.uint32)
    tcnt = np.array([2, 1, 9, 9, 9, 4, 2, 50,   1, 3,      1, 1, 1, 1], np.uint32)
    off = np.array([0, 8, 8, 10, 14], np.uint64)
    kid, ksc, kcn, kn = TR.keywords((tid, tcnt, off), w, 3)
    # document 0: the scores are 2, 2, -, -, -, 2, 2 and id 9 >= nweights: four ties, the id decides
    assert kid[0].tolist() == [0, 1, 6] and kcn[0].tolist() == [2, 1, 4] and _f32(ksc[0]) == _f32([2, 2, 2])
    # document 1 is empty; document 2: +Inf first; document 3 has no candidate (0, negative, NaN, id 8)
    assert kn.tolist() == [3, 0, 2, 0]
    assert kid[1].tolist() == [U, U, U] and _f32(ksc[1]) == [0, 0, 0] and kcn[1].tolist() == [0, 0, 0]
    assert kid[2].tolist() == [5, 6, U] and kcn[2].tolist() == [1, 3, 0] and _f32(ksc[2]) == _f32([np.inf, 1.5, 0])
    assert kid[3].tolist() == [U, U, U]
    kid, ksc, kcn, kn = TR.keywords((tid, tcnt, off), w, 5)
    assert kid[0].tolist() == [0, 1, 6, 7, U] and kn.tolist() == [4, 0, 2, 0]
    kid, ksc, kcn, kn = TR.keywords((tid, tcnt, off), w, 1)
    assert kid[:, 0].tolist() == [0, U, 5, U] and kid.shape == (4, 1)
    # one f32 conversion and one f32 multiply: 2^24 + 3 rounds to 2^24 + 4 before the product
    kid, ksc, kcn, kn = TR.keywords((np.array([0], np.uint32), np.array([2**24 + 3], np.uint32), np.array([0, 1], np.uint64)),
                                    np.array([0.1], np.float32), 2)
    assert _f32(ksc[0]) == _f32([np.float32(2**24 + 4) * np.float32(0.1), 0]) and kcn[0].tolist() == [2**24 + 3, 0]
    # no weights at all: nothing is a candidate
    kid, ksc, kcn, kn = TR.keywords((tid, tcnt, off), np.zeros(0, np.float32), 2)
    assert kn.tolist() == [0, 0, 0, 0] and (kid == U).all()
