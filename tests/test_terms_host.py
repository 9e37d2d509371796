"""CPU: the host side of the term-count and keyword calls (jb_terms_work_bytes, the argument checks of
jb_terms_device / jb_keywords_device / jb_keywords_batch).  No kernel is launched here."""
import ctypes as C

import numpy as np

import jiebahip as J

NEW = ["jb_terms_work_bytes", "jb_terms_device", "jb_keywords_device", "jb_keywords_batch"]


def test_exports():
    L = J.lib()
    for name in NEW:
        assert name in J.EXPORTS and hasattr(L, name), name
    assert J.JB_KW_MAXK >= 64


def test_null_and_zero_arguments():
    L = J.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    # (a null ctx: nothing can be queued)
    assert L.jb_terms_device(None, p, 1, p, p, 1, None, p, p, 1, p, p, p, 1 << 20) == J.JB_EINVAL
    assert L.jb_terms_device(None, None, 0, None, None, 0, None, None, None, 0, None, None, None, 0) == J.JB_EINVAL
    assert L.jb_keywords_device(None, p, p, p, 1, 1, p, 1, 20, None, p, p, p, p) == J.JB_EINVAL
    assert L.jb_keywords_batch(None, p, p, 1, 1, p, 1, 20, p, p, p, p) == J.JB_EINVAL
    assert "null" in L.jb_last_error().decode()
    # topk: 0 is a bad argument, more than JB_KW_MAXK an unsupported size
    assert L.jb_keywords_device(None, p, p, p, 1, 1, p, 1, 0, None, p, p, p, p) == J.JB_EINVAL
    assert L.jb_keywords_device(None, p, p, p, 1, 1, p, 1, J.JB_KW_MAXK + 1, None, p, p, p, p) == J.JB_ELIMIT
    assert "JB_KW_MAXK" in L.jb_last_error().decode()
    assert L.jb_keywords_batch(None, p, p, 1, 1, p, 1, 0, p, p, p, p) == J.JB_EINVAL
    assert L.jb_keywords_batch(None, p, p, 1, 1, p, 1, J.JB_KW_MAXK + 1, p, p, p, p) == J.JB_ELIMIT
    assert L.jb_keywords_device(None, p, p, p, 1, 1, p, 1, J.JB_KW_MAXK, None, p, p, p, p) == J.JB_EINVAL  # (the ctx)


def test_work_bytes():
    wb = J.terms_work_bytes
    assert wb(1, 1) > 0 and wb(0, 0) > 0
    T = J.JB_TERMS_TILE
    sizes = [0, 1, T - 1, T, T + 1, 2 * T, 10 * T + 5, 1 << 20, (1 << 20) + 1, 1 << 27, (1 << 31) - 1]
    for nd in (0, 1, 1000, 1 << 20, (1 << 32) - 1):
        vals = [wb(n, nd) for n in sizes]
        assert vals == sorted(vals), (nd, vals)
    for n in sizes:
        vals = [wb(n, nd) for nd in (0, 1, 1000, 1 << 20, (1 << 32) - 1)]
        assert vals == sorted(vals), (n, vals)
    # whole tiles of two 8-byte entries per token, and a little per tile
    assert wb(T, 1) >= 16 * T and wb(T + 1, 1) >= 32 * T and wb(T, 1) < wb(T + 1, 1)
    assert wb(1 << 27, 1) < 17 * (1 << 27)
