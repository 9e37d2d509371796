"""CPU: jb_join, the host form of the joined-text rule (jieba-go_amd/csrc/jb_join.cpp), against join_ref.py,
byte for byte; jb_join_work_bytes; the limits.  The hand cases take their spans from the oracle and the mode
references over tests/golden/mini_dict.txt; their expected strings are written out below."""
import ctypes as C

import numpy as np
import pytest

import full_ref as F
import jiebahip as J
import join_ref as JR
import oracle as O
import search_ref as R

MIXED = "english번역『하다』今天天氣很好，ステーションabc1231+1=2我昨天去上海*important*去"  # (test_gpu_ids.MIXED)
INVALID = b"\xff\xfe" + "中文".encode() + b"\x80abc\xe4\xb8"
# mini_dict.txt, hmm off, the token lists documented in test_gpu_ids.py
MIXED_CUT = ("english 번 역 『 하 다 』 今天 天 氣 很 好 ， ス テ ー シ ョ ン abc1231 + 1 = 2 我 昨天 去 上海 * "
             "important * 去")
MIXED_FULL = MIXED_CUT.replace("今天 天 氣", "今天 天天 氣")
INVALID_ALL = "中 文 � abc � �"
HAND = {"cut": [MIXED_CUT, INVALID_ALL, "这 一刹那"], "search": [MIXED_CUT, INVALID_ALL, "这 一刹 刹那 一刹那"],
        "full": [MIXED_FULL, INVALID_ALL, "这 一刹 一刹那 刹那"]}
TEXTS = [MIXED, INVALID, "这一刹那"]


def test_exports():
    L = J.lib()
    for name in ("jb_join_work_bytes", "jb_join", "jb_join_device", "jb_joined_free", "jb_cut_batch_join"):
        assert name in J.EXPORTS and hasattr(L, name), name


def host(case, out_cap=None):
    return J.join(case.text, case.starts, case.ends, case.doc_tok, case.sep, case.term, ntok=case.ntok, cap=case.cap,
                  nbytes=case.nbytes, out_cap=out_cap)


def check(case):
    want, woff = case.want()
    out, off, nout = host(case)
    assert nout == len(want) and off.tolist() == woff, case
    assert out.tobytes() == want, case
    return nout


@pytest.mark.parametrize("mode", ["cut", "search", "full"])
def test_hand_cases(mini_paths, mode):
    o = O.Oracle.from_files(mini_paths[0], mini_paths[1], 0)
    buf, off = R.batch_of(TEXTS)
    if mode == "cut":
        s, e, d = o.cut_batch(buf, off, False)
    elif mode == "search":
        s, e, d = R.expected(o, buf, off, False)
    else:
        s, e, d = F.expected(o, buf[:int(off[-1])], off)
    text = bytes(buf[:int(off[-1])])
    out, ooff, nout = J.join(text, s, e, d, " ", "\n")
    want = "".join(h + "\n" for h in HAND[mode]).encode()
    assert out.tobytes() == want
    assert ooff.tolist() == np.cumsum([0] + [len(h.encode()) + 1 for h in HAND[mode]]).tolist() and nout == len(want)
    assert JR.join_ref(text, s, e, d)[0] == want
    # another separator, no terminator
    out, ooff, _ = J.join(text, s, e, d, "／", "")
    assert out.tobytes().decode() == "".join(h.replace(" ", "／") for h in HAND[mode])


def test_small_shapes():
    check(JR.Case("one empty document", b"abc", [], [], [0, 0]))
    check(JR.Case("no document", b"abc", [0], [3], [0]))
    check(JR.Case("empty text", b"", [], [], [0, 0, 0], b"", b""))
    check(JR.Case("empty documents in a row", b"abcd", [0, 2], [2, 4], [0, 0, 0, 1, 1, 1, 2, 2]))
    check(JR.Case("tokens outside every document", b"abcdef", [0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [1, 2, 4]))
    check(JR.Case("one long key", bytes(range(32, 127)) * 40, [0, 5], [3800, 6], [0, 2], b"--"))
    for sep in JR.SEPS:
        for term in JR.SEPS:
            check(JR.from_keys("separators", [[b"a", b"\xff", b"cd"], [], [b"\xe4\xb8\xad"]], sep, term))


def test_random_span_lists():
    kinds = set()
    for seed in range(400):
        case = JR.random_case(seed)
        nout = check(case)
        kinds.add((case.ntok > case.cap, int(case.doc_tok[-1]) > case.ntok, len(case.sep), len(case.term)))
        if seed % 8 == 0:
            want, woff = case.want()
            for cap in JR.out_caps(nout):
                buf = np.full(cap + 16, 0xA5, np.uint8)
                n = C.c_uint64()
                off = np.empty(len(case.doc_tok), np.uint64)
                J._check(J.lib().jb_join(case.text, case.nbytes, case.starts.ctypes.data, case.ends.ctypes.data,
                                         case.doc_tok.ctypes.data, case.ntok, case.cap, len(case.doc_tok) - 1, case.sep,
                                         len(case.sep), case.term, len(case.term), buf.ctypes.data, cap, off.ctypes.data,
                                         C.byref(n)))
                assert n.value == nout and off.tolist() == woff, (case, cap)
                m = min(cap, nout)
                assert buf[:m].tobytes() == want[:m] and (buf[m:] == 0xA5).all(), (case, cap)
    assert any(k[0] for k in kinds) and any(k[1] for k in kinds)
    assert {k[2] for k in kinds} == {0, 1, 3, 8} and {k[3] for k in kinds} == {0, 1, 3, 8}


def test_work_bytes():
    prev = 0
    for ntok in (0, 1, J.JB_JOIN_TILE - 1, J.JB_JOIN_TILE, J.JB_JOIN_TILE + 1, 10 ** 6, 10 ** 9, 2 ** 32 - 4096):
        w = J.join_work_bytes(ntok, 7)
        assert w > 0 and w >= prev
        prev = w
    prev = 0
    for ndocs in (0, 1, 255, 256, 257, 10 ** 6, 2 ** 32 - 1):
        w = J.join_work_bytes(1000, ndocs)
        assert w > 0 and w >= prev
        prev = w


def _rc(**kw):
    a = dict(text=b"abc", nbytes=3, s=np.array([0], np.uint32), e=np.array([3], np.uint32),
             d=np.array([0, 1], np.uint64), ntok=1, cap=1, ndocs=1, sep=b" ", seplen=1, term=b"\n", termlen=1,
             out=np.zeros(16, np.uint8), out_cap=16, off=np.zeros(2, np.uint64), n=C.c_uint64())
    a.update(kw)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return J.lib().jb_join(a["text"], a["nbytes"], p(a["s"]), p(a["e"]), p(a["d"]), a["ntok"], a["cap"], a["ndocs"],
                           a["sep"], a["seplen"], a["term"], a["termlen"], p(a["out"]), a["out_cap"], p(a["off"]),
                           C.byref(a["n"]) if a["n"] is not None else None)


def test_limits():
    assert _rc() == J.JB_OK
    assert _rc(sep=b"123456789", seplen=9) == J.JB_ELIMIT and b"separator" in J.lib().jb_last_error()
    assert _rc(term=b"123456789", termlen=9) == J.JB_ELIMIT
    assert _rc(sep=b"12345678", seplen=8, term=b"12345678", termlen=8, out_cap=0, out=None) == J.JB_OK
    assert _rc(nbytes=2 ** 31) == J.JB_ELIMIT
    assert _rc(cap=2 ** 32 - J.JB_JOIN_TILE) == J.JB_ELIMIT
    for k in ("text", "s", "e", "d", "sep", "term", "out", "off", "n"):
        assert _rc(**{k: None}) == J.JB_EINVAL, k
    # null is fine where the length is 0
    assert _rc(sep=None, seplen=0, term=None, termlen=0) == J.JB_OK
    assert _rc(s=None, e=None, cap=0, ntok=0) == J.JB_OK
    assert _rc(text=None, nbytes=0) == J.JB_OK
