"""CPU: jb_filter, the host form of the token filter's rule (jieba-go_amd/csrc/jb_filter.cpp), against
filter_ref.py, exactly, on every output: seeded span lists (overlapping, bad, counts past the arrays), every
class, the rune bounds, stop keys of every storage form, out_cap below the kept count between guard values,
doc_tok entries beyond the list, empty documents, the accounting identity, the size helper and every error
code.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as F
from filter_cases import HAN256, LENGTH_PIECES, NEAR_KEYS, PIECES, RUNE_BOUNDS, STOP_KEYS, spans_of
import jiebahip as J
import oracle as O
import search_ref as R

NEW = ["jb_stopwords_set", "jb_stopwords_size", "jb_filter_work_bytes", "jb_filter", "jb_filter_device",
       "jb_cut_batch_filter", "jb_batch_filter_set"]
GUARD = 0xA5A5A5A5
ALL = F.HAN | F.ALNUM | F.NUM | F.OTHER | F.INVALID


def test_exports():
    L = J.lib()
    for name in NEW:
        assert name in J.EXPORTS and hasattr(L, name), name
    assert (J.JB_TC_HAN, J.JB_TC_ALNUM, J.JB_TC_NUM, J.JB_TC_OTHER, J.JB_TC_INVALID) == (
        F.HAN, F.ALNUM, F.NUM, F.OTHER, F.INVALID)
    assert (J.JB_FILTER_STOP, J.JB_FILTER_TILE) == (F.STOP, F.TILE)
    assert C.sizeof(J.jb_filter_rule) == 16


def raw(text, s, e, dt, rule, stop=None, ntok=None, cap=None, nbytes=None, out_cap=None, src=True):
    """jb_filter with guard words behind every output: (rc, out_start, out_end, out_src, out_doc_tok, n, stats)."""
    t = np.frombuffer(bytes(text) + b"\0", np.uint8)
    s, e = np.ascontiguousarray(s, np.uint32), np.ascontiguousarray(e, np.uint32)
    dt = np.ascontiguousarray(dt, np.uint64)
    nd = len(dt) - 1
    cap = len(s) if cap is None else cap
    ntok = len(s) if ntok is None else ntok
    nbytes = len(text) if nbytes is None else nbytes
    out_cap = cap if out_cap is None else out_cap
    os_, oe, osrc = (np.full(out_cap + 3, GUARD, np.uint32) for _ in range(3))
    odt = np.full(nd + 1 + 3, GUARD, np.uint64)
    n = np.full(2, GUARD, np.uint64)
    st = np.full(5 + 3, GUARD, np.uint64)
    p = lambda a: a.ctypes.data if a.size else None
    rc = J.lib().jb_filter(t.ctypes.data, nbytes, p(s), p(e), dt.ctypes.data, ntok, cap, nd, C.byref(rule),
                           stop.h if stop is not None else None, os_.ctypes.data, oe.ctypes.data,
                           osrc.ctypes.data if src else None, out_cap, odt.ctypes.data, n.ctypes.data, st.ctypes.data)
    return rc, os_, oe, osrc, odt, n, st


def check(text, s, e, dt, flags=0, drop=0, min_runes=0, max_runes=0, stop_keys=None, src=True, **kw):
    stop = J.Vocab(stop_keys) if stop_keys is not None else None
    rule = J.jb_filter_rule(flags, drop, min_runes, max_runes)
    keys = {k.encode() if isinstance(k, str) else k for k in stop_keys or ()}
    ref = F.filter_ref(text, s, e, dt, flags, drop, min_runes, max_runes, keys, **kw)
    rc, os_, oe, osrc, odt, n, st = raw(text, s, e, dt, rule, stop, src=src, **kw)
    assert rc == J.JB_OK, J.lib().jb_last_error()
    w = len(ref[0])
    assert os_[:w].tolist() == ref[0] and oe[:w].tolist() == ref[1]
    if src:
        assert osrc[:w].tolist() == ref[2]
    else:
        assert (osrc == GUARD).all()
    # nothing behind the entries the rule writes is touched
    assert (os_[w:] == GUARD).all() and (oe[w:] == GUARD).all() and (osrc[w:] == GUARD).all()
    nd = len(dt) - 1
    assert odt[:nd + 1].tolist() == ref[3] and (odt[nd + 1:] == GUARD).all()
    assert int(n[0]) == ref[4] and n[1] == GUARD
    assert st[:5].tolist() == ref[5] and (st[5:] == GUARD).all()
    assert int(st[0]) == int(n[0]) + int(st[1:5].sum())  # the accounting identity
    return ref


def test_every_class():
    text, s, e = spans_of(PIECES)
    dt = [0, len(s)]
    want = [F.HAN, F.ALNUM, F.NUM, F.NUM, F.ALNUM, F.ALNUM, F.OTHER, F.INVALID, F.OTHER, F.OTHER, F.OTHER, F.ALNUM,
            F.ALNUM, F.NUM, F.HAN, F.HAN, F.OTHER, F.OTHER, F.HAN, F.OTHER, F.HAN, F.ALNUM, F.INVALID, F.OTHER, F.HAN]
    assert [F.token_class(p) for p in PIECES] == want
    for cls in (F.HAN, F.ALNUM, F.NUM, F.OTHER, F.INVALID):
        ref = check(text, s, e, dt, drop=cls)
        assert ref[2] == [k for k in range(len(s)) if want[k] != cls]
        assert ref[5][2] == want.count(cls)
        check(text, s, e, dt, drop=ALL & ~cls)
    assert check(text, s, e, dt, drop=ALL)[4] == 0
    assert check(text, s, e, dt)[4] == len(s)
    # a Han rune cut short by e, and a lone continuation byte, one span each over the same bytes
    t = "中".encode()
    assert check(t, [0, 0, 0, 1, 2], [3, 2, 1, 2, 3], [0, 5], drop=F.HAN)[2] == [1, 2, 3, 4]
    assert check(t, [0, 0, 0, 1, 2], [3, 2, 1, 2, 3], [0, 5], drop=F.INVALID)[2] == [0, 1]


@pytest.mark.parametrize("lo,hi", RUNE_BOUNDS)
def test_rune_bounds(lo, hi):
    text, s, e = spans_of(PIECES + LENGTH_PIECES)
    ref = check(text, s, e, [0, len(s)], min_runes=lo, max_runes=hi)
    n = [F.runes(text[a:b], F.token_class(text[a:b])) for a, b in zip(s, e)]
    assert ref[2] == [k for k in range(len(s)) if n[k] >= lo and not (hi and n[k] > hi)]
    by = dict(zip(PIECES, n[:len(PIECES)]))
    assert by[HAN256] == 256 and by["😀".encode() * 256 + b"\xf0"] == 256 and by[b"\x80"] == 1 and by[b"\xbf\xbf"] == 0
    assert n[-3:] == [256, 0, 0] and n[-4] == 256


def test_stop_keys():
    keys, near = STOP_KEYS, NEAR_KEYS
    text, s, e = spans_of(keys + near + keys)
    dt = [0, 5, 5, len(s)]
    ref = check(text, s, e, dt, flags=F.STOP, stop_keys=keys)
    # every key is found, the replaced byte finds EF BF BD, and nothing near a key does
    nk = len(keys)
    assert ref[2] == [k for k in range(nk, nk + len(near)) if near[k - nk] not in (b"\x80", b"\xff")]
    assert ref[5][4] == 2 * nk + 2
    assert check(text, s, e, dt, flags=F.STOP, stop_keys=[])[4] == len(s)
    assert check(text, s, e, dt, flags=0, stop_keys=keys)[4] == len(s)
    # the order of the reasons: class before length before stop
    ref = check(text, s, e, dt, flags=F.STOP, drop=F.NUM, min_runes=2, stop_keys=keys)
    assert ref[5] == F.filter_ref(text, s, e, dt, F.STOP, F.NUM, 2, 0, set(keys))[5]
    assert ref[5][2] == 2 * 1 + 2 and ref[5][3] > 0 and ref[5][4] > 0  # (123 twice, 1234 and 12)


def test_out_cap_and_no_src():
    text, s, e = spans_of(PIECES)
    dt = [0, 3, len(s)]
    kept = check(text, s, e, dt, drop=F.OTHER)[4]
    for oc in (0, 1, kept - 1, kept, kept + 5):
        ref = check(text, s, e, dt, drop=F.OTHER, out_cap=oc)
        assert ref[4] == kept and len(ref[0]) == min(oc, kept)
        check(text, s, e, dt, drop=F.OTHER, out_cap=oc, src=False)


def test_doc_tok_and_clamps():
    text, s, e = spans_of(PIECES)
    n = len(s)
    check(text, s, e, [0, 0, 2, 2, 2, 7, n, n], drop=F.ALNUM)  # empty documents
    check(text, s, e, [3, 5, n + 4, 2 ** 63, 2 ** 64 - 1], drop=F.ALNUM)  # entries beyond nt, tokens of no document
    check(text, s, e, [n, 5, 0], drop=F.ALNUM)  # (decreasing: every entry on its own)
    check(text, s, e, [0], drop=F.ALNUM)  # no document
    for ntok, cap in ((n + 9, n), (n, n - 4), (3, n), (0, n), (n, 0), (2 ** 40, 5)):
        ref = check(text, s[:cap], e[:cap], [0, 2, n], drop=F.ALNUM, ntok=ntok, cap=cap)
        assert ref[5][0] == min(ntok, cap)
    check(b"", [], [], [0, 0], drop=F.ALNUM)
    # nbytes below the text: the spans past it are bad
    ref = check(text, s, e, [0, n], nbytes=10)
    assert ref[5][1] == sum(1 for b in e if b > 10)


def test_seeded_span_lists():
    rng = np.random.default_rng(20240607)
    alphabet = [b"a", b"7", "中".encode(), "的".encode(), "，".encode(), b"\x80", b"\xe4", b" ", "😀".encode(), b"Q"]
    stop_keys = [b"a", b"7", "的".encode(), "中的".encode(), b"\xef\xbf\xbd", b"aa7", b"a" * 9, "，".encode() * 9]
    for _ in range(150):
        text = b"".join(alphabet[i] for i in rng.integers(0, len(alphabet), int(rng.integers(0, 300))))
        nb = len(text)
        n = int(rng.integers(0, 200))
        s = rng.integers(0, nb + 1, n)
        ln = np.where(rng.random(n) < 0.5, rng.integers(0, 5, n), rng.integers(0, 40, n))
        e = np.minimum(s + ln, nb)
        kind = rng.integers(0, 16, n)
        e = np.where(kind == 0, s, e)
        s, e = np.where(kind == 1, e, s), np.where(kind == 1, s, e)
        e = np.where(kind == 2, nb + 1 + rng.integers(0, 1000, n), e)
        s = np.where(kind == 3, 0xFFFFFFF0, s)
        e = np.where(kind == 3, 0xFFFFFFFF, e)
        nd = int(rng.integers(0, 9))
        dt = np.sort(rng.integers(0, n + 4, nd + 1))
        ntok, cap = n, n
        k = int(rng.integers(0, 3))
        if k == 1:
            ntok, cap = int(rng.integers(0, 2 * n + 2)), int(rng.integers(0, n + 1))
        if k == 2:
            ntok = int(rng.integers(0, n + 1))
        check(text, s[:cap], e[:cap], dt, flags=int(rng.integers(0, 2)), drop=int(rng.integers(0, 32)),
              min_runes=int(rng.integers(0, 4)), max_runes=int(rng.integers(0, 6)), stop_keys=stop_keys, ntok=ntok, cap=cap,
              out_cap=int(rng.integers(0, n + 2)), src=bool(rng.integers(0, 2)))


TEXTS = ["english번역『하다』今天天氣很好，ステーションabc1231+1=2我昨天去上海*important*去",
         b"\xff\xfe" + "中文".encode() + b"\x80abc\xe4\xb8", "这一刹那", "", "这一刹那的上海, 2024 年 x86"]


@pytest.mark.parametrize("hmm", [False, True])
def test_mini_dictionary_cuts(mini_paths, hmm):
    o = O.Oracle.from_files(mini_paths[0], mini_paths[1], 0)
    buf, off = R.batch_of(TEXTS)
    text = bytes(buf[:int(off[-1])])
    for s, e, dt in (o.cut_batch(buf, off, hmm), R.expected(o, buf, off, hmm)):
        ref = check(text, s, e, dt, flags=F.STOP, drop=F.OTHER | F.INVALID, min_runes=2, stop_keys=["上海", "abc1231"])
        words = [text[a:b].decode() for a, b in zip(ref[0], ref[1])]
        assert "今天" in words and "上海" not in words and "，" not in words and "abc1231" not in words
        assert all(len(w) >= 2 for w in words)
        # the module-level wrapper returns the same arrays
        got = J.filter_spans(text, s, e, dt, J.filter_rule(("other", "invalid"), 2, 0, True), J.Vocab(["上海", "abc1231"]))
        assert got[0][:got[4]].tolist() == ref[0] and got[3].tolist() == ref[3] and got[5].tolist() == ref[5]


def test_work_bytes():
    prev = 0
    for n in (0, 1, 63, 2047, 2048, 2049, 10 ** 6, 2 ** 31, 2 ** 32):
        for nd in (0, 1, 10 ** 6):
            b = J.filter_work_bytes(n, nd)
            assert b > 0 and b >= prev and b >= J.filter_work_bytes(n, 0)
        assert J.filter_work_bytes(n, 0) >= prev
        prev = J.filter_work_bytes(n, 0)
    assert J.filter_work_bytes(2 ** 64 - 1, 2 ** 32 - 1) > 0
    # one bit per token and about 40 bytes per tile
    assert J.filter_work_bytes(2048 * 1000, 0) <= 2048 * 1000 // 8 + 48 * 1000 + 1024


def test_errors():
    L = J.lib()
    text, s, e = spans_of([b"ab", b"cd"])
    t = np.frombuffer(text, np.uint8)
    s, e = np.array(s, np.uint32), np.array(e, np.uint32)
    dt = np.array([0, 2], np.uint64)
    os_, oe, osrc = np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    odt, n, st = np.zeros(2, np.uint64), np.zeros(1, np.uint64), np.zeros(5, np.uint64)
    stop = J.Vocab([b"ab"])

    def call(rule=J.jb_filter_rule(0, 0, 0, 0), stop=None, nbytes=4, cap=2, **over):
        a = dict(text=t.ctypes.data, start=s.ctypes.data, end=e.ctypes.data, dt=dt.ctypes.data, os=os_.ctypes.data,
                 oe=oe.ctypes.data, osrc=osrc.ctypes.data, odt=odt.ctypes.data, n=n.ctypes.data, st=st.ctypes.data,
                 out_cap=2)
        a.update(over)
        return L.jb_filter(a["text"], nbytes, a["start"], a["end"], a["dt"], 2, cap, 1,
                           C.byref(rule) if rule is not None else None, stop.h if stop else None, a["os"], a["oe"],
                           a["osrc"], a["out_cap"], a["odt"], a["n"], a["st"])

    assert call() == J.JB_OK and n[0] == 2
    assert call(osrc=None) == J.JB_OK
    assert call(rule=J.jb_filter_rule(J.JB_FILTER_STOP, 0, 0, 0), stop=stop) == J.JB_OK and n[0] == 1
    # arrays of capacity 0 may be NULL
    assert call(cap=0, start=None, end=None) == J.JB_OK and call(out_cap=0, os=None, oe=None, osrc=None) == J.JB_OK
    assert call(nbytes=0, text=None) == J.JB_OK and n[0] == 0 and st[1] == 2
    for bad in ("text", "start", "end", "dt", "os", "oe", "odt", "n", "st"):
        assert call(**{bad: None}) == J.JB_EINVAL, bad
    assert call(rule=None) == J.JB_EINVAL
    assert call(rule=J.jb_filter_rule(2, 0, 0, 0)) == J.JB_EINVAL  # an unknown flag
    assert call(rule=J.jb_filter_rule(0, 32, 0, 0)) == J.JB_EINVAL  # an unknown class
    assert call(rule=J.jb_filter_rule(J.JB_FILTER_STOP, 0, 0, 0)) == J.JB_EINVAL  # no stop set
    # outputs must not alias inputs
    assert call(os=s.ctypes.data) == J.JB_EINVAL and call(oe=e.ctypes.data) == J.JB_EINVAL
    assert call(osrc=s.ctypes.data) == J.JB_EINVAL and call(os=e.ctypes.data) == J.JB_EINVAL
    assert call(odt=dt.ctypes.data) == J.JB_EINVAL and call(oe=os_.ctypes.data) == J.JB_EINVAL
    assert call(rule=J.jb_filter_rule(0, 0, 256, 0)) == J.JB_ELIMIT and call(rule=J.jb_filter_rule(0, 0, 0, 256)) == J.JB_ELIMIT
    assert call(rule=J.jb_filter_rule(0, 0, 255, 255)) == J.JB_OK
    assert call(nbytes=2 ** 31) == J.JB_ELIMIT
    assert call(cap=2 ** 32 - 2048) == J.JB_ELIMIT
    with pytest.raises(ValueError):
        J.filter_rule(("han", "kana"))
    assert J.filter_rule(("han", "num"), 1, 2, True).drop_classes == 5
