"""CPU: jb_charspans, the host form of the character-offset rule (jieba-go_amd/csrc/jb_charspans.cpp), against
charspans_ref.py for both units, and for valid UTF-8 against Python's own str and UTF-16 indexing;
jb_charspans_work_bytes; the clamps; the limits; in-place output."""
import numpy as np
import pytest

import charspans_ref as CR
import codepoint_cases as CC
import jiebahip as J

UNITS = [J.JB_UNIT_RUNE, J.JB_UNIT_UTF16]
UNTOUCHED = 0xFFFFFFFE  # what jiebahip.charspans leaves in the entries the rule does not write


def test_exports():
    L = J.lib()
    for name in ("jb_charspans_work_bytes", "jb_charspans", "jb_charspans_device", "jb_cut_batch_charspans"):
        assert name in J.EXPORTS and hasattr(L, name), name
    assert (J.JB_UNIT_RUNE, J.JB_UNIT_UTF16, J.JB_CHAR_NONE) == (CR.RUNE, CR.UTF16, CR.NONE)


def host(case, unit, inplace=False):
    return J.charspans(case.text, case.doc_off, case.starts, case.ends, case.doc_tok, unit, ntok=case.ntok, cap=case.cap,
                       inplace=inplace)


def check(case, unit):
    wcs, wce, wun = case.want(unit)
    cs, ce, un = host(case, unit)
    n = len(wcs)
    assert un.tolist() == wun, (case, unit)
    assert cs[:n].tolist() == wcs and ce[:n].tolist() == wce, (case, unit)
    assert (cs[n:] == UNTOUCHED).all() and (ce[n:] == UNTOUCHED).all(), (case, "written past min(ntok, cap)")
    ics, ice, iun = host(case, unit, inplace=True)  # cstart is start, cend is end
    assert ics[:n].tolist() == wcs and ice[:n].tolist() == wce and iun.tolist() == wun, (case, unit, "in place")
    assert ics[n:].tolist() == case.starts[n:].tolist() and ice[n:].tolist() == case.ends[n:].tolist()


def check_python(docs, unit):
    """Valid UTF-8 documents, one span per rune and per pair of runes: the offsets index Python's own str (and
    its UTF-16 form with doubled offsets)."""
    text, off, s, e, tok = CR.rune_spans(docs)
    cs, ce, un = J.charspans(text, off, s, e, tok, unit)
    for d, doc in enumerate(docs):
        u = doc.decode("utf-8")
        u16 = u.encode("utf-16-le")
        assert un[d] == (len(u) if unit == J.JB_UNIT_RUNE else len(u16) // 2)
        for k in range(tok[d], tok[d + 1]):
            piece = doc[s[k] - off[d]:e[k] - off[d]].decode("utf-8")
            if unit == J.JB_UNIT_RUNE:
                assert u[cs[k]:ce[k]] == piece
            else:
                assert u16[2 * cs[k]:2 * ce[k]].decode("utf-16-le") == piece


@pytest.mark.parametrize("unit", UNITS)
def test_against_python_itself(unit):
    docs = ["a中𠀀b😀é", "", "今天天氣很好，ステーションabc", "𠀀𠀀😀", "é", "\U0010FFFF￿ࠀ߿\u0080\x7f\x00",
            "".join(map(chr, CC.T_RUNES))]
    check_python([d.encode() for d in docs], unit)
    buf, off = CC.corpus_D()
    check_python(CC.docs_of(buf, off)[::97], unit)  # (24 consecutive scalars each, a share of them)


@pytest.mark.parametrize("unit", UNITS)
def test_small_shapes(unit):
    check(CR.Case("no document", b"", [0], [], [], [0]), unit)
    check(CR.Case("no document, a token", b"", [0], [0], [0], [0]), unit)
    check(CR.Case("one empty document", b"", [0, 0], [0], [0], [0, 1]), unit)
    check(CR.Case("empty documents in a row", CR.R4 + CR.R3, [0, 0, 0, 4, 4, 4, 7, 7], [0, 4, 0, 7, 7],
                  [4, 7, 0, 7, 7], [0, 0, 0, 1, 2, 3, 4, 5]), unit)
    check(CR.Case("tokens outside every document", b"abcdef", [0, 3, 6], [0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [1, 2, 4]), unit)
    check(CR.Case("a span across two documents", b"abcdef", [0, 3, 6], [2, 2, 3], [4, 3, 4], [0, 2, 3]), unit)
    for rune in (CR.R2, CR.R3, CR.R4, CR.EMOJI):
        check(CR.from_docs("positions inside runes", [b"a" + rune + b"b" + rune, rune], every_byte=True), unit)


@pytest.mark.parametrize("unit", UNITS)
def test_malformed_input(unit):
    docs = [b"a" + m + b"b" + m for m in CR.MALFORMED + CR.TRUNCATED]
    check(CR.from_docs("malformed, one document each", docs, every_byte=True), unit)
    check(CR.from_docs("malformed, one document", [b"".join(docs)], every_byte=True), unit)
    # the example of the header: a document ends in E4 B8, the next begins with 80; three runes of their own
    case = CR.from_docs("E4 B8 | 80", [b"\xe4\xb8", b"\x80"])
    check(case, unit)
    assert case.want(unit) == ([0, 1, 0], [1, 2, 1], [2, 1])
    whole = CR.from_docs("E4 B8 80", [b"\xe4\xb8\x80"])
    assert whole.want(unit) == ([0], [1], [1])
    for trunc in CR.TRUNCATED:
        for ncont in (1, 2, 3):
            check(CR.from_docs("truncated", CR.boundary_docs(20, 0, trunc, ncont), every_byte=True), unit)


_CORPORA = {}


def _corpus_cases(name):
    """The cases over a whole corpus, built once and shared by both units."""
    if name not in _CORPORA:
        buf, off = {"T": CC.corpus_T, "M": CC.corpus_M}[name]()
        docs = CC.docs_of(buf, off)
        _CORPORA[name] = (CR.from_docs(name, docs), CR.from_docs(name + " as one document", [b"".join(docs)]))
    return _CORPORA[name]


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("name", ["T", "M"])
def test_codepoint_corpora(name, unit):
    """corpus_T (every truncation of a rune at a document end) and corpus_M (all 235,904 malformed sequences),
    each whole, as one batch and as one document."""
    for case in _corpus_cases(name):
        check(case, unit)


def test_utf16_counts_two_only_for_valid_astral_runes():
    docs = [CR.R4, CR.EMOJI, b"\xf4\x8f\xbf\xbf", b"\xf0\x90\x80\x80", b"\xf0\x8f\xbf\xbf", b"\xf4\x90\x80\x80", b"\xf0\xa0\x80",
            b"\xef\xbf\xbf"]
    text, off, s, e, tok = CR.rune_spans(docs)
    _, _, un = J.charspans(text, off, s, e, tok, "utf16")
    assert un.tolist() == [2, 2, 2, 2, 4, 4, 3, 1]
    _, _, un = J.charspans(text, off, s, e, tok, "rune")
    assert un.tolist() == [1, 1, 1, 1, 4, 4, 3, 1]


@pytest.mark.parametrize("unit", UNITS)
def test_random_cases_and_clamps(unit):
    kinds = set()
    for seed in range(300):
        case = CR.random_case(seed)
        check(case, unit)
        kinds.add((case.ntok > case.cap, int(case.doc_tok[-1]) > case.ntok, int(case.doc_tok[0]) > 0))
    assert any(k[0] for k in kinds) and any(k[1] for k in kinds) and any(k[2] for k in kinds)


def test_work_bytes():
    prev = 0
    T = J.JB_CHARSPANS_TILE
    for nb in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5, 10 ** 6, 2 ** 30, 2 ** 31 - 1):
        w = J.charspans_work_bytes(nb, 7)
        assert w > 0 and w >= prev
        prev = w
    prev = 0
    for ndocs in (0, 1, 255, 256, 257, 10 ** 6, 2 ** 32 - 1):
        w = J.charspans_work_bytes(1000, ndocs)
        assert w > 0 and w >= prev
        prev = w


def _rc(**kw):
    a = dict(text=b"abc", nbytes=3, off=np.array([0, 3], np.uint64), ndocs=1, s=np.array([0], np.uint32),
             e=np.array([3], np.uint32), d=np.array([0, 1], np.uint64), ntok=1, cap=1, unit=0,
             cs=np.zeros(1, np.uint32), ce=np.zeros(1, np.uint32), un=np.zeros(1, np.uint32))
    a.update(kw)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return J.lib().jb_charspans(a["text"], a["nbytes"], p(a["off"]), a["ndocs"], p(a["s"]), p(a["e"]), p(a["d"]), a["ntok"],
                                a["cap"], a["unit"], p(a["cs"]), p(a["ce"]), p(a["un"]))


def test_limits():
    assert _rc() == J.JB_OK
    assert _rc(unit=2) == J.JB_EINVAL and b"unit" in J.lib().jb_last_error()
    assert _rc(unit=-1) == J.JB_EINVAL
    assert _rc(nbytes=2 ** 31, off=np.array([0, 2 ** 31], np.uint64)) == J.JB_ELIMIT
    assert _rc(cap=2 ** 32 - J.JB_JOIN_TILE) == J.JB_ELIMIT
    for k in ("text", "off", "s", "e", "d", "cs", "ce", "un"):
        assert _rc(**{k: None}) == J.JB_EINVAL, k
    # doc_off: decreasing, not from 0, not up to nbytes
    assert _rc(off=np.array([0, 2, 1, 3], np.uint64), ndocs=3, d=np.array([0, 1, 1, 1], np.uint64),
               un=np.zeros(3, np.uint32)) == J.JB_EINVAL
    assert _rc(off=np.array([1, 3], np.uint64)) == J.JB_EINVAL
    assert _rc(off=np.array([0, 2], np.uint64)) == J.JB_EINVAL
    assert _rc(off=np.array([0, 4], np.uint64)) == J.JB_EINVAL
    # null is fine where the capacity is 0
    assert _rc(s=None, e=None, cs=None, ce=None, cap=0, ntok=0) == J.JB_OK
    assert _rc(s=None, e=None, cs=None, ce=None, cap=0, ntok=5) == J.JB_OK
    assert _rc(text=None, nbytes=0, off=np.array([0, 0], np.uint64), s=np.array([0], np.uint32),
               e=np.array([0], np.uint32)) == J.JB_OK
    assert _rc(text=None, nbytes=0, off=np.array([0], np.uint64), ndocs=0, un=None, d=np.array([0], np.uint64)) == J.JB_OK
    with pytest.raises(ValueError):
        J.charspans(b"abc", [0, 3], [0], [3], [0, 1], "utf8")
