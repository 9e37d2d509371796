"""GPU: character offsets (jb_charspans_device, jb_cut_batch_charspans; jb_charspans.hip) against jb_charspans,
the host form of the rule, and against charspans_ref.py, exactly, in runes and in UTF-16 code units.  Most
tests hand the kernels spans they built themselves, so the conversion is checked independently of
segmentation.  The outputs, doc_units and the work buffer lie between canaries that must not change; the
text's 64 padding bytes are continuation bytes, which a sequence cut short by the text's end must not take."""
import os
import subprocess

import numpy as np
import pytest

import charspans_ref as CR
import codepoint_cases as CC
import full_ref as F
import jiebahip as J
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNITS = [J.JB_UNIT_RUNE, J.JB_UNIT_UTF16]
W, T = CR.W, J.JB_CHARSPANS_TILE
NG = 16                 # canary entries on each side of an output, canary bytes x 4 around the work buffer
FILL = 0xFFFFFFFE       # what the outputs hold before the call (never a result: units stay below 2^31)
CANARY = 0x7A7A7A7A
MODES = [("cut", False), ("cut", True), ("search", True), ("full", False)]


@pytest.fixture(scope="module")
def tk(mini_paths):
    t = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    yield t
    t.close()


@pytest.fixture(scope="module")
def syn_tk(syn_small):
    t = J.Tokenizer(J.make_config(dict_path=syn_small[0], emit_path=syn_small[1]))
    yield t
    t.close()


def _dev(a, dtype, view):
    import torch
    a = np.ascontiguousarray(a, dtype)
    if len(a) == 0:
        a = np.zeros(1, dtype)
    return torch.from_numpy(a.view(view).copy()).cuda()


def _guarded(n, fill):
    """A device array of n u32 entries holding `fill`, between NG canary entries on each side."""
    import torch
    t = torch.full((n + 2 * NG,), fill, dtype=torch.int64, device="cuda").to(torch.int32)  # (fill & 0xFFFFFFFF)
    t[:NG] = CANARY
    t[NG + n:] = CANARY
    return t


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev_text(text, shift=4):
    """The text on the device at an address that is `shift` past a 256-byte boundary, then 64 bytes of 0x80."""
    import torch
    raw = np.concatenate([np.zeros(shift, np.uint8), np.frombuffer(bytes(text), np.uint8), np.full(64, 0x80, np.uint8)])
    d = torch.from_numpy(raw).cuda()
    assert d.data_ptr() % 256 == 0
    return d, d.data_ptr() + shift


def dev_charspans(tk, case, unit, inplace=False, shift=4, work=None, expect_error=None):
    """jb_charspans_device on the case's arrays -> (cstart[cap], cend[cap], doc_units[ndocs]).  The span arrays
    are allocations of exactly cap entries; outputs start as FILL (in place: as the spans) and they, doc_units and
    the work buffer lie between canaries.  work = (missing bytes, misalignment) asks for a bad work buffer."""
    import torch
    nd, cap = len(case.doc_off) - 1, case.cap
    keep, p_text = dev_text(case.text, shift)
    d_off = _dev(case.doc_off, np.uint64, np.int64)
    d_tok = _dev(case.doc_tok, np.uint64, np.int64)
    d_n = torch.tensor([case.ntok], dtype=torch.int64, device="cuda")
    if inplace:
        o_s, o_e = _guarded(cap, 0), _guarded(cap, 0)
        o_s[NG:NG + cap] = _dev(case.starts[:cap], np.uint32, np.int32)[:cap]
        o_e[NG:NG + cap] = _dev(case.ends[:cap], np.uint32, np.int32)[:cap]
        p_s, p_e = o_s.data_ptr() + 4 * NG, o_e.data_ptr() + 4 * NG
    else:
        d_s, d_e = _dev(case.starts[:cap], np.uint32, np.int32), _dev(case.ends[:cap], np.uint32, np.int32)
        o_s, o_e = _guarded(cap, FILL), _guarded(cap, FILL)
        p_s, p_e = d_s.data_ptr(), d_e.data_ptr()
    o_u = _guarded(nd, FILL)
    need = J.charspans_work_bytes(case.nbytes, nd)
    missing, misalign = work or (0, 0)
    wk = torch.full((need + 8 * NG + 8,), 0x5B, dtype=torch.uint8, device="cuda")
    wk[:4 * NG] = 0x7A
    wk[4 * NG + need:] = 0x7A
    args = (p_text, case.nbytes, d_off.data_ptr(), nd, p_s, p_e, d_tok.data_ptr(), d_n.data_ptr(), cap, unit,
            o_s.data_ptr() + 4 * NG, o_e.data_ptr() + 4 * NG, o_u.data_ptr() + 4 * NG, wk.data_ptr() + 4 * NG + misalign,
            need - missing, torch.cuda.current_stream().cuda_stream)
    if expect_error is not None:
        with pytest.raises(J.JbError) as ei:
            tk.charspans_device(*args)
        assert ei.value.code == expect_error
    else:
        tk.charspans_device(*args)
    torch.cuda.synchronize()
    del keep
    s, e, u, wb = _u32(o_s), _u32(o_e), _u32(o_u), wk.cpu().numpy()
    for a, n in ((s, cap), (e, cap), (u, nd)):
        assert (a[:NG] == CANARY).all() and (a[NG + n:] == CANARY).all(), f"{case}: written outside an output"
    assert (wb[:4 * NG] == 0x7A).all() and (wb[4 * NG + need:] == 0x7A).all(), f"{case}: written outside the work buffer"
    return s[NG:NG + cap], e[NG:NG + cap], u[NG:NG + nd]


def check(tk, case, units=UNITS, ref=True, inplace=(False, True), shift=4):
    """device == jb_charspans (== charspans_ref unless ref is False), entry for entry, separate and in place."""
    for unit in units:
        hcs, hce, hun = J.charspans(case.text, case.doc_off, case.starts, case.ends, case.doc_tok, unit, ntok=case.ntok,
                                    cap=case.cap)
        n = min(case.ntok, case.cap)
        if ref:
            wcs, wce, wun = case.want(unit)
            assert hcs[:n].tolist() == wcs and hce[:n].tolist() == wce and hun.tolist() == wun, (case, unit, "jb_charspans")
        for ip in inplace:
            cs, ce, un = dev_charspans(tk, case, unit, inplace=ip, shift=shift)
            label = (case, "utf16" if unit else "rune", "in place" if ip else "separate")
            assert un.tolist() == hun.tolist(), label
            bad = np.flatnonzero((cs[:n] != hcs[:n]) | (ce[:n] != hce[:n]))
            if len(bad):
                k = int(bad[0])
                raise AssertionError(f"{label}: token {k} [{case.starts[k]}, {case.ends[k]}): got ({cs[k]}, {ce[k]}) "
                                     f"want ({hcs[k]}, {hce[k]}); {len(bad)} of {n} differ")
            rest_s, rest_e = (case.starts[n:case.cap], case.ends[n:case.cap]) if ip else (FILL, FILL)
            assert (cs[n:] == rest_s).all() and (ce[n:] == rest_e).all(), (label, "written at or past min(ntok, cap)")


# ---- 1. runes against the word and the tile -----------------------------------------------------------------
@pytest.mark.parametrize("edge", [W, T, 2 * T])
def test_every_rune_byte_first_in_a_word_and_in_a_tile(tk, edge):
    """Runes of width 2, 3 and 4 with each of their bytes in turn at the first byte of a bitmap word / a tile;
    a span from and to every byte, so positions inside the runes too."""
    for rune in (CR.R2, CR.R3, CR.R4, CR.EMOJI):
        for k in range(len(rune)):
            text = CR.at_offset(edge, rune, k)
            assert text[edge - k:edge - k + len(rune)] == rune
            check(tk, CR.from_docs(f"byte {k} of a {len(rune)}-byte rune at {edge}", [text], every_byte=edge == W),
                  inplace=(k % 2 == 1,))


@pytest.mark.parametrize("edge", [W, T])
@pytest.mark.parametrize("trunc", CR.TRUNCATED)
def test_truncated_lead_at_a_document_end(tk, edge, trunc):
    """A document ends in C3, E4 B8 or F0 A0 80 and the next begins with 1 to 3 continuation bytes: every one of
    those bytes is a rune of its own.  The boundary stands at -3 .. +3 around a word and a tile boundary."""
    for ncont in (1, 2, 3):
        for delta in range(-3, 4):
            docs = CR.boundary_docs(edge, delta, trunc, ncont)
            case = CR.from_docs(f"{trunc.hex()} | {ncont} x cont at {edge}{delta:+d}", docs)
            cut = edge + delta
            wcs, wce, wun = case.want(J.JB_UNIT_RUNE)
            # (the model itself: the lead and each continuation byte count one)
            k0 = int(case.doc_tok[1])
            assert case.starts[k0 - len(trunc)] == cut - len(trunc) and wce[k0 - 1] - wcs[k0 - len(trunc)] == len(trunc)
            assert wcs[k0:k0 + ncont] == list(range(ncont)) and case.ends[k0 + ncont - 1] == cut + ncont
            check(tk, case, inplace=((delta + ncont) % 2 == 0,))
            # the same bytes as one document: the sequence is whole again where it is valid
            whole = CR.from_docs("joined", [b"".join(docs)])
            check(tk, whole, inplace=(False,))


def test_text_end_cuts_a_lead_short(tk):
    """The text itself ends in a truncated lead, and the padding after it is continuation bytes."""
    for n in (1, W - 1, W, W + 1, T - 1, T, T + 1):
        for trunc in CR.TRUNCATED:
            if len(trunc) <= n:
                check(tk, CR.from_docs(f"{n} bytes ending in {trunc.hex()}", [CR.filler(n - len(trunc), n) + trunc]),
                      inplace=(False,))


# ---- 2. sizes, documents ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [0, 1, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 5])
def test_text_sizes(tk, nbytes):
    check(tk, CR.from_docs(f"{nbytes} bytes", [CR.filler(nbytes, nbytes)], every_byte=nbytes <= W + 1))
    if nbytes > 1:
        a = nbytes // 3
        check(tk, CR.from_docs(f"{nbytes} bytes in three documents", [CR.filler(a, 1), CR.filler(nbytes - 2 * a, 2),
                                                                      CR.filler(a, 3)]))


def test_no_document_and_one(tk):
    check(tk, CR.Case("no document", b"", [0], [], [], [0]))
    check(tk, CR.Case("no document, tokens", b"", [0], [0, 0], [0, 0], [0]))
    check(tk, CR.Case("one empty document", b"", [0, 0], [0], [0], [0, 1]))
    check(tk, CR.from_docs("one document", [CR.filler(300, 4)]))
    check(tk, CR.Case("one document, no token", CR.filler(300, 4), [0, 300], [], [], [0, 0]))


def test_empty_documents(tk):
    body = [CR.filler(T - 7, 1), CR.filler(14, 2), CR.filler(T + 9, 3)]
    for docs in ([b"", b""] + body, body[:1] + [b"", b"", b""] + body[1:], body + [b"", b""],
                 [b""] + body[:1] + [b""] + body[1:2] + [b"", b""] + body[2:] + [b""]):
        case = CR.from_docs("empty documents", docs)
        # a token of length 0 in every empty document as well
        s, e, tok = case.starts.tolist(), case.ends.tolist(), case.doc_tok.tolist()
        for d in reversed(range(len(docs))):
            if not docs[d]:
                s.insert(tok[d], int(case.doc_off[d]))
                e.insert(tok[d], int(case.doc_off[d]))
                tok[d + 1:] = [x + 1 for x in tok[d + 1:]]
        check(tk, CR.Case("empty documents with tokens", case.text, case.doc_off, s, e, tok))


def test_5000_empty_documents_at_a_tile_boundary(tk):
    """The tile boundary splits a rune, and 5,000 empty documents stand there: the rune's lead ends a document."""
    for k in (0, 1):
        head = CR.at_offset(T, CR.R3, k)[:T]  # (with k = 1 the tile's last byte is the lead of a rune cut short)
        tail = CR.at_offset(T, CR.R3, k)[T:]
        docs = [head] + [b""] * 5000 + [tail, CR.filler(50, 9)]
        text, off, s, e, tok = CR.rune_spans(docs)
        check(tk, CR.Case(f"5000 empty documents, k={k}", text, off, s, e, tok))


# ---- 3. untrusted spans, clamps -----------------------------------------------------------------------------------
def test_malformed_spans_and_clamps(tk):
    kinds = set()
    for seed in range(40):
        case = CR.random_case(seed)
        kinds.add((case.ntok > case.cap, int(case.doc_tok[-1]) > case.ntok, int(case.doc_tok[0]) > 0))
        check(tk, case)
    assert kinds >= {(True, False, False), (False, True, False)} and any(k[2] for k in kinds)
    for seed in (101, 102, 103, 105, 106, 107):  # (the same over several tiles of text)
        check(tk, CR.random_case(seed, nbytes=2 * T + 11 * seed, max_docs=40), inplace=(seed % 2 == 0,))


def test_hand_spans(tk):
    """s > e, e past the document, s before it, s == e, and positions inside a rune, written out."""
    text = "a中𠀀".encode() + "é😀".encode()   # documents [0, 8) and [8, 14)
    s = [0, 1, 2, 4, 5, 8, 3, 0, 6, 8, 9, 10, 12, 14, 7, 8]
    e = [1, 4, 3, 4, 8, 8, 2, 9, 9, 10, 10, 14, 13, 14, 9, 15]
    case = CR.Case("hand", text, [0, 8, 14], s, e, [0, 9, 16])
    N = CR.NONE
    assert case.want(J.JB_UNIT_RUNE) == ([0, 1, 2, 2, 3, 3, N, N, N, 0, 1, 1, 2, 2, N, N],
                                         [1, 2, 2, 2, 3, 3, N, N, N, 1, 1, 2, 2, 2, N, N], [3, 2])
    assert case.want(J.JB_UNIT_UTF16) == ([0, 1, 2, 2, 4, 4, N, N, N, 0, 1, 1, 3, 3, N, N],
                                          [1, 2, 2, 2, 4, 4, N, N, N, 1, 1, 3, 3, 3, N, N], [4, 3])
    check(tk, case)


def test_cap_and_count(tk):
    base = CR.from_docs("cap", [CR.filler(700, 5), CR.filler(T, 6), b"", CR.filler(90, 7)])
    n = len(base.starts)
    for ntok, cap, tok in ((n + 40, n // 2, base.doc_tok), (n // 3, n, base.doc_tok), (n, n, base.doc_tok + np.uint64(5)),
                           (n, n, np.minimum(base.doc_tok * np.uint64(2), np.uint64(n + 9))), (0, n, base.doc_tok),
                           (n, 0, base.doc_tok)):
        check(tk, CR.Case(f"ntok={ntok} cap={cap}", base.text, base.doc_off, base.starts[:cap], base.ends[:cap], tok,
                          ntok=ntok, cap=cap))


def test_bad_work_buffer(tk):
    case = CR.from_docs("work", [CR.filler(300, 8)])
    for work in ((8, 0), (0, 4), (0, 1)):
        for ip in (False, True):
            cs, ce, un = dev_charspans(tk, case, J.JB_UNIT_UTF16, inplace=ip, work=work, expect_error=J.JB_EINVAL)
            # (nothing was queued)
            assert (un == FILL).all()
            assert (cs == (case.starts if ip else FILL)).all() and (ce == (case.ends if ip else FILL)).all()
    with pytest.raises(J.JbError) as ei:
        tk.charspans_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0)
    assert ei.value.code == J.JB_EINVAL


def test_text_alignment(tk):
    case = CR.random_case(104, nbytes=T + 77, max_docs=5)
    for shift in (0, 4, 8, 12, 20):
        check(tk, case, shift=shift, inplace=(False,))


# ---- 4. the real chain ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(syn_small):
    buf, off, _ = syn_small[2].corpus(synth.KIND_DOCS, 3, target_bytes=960 << 10)
    assert int(off[-1]) <= 1 << 20
    return np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(off, np.uint64)


def _cut_device(tk, mode, hmm, d_text, nb, d_off, nd, st):
    if mode == "cut":
        return tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, st)
    if mode == "search":
        return tk.cut_device_search(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, st)
    return tk.cut_device_full(d_text.data_ptr(), nb, d_off.data_ptr(), nd, st)


@pytest.mark.parametrize("mode,hmm", MODES)
def test_real_chain(syn_tk, corpus, mode, hmm):
    """cut_device / cut_device_search / cut_device_full, then charspans_device on the ctx-owned results, for both
    units, against the host rule applied to the same spans."""
    import torch
    buf, off = corpus
    nb, nd = int(off[-1]), len(off) - 1
    d_text = torch.from_numpy(np.concatenate([buf[:nb], np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    ps, pe, pd, pn = _cut_device(syn_tk, mode, hmm, d_text, nb, d_off, nd, st)
    torch.cuda.synchronize()
    ntok = int(J.dev_to_host(pn, 8, np.uint64)[0])
    assert 100_000 < ntok <= nb
    s, e = J.dev_to_host(ps, 4 * ntok, np.uint32), J.dev_to_host(pe, 4 * ntok, np.uint32)
    tok = J.dev_to_host(pd, 8 * (nd + 1), np.uint64)
    need = J.charspans_work_bytes(nb, nd)
    wk = torch.empty(need, dtype=torch.uint8, device="cuda")
    text = bytes(buf[:nb])
    for unit in UNITS:
        o_s, o_e, o_u = _guarded(nb, FILL), _guarded(nb, FILL), _guarded(nd, FILL)
        syn_tk.charspans_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, ps, pe, pd, pn, nb, unit, o_s.data_ptr() + 4 * NG,
                                o_e.data_ptr() + 4 * NG, o_u.data_ptr() + 4 * NG, wk.data_ptr(), need, st)
        torch.cuda.synchronize()
        hcs, hce, hun = J.charspans(text, off, s, e, tok, unit)
        cs, ce, un = _u32(o_s), _u32(o_e), _u32(o_u)
        assert (cs[:NG] == CANARY).all() and (ce[:NG] == CANARY).all() and (cs[NG + nb:] == CANARY).all()
        assert np.array_equal(cs[NG:NG + ntok], hcs) and np.array_equal(ce[NG:NG + ntok], hce)
        assert (cs[NG + ntok:NG + nb] == FILL).all() and (ce[NG + ntok:NG + nb] == FILL).all()
        assert np.array_equal(un[NG:NG + nd], hun) and (hcs != CR.NONE).all()
        # the corpus is valid UTF-8: the offsets index Python's str (a share of the documents)
        for d in range(0, nd, max(1, nd // 40)):
            doc = text[int(off[d]):int(off[d + 1])]
            u = doc.decode("utf-8")
            u16 = u.encode("utf-16-le")
            assert hun[d] == (len(u16) // 2 if unit else len(u))
            for k in range(int(tok[d]), int(tok[d + 1])):
                piece = text[s[k]:e[k]].decode("utf-8")
                got = u16[2 * hcs[k]:2 * hce[k]].decode("utf-16-le") if unit else u[hcs[k]:hce[k]]
                assert got == piece
    # the spans themselves were not touched by the separate-output calls
    assert np.array_equal(J.dev_to_host(ps, 4 * ntok, np.uint32), s)


@pytest.mark.parametrize("unit", UNITS)
def test_every_scalar(tk, unit):
    """codepoint_cases.corpus_S: one document per Unicode scalar value, as one batch, one span per rune."""
    buf, off = CC.corpus_S()
    off = np.ascontiguousarray(off, np.uint64)
    s, e, tok = CR.valid_rune_spans(buf, off)
    case = CR.Case("S", bytes(np.asarray(buf, np.uint8)[:int(off[-1])]), off, s, e, tok)
    check(tk, case, units=[unit], ref=False, inplace=(unit == J.JB_UNIT_UTF16,))
    # the rule, by numpy: token k of document d is rune k - doc_tok[d]; in UTF-16 the runes of four bytes count 2
    hcs, hce, hun = J.charspans(case.text, off, s, e, tok, unit)
    d_of = np.searchsorted(tok, np.arange(len(s)), side="right") - 1
    two = ((e - s) == 4).astype(np.int64) if unit else np.zeros(len(s), np.int64)
    before = np.concatenate([[0], np.cumsum(1 + two)])
    assert np.array_equal(hcs, before[:-1] - before[tok[d_of].astype(np.int64)])
    assert np.array_equal(hce, before[1:] - before[tok[d_of].astype(np.int64)])
    assert np.array_equal(hun, np.diff(before[tok.astype(np.int64)]))
    k = 5000  # (and the Python statement of the rule on the first documents)
    wcs, wce, wun = CR.charspans_ref(case.text, off[:k + 1], s[:int(tok[k])], e[:int(tok[k])], tok[:k + 1], unit)
    assert hcs[:int(tok[k])].tolist() == wcs and hce[:int(tok[k])].tolist() == wce and hun[:k].tolist() == wun


@pytest.mark.parametrize("name", ["T", "M"])
def test_malformed_corpora(tk, name):
    """corpus_T and corpus_M whole: a span of 1 to 4 bytes from every byte, cut at its document's end."""
    buf, off = {"T": CC.corpus_T, "M": CC.corpus_M}[name]()
    off = np.ascontiguousarray(off, np.uint64)
    n = int(off[-1])
    # every byte starts a span of 1 to 4 bytes that stays in its document, so positions inside runes too
    s = np.arange(n, dtype=np.uint32)
    doc_end = off[np.searchsorted(off, s, side="right")].astype(np.uint32)
    e = np.minimum(s + 1 + (s % 4), doc_end).astype(np.uint32)
    tok = off.copy()
    case = CR.Case(name, bytes(np.asarray(buf, np.uint8)[:n]), off, s, e, tok)
    check(tk, case, ref=False, inplace=(False,))
    # the Python statement of the rule: corpus_T whole, of corpus_M every 13th document (each decodes on its own,
    # since a document's end is the limit; jb_charspans meets the whole of M in test_charspans_host.py)
    nd = len(off) - 1
    pick = np.zeros(nd, bool)
    pick[::13 if name == "M" else 1] = True
    lens = np.diff(off.astype(np.int64))
    bytesel = np.repeat(pick, lens)
    sub = np.asarray(buf, np.uint8)[:n][bytesel].tobytes()
    sub_off = np.concatenate([[0], np.cumsum(lens[pick])]).astype(np.uint64)
    sub_s = np.arange(len(sub), dtype=np.uint32)
    sub_e = sub_s + (e - s)[bytesel]
    assert len(sub_off) - 1 >= (18_000 if name == "M" else nd)
    for unit in UNITS:
        hcs, hce, hun = J.charspans(case.text, off, s, e, tok, unit)
        wcs, wce, wun = CR.charspans_ref(sub, sub_off, sub_s, sub_e, sub_off, unit)
        assert hcs[bytesel].tolist() == wcs and hce[bytesel].tolist() == wce and hun[pick].tolist() == wun


# ---- 5. host text in ----------------------------------------------------------------------------------------------
def _host_cut(tk, buf, off, mode, hmm):
    return {"cut": lambda: tk.cut_batch(buf, off, hmm), "search": lambda: tk.cut_batch_search(buf, off, hmm),
            "full": lambda: tk.cut_batch_full(buf, off)}[mode]()


@pytest.mark.parametrize("mode,hmm", MODES)
def test_cut_batch_charspans(syn_tk, corpus, mode, hmm):
    buf, off = corpus
    s, e, d = _host_cut(syn_tk, buf, off, mode, hmm)
    base = int(off[0])
    text = bytes(buf[base:int(off[-1])])
    for unit in UNITS:
        hcs, hce, hun = J.charspans(text, off - off[0], s - np.uint64(base), e - np.uint64(base), d, unit)
        out = None
        for rep in range(2):  # (the second call reuses the arrays and the ctx's buffers)
            cs, ce, tok, un, out = syn_tk.cut_batch_charspans(buf, off, hmm, mode, "utf16" if unit else "rune", out)
            assert np.array_equal(tok, d) and np.array_equal(un, hun)
            assert np.array_equal(cs, hcs) and np.array_equal(ce, hce)
    # a sub-batch that does not start at 0: the offsets are per document, so they are the same
    a, b = 5, 25
    cs, ce, tok, un, _ = syn_tk.cut_batch_charspans(buf, off[a:b + 1], hmm, J._MODES[mode], J.JB_UNIT_RUNE)
    hcs, hce, hun = J.charspans(text, off - off[0], s - np.uint64(base), e - np.uint64(base), d, "rune")
    k0, k1 = int(d[a]), int(d[b])
    assert np.array_equal(tok, d[a:b + 1] - d[a]) and np.array_equal(un, hun[a:b])
    assert np.array_equal(cs, hcs[k0:k1]) and np.array_equal(ce, hce[k0:k1])


def test_cut_batch_charspans_cap_protocol(tk):
    """Arrays that are too small: JB_ELIMIT with the complete count, and nothing written into them."""
    texts = ["今天天氣很好，我昨天去上海", "这一刹那𠀀😀abc"]
    docs = [t.encode() for t in texts]
    buf = np.frombuffer(b"".join(docs) + b"\0" * 16, np.uint8)
    off = np.cumsum([0] + [len(x) for x in docs]).astype(np.uint64)
    s, e, d = tk.cut_batch(buf, off, True)
    n = len(s)
    import ctypes as C
    for cap in (0, 1, n - 1):
        cs, ce = np.full(max(cap, 1), 0xA5A5A5A5, np.uint32), np.full(max(cap, 1), 0xA5A5A5A5, np.uint32)
        tok, un, cnt = np.full(3, 77, np.uint64), np.full(2, 77, np.uint32), C.c_uint64()
        rc = J.lib().jb_cut_batch_charspans(tk.h, buf.ctypes.data, off.ctypes.data, 2, 1, J.JB_MODE_CUT, J.JB_UNIT_RUNE,
                                            cs.ctypes.data, ce.ctypes.data, cap, tok.ctypes.data, C.byref(cnt),
                                            un.ctypes.data)
        assert rc == J.JB_ELIMIT and cnt.value == n
        assert (cs == 0xA5A5A5A5).all() and (ce == 0xA5A5A5A5).all() and (tok == 77).all() and (un == 77).all()
    # the binding grows the arrays and asks again
    out = (np.empty(1, np.uint32), np.empty(1, np.uint32), np.empty(3, np.uint64), np.empty(2, np.uint32))
    cs, ce, tok, un, out = tk.cut_batch_charspans(buf, off, True, "cut", "rune", out)
    assert len(cs) == n and len(out[0]) == n and np.array_equal(tok, d) and un.tolist() == [len(t) for t in texts]
    for mode, unit in ((3, 0), (0, 2)):
        with pytest.raises(J.JbError) as ei:
            tk.cut_batch_charspans(buf, off, True, mode, unit)
        assert ei.value.code == J.JB_EINVAL
    with pytest.raises(J.JbError) as ei:
        tk.cut_batch_charspans(buf, [0, 7, 3], True)
    assert ei.value.code == J.JB_EINVAL
    cs, ce, tok, un, _ = tk.cut_batch_charspans(np.zeros(1, np.uint8), np.zeros(1, np.uint64), True)
    assert len(cs) == 0 and tok.tolist() == [0] and len(un) == 0


def test_cut_batch_charspans_full_mode_regrow(mini_paths):
    """Full mode with more spans than bytes (F.chain_dict(12) on 甲 x 200): the call grows the kept span arrays
    and repeats the cut; a second document shows that the offsets restart."""
    tf = J.Tokenizer(J.make_config(dict_bytes=F.chain_dict(12).encode(), emit_path=mini_paths[1]))
    try:
        docs = [("甲" * 200).encode(), ("𠀀" + "甲" * 150).encode()]
        buf = np.frombuffer(b"".join(docs) + b"\0" * 16, np.uint8)
        off = np.cumsum([0] + [len(x) for x in docs]).astype(np.uint64)
        s, e, d = tf.cut_batch_full(buf, off)
        assert len(s) > int(off[-1])
        text = bytes(buf[:int(off[-1])])
        for unit in UNITS:
            hcs, hce, hun = J.charspans(text, off, s, e, d, unit)
            for rep in range(2):
                cs, ce, tok, un, _ = tf.cut_batch_charspans(buf, off, False, "full", unit)
                assert np.array_equal(tok, d) and np.array_equal(un, hun)
                assert np.array_equal(cs, hcs) and np.array_equal(ce, hce)
            assert hun.tolist() == [200, 151 + unit] and int(hce[int(d[1]):].max()) == 151 + unit
        # the caller's arrays too small for a list that is also longer than the kept arrays: JB_ELIMIT with the
        # complete count, nothing else written
        import ctypes as C
        nfull = len(s)
        cs, ce = np.full(16, 0xA5A5A5A5, np.uint32), np.full(16, 0xA5A5A5A5, np.uint32)
        tok, un, cnt = np.full(3, 77, np.uint64), np.full(2, 77, np.uint32), C.c_uint64()
        rc = J.lib().jb_cut_batch_charspans(tf.h, buf.ctypes.data, off.ctypes.data, 2, 0, J.JB_MODE_FULL, J.JB_UNIT_RUNE,
                                            cs.ctypes.data, ce.ctypes.data, 16, tok.ctypes.data, C.byref(cnt),
                                            un.ctypes.data)
        assert rc == J.JB_ELIMIT and cnt.value == nfull
        assert (cs == 0xA5A5A5A5).all() and (ce == 0xA5A5A5A5).all() and (tok == 77).all() and (un == 77).all()
        # and the plain cut through the same tokenizer afterwards
        s, e, d = tf.cut_batch(buf, off, False)
        cs, ce, tok, un, _ = tf.cut_batch_charspans(buf, off, False, "cut", "rune")
        hcs, hce, _ = J.charspans(text, off, s, e, d, "rune")
        assert np.array_equal(cs, hcs) and np.array_equal(ce, hce) and np.array_equal(tok, d)
    finally:
        tf.close()


def test_cut_batch_charspans_passes_the_cut_errors(mini_paths):
    import search_ref as R
    bad = J.Tokenizer(J.make_config(dict_bytes=R.PLAINW0_DICT.encode(), emit_path=mini_paths[1]))
    try:
        t = "甲乙丙丁戊甲乙丙".encode()  # (an input on which the reference panics)
        for mode in ("cut", "search"):
            with pytest.raises(J.JbError) as ei:
                bad.cut_batch_charspans(np.frombuffer(t + b"\0" * 16, np.uint8), [0, len(t)], False, mode)
            assert ei.value.code == J.JB_EPANIC
        assert [w for w, _, _ in bad.tokenize(["甲乙丙丁"], hmm=False)[0]] == bad.Cut("甲乙丙丁", False)
    finally:
        bad.close()


# ---- 6. tokenize ------------------------------------------------------------------------------------------------
def test_tokenize(tk, kats):
    """jieba's tokenize on the reference's test sentences with an astral rune and an emoji added."""
    texts = [c["text"] for c in kats["cut_real_data"]["cases"]] + [c["text"] for c in kats["split_text"]["cases"]]
    texts = list(dict.fromkeys(t for t in texts if t))
    texts = texts + ["𠀀" + t + "😀" for t in texts] + [t[:len(t) // 2] + "😀𠀀" + t[len(t) // 2:] for t in texts] + ["", "😀"]
    cuts = {"default": tk.Cut, "search": tk.CutForSearch, "full": lambda t, h: tk.CutAll(t)}
    for mode, cut in cuts.items():
        for hmm in (False, True):
            runes = tk.tokenize(texts, mode=mode, hmm=hmm)
            u16 = tk.tokenize(texts, mode=mode, hmm=hmm, unit="utf16")
            assert len(runes) == len(u16) == len(texts)
            for t, toks, toks16 in zip(texts, runes, u16):
                assert [w for w, _, _ in toks] == cut(t, hmm), (mode, hmm, t)
                for (w, a, b), (w16, a16, b16) in zip(toks, toks16):
                    assert w == t[a:b] and 0 <= a < b <= len(t), (mode, hmm, t, w, a, b)
                    assert w16 == w and a16 == len(t[:a].encode("utf-16-le")) // 2
                    assert b16 == len(t[:b].encode("utf-16-le")) // 2
    # (an emoji is a token only in a block with an alnum byte, as in Cut)
    assert tk.tokenize(["𠀀今天a😀天氣"], hmm=False)[0] == [("𠀀", 0, 1), ("今天", 1, 3), ("a", 3, 4), ("😀", 4, 5), ("天", 5, 6),
                                                           ("氣", 6, 7)]
    assert tk.tokenize(["𠀀今天a😀天氣"], hmm=False, unit="utf16")[0] == [("𠀀", 0, 2), ("今天", 2, 4), ("a", 4, 5), ("😀", 5, 7),
                                                                         ("天", 7, 8), ("氣", 8, 9)]
    t = "我爱𠀀北京😀天安门"
    assert tk.tokenize([t], hmm=False)[0] == [(t[a:b], a, b) for a, b in zip(*_rune_bounds(tk, t))]
    assert tk.tokenize([]) == []
    with pytest.raises(ValueError):
        tk.tokenize(["a"], mode="cut")
    with pytest.raises(ValueError):
        tk.tokenize(["a"], unit="utf8")


def _rune_bounds(tk, t):
    """The token bounds of Cut(t, False) in characters, from the words themselves."""
    a, b, p = [], [], 0
    for w in tk.Cut(t, False):
        p = t.index(w, p)
        a.append(p)
        b.append(p + len(w))
        p += len(w)
    return a, b


# ---- 7. run to run, the profile -----------------------------------------------------------------------------------
def test_run_to_run_identity(syn_tk, syn_small):
    """8 MiB of text, the same call three times: identical spans, counts and lengths."""
    buf, off, _ = syn_small[2].corpus(synth.KIND_DOCS, 5, target_bytes=8 << 20)
    buf, off = np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(off, np.uint64)
    first = None
    out = None
    for rep in range(3):
        cs, ce, tok, un, out = syn_tk.cut_batch_charspans(buf, off, True, "cut", "utf16", out)
        got = (cs.copy(), ce.copy(), tok.copy(), un.copy())
        if first is None:
            first = got
            assert len(cs) > 500_000 and int(un.sum()) > 2_000_000 and (cs <= ce).all()
        else:
            assert all(np.array_equal(x, y) for x, y in zip(first, got))


def test_profile_lists_the_kernels(tk):
    case = CR.from_docs("profile", [CR.filler(3 * T, 17)])
    tk.profile(True)
    try:
        tk.profile_reset()
        dev_charspans(tk, case, J.JB_UNIT_UTF16)
        prof = tk.profile_read()
    finally:
        tk.profile(False)
    for k in ("k_cs_class", "k_cs_scan", "k_cs_lookup"):
        assert prof[k][1] == 1, prof


def test_cpp_consumer(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "cpp_charspans_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_charspans_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "charspans ok" in r.stdout, r.stdout + r.stderr
