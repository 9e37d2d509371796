"""CPU: jb_textrank, the host form of the TextRank rule, against textrank_ref.py bit for bit (ids, f32 score
bits, kw_n), the rule's distance from plain f64 Jacobi within its derived bound, and the argument checks of
the TextRank calls.  No kernel is launched here."""
import numpy as np
import pytest

import jiebahip as J
import textrank_cases as TC
import textrank_ref as KR

NEW = ["jb_textrank_work_bytes", "jb_textrank", "jb_textrank_device", "jb_textrank_batch"]
CASES = TC.host_cases()


def host(case):
    return J.textrank(case.ids, case.doc_tok, case.term_id, case.term_off, case.keep, **case.args())


def test_exports():
    L = J.lib()
    for name in NEW:
        assert name in J.EXPORTS and hasattr(L, name), name
    assert J.JB_TR_MAXSPAN == 32 and J.JB_TR_MAXITER == 100


def test_the_hand_case_by_hand():
    """a b a c: W and out as written out in textrank_cases.py, then the scores from them."""
    for span in (2, 3):
        W, out = KR.graph(TC.HAND, TC.ALL, span, lambda x: True)
        assert W == TC.HAND_W[span] and out == TC.HAND_OUT[span]
        ws, S = KR.fixed_ws(TC.HAND_W[span], TC.HAND_OUT[span], 10)
        assert S == 62 - 2  # n = 3
        top = KR.best(KR.scores(ws), 20)
        assert top[0] == (TC.A, 1.0)  # the best node's score is 1 by the normalisation
        kid, ksc, kn = J.textrank(TC.HAND, [0, 4], [0, 1, 2], [0, 3], TC.ALL, span=span)
        assert kn.tolist() == [3] and kid[0, :3].tolist() == [i for i, _ in top]
        assert ksc[0, :3].tolist() == [s for _, s in top]
        assert (kid[0, 3:] == KR.UNK).all() and (ksc[0, 3:] == 0).all()
    # one round by hand, span 2: ws = 1/3 each, S = 60; a gets 2 r[b] + r[c], b gets 2 r[a], c gets r[a]
    ws, _ = KR.fixed_ws(TC.HAND_W[2], TC.HAND_OUT[2], 1)
    third = 1.0 / 3.0
    ra, rb, rc = int(third / 3.0 * 2.0 ** 60), int(third / 2.0 * 2.0 ** 60), int(third / 1.0 * 2.0 ** 60)
    assert ws[TC.A] == (1.0 - 0.85) + 0.85 * (float(2 * rb + rc) * 2.0 ** -60)
    assert ws[TC.B] == (1.0 - 0.85) + 0.85 * (float(2 * ra) * 2.0 ** -60)
    assert ws[TC.C_] == (1.0 - 0.85) + 0.85 * (float(ra) * 2.0 ** -60)


def test_the_self_loop():
    kid, ksc, kn = J.textrank([7, 7], [0, 2], [7], [0, 1], TC.ALL, span=2, topk=3)
    assert kn.tolist() == [1] and kid.tolist() == [[7, KR.UNK, KR.UNK]] and ksc.tolist() == [[1.0, 0.0, 0.0]]
    # a lone token has no event: no node
    kid, ksc, kn = J.textrank([7], [0, 1], [7], [0, 1], TC.ALL, span=2, topk=3)
    assert kn.tolist() == [0] and (kid == KR.UNK).all()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_matches_the_reference_bit_for_bit(case):
    TC.same(host(case), case, "jb_textrank")


def test_the_cases_cover_what_they_say():
    by = {c.name: c for c in CASES}
    wid, _, wn = TC.want(by["mixed-i10-s5-k64"])
    docs, _ = TC.mixed_docs()
    assert wn[0] == 3 and wn[1] == 1  # the hand case and a a
    assert wn[3] == 0 and wn[4] == 0 and wn[5] == 0 and wn[7] == 0  # empty, all-UNK, all-unkept, one token
    assert wn[6] == 2 and set(wid[6, :2].tolist()) == {1, 2}  # ids 50 and 60 are >= nkeep
    assert wn[8] == 1  # 8 _ 8 with span 5: a self loop across an unkept token
    assert 20 < wn.max() < 64  # fewer nodes than topk 64, more than topk 20
    assert (TC.want(by["no-document-has-a-node"])[2] == 0).all()
    full = TC.want(by["mixed-i10-s5-k20"])
    over = TC.want(by["overflowed-csr"])
    assert (over[2][-2:] == 0).all() and over[2][-3] != 0 and np.array_equal(over[0][:-2], full[0][:-2])
    lacks = TC.want(by["csr-lacks-an-id"])
    assert np.array_equal(lacks[0][:-1], full[0][:-1]) and not np.array_equal(lacks[0][-1], full[0][-1])
    short = TC.want(by["ids_cap<ntok"])
    assert np.array_equal(short[1][:-1], full[1][:-1]) and not np.array_equal(short[1][-1], full[1][-1])
    assert np.array_equal(TC.want(by["ntok<ids_cap"])[0], full[0])


def test_two_batches_give_the_rows_of_one():
    """No pair crosses a document boundary: every document alone gives its row of the batch."""
    docs, keep = TC.mixed_docs()
    whole = host(TC.Case("whole", docs, keep, span=32, topk=64))
    for lo, hi in ((0, 6), (6, len(docs))):
        part = host(TC.Case("part", docs[lo:hi], keep, span=32, topk=64))
        for x, y in zip(part, whole):
            assert np.array_equal(x.view(np.uint32), y[lo:hi].view(np.uint32))


@pytest.mark.parametrize("n,seed", TC.ZIPF)
def test_zipf_documents(n, seed):
    """jb_textrank equals the reference on a seeded Zipf document, and the rule stays within its derived
    distance of plain f64 Jacobi: every r is truncated by less than 2^-S, a round's sum over a row by less
    than out * 2^-S, and the error of a round carries into the next damped by 0.85, so the total stays
    under max(out) * 2^-S / (1 - 0.85); 1e-12 * max(ws) covers the f64 rounding of both iterations."""
    case = TC.zipf_case(n, seed)
    TC.same(host(case), case, "jb_textrank")
    ids = case.ids.tolist()
    W, out = KR.graph(ids, case.keep, 5, lambda x: True)
    ws, S = KR.fixed_ws(W, out, 10)
    jac = KR.jacobi_ws(W, out, 10)
    err = max(abs(ws[a] - jac[a]) for a in out)
    bound = max(out.values()) * 2.0 ** -S / (1 - 0.85) + 1e-12 * max(jac.values())
    print(f"zipf {n}: {len(out)} nodes, S = {S}, |ws - jacobi| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # the same top 20 as plain Jacobi wherever Jacobi's 20th and 21st are further apart than the error allows
    order = sorted(jac, key=lambda a: (-jac[a], a))
    if len(order) > 20 and jac[order[19]] - jac[order[20]] > 2 * bound:
        assert {i for i, _ in KR.best(KR.scores(ws), 20)} == set(order[:20])
    # jieba's in-place form, for the record: close, not promised to match
    inp = KR.inplace_ws(W, out, 10)
    top_in = set(sorted(inp, key=lambda a: (-inp[a], a))[:20])
    print(f"zipf {n}: top 20 shared with the in-place form: {len(top_in & set(order[:20]))}")


def raw(case, **kw):
    """jb_textrank itself, its return code included; kw replaces arguments (None: a null pointer)."""
    a = dict(ids=case.ids, doc_tok=case.doc_tok, term_id=case.term_id, term_off=case.term_off, keep=case.keep,
             span=5, iters=10, topk=20, ids_cap=len(case.ids), cap=len(case.term_id))
    a.update(kw)
    nd = len(case.doc_tok) - 1
    out = [np.full(nd * 64, 0x55555555, np.uint32), np.full(nd * 64, np.nan, np.float32), np.full(nd, 0x55555555, np.uint32)]
    p = lambda x: x.ctypes.data if x is not None else None  # noqa: E731
    rc = J.lib().jb_textrank(p(a["ids"]), a["ids_cap"], p(a["doc_tok"]), len(case.ids), nd, p(a["term_id"]),
                             p(a["term_off"]), a["cap"], p(a["keep"]), len(case.keep), a["span"], a["iters"], a["topk"],
                             p(out[0]) if a.get("out", 1) else None, p(out[1]), p(out[2]))
    return rc, out


def test_argument_errors_and_limits():
    docs, keep = TC.mixed_docs()
    case = TC.Case("errors", docs, keep)
    untouched = lambda out: (out[0] == 0x55555555).all() and (out[2] == 0x55555555).all()  # noqa: E731
    for kw, code, word in (({"span": 1}, J.JB_EINVAL, "span"), ({"span": 0}, J.JB_EINVAL, "span"),
                           ({"span": 33}, J.JB_ELIMIT, "JB_TR_MAXSPAN"), ({"iters": 101}, J.JB_ELIMIT, "JB_TR_MAXITER"),
                           ({"topk": 0}, J.JB_EINVAL, "topk"), ({"topk": 65}, J.JB_ELIMIT, "JB_KW_MAXK"),
                           ({"ids": None}, J.JB_EINVAL, "null"), ({"doc_tok": None}, J.JB_EINVAL, "null"),
                           ({"term_id": None}, J.JB_EINVAL, "null"), ({"term_off": None}, J.JB_EINVAL, "null"),
                           ({"keep": None}, J.JB_EINVAL, "null"), ({"out": 0}, J.JB_EINVAL, "null"),
                           ({"ids_cap": 2**32 - 4096}, J.JB_ELIMIT, "id list"), ({"cap": 2**32 - 4096}, J.JB_ELIMIT, "term list")):
        rc, out = raw(case, **kw)
        assert rc == code and word in J.lib().jb_last_error().decode() and untouched(out), kw
    for kw in ({"span": 2}, {"span": 32}, {"iters": 0}, {"iters": 100}, {"topk": 1}, {"topk": 64}):
        rc, out = raw(case, **kw)
        assert rc == J.JB_OK and not untouched(out), kw
    with pytest.raises(J.JbError) as ei:
        J.textrank(case.ids, case.doc_tok, case.term_id, case.term_off, case.keep, span=40)
    assert ei.value.code == J.JB_ELIMIT
    # no document: valid, nothing is written (with or without output pointers)
    assert J.lib().jb_textrank(None, 0, case.doc_tok.ctypes.data, 0, 0, None, case.term_off.ctypes.data, 0, None, 0, 5, 10,
                               20, None, None, None) == J.JB_OK


def test_null_arguments_of_the_device_calls():
    L = J.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    # (a null ctx: nothing can be queued; the limits are reported before it is looked at)
    assert L.jb_textrank_device(None, p, 1, p, p, 1, p, p, 1, p, 1, 5, 10, 20, None, p, p, p, p, 1 << 20) == J.JB_EINVAL
    assert "null" in L.jb_last_error().decode()
    assert L.jb_textrank_device(None, p, 1, p, p, 1, p, p, 1, p, 1, 33, 10, 20, None, p, p, p, p, 1 << 20) == J.JB_ELIMIT
    assert L.jb_textrank_batch(None, p, p, 1, 1, p, 1, 5, 10, 20, p, p, p) == J.JB_EINVAL
    assert L.jb_textrank_batch(None, p, p, 1, 1, p, 1, 5, 10, 0, p, p, p) == J.JB_EINVAL
    assert L.jb_textrank_batch(None, p, p, 1, 1, p, 1, 5, 101, 20, p, p, p) == J.JB_ELIMIT


def test_work_bytes_is_non_decreasing_and_never_zero():
    w = J.textrank_work_bytes
    assert w(0, 0, 0) > 0
    sizes = [0, 1, 255, 256, 257, 4096, 100_000, 2**31]
    for a in sizes:
        for b in sizes:
            for nd in (0, 1, 1000, 2**32 - 1):
                base = w(a, b, nd)
                assert base >= 6 * a + 28 * b + 4 * nd
                assert w(a + 1, b, nd) >= base and w(a, b + 1, nd) >= base and w(a, b, min(nd + 1, 2**32 - 1)) >= base
    assert w(10**6, 10**6, 10) < w(10**7, 10**6, 10) < w(10**7, 10**7, 10) < w(10**7, 10**7, 10**6)
