"""CPU: the BM25 rule on host arrays (jb_bm25_avgdl, jb_bm25_norms, jb_bm25_idf, jb_bm25_search;
jieba-go_amd/csrc/jb_bm25.cpp) against bm25_ref.py's numpy restatement on every case of bm25_cases.py, bit for
bit; a derived bound against the plain f64 sum; the size helper; every argument error."""
import ctypes as C

import numpy as np
import pytest

import bm25_cases as BC
import bm25_ref as BR
import jiebahip as J

CASES = list(BC.all_cases())
assert J.JB_BM25_TILE == BC.TILE and J.JB_BM25_MAXQ == BC.MAXQ and J.JB_BM25_WMAX == float(BR.WMAX)


def host(c, topk):
    _, nm, wt = BR.inputs(c)
    return J.bm25_search(c["post_doc"], c["post_tf"], c["post_off"], nm, wt, c["k1"], c["q_id"], c["q_off"], topk,
                         npost=c["npost"], nids=c["nids"], ndocs=c["ndocs"], nweights=c["nweights"], q_cap=c["q_cap"])


@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_norms_and_weights_are_the_reference_bits(c):
    avg, nm, _ = BR.inputs(c)
    if c["ndocs"]:
        assert J.bm25_avgdl(c["doc_len"]) == avg
    got = J.bm25_norms(c["doc_len"], c["k1"], c["b"], avg)
    assert got.tobytes() == nm.tobytes()
    for n in (c["ndocs"], 1, 10 ** 9, (1 << 53) - 1):
        assert J.bm25_idf(c["post_off"], n).tobytes() == BR.idf(c["post_off"], n).tobytes(), n


@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_search_is_the_reference(c):
    for topk in c["topks"]:
        rd, rs, rn = host(c, topk)
        wd, ws, wn = BR.want(c, topk)
        assert np.array_equal(rn, wn), (topk, rn, wn)
        assert np.array_equal(rd, wd) and np.array_equal(rs, ws), topk
    m = BR.matrix(c)[0]
    if c["label"] == "ties":  # topk cuts inside a tie that crosses the tiles: the lowest documents win
        rd, rs, rn = host(c, 10)
        assert rn[0] == 10 and rd[0].tolist() == list(range(10)) and len(set(rs[0].tolist())) == 1
        assert (m[0] == m[0][0]).all()
    if c["label"] == "ties-small":
        assert host(c, 64)[2][0] == 50  # fewer candidates than topk
    if c["label"].startswith("ndocs=") and c["ndocs"] > 1:
        assert not m[1].any() and not m[2].any() and m[4].any()  # empty, unknown ids only, the long query
        assert np.array_equal(m[3], 3 * BR.scores(c["post_doc"], c["post_tf"], c["post_off"], c["npost"], c["nids"],
                                                  BR.inputs(c)[1], c["ndocs"], BR.inputs(c)[2], c["nweights"], c["k1"],
                                                  np.array([3], np.uint32), 1, np.array([0, 1], np.uint64))[0][0])


def test_the_cases_reach_what_they_are_for():
    by = {c["label"]: c for c in CASES}
    m = BR.matrix(by["weights"])[0]
    assert not m[0].any() and not m[3].any(), "weights 0 and +Inf do not take part"
    w6 = BR.scores(*[by["weights"][k] for k in ("post_doc", "post_tf", "post_off", "npost", "nids")],
                   BR.inputs(by["weights"])[1], by["weights"]["ndocs"], BR.inputs(by["weights"])[2], BC.NIDS,
                   by["weights"]["k1"], np.array([6, 5, 1, 2], np.uint32), 4, np.array([0, 1, 4], np.uint64))[0]
    assert w6[0].any() and not w6[1].any(), "JB_BM25_WMAX itself takes part; above it, negative and NaN do not"
    c = by["offsets-decrease"]
    last = BR.matrix(c)[0][-1]
    alone = BR.scores(c["post_doc"], c["post_tf"], c["post_off"], c["npost"], c["nids"], BR.inputs(c)[1], c["ndocs"],
                      BR.inputs(c)[2], c["nweights"], c["k1"], np.array([2], np.uint32), 1, np.array([0, 1], np.uint64))[0][0]
    assert last.any() and np.array_equal(last, alone), "the id whose offsets decrease has no postings"
    c = by["ndocs=%d" % (2 * BC.TILE + 3)]
    long_q = BR.matrix(c)[2][4]
    po = c["post_off"].astype(np.int64)
    n14 = np.bincount(c["post_doc"][po[1]:po[5]], minlength=c["ndocs"])  # how many of the ids 1 .. 4 a document holds
    assert np.array_equal(long_q, n14 * (BC.MAXQ // 4)), "each of the four ids counts MAXQ / 4 times and id 6 never"
    assert (n14[c["post_doc"][po[6]:po[7]]] == 0).any(), "some document holds id 6 and none of the four"
    assert BR.matrix(by["k1=0"])[0].any() and BR.matrix(by["tf=0"])[0].any()
    assert (BR.want(by["docs>=ndocs"], 10)[0][BR.want(by["docs>=ndocs"], 10)[0] != BC.UNK] < 260).all()


@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_score_is_within_the_truncation_of_the_plain_sum(c):
    """Derived, not measured.  A contribution is x = w * (num / den) in f64 and the score adds trunc(x * 2^24):
    the multiplication by 2^24 only changes the exponent and the u64 sum is exact, so each contribution loses less
    than 2^-24 and gains nothing.  The reference sums the same f64 x without the truncation (in extended
    precision: at most 1024 adds of values below 2^27, each within 2^-64 of the running sum, far below 1e-9).  So
    score / 2^24 lies within nterms * 2^-24 below the plain sum and no more than 1e-9 above it."""
    m, plain, nterms = BR.matrix(c)
    if not m.size:
        return
    rd, rs, rn = host(c, 64)
    for q in range(len(rn)):
        for r in range(int(rn[q])):
            d = int(rd[q, r])
            got = np.longdouble(int(rs[q, r])) / np.longdouble(2.0 ** 24)
            assert plain[q, d] - nterms[q, d] * np.longdouble(2.0 ** -24) <= got <= plain[q, d] + np.longdouble(1e-9), (q, d)


def test_work_bytes():
    f = J.bm25_work_bytes
    assert f(0, 0, 0) > 0 and f(0, 0, 1) > 0
    last = 0
    for n in (0, 1, BC.TILE - 1, BC.TILE, BC.TILE + 1, 10 * BC.TILE, 1 << 27, 0xFFFFFFFF):
        cur = f(7, n, 10)
        assert cur >= last and cur >= 7 * n * 8
        assert f(8, n, 10) >= cur and f(7, n, 64) >= cur and f(7, n, 11) >= cur
        last = cur
    for nq in (0, 1, 1000, 0xFFFFFFFF):
        assert f(nq, 0xFFFFFFFF, 64) >= f(nq, 70000, 64) >= f(nq, 70000, 1) > 0
    assert f(1024, 73443, 10) >= 1024 * 73443 * 8 + 1024 * 9 * (10 * 12 + 4)


def test_errors():
    L = J.lib()
    pd, pt, po = np.array([0, 1], np.uint32), np.array([1, 2], np.uint32), np.array([0, 2], np.uint64)
    nm, wt = np.array([1.0, 1.0], np.float32), np.array([1.0], np.float32)
    qi, qo = np.array([0], np.uint32), np.array([0, 1], np.uint64)
    rd, rs, rn = np.zeros(3, np.uint32), np.zeros(3, np.uint64), np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(pd_=p(pd), pt_=p(pt), po_=p(po), npost=2, nids=1, nm_=p(nm), ndocs=2, wt_=p(wt), nw=1, k1=1.2, qi_=p(qi), qcap=1,
             qo_=p(qo), nq=1, topk=3, rd_=p(rd), rs_=p(rs), rn_=p(rn)):
        return L.jb_bm25_search(pd_, pt_, po_, npost, nids, nm_, ndocs, wt_, nw, k1, qi_, qcap, qo_, nq, topk, rd_, rs_, rn_)

    assert call() == J.JB_OK and rn[0] == 2 and rd.tolist() == [1, 0, J.JB_ID_UNK] and rs[2] == 0 and rs[0] > rs[1] > 0
    for kw in (dict(pd_=None), dict(pt_=None), dict(po_=None), dict(nm_=None), dict(wt_=None), dict(qi_=None),
               dict(qo_=None), dict(rd_=None), dict(rs_=None), dict(rn_=None)):
        assert call(**kw) == J.JB_EINVAL, kw
    # arrays of capacity 0 may be NULL
    assert call(pd_=None, pt_=None, npost=0) == J.JB_OK and rn[0] == 0
    assert call(nm_=None, ndocs=0) == J.JB_OK and rn[0] == 0
    assert call(wt_=None, nw=0) == J.JB_OK and rn[0] == 0
    assert call(qi_=None, qcap=0) == J.JB_OK and rn[0] == 0
    assert call(rd_=None, rs_=None, rn_=None, nq=0) == J.JB_OK
    # an output that is an input or another output
    assert call(rd_=p(pd)) == J.JB_EINVAL and call(rd_=p(qi)) == J.JB_EINVAL and call(rs_=p(po)) == J.JB_EINVAL
    assert call(rn_=p(pt)) == J.JB_EINVAL and call(rn_=p(rd)) == J.JB_EINVAL and call(rs_=p(qo)) == J.JB_EINVAL
    assert b"output" in L.jb_last_error()
    # the limits
    assert call(topk=0) == J.JB_EINVAL and call(topk=J.JB_KW_MAXK + 1) == J.JB_ELIMIT
    big = [np.zeros(64, np.uint32), np.zeros(64, np.uint64)]
    assert call(topk=64, rd_=p(big[0]), rs_=p(big[1])) == J.JB_OK
    for k1 in (-0.5, 64.5, float("nan"), float("inf")):
        assert call(k1=k1) == J.JB_EINVAL, k1
    assert call(k1=0.0) == J.JB_OK and call(k1=64.0) == J.JB_OK
    # the parameters of the norms and the weights
    dl, out = np.array([3, 5], np.uint32), np.zeros(2, np.float32)
    norms = lambda k1=1.2, b=0.75, avg=4.0, dl_=p(dl), n=2, out_=p(out): L.jb_bm25_norms(dl_, n, k1, b, avg, out_)  # noqa: E731
    assert norms() == J.JB_OK
    for kw in (dict(k1=-1.0), dict(k1=65.0), dict(k1=float("nan")), dict(b=-0.1), dict(b=1.1), dict(b=float("nan")),
               dict(avg=0.0), dict(avg=-1.0), dict(avg=float("inf")), dict(avg=float("nan")), dict(dl_=None),
               dict(out_=None), dict(out_=p(dl))):
        assert norms(**kw) == J.JB_EINVAL, kw
    assert norms(dl_=None, out_=None, n=0) == J.JB_OK
    av = C.c_double()
    assert L.jb_bm25_avgdl(p(dl), 2, C.byref(av)) == J.JB_OK and av.value == 4.0
    assert L.jb_bm25_avgdl(p(dl), 0, C.byref(av)) == J.JB_EINVAL
    assert L.jb_bm25_avgdl(p(np.zeros(2, np.uint32)), 2, C.byref(av)) == J.JB_EINVAL
    assert L.jb_bm25_avgdl(p(dl), 2, None) == J.JB_EINVAL and L.jb_bm25_avgdl(None, 2, C.byref(av)) == J.JB_EINVAL
    big_len = np.full(3, 0xFFFFFFFF, np.uint32)  # the sum is taken in 64 bits
    assert L.jb_bm25_avgdl(p(big_len), 3, C.byref(av)) == J.JB_OK and av.value == float(0xFFFFFFFF)
    w = np.zeros(1, np.float32)
    assert L.jb_bm25_idf(p(po), 1, 2, p(w)) == J.JB_OK and w[0] == np.float32(J.go_log(1.0 + 0.5 / 2.5))
    assert L.jb_bm25_idf(p(po), 1, 1 << 53, p(w)) == J.JB_ELIMIT and L.jb_bm25_idf(p(po), 1, (1 << 53) - 1, p(w)) == J.JB_OK
    assert L.jb_bm25_idf(None, 1, 2, p(w)) == J.JB_EINVAL and L.jb_bm25_idf(p(po), 1, 2, None) == J.JB_EINVAL
    assert L.jb_bm25_idf(p(po), 0, 2, None) == J.JB_OK
    down = np.array([5, 2, 9], np.uint64)  # offsets that decrease: df 0; a list longer than the corpus: df = ndocs_total
    w2 = np.ones(2, np.float32)
    assert L.jb_bm25_idf(p(down), 2, 3, p(w2)) == J.JB_OK and w2[0] == 0 and w2[1] == np.float32(J.go_log(1.0 + 0.5 / 3.5))
