"""The BM25 rule of include/jiebahip.h (jb_bm25_*) restated in numpy, independent of the library's code but for
the logarithm, which is Go's math.Log as the existing jb_go_log binding gives it.  numpy's float64 arithmetic is
IEEE with one rounding per operation, and every score is a sum of integers, so the library must give these very
bits.  The scores go into a dense u64 matrix with np.add.at; the order is np.lexsort's."""
import numpy as np

import jiebahip as J

MAXQ = 1024
WMAX = np.float32(2.0 ** 20)
UNK = 0xFFFFFFFF


def avgdl(doc_len):
    dl = np.asarray(doc_len, np.uint32)
    return float(np.float64(int(dl.astype(np.uint64).sum())) / np.float64(len(dl)))


def norms(doc_len, k1, b, avg):
    dl = np.asarray(doc_len, np.uint32).astype(np.float64)
    r = dl / np.float64(avg)
    s = (np.float64(1.0) - np.float64(b)) + np.float64(b) * r
    return (np.float64(k1) * s).astype(np.float32)


def idf(post_off, ndocs_total):
    po = [int(x) for x in np.asarray(post_off, np.uint64)]
    out = np.zeros(len(po) - 1, np.float32)
    for t in range(len(po) - 1):
        df = min(po[t + 1] - po[t], ndocs_total) if po[t + 1] > po[t] else 0
        if df:
            q = (np.float64(ndocs_total - df) + np.float64(0.5)) / (np.float64(df) + np.float64(0.5))
            out[t] = np.float32(J.go_log(float(np.float64(1.0) + q)))
    return out


def scores(post_doc, post_tf, post_off, npost, nids, norm, ndocs, weight, nweights, k1, q_id, q_cap, q_off):
    """The dense u64 score matrix [nq, ndocs] and, per query, how many postings contributed (for the bound)."""
    pd, pt = np.asarray(post_doc, np.uint32), np.asarray(post_tf, np.uint32)
    po = [int(x) for x in np.asarray(post_off, np.uint64)]
    nm, wt = np.asarray(norm, np.float32), np.asarray(weight, np.float32)
    qi = np.asarray(q_id, np.uint32)
    qo = [int(x) for x in np.asarray(q_off, np.uint64)]
    nq = len(qo) - 1
    m = np.zeros((nq, ndocs), np.uint64)
    # the same f64 contributions summed without the truncation, for the sanity bound (the adds in extended
    # precision, so that the sum's own rounding stays far below the bound)
    plain = np.zeros((nq, ndocs), np.longdouble)
    nterms = np.zeros((nq, ndocs), np.int64)
    k1p1 = np.float64(k1) + np.float64(1.0)
    for q in range(nq):
        lo, hi = min(qo[q], q_cap), min(qo[q + 1], q_cap)
        for t in qi[lo:max(lo, min(hi, lo + MAXQ))].tolist():
            if t >= nids or t >= nweights:
                continue
            w = wt[t]
            if not (w > 0 and w <= WMAX):
                continue
            a, z = min(po[t], npost), min(po[t + 1], npost)
            if z <= a:
                continue
            d, tf = pd[a:z], pt[a:z]
            ok = (d < ndocs) & (tf > 0)
            d, tf = d[ok], tf[ok]
            ok = nm[d] >= 0
            d, tf = d[ok].astype(np.int64), tf[ok].astype(np.float64)
            x = np.float64(w) * ((tf * k1p1) / (tf + nm[d].astype(np.float64)))
            np.add.at(m[q], d, (x * np.float64(16777216.0)).astype(np.uint64))
            np.add.at(plain[q], d, x.astype(np.longdouble))
            np.add.at(nterms[q], d, 1)
    return m, plain, nterms


def rank(m, topk):
    """The rows of a search from the dense matrix: (res_doc u32[nq, topk], res_score u64[nq, topk], res_n)."""
    nq, ndocs = m.shape
    rd = np.full((nq, topk), UNK, np.uint32)
    rs = np.zeros((nq, topk), np.uint64)
    rn = np.zeros(nq, np.uint32)
    for q in range(nq):
        cand = np.flatnonzero(m[q] > 0)
        order = cand[np.lexsort((cand, ~m[q][cand]))][:topk]  # score descending, then document ascending
        rn[q] = len(order)
        rd[q, :len(order)] = order
        rs[q, :len(order)] = m[q][order]
    return rd, rs, rn


def search(post_doc, post_tf, post_off, npost, nids, norm, ndocs, weight, nweights, k1, q_id, q_cap, q_off, topk):
    m, _, _ = scores(post_doc, post_tf, post_off, npost, nids, norm, ndocs, weight, nweights, k1, q_id, q_cap, q_off)
    return rank(m, topk)


_CACHE = {}


def inputs(c):
    """avgdl, norm and weight of a case of bm25_cases.py by this reference (computed once per case)."""
    key = ("in", c["label"])
    if key not in _CACHE:
        avg = avgdl(c["doc_len"]) if c["ndocs"] else 1.0
        nm = norms(c["doc_len"], c["k1"], c["b"], avg)
        wt = idf(c["post_off"], c["ndocs"]) if c["weight"] is None else np.asarray(c["weight"], np.float32)
        _CACHE[key] = (avg, nm, wt)
    return _CACHE[key]


def matrix(c):
    """The case's dense matrices (scores, plain sums, contributions per cell), computed once per case."""
    key = ("m", c["label"])
    if key not in _CACHE:
        _, nm, wt = inputs(c)
        _CACHE[key] = scores(c["post_doc"], c["post_tf"], c["post_off"], c["npost"], c["nids"], nm, c["ndocs"], wt,
                             c["nweights"], c["k1"], c["q_id"], c["q_cap"], c["q_off"])
    return _CACHE[key]


def want(c, topk):
    key = ("w", c["label"], topk)
    if key not in _CACHE:
        _CACHE[key] = rank(matrix(c)[0], topk)
    return _CACHE[key]
