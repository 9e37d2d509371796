"""Reference for the TextRank calls (jb_textrank, jb_textrank_device; jiebahip.h), in pure Python ints and
floats, written from the rule in the header: the co-occurrence matrix W as a dict, the fixed-point Jacobi
iteration with Python's unbounded ints and IEEE doubles.  It also holds a plain f64 Jacobi and jieba's
in-place update, for the sanity checks.  A helper, not a test."""
import math
import struct

import numpy as np

UNK = 0xFFFFFFFF
D = 0.85


def f32(x):
    """x rounded to f32 (nearest even), as a Python float."""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def row_has(term_id, a, b, x):
    """The binary search of the rule: the first index in [a, b) whose id is >= x holds x."""
    lo, hi = a, b
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if term_id[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo < b and term_id[lo] == x


def graph(ids, keep, span, has):
    """W ({a: {b: weight}}) and out ({a: sum of its row}) of one document's id list; has(id) says whether
    the id is in the document's CSR row."""
    kept = [x != UNK and x < len(keep) and keep[x] != 0 and has(x) for x in ids]
    W = {}
    for k in range(len(ids)):
        if not kept[k]:
            continue
        for j in range(k + 1, min(k + span, len(ids))):
            if not kept[j]:
                continue
            a, b = ids[k], ids[j]
            W.setdefault(a, {}).setdefault(b, 0)
            W[a][b] += 1
            W.setdefault(b, {}).setdefault(a, 0)
            W[b][a] += 1
    out = {a: sum(row.values()) for a, row in W.items()}
    return W, out


def fixed_ws(W, out, iters):
    """The rule's iteration: {node: ws}, and S."""
    n = len(out)
    S = 62 - n.bit_length()
    ws = {a: 1.0 / float(n) for a in out}
    for _ in range(iters):
        r = {a: int((ws[a] / float(out[a])) * 2.0 ** S) for a in out}
        acc = {a: sum(w * r[b] for b, w in W[a].items()) for a in out}
        for a in out:
            assert acc[a] < 1 << 64
            ws[a] = (1.0 - D) + D * (float(acc[a]) * 2.0 ** -S)  # (float(int): to nearest even)
    return ws, S


def jacobi_ws(W, out, iters):
    """Plain f64 Jacobi, sums in sorted order of the neighbour."""
    n = len(out)
    ws = {a: 1.0 / n for a in out}
    for _ in range(iters):
        ws = {a: (1.0 - D) + D * math.fsum(W[a][b] / out[b] * ws[b] for b in sorted(W[a])) for a in out}
    return ws


def inplace_ws(W, out, iters):
    """jieba's UndirectWeightedGraph.rank before the normalisation: in place, in sorted order of the node."""
    n = len(out)
    ws = {a: 1.0 / n for a in out}
    order = sorted(out)
    for _ in range(iters):
        for a in order:
            s = 0.0
            for b in sorted(W[a]):
                s += W[a][b] / out[b] * ws[b]
            ws[a] = (1.0 - D) + D * s
    return ws


def scores(ws):
    """{node: the f32 score}: jieba's normalisation."""
    mn, mx = min(ws.values()), max(ws.values())
    return {a: f32((w - mn / 10.0) / (mx - mn / 10.0)) for a, w in ws.items()}


def best(sc, topk):
    """[(id, score)]: score descending, ties by id ascending."""
    return sorted(sc.items(), key=lambda t: (-t[1], t[0]))[:topk]


def textrank(ids, doc_tok, term_id, term_off, keep, span=5, iters=10, topk=20, ntok=None, ids_cap=None, cap=None):
    """The whole call: (kw_id u32[ndocs, topk], kw_score f32, kw_n u32[ndocs])."""
    ids = [int(x) for x in ids]
    term_id = [int(x) for x in term_id]
    keep = [int(x) for x in keep]
    n_all = min(len(ids) if ntok is None else int(ntok), len(ids) if ids_cap is None else int(ids_cap))
    cap = len(term_id) if cap is None else int(cap)
    nd = len(doc_tok) - 1
    kid = np.full((nd, topk), UNK, np.uint32)
    ksc = np.zeros((nd, topk), np.float32)
    kn = np.zeros(nd, np.uint32)
    for d in range(nd):
        a, b = int(term_off[d]), int(term_off[d + 1])
        if b > cap or a > b:
            continue
        t0, t1 = min(int(doc_tok[d]), n_all), min(int(doc_tok[d + 1]), n_all)
        W, out = graph(ids[t0:t1], keep, span, lambda x: row_has(term_id, a, b, x))
        if not out:
            continue
        ws, _ = fixed_ws(W, out, iters)
        top = best(scores(ws), topk)
        for r, (i, s) in enumerate(top):
            kid[d, r], ksc[d, r] = i, s
        kn[d] = len(top)
    return kid, ksc, kn
