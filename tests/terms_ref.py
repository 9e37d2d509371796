"""Reference for the term-count and keyword calls (jb_terms_device, jb_keywords_device; jiebahip.h),
in numpy: np.unique per document, and np.lexsort over (id, -score).  A helper, not a test."""
import numpy as np

UNK = 0xFFFFFFFF


def terms(ids, doc_tok, ntok, ids_cap):
    """The CSR (term_id u32, term_cnt u32, term_off u64[ndocs + 1]) of an id list: token k takes part iff
    k < min(ntok, ids_cap) and ids[k] != UNK; document d's tokens are [doc_tok[d], doc_tok[d+1]) clamped
    to that bound; its terms are its distinct ids, ascending, with their counts."""
    ids = np.asarray(ids, np.uint32)
    n = min(int(ntok), int(ids_cap))
    tid, tcnt, off = [], [], [0]
    for d in range(len(doc_tok) - 1):
        a, b = min(int(doc_tok[d]), n), min(int(doc_tok[d + 1]), n)
        x = ids[a:b]
        u, c = np.unique(x[x != UNK], return_counts=True)
        tid.append(u.astype(np.uint32))
        tcnt.append(c.astype(np.uint32))
        off.append(off[-1] + len(u))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)  # noqa: E731
    return cat(tid, np.uint32), cat(tcnt, np.uint32), np.array(off, np.uint64)


def keywords(csr, weights, topk):
    """Per document the topk candidates (id < len(weights) and weights[id] > 0) by
    np.float32(cnt) * weights[id] descending, ties by id ascending: (kw_id u32[ndocs, topk],
    kw_score f32, kw_cnt u32, kw_n u32[ndocs]); the slots past kw_n are (UNK, 0.0, 0)."""
    tid, tcnt, off = csr
    w = np.asarray(weights, np.float32)
    nd = len(off) - 1
    kid = np.full((nd, topk), UNK, np.uint32)
    ksc = np.zeros((nd, topk), np.float32)
    kcn = np.zeros((nd, topk), np.uint32)
    kn = np.zeros(nd, np.uint32)
    for d in range(nd):
        i, c = tid[int(off[d]):int(off[d + 1])], tcnt[int(off[d]):int(off[d + 1])]
        inside = i < len(w)
        i, c = i[inside], c[inside]
        with np.errstate(invalid="ignore"):
            cand = w[i] > 0  # (False for NaN)
        i, c = i[cand], c[cand]
        score = c.astype(np.float32) * w[i]
        order = np.lexsort((i, -score))[:topk]
        k = len(order)
        kid[d, :k], ksc[d, :k], kcn[d, :k], kn[d] = i[order], score[order], c[order], k
    return kid, ksc, kcn, kn
