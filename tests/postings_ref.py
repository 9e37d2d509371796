"""Reference for the postings calls (jb_postings, jb_postings_device, jb_postings_batch; jiebahip.h), twice over:
a plain Python dict of lists filled row by row, and numpy's stable argsort over the participating entries with
searchsorted for the offsets.  The two must agree (tests/test_postings_host.py asks that of every CPU case).
A helper, not a test."""
import numpy as np


def _n(term_off, nterms, cap):
    return min(int(nterms), int(cap), int(term_off[-1]))


def postings_dict(term_id, term_cnt, term_off, nterms, cap, nids, doc_base=0):
    """(post_doc u32, post_tf u32, post_off u64[nids + 1]): the lists of a dict filled row by row, in id order.
    term_off must be non-decreasing from 0."""
    n = _n(term_off, nterms, cap)
    ids, cnts, off = [int(x) for x in term_id[:n]], [int(x) for x in term_cnt[:n]], [int(x) for x in term_off]
    lists = {}
    for d in range(len(off) - 1):
        for i in range(min(off[d], n), min(off[d + 1], n)):
            if ids[i] < nids:
                lists.setdefault(ids[i], []).append(((doc_base + d) & 0xFFFFFFFF, cnts[i]))
    post_off = np.zeros(nids + 1, np.uint64)
    docs, tfs = [], []
    for t in sorted(lists):
        post_off[t + 1] = len(lists[t])
        docs += [p[0] for p in lists[t]]
        tfs += [p[1] for p in lists[t]]
    post_off = np.cumsum(post_off, dtype=np.uint64)
    return np.array(docs, np.uint32), np.array(tfs, np.uint32), post_off


def postings_np(term_id, term_cnt, term_off, nterms, cap, nids, doc_base=0):
    """The same by np.argsort(kind="stable") and np.searchsorted."""
    n = _n(term_off, nterms, cap)
    ids = np.asarray(term_id, np.uint32)[:n].astype(np.int64)
    cnt = np.asarray(term_cnt, np.uint32)[:n]
    off = np.asarray(term_off, np.uint64).astype(np.int64)
    doc = np.searchsorted(off, np.arange(n, dtype=np.int64), side="right") - 1
    take = np.flatnonzero(ids < nids)
    order = take[np.argsort(ids[take], kind="stable")]
    post_off = np.searchsorted(ids[order], np.arange(nids + 1, dtype=np.int64), side="left").astype(np.uint64)
    return ((doc[order] + doc_base) & 0xFFFFFFFF).astype(np.uint32), cnt[order].copy(), post_off


def postings(term_id, term_cnt, term_off, nterms=None, cap=None, nids=0, doc_base=0):
    """postings_np with the lengths defaulted (what the GPU tests compare with)."""
    nterms = len(term_id) if nterms is None else nterms
    cap = len(term_id) if cap is None else cap
    return postings_np(term_id, term_cnt, term_off, nterms, cap, nids, doc_base)


def random_csr(rng, n, ndocs, id_hi, empty=0.3):
    """A CSR of n entries over ndocs rows of random lengths (a share `empty` of them empty), ids random below
    id_hi, counts 1 .. 1000.  Returns (term_id, term_cnt, term_off)."""
    cuts = np.sort(rng.integers(0, n + 1, max(ndocs - 1, 0)))
    if ndocs > 2 and n:  # empty rows: repeat some cut points
        k = rng.random(len(cuts)) < empty
        cuts[k] = cuts[np.maximum(np.flatnonzero(k) - 1, 0)]
        cuts = np.sort(cuts)
    off = np.concatenate([[0], cuts, [n]]).astype(np.uint64) if ndocs else np.zeros(1, np.uint64)
    return rng.integers(0, id_hi, n).astype(np.uint32), rng.integers(1, 1001, n).astype(np.uint32), off
