"""The cases both TextRank test files run (test_textrank_host.py on jb_textrank, test_gpu_textrank.py on
jb_textrank_device): id lists with their document offsets, CSR rows and keep masks, and the reference's
answer for each (textrank_ref.py), computed once per case and shared.  A helper, not a test."""
import functools

import numpy as np

import terms_ref as TR
import textrank_ref as KR

UNK = KR.UNK
A, B, C_ = 0, 1, 2  # the hand case's ids


class Case:
    """One call: the arguments of jb_textrank.  term_id / term_off default to the CSR of the id list."""

    def __init__(self, name, docs, keep, span=5, iters=10, topk=20, ntok=None, ids_cap=None, cap=None, csr=None,
                 pad=0):
        self.name = name
        self.ids = np.array([x for d in docs for x in d] + [7] * pad, np.uint32)  # (pad: entries past ntok)
        self.doc_tok = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
        self.keep = np.asarray(keep, np.uint8)
        self.span, self.iters, self.topk = span, iters, topk
        self.ntok = len(self.ids) - pad if ntok is None else ntok
        self.ids_cap = len(self.ids) if ids_cap is None else ids_cap
        if csr is None:
            tid, _, toff = TR.terms(self.ids, self.doc_tok, self.ntok, self.ids_cap)
        else:
            tid, toff = csr
        self.term_id, self.term_off = np.asarray(tid, np.uint32), np.asarray(toff, np.uint64)
        self.cap = len(self.term_id) if cap is None else cap

    def args(self):
        return dict(span=self.span, iters=self.iters, topk=self.topk, ntok=self.ntok, ids_cap=self.ids_cap,
                    cap=self.cap)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _want(case):
    return KR.textrank(case.ids, case.doc_tok, case.term_id, case.term_off, case.keep, **case.args())


def want(case):
    """The reference's (kw_id, kw_score, kw_n) of the case: computed once, not to be changed."""
    return _want(case)


def same(got, case, label):
    """got == the reference bit for bit: ids, f32 score bits and kw_n."""
    wid, wsc, wn = want(case)
    gid, gsc, gn = got
    assert np.array_equal(gn, wn), f"{label} {case}: kw_n differs at {np.flatnonzero(gn != wn)[:5].tolist()}: got " \
                                   f"{gn[gn != wn][:5].tolist()} want {wn[gn != wn][:5].tolist()}"
    bad = np.flatnonzero((gid != wid).any(axis=1) | (gsc.view(np.uint32) != wsc.view(np.uint32)).any(axis=1))
    if len(bad):
        d = int(bad[0])
        raise AssertionError(f"{label} {case}: {len(bad)} rows differ; first document {d}:\n got  {gid[d].tolist()} "
                             f"{gsc[d].tolist()}\n want {wid[d].tolist()} {wsc[d].tolist()}")


ALL = np.ones(64, np.uint8)
HAND = [A, B, A, C_]
# the hand case's matrix and row sums, per span (events: pairs k < j with j - k < span)
HAND_W = {2: {A: {B: 2, C_: 1}, B: {A: 2}, C_: {A: 1}},
          3: {A: {A: 2, B: 2, C_: 1}, B: {A: 2, C_: 1}, C_: {A: 1, B: 1}}}
HAND_OUT = {2: {A: 3, B: 2, C_: 1}, 3: {A: 5, B: 3, C_: 2}}


def zipf_doc(n, seed, vocab=5000):
    rng = np.random.default_rng(seed)
    return (rng.zipf(1.3, n) % vocab).astype(np.uint32).tolist()


def mixed_docs():
    """Documents of every small kind, and a few random ones of 30 to 300 tokens over 40 ids."""
    rng = np.random.default_rng(101)
    keep = np.ones(48, np.uint8)
    keep[[5, 6, 7]] = 0  # the unkept ids; ids 48.. are >= nkeep
    docs = [HAND, [A, A], [3, 4, 3], [], [UNK, UNK, UNK], [5, 6, 7, 5], [1, 50, 2, 60, 1, 2], [9], [8, 5, 8],
            [UNK, 2, UNK, UNK, UNK, UNK, 3, 2]]
    for n in (30, 77, 300):
        d = rng.integers(0, 40, n).astype(np.uint32)
        d[rng.random(n) < 0.1] = UNK
        docs.append(d.tolist())
    return docs, keep


def host_cases():
    """Every case of the issue's list for the host function; the device test runs the same ones."""
    docs, keep = mixed_docs()
    cases = [Case("hand-span2", [HAND], ALL, span=2), Case("hand-span3", [HAND], ALL, span=3),
             Case("self-loop", [[A, A]], ALL, span=2), Case("no-document-has-a-node", [[], [UNK, UNK], [5, 5]], keep)]
    for iters in (0, 1, 10):
        for span in (2, 5, 32):
            for topk in (1, 20, 64):
                cases.append(Case(f"mixed-i{iters}-s{span}-k{topk}", docs, keep, span=span, iters=iters, topk=topk))
    n = sum(len(d) for d in docs)
    # the id array is shorter than the token count says, and the other way round
    cases.append(Case("ids_cap<ntok", docs, keep, ids_cap=n - 150, ntok=n))
    cases.append(Case("ntok<ids_cap", docs, keep, pad=40))
    # an overflowed CSR: the rows that pass cap give kw_n = 0, the others are as before
    full = Case("full", docs, keep)
    cases.append(Case("overflowed-csr", docs, keep, csr=(full.term_id, full.term_off), cap=len(full.term_id) - 45))
    # a caller's CSR that lacks an id: the last document's most frequent id is taken out of its row
    last = np.array(docs[-1], np.uint32)
    vals, cnts = np.unique(last[last != UNK], return_counts=True)
    gone = int(vals[np.argmax(cnts)])
    a, b = int(full.term_off[-2]), int(full.term_off[-1])
    row = full.term_id[a:b]
    tid = np.concatenate([full.term_id[:a], row[row != gone]])
    toff = full.term_off.copy()
    toff[-1] -= 1
    assert keep[gone] and len(tid) == len(full.term_id) - 1
    cases.append(Case("csr-lacks-an-id", docs, keep, csr=(tid, toff)))
    return cases


ZIPF = [(50, 11), (2000, 13), (20_000, 17)]  # (tokens, seed)


def zipf_case(n, seed, **kw):
    keep = (np.random.default_rng(seed + 1).random(5000) < 0.8).astype(np.uint8)
    return Case(f"zipf-{n}", [zipf_doc(n, seed)], keep, **kw)
