"""The collocation rule of include/jiebahip.h in plain Python: dicts over the id list, document by document, and
jiebahip.go_log for the logarithm.  What jb_colloc_count and jb_colloc_score are checked against
(tests/test_colloc_host.py); the device is checked against those (tests/test_gpu_colloc.py)."""
import math

import numpy as np

import jiebahip as J

CONTIG = 1
NPMI, RATIO, COUNT = 0, 1, 2
LIM = 1 << 53


def count(ids, doc_tok, nuni, keep=None, flags=0, starts=None, ends=None, ntok=None, ids_cap=None, nslots=0,
          uni=None, table=None):
    """-> (pairs: dict (a, b) -> count, uni: list of nuni counts, totals: dict).  uni and table, when given, are
    those of earlier batches and are added to; nslots 0 means no limit, else new keys are accepted in token order
    while fewer than nslots // 2 are in the table."""
    ids_cap = len(ids) if ids_cap is None else ids_cap
    ntok = ids_cap if ntok is None else ntok
    n = min(ntok, ids_cap)
    uni = [0] * nuni if uni is None else uni
    table = {} if table is None else table
    keep = [] if keep is None else [int(x) for x in keep]
    known = pairs = dropped = 0

    def kept(t):
        if t >= nuni:
            return False
        return not keep or (t < len(keep) and keep[t] != 0)

    for d in range(len(doc_tok) - 1):
        lo, hi = min(int(doc_tok[d]), n), min(int(doc_tok[d + 1]), n)
        for k in range(lo, hi):
            a = int(ids[k])
            if a < nuni:
                uni[a] += 1
                known += 1
            if k + 1 >= hi:
                continue
            b = int(ids[k + 1])
            if not (kept(a) and kept(b)):
                continue
            if (flags & CONTIG) and int(ends[k]) != int(starts[k + 1]):
                continue
            pairs += 1
            if (a, b) in table:
                table[(a, b)] += 1
            elif nslots == 0 or len(table) < nslots // 2:
                table[(a, b)] = 1
            else:
                dropped += 1
    return table, uni, dict(tokens=n, known=known, pairs=pairs, dropped=dropped, distinct=len(table))


def score_one(a, b, c, uni, nuni, N, scorer, m):
    """The f32 score of a pair, or None when it is no candidate before the threshold."""
    if a >= nuni or b >= nuni or c < m:
        return None
    ca, cb = int(uni[a]), int(uni[b])
    if ca == 0 or cb == 0 or c >= N or max(c, ca, cb, N) >= LIM:
        return None
    if scorer == NPMI:
        pa, pb, pab = ca / N, cb / N, c / N
        s = J.go_log(pab / (pa * pb)) / (0.0 - J.go_log(pab))
    elif scorer == RATIO:
        s = (((c - m) / ca) / cb) * N
    else:
        s = float(c)
    return np.float32(s)


def score(pairs, uni, nuni, N, scorer, m, threshold, topn=0):
    """pairs: iterable of (a, b, c) -> the candidates [(a, b, c, f32 score)] in the rule's order."""
    thr = np.float32(threshold)
    out = []
    for a, b, c in pairs:
        s = score_one(int(a), int(b), int(c), uni, nuni, int(N), scorer, m)
        if s is None or math.isnan(float(s)) or not (s >= thr):
            continue
        out.append((int(a), int(b), int(c), s))
    out.sort(key=lambda r: (-float(r[3]), -r[2], r[0], r[1]))
    return out[:topn] if topn else out
