"""CPU: jb_colloc_count and jb_colloc_score, the host form of the collocation rule (jieba-go_amd/csrc/
jb_colloc.cpp), against colloc_ref.py on the cases the GPU tests run (colloc_cases.py): pairs, unigrams, totals,
the drop behaviour, the three scorers with thresholds at and one ulp above a score, the order, the size helpers'
monotonicity and every argument error."""
import ctypes as C

import numpy as np
import pytest

import colloc_cases as CC
import colloc_ref as CR
import jiebahip as J

CASES = list(CC.all_cases())
SCORES = list(CC.score_cases())
_WANT = {}


def want_of(c):
    """The reference over a case's batches, computed once: (pairs, uni, totals)."""
    if c["label"] not in _WANT:
        table, uni, tot = {}, [0] * c["nuni"], dict(tokens=0, known=0, pairs=0, dropped=0, distinct=0)
        for b in c["batches"]:
            table, uni, t = CR.count(b["ids"], b["doc_tok"], c["nuni"], c["keep"], c["flags"], b["starts"], b["ends"],
                                     b["ntok"], b["ids_cap"], c["nslots"] if c["drops"] else 0, uni, table)
            for k in ("tokens", "known", "pairs", "dropped"):
                tot[k] += t[k]
            tot["distinct"] = t["distinct"]
        _WANT[c["label"]] = (table, uni, tot)
    return _WANT[c["label"]]


def host(c):
    """jb_colloc_count over a case's batches, merged in Python: (pairs, uni, totals).  A case with drops has one batch."""
    uni = np.zeros(c["nuni"], np.uint64)
    table, tot = {}, dict(tokens=0, known=0, pairs=0, dropped=0, distinct=0)
    for b in c["batches"]:
        r = J.colloc_count(b["ids"], b["doc_tok"], uni, c["keep"], c["flags"], b["starts"], b["ends"], b["ntok"],
                           b["ids_cap"], c["nslots"] if c["drops"] else 0)
        keys = list(zip(r.a.tolist(), r.b.tolist()))
        assert keys == sorted(keys) and len(set(keys)) == len(keys), "sorted by key, each key once"
        assert r.score.tolist() == [float(np.float32(x)) for x in r.count.tolist()]
        assert r.distinct == len(keys)
        for k, n in zip(keys, r.count.tolist()):
            table[k] = table.get(k, 0) + n
        for k, v in zip(("tokens", "known", "pairs", "dropped"), r.totals()):
            tot[k] += v
    tot["distinct"] = len(table)
    return table, uni.tolist(), tot


def test_exports_and_constants():
    L = J.lib()
    for name in ("jb_colloc_table_bytes", "jb_colloc_work_bytes", "jb_colloc_init_device", "jb_colloc_add_device",
                 "jb_colloc_score_device", "jb_colloc_read", "jb_colloc_result_free", "jb_colloc_count",
                 "jb_colloc_score", "jb_colloc_batch"):
        assert name in J.EXPORTS and hasattr(L, name), name
    assert (J.JB_COLLOC_TILE, J.JB_COLLOC_LDS, J.JB_COLLOC_SHARE) == (CC.TILE, CC.LDS, CC.SHARE)
    assert (J.JB_COLLOC_NPMI, J.JB_COLLOC_RATIO, J.JB_COLLOC_COUNT) == (CR.NPMI, CR.RATIO, CR.COUNT)
    assert J.JB_COLLOC_CONTIG == CR.CONTIG == CC.CONTIG and J.JB_ID_UNK == CC.UNK


@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_count_is_the_reference(c):
    wt, wu, wtot = want_of(c)
    gt, gu, gtot = host(c)
    assert gtot == wtot, f"totals {gtot}, want {wtot}"
    assert gu == wu, "uni differs"
    assert gt == wt, "pairs differ"
    assert sum(gt.values()) + gtot["dropped"] == gtot["pairs"] and sum(gu) == gtot["known"]


def test_cases_cover_what_they_claim():
    by = {c["label"]: c for c in CASES}
    t, u, tot = want_of(by["one hot pair"])
    assert t == {(2, 2): 4 * CC.T - 1} and u == [0, 0, 4 * CC.T] and tot["dropped"] == 0
    t, u, tot = want_of(by["documents of 1 and 2 tokens"])
    assert t == {(1, 2): 2}  # documents [0] [1 2] [0] [1 2]
    assert tot["pairs"] == 2 and tot["known"] == 6
    t, u, tot = want_of(by["nslots=8"])
    assert tot["distinct"] == 4 and tot["dropped"] > 0
    assert want_of(by["nuni=0"])[2] == dict(tokens=CC.T + 77, known=0, pairs=0, dropped=0, distinct=0)
    a = want_of(by["contiguous over gaps and overlaps"])[2]["pairs"]
    b = want_of(by["the same spans without the flag"])[2]["pairs"]
    assert 0 < a < b and want_of(by["null spans without the flag"])[0] == want_of(by["the same spans without the flag"])[0]
    assert want_of(by["tokens of no document"])[2]["known"] == CC.T + 21 - 7
    assert want_of(by["ntok above ids_cap"])[2]["tokens"] == 2 * CC.T + 9
    assert want_of(by["ids_cap below the list"])[2]["tokens"] == CC.T + 3
    for n in (CC.T, CC.T + 1, 3 * CC.T + 5):  # no pair straddles a boundary, whatever the run of empty documents
        ids = by[f"edges ntok={n}"]["batches"][0]["ids"]
        t = want_of(by[f"edges ntok={n}"])[0]
        inside = sum(1 for k in range(n - 1) if k + 1 not in (CC.T - 1, CC.T, CC.T + 1))
        assert sum(t.values()) == inside and len(ids) == n


def _cand(r):
    return list(zip(r.a.tolist(), r.b.tolist(), r.count.tolist(), r.score.tolist()))


def _ref(rows):
    return [(a, b, c, float(s)) for a, b, c, s in rows]


@pytest.mark.parametrize("c", SCORES, ids=[c["label"] for c in SCORES])
def test_score_is_the_reference(c):
    rows = list(zip(c["a"].tolist(), c["b"].tolist(), c["count"].tolist()))
    for scorer in (CR.NPMI, CR.RATIO, CR.COUNT):
        full = CR.score(rows, c["uni"], c["nuni"], c["N"], scorer, c["m"], -np.inf)
        got = J.colloc_score(c["a"], c["b"], c["count"], c["uni"], c["N"], scorer, c["m"], -np.inf, nuni=c["nuni"])
        assert _cand(got) == _ref(full), f"scorer {scorer}"
        thresholds = [np.nan, np.inf, 0.0]
        for _, _, _, s in full:  # at a pair's f32 score and one ulp above it
            thresholds += [s, np.nextafter(s, np.float32(np.inf))]
        for thr in thresholds:
            want = CR.score(rows, c["uni"], c["nuni"], c["N"], scorer, c["m"], thr)
            got = J.colloc_score(c["a"], c["b"], c["count"], c["uni"], c["N"], scorer, c["m"], float(thr), nuni=c["nuni"])
            assert _cand(got) == _ref(want), f"scorer {scorer} threshold {thr}"
        for topn in (1, 3, 1000):
            got = J.colloc_score(c["a"], c["b"], c["count"], c["uni"], c["N"], scorer, c["m"], -np.inf, topn, nuni=c["nuni"])
            assert _cand(got) == _ref(full[:topn])


def test_score_cases_cover_what_they_claim():
    by = {c["label"]: c for c in SCORES}
    c = by["hand-made"]
    rows = list(zip(c["a"].tolist(), c["b"].tolist(), c["count"].tolist()))
    full = CR.score(rows, c["uni"], c["nuni"], c["N"], CR.RATIO, c["m"], -np.inf)
    keys = {(a, b) for a, b, _, _ in full}
    assert (0, 1) in keys and [s for a, b, n, s in full if (a, b, n) == (0, 1, c["m"])] == [0.0]  # c = m scores 0
    assert len([1 for a, b, n, _ in full if (a, b) == (0, 1)]) == 1  # c = m - 1 is out
    for k in ((0, 2), (2, 0), (0, 4), (1, 3), (0, 3)):  # ca or cb 0, a count of 2^53, c >= N
        assert k not in keys
    assert (0, 0) in keys  # c = N - 1
    small = CR.score(rows, c["uni"], 6, c["N"], CR.RATIO, c["m"], -np.inf)
    assert {(a, b) for a, b, _, _ in small} == {k for k in keys if max(k) < 6} != keys
    npmi = CR.score(rows, c["uni"], c["nuni"], c["N"], CR.NPMI, c["m"], -np.inf)
    sane = [s for a, b, n, s in npmi if n <= min(int(c["uni"][a]), int(c["uni"][b]))]  # (counts a corpus can give)
    assert len(sane) >= 5 and all(-1.0 <= s <= 1.0 for s in sane)
    t = by["ties"]
    rows = list(zip(t["a"].tolist(), t["b"].tolist(), t["count"].tolist()))
    got = CR.score(rows, t["uni"], t["nuni"], t["N"], CR.RATIO, t["m"], -np.inf)
    order = [(a, b) for a, b, _, _ in got]
    assert order.index((4, 5)) < order.index((5, 4)) < order.index((2, 3)) < order.index((3, 2))  # count, then key
    assert got[order.index((4, 5))][3] == got[order.index((2, 3))][3]
    assert CR.score(rows, t["uni"], t["nuni"], 1 << 53, CR.COUNT, 1, -np.inf) == []


def test_size_helpers():
    tb, wb = J.colloc_table_bytes, J.colloc_work_bytes
    assert tb(0) > 0 and wb(0, 0) > 0
    last = 0
    for n in (0, 1, 7, 8, 9, 1000, 1024, 1025, 1 << 20, (1 << 30) - 1, 1 << 30, 1 << 31, 1 << 50, (1 << 64) - 1):
        assert tb(n) >= last
        last = tb(n)
    assert tb(1024) == 256 + 16 * 1024 and tb(9) == tb(16)
    last = 0
    for n in (0, 1, 255, 256, 257, 100000, 1 << 32, 1 << 61, (1 << 64) - 1):
        assert wb(n, 0) >= last and wb(n, 0) <= wb(n, 5) <= wb(n, (1 << 32) - 1)
        last = wb(n, 0)
    assert wb(1000, 3) >= 1000 * 4 + 1001 // 8


def _count_rc(ids, ids_cap, doc_tok, ndocs, keep, nkeep, flags, st, en, nslots, uni, nuni, out=True):
    r = J.jb_colloc_result()
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    rc = J.lib().jb_colloc_count(p(ids), ids_cap, p(doc_tok), ids_cap, ndocs, p(keep), nkeep, flags, p(st), p(en), nslots,
                                 p(uni), nuni, C.byref(r) if out else None)
    J.lib().jb_colloc_result_free(C.byref(r))
    return rc


def test_argument_errors():
    ids, dt = np.array([0, 1, 0], np.uint32), np.array([0, 3], np.uint64)
    uni, keep = np.zeros(2, np.uint64), np.ones(2, np.uint8)
    ok = (ids, 3, dt, 1, keep, 2, 0, None, None, 0, uni, 2)
    assert _count_rc(*ok) == J.JB_OK and uni.tolist() == [2, 1]

    def bad(i, v, code=J.JB_EINVAL):
        a = list(ok)
        a[i] = v
        assert _count_rc(*a) == code, (i, v)

    bad(0, None)
    bad(2, None)
    bad(4, None)
    bad(10, None)
    bad(6, 2)
    bad(6, J.JB_COLLOC_CONTIG)  # the flag without spans
    bad(9, 12)
    bad(9, 4)
    bad(9, 1 << 31, J.JB_ELIMIT)
    bad(1, (1 << 32) - J.JB_COLLOC_TILE, J.JB_ELIMIT)
    assert _count_rc(*ok, out=False) == J.JB_EINVAL
    assert uni.tolist() == [2, 1], "a refused call adds nothing"
    # nothing to read needs no arrays
    assert _count_rc(None, 0, dt, 1, None, 0, 0, None, None, 0, None, 0) == J.JB_OK
    a = np.zeros(1, np.uint32)
    c = np.ones(1, np.uint64)
    r = J.jb_colloc_result()
    L = J.lib()
    for args, code in (((a.ctypes.data, a.ctypes.data, c.ctypes.data, 1, uni.ctypes.data, 2, 10, 3, 1, 0.0, 0), J.JB_EINVAL),
                       ((a.ctypes.data, a.ctypes.data, c.ctypes.data, 1, uni.ctypes.data, 2, 10, -1, 1, 0.0, 0), J.JB_EINVAL),
                       ((a.ctypes.data, a.ctypes.data, c.ctypes.data, 1, uni.ctypes.data, 2, 10, 0, 0, 0.0, 0), J.JB_EINVAL),
                       ((a.ctypes.data, a.ctypes.data, c.ctypes.data, 1, None, 2, 10, 0, 1, 0.0, 0), J.JB_EINVAL),
                       ((None, a.ctypes.data, c.ctypes.data, 1, uni.ctypes.data, 2, 10, 0, 1, 0.0, 0), J.JB_EINVAL),
                       ((None, None, None, 0, None, 0, 10, 0, 1, 0.0, 0), J.JB_OK)):
        assert L.jb_colloc_score(*args, C.byref(r)) == code, args
        L.jb_colloc_result_free(C.byref(r))
    assert L.jb_colloc_score(None, None, None, 0, None, 0, 10, 0, 1, 0.0, 0, None) == J.JB_EINVAL
    L.jb_colloc_result_free(None)
