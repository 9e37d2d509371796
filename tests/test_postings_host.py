"""CPU: jb_postings, the host form of the postings rule (jieba-go_amd/csrc/jb_postings.cpp), against
postings_ref.py's two implementations, which must also agree with each other, on the cases the GPU tests run
(postings_cases.py); transposing twice, the list lengths against df_ref, the cap protocol, the size helper and
every error code."""
import ctypes as C

import numpy as np
import pytest

import df_ref as DR
import jiebahip as J
import postings_cases as PC
import postings_ref as PR

CASES = list(PC.all_cases())


def run(c, pcap=None):
    return J.postings(c["term_id"], c["term_cnt"], c["term_off"], c["nids"], c["doc_base"], c["nterms"], c["cap"], pcap)


def same(got, want, label):
    for g, w, name in zip(got, want, ("post_doc", "post_tf", "post_off")):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{label}: {name} differs"


@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_host_rule_is_the_reference(c):
    args = (c["term_id"], c["term_cnt"], c["term_off"], c["nterms"], c["cap"], c["nids"], c["doc_base"])
    want = PR.postings_np(*args)
    same(PR.postings_dict(*args), want, c["label"] + " (dict against numpy)")
    pd, pt, po, n = run(c)
    assert n == int(want[2][-1]) == len(want[0])
    same((pd[:n], pt[:n], po), want, c["label"])
    assert not pd[n:].any() and not pt[n:].any(), "written past the result"
    # the list lengths are the document frequencies
    nn = min(c["nterms"], c["cap"], int(c["term_off"][-1]))
    assert np.array_equal(np.diff(po.astype(np.int64)), DR.df(c["term_id"], nn, nn, c["nids"]))


def test_cases_cover_what_they_claim():
    by = {c["label"]: c for c in CASES}
    assert (by["length 70001"]["term_id"] >= 256).sum() > 1000
    z = by["zipf"]
    top = np.bincount(z["term_id"][z["term_id"] < z["nids"]]).max()
    assert top > PC.TILE, "an id that fills more than a tile"
    for label in ("repeats", "repeats two digits"):
        c = by[label]
        pd, pt, po, n = run(c)
        for t in range(c["nids"]):
            lst = pt[int(po[t]):int(po[t + 1])].astype(np.int64)
            assert (np.diff(lst) > 0).all(), "input order inside a list"
        assert n > 3 * PC.TILE * 0.8


def test_transposing_twice_is_the_identity():
    rng = np.random.default_rng(127)
    for ndocs, nids, n in ((1, 1, 50), (37, 19, 900), (500, 3000, 30_000)):
        # a CSR with distinct ascending ids in every row, as jb_terms_device writes it
        rows = [np.sort(rng.choice(nids, min(nids, int(rng.integers(0, 2 * n // ndocs + 2))), replace=False))
                for _ in range(ndocs)]
        ti = np.concatenate(rows).astype(np.uint32)
        tc = rng.integers(1, 1000, len(ti)).astype(np.uint32)
        to = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
        pd, pt, po, m = J.postings(ti, tc, to, nids)
        assert m == len(ti)
        # the postings read as a CSR with the roles of id and document swapped, inverted again
        bd, bt, bo, m2 = J.postings(pd, pt, po, ndocs)
        assert m2 == len(ti) and np.array_equal(bd, ti) and np.array_equal(bt, tc) and np.array_equal(bo, to)


def test_cap_protocol():
    c = [x for x in CASES if x["label"] == "length 8193"][0]
    pd, pt, po, n = run(c)
    assert n > 4000
    for pcap in (0, n // 2, n):
        qd, qt, qo, m = run(c, pcap)
        assert m == n and np.array_equal(qo, po), "post_off and nposts are complete"
        k = min(pcap, n)
        assert len(qd) == pcap and np.array_equal(qd[:k], pd[:k]) and np.array_equal(qt[:k], pt[:k])
    # arrays of exactly pcap entries between guards
    pcap = n // 2
    qd, qt = np.full(pcap + 8, 0xABABABAB, np.uint32), np.full(pcap + 8, 0xABABABAB, np.uint32)
    qo, m = np.zeros(c["nids"] + 1, np.uint64), C.c_uint64()
    rc = J.lib().jb_postings(c["term_id"].ctypes.data, c["term_cnt"].ctypes.data, c["term_off"].ctypes.data, c["nterms"],
                             c["cap"], len(c["term_off"]) - 1, c["nids"], 0, qd.ctypes.data, qt.ctypes.data, pcap,
                             qo.ctypes.data, C.byref(m))
    assert rc == J.JB_OK and m.value == n
    assert (qd[pcap:] == 0xABABABAB).all() and (qt[pcap:] == 0xABABABAB).all()
    assert np.array_equal(qd[:pcap], pd[:pcap])


def test_work_bytes():
    f = J.postings_work_bytes
    assert f(0, 0, 0) > 0
    last = 0
    for n in (0, 1, PC.TILE - 1, PC.TILE, PC.TILE + 1, 10 * PC.TILE, 1 << 27, (1 << 32) - PC.TILE - 1):
        cur = f(n, 10, 10)
        assert cur >= last and cur >= 24 * n
        assert f(n, 1 << 32, 10) >= cur and f(n, 10, 0xFFFFFFFF) >= cur
        last = cur


def test_errors():
    L = J.lib()
    ti, tc, to = np.array([1, 2], np.uint32), np.array([1, 1], np.uint32), np.array([0, 2], np.uint64)
    pd, pt, po, n = np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(4, np.uint64), C.c_uint64()
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(ti_=p(ti), tc_=p(tc), to_=p(to), cap=2, ndocs=1, nids=3, base=0, pd_=p(pd), pt_=p(pt), pcap=2, po_=p(po),
             n_=C.addressof(n)):
        return L.jb_postings(ti_, tc_, to_, 2, cap, ndocs, nids, base, pd_, pt_, pcap, po_, n_)

    assert call() == J.JB_OK and n.value == 2 and po.tolist() == [0, 0, 1, 2]
    for kw in (dict(ti_=None), dict(tc_=None), dict(to_=None), dict(pd_=None), dict(pt_=None), dict(po_=None),
               dict(n_=None)):
        assert call(**kw) == J.JB_EINVAL, kw
    # arrays of capacity 0 may be NULL
    assert call(ti_=None, tc_=None, cap=0) == J.JB_OK and n.value == 0
    assert call(pd_=None, pt_=None, pcap=0) == J.JB_OK and n.value == 2
    # an output that is an input or another output
    assert call(pd_=p(ti)) == J.JB_EINVAL and call(pt_=p(tc)) == J.JB_EINVAL and call(pt_=p(pd)) == J.JB_EINVAL
    assert call(po_=p(to)) == J.JB_EINVAL and call(n_=p(po)) == J.JB_EINVAL
    assert b"output" in L.jb_last_error()
    # the limits
    assert call(cap=(1 << 32) - PC.TILE) == J.JB_ELIMIT
    assert call(base=0xFFFFFFFF, ndocs=2, to_=p(np.array([0, 1, 2], np.uint64))) == J.JB_ELIMIT
    big = np.array([0, 2], np.uint64)
    assert call(base=0xFFFFFFFF, ndocs=1, to_=p(big)) == J.JB_OK and pd.tolist() == [0xFFFFFFFF, 0xFFFFFFFF]
    # nids = 0 is valid
    po[:] = 9
    assert call(nids=0) == J.JB_OK and n.value == 0 and po[0] == 0 and po[1] == 9
