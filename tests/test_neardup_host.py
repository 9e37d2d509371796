"""CPU: jb_neardup and jb_neardup_labels, the host form of the near-duplicate rule (jieba-go_amd/csrc/
jb_neardup.cpp), against neardup_ref.py on the cases the GPU tests run (neardup_cases.py): every output byte for
byte, the cap protocol, the labels on the rule's CSRs and on a hostile one, every error code, the size helper, and
the host chain jb_minhash -> jb_minhash_bands -> jb_neardup -> labels on text with planted copies."""
import ctypes as C

import numpy as np
import pytest

import jiebahip as J
import neardup_cases as NC
import neardup_ref as NR

CASES = list(NC.all_cases())
_WANT = {}


def want_of(c):
    """The reference's result for a case, computed once."""
    if c["label"] not in _WANT:
        _WANT[c["label"]] = NR.neardup(c["key"], c["sig"], c["W"], c["min_agree"])
    return _WANT[c["label"]]


def run(c, pcap=None):
    return J.neardup(c["key"], c["sig"], c["W"], c["min_agree"], pcap)


def test_exports_and_constants():
    L = J.lib()
    for name in ("jb_neardup_work_bytes", "jb_neardup", "jb_neardup_device", "jb_neardup_labels", "jb_neardup_sig"):
        assert name in J.EXPORTS and hasattr(L, name), name
    assert J.JB_ND_TILE == NC.TILE and J.JB_ND_MAXWIN == 64 and J.JB_ND_NSTAT == 3 and J.JB_MH_NOKEY == NC.NOKEY


@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_host_rule_is_the_reference(c):
    wd, wa, wo, ws = want_of(c)
    pd, pa, po, n, st = run(c)
    assert n == len(wd) == int(wo[-1]), f"npairs {n}, want {len(wd)}"
    assert st.tolist() == ws.tolist(), f"stat {st.tolist()}, want {ws.tolist()}"
    for g, w, name in ((pd, wd, "pair_doc"), (pa, wa, "pair_agree"), (po, wo, "pair_off")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{c['label']}: {name} differs"
    nd = len(c["key"])
    assert np.array_equal(J.neardup_labels(po, pd), NR.labels(wo, wd, nd))


def test_cases_cover_what_they_claim():
    by = {c["label"]: c for c in CASES}
    for W in (1, 2, 63, 64):
        c = by[f"one bucket W={W}"]
        pd, pa, po, n, st = run(dict(c, sig=np.zeros_like(c["sig"])))  # (every candidate verifies)
        assert st[J.JB_ND_NTRUNC] == len(c["key"]) - 1 - W > 0
        assert (J.neardup_labels(po, pd) == 0).all(), "consecutive members are candidates: the chain stays connected"
    pd, pa, po, n, st = run(by["beyond the window in the first band"])
    assert n == 2 and pd.tolist() == [0, 1] and po.tolist() == [0, 0, 1, 2, 2, 2, 2] and st.tolist() == [12, 2, 1]
    pd, pa, po, n, st = run(by["inside the window in the first band"])
    assert n == 3 and pd.tolist() == [0, 0, 1] and st.tolist() == [12, 3, 0]
    pd, pa, po, n, st = run(by["one value in two bands"])
    assert n == 1 and pd.tolist() == [2] and po.tolist() == [0, 0, 0, 0, 1, 1, 1] and st.tolist() == [9, 1, 0]
    pd, pa, po, n, st = run(by["several common bands"])
    # (0,1) at band 0; (2,3) at band 0; then band 1: (0,2), (1,2), (0,4), (1,4), (2,4); band 2: (3,4), (0,3) ...
    assert po.tolist() == [0, 0, 1, 3, 6, 10, 10]
    assert pd.tolist() == [0, 0, 1, 2, 0, 1, 0, 1, 2, 3]  # row 3: band 0 first; row 4: band 1 before band 2
    pd, pa, po, n, st = run(by["key parts"])
    assert n == len(by["key parts"]["key"]) // 2 and st[J.JB_ND_NCAND] == n, "only the planted twins share a bucket"
    assert run(by["all nokey"])[3] == 0 and run(by["all nokey"])[4].tolist() == [0, 0, 0]
    for K in (1, 64, 65, 100):
        pd, pa, po, n, st = run(by[f"threshold K={K} min_agree={K}"])
        assert st[J.JB_ND_NCAND] == 10 and set(pa.tolist()) == {K}, "only agree == K passes min_agree = K"
        assert n == (1 if K > 1 else 4)  # (with one slot, three rows are equal and so are the other two)
        if K > 1:
            pd, pa, po, n, st = run(by[f"threshold K={K} min_agree=1"])
            assert 0 not in pa.tolist() and 1 in pa.tolist() and K - 1 in pa.tolist() and n < 10
    c = by["runs across tiles"]
    assert c["key"].size == 2 * NC.TILE + 1
    assert sum(want_of(by[f"entries={n}"])[3][J.JB_ND_NCAND] > 0 for n in (NC.TILE - 1, NC.TILE, NC.TILE + 1)) == 3
    assert want_of(by["mixed"])[3][J.JB_ND_NTRUNC] == 0 and len(want_of(by["mixed"])[0]) > 100
    assert want_of(by["crowded"])[3][J.JB_ND_NTRUNC] > 0


def test_cap_protocol():
    c = [x for x in CASES if x["label"] == "crowded"][0]
    pd, pa, po, n, st = run(c)
    assert n > 1000
    for pcap in (0, n - 1, n):
        qd, qa, qo, m, qs = run(c, pcap)
        assert m == n and np.array_equal(qo, po) and np.array_equal(qs, st), "pair_off, npairs and stat are complete"
        assert len(qd) == pcap and np.array_equal(qd, pd[:pcap]) and np.array_equal(qa, pa[:pcap])
    # arrays of exactly pcap entries between guards
    pcap = n // 2
    qd, qa = np.full(pcap + 8, 0xABABABAB, np.uint32), np.full(pcap + 8, 0xABABABAB, np.uint32)
    qo, qs, m = np.zeros(len(c["key"]) + 1, np.uint64), np.zeros(3, np.uint64), C.c_uint64()
    nd, B = c["key"].shape
    rc = J.lib().jb_neardup(c["key"].ctypes.data, c["sig"].ctypes.data, nd, B, c["sig"].shape[1], c["W"], c["min_agree"],
                            qd.ctypes.data, qa.ctypes.data, pcap, qo.ctypes.data, C.byref(m), qs.ctypes.data)
    assert rc == J.JB_OK and m.value == n
    assert (qd[pcap:] == 0xABABABAB).all() and (qa[pcap:] == 0xABABABAB).all() and np.array_equal(qd[:pcap], pd[:pcap])


def test_labels_on_a_hostile_csr():
    rng = np.random.default_rng(263)
    nd = 60
    for trial in range(20):
        pd = rng.integers(0, nd + 5, 200).astype(np.uint32)  # entries >= j, and >= ndocs, are skipped
        po = np.sort(rng.integers(0, 260, nd + 1)).astype(np.uint64)  # offsets past pcap
        if trial % 2:
            po = rng.integers(0, 1 << 40, nd + 1).astype(np.uint64)  # and decreasing
        for pcap in (200, 150, 0):
            got = J.neardup_labels(po, pd[:max(pcap, 1)], pcap)
            assert np.array_equal(got, NR.labels(po, pd, nd, pcap)), (trial, pcap)
    assert len(J.neardup_labels(np.zeros(1, np.uint64), np.zeros(0, np.uint32))) == 0
    assert J.lib().jb_neardup_labels(None, None, 0, 0, None) == J.JB_EINVAL
    lab = np.zeros(2, np.uint32)
    assert J.lib().jb_neardup_labels(np.zeros(3, np.uint64).ctypes.data, None, 1, 2, lab.ctypes.data) == J.JB_EINVAL
    assert J.lib().jb_neardup_labels(np.zeros(3, np.uint64).ctypes.data, None, 0, 2, None) == J.JB_EINVAL


def test_work_bytes():
    f = J.neardup_work_bytes
    assert f(0, 0) > 0 and f(0, 256) > 0 and f(0xFFFFFFFF, 0) > 0
    last = 0
    for nd in (0, 1, NC.TILE - 1, NC.TILE, NC.TILE + 1, 10 * NC.TILE, 1 << 22, 1 << 27, 0xFFFFFFFF):
        row = [f(nd, B) for B in (0, 1, 2, 31, 32, 33, 256, 0xFFFFFFFF)]
        assert row == sorted(row) and row[1] >= last and row[1] >= 24 * nd
        last = row[1]
        if nd * 32 < (1 << 32):
            assert row[4] >= 24 * nd * 32


def test_errors():
    L = J.lib()
    key = np.array([[1, 2], [1, 3]], np.uint64)
    sig = np.array([[4, 5, 6], [4, 5, 7]], np.uint32)
    pd, pa, po, st, n = np.full(2, 9, np.uint32), np.full(2, 9, np.uint32), np.full(3, 9, np.uint64), np.full(3, 9, np.uint64), C.c_uint64(9)
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(key_=p(key), sig_=p(sig), ndocs=2, B=2, K=3, W=64, m=2, pd_=p(pd), pa_=p(pa), pcap=2, po_=p(po),
             n_=C.addressof(n), st_=p(st)):
        return L.jb_neardup(key_, sig_, ndocs, B, K, W, m, pd_, pa_, pcap, po_, n_, st_)

    def untouched():
        return (pd == 9).all() and (pa == 9).all() and (po == 9).all() and (st == 9).all() and n.value == 9

    for kw in (dict(key_=None), dict(sig_=None), dict(pd_=None), dict(pa_=None), dict(po_=None), dict(n_=None),
               dict(st_=None), dict(B=0), dict(K=0), dict(W=0), dict(m=0)):
        assert call(**kw) == J.JB_EINVAL and untouched(), kw
    # an output that is an input or another output
    for kw in (dict(pd_=p(sig)), dict(pa_=p(pd)), dict(po_=p(key)), dict(n_=p(po)), dict(st_=p(po)), dict(st_=C.addressof(n))):
        assert call(**kw) == J.JB_EINVAL and untouched(), kw
    assert b"output" in L.jb_last_error()
    # the limits
    for kw in (dict(B=257), dict(K=257), dict(W=65), dict(m=4), dict(ndocs=(1 << 31) - NC.TILE // 2, B=2),
               dict(ndocs=0xFFFFFFFF, B=1), dict(ndocs=0xFFFFFFFF, B=256)):
        assert call(**kw) == J.JB_ELIMIT and untouched(), kw
    # the edges of the limits, and arrays of capacity 0 may be NULL
    assert call(W=64, m=3) == J.JB_OK and n.value == 0 and po.tolist() == [0, 0, 0] and st.tolist() == [4, 1, 0]
    assert call() == J.JB_OK and n.value == 1 and pd[0] == 0 and pa[0] == 2 and po.tolist() == [0, 0, 1]
    assert call(pd_=None, pa_=None, pcap=0) == J.JB_OK and n.value == 1
    assert call(key_=None, sig_=None, ndocs=0) == J.JB_OK and n.value == 0 and po[0] == 0 and st.tolist() == [0, 0, 0]
    k256 = np.zeros((2, 256), np.uint64)
    s256 = np.zeros((2, 256), np.uint32)
    assert call(key_=p(k256), sig_=p(s256), B=256, K=256, m=256) == J.JB_OK and n.value == 1 and pa[0] == 256


def words(rng, n):
    return ["w%d" % int(rng.integers(0, 5000)) for _ in range(n)]


def planted_docs(seed=271, ndocs=40):
    """Documents of ASCII words; a few are byte-identical copies and a few one-word edits of earlier ones.  Returns
    (documents as word lists, [(copy, original)], [(edit, original)])."""
    rng = np.random.default_rng(seed)
    docs = [words(rng, int(rng.integers(40, 90))) for _ in range(ndocs)]
    docs[3] = []
    docs[17] = words(rng, 2)  # shorter than a shingle
    exact, edited = [(9, 2), (25, 2), (31, 11), (39, 0)], [(14, 5), (28, 20)]
    for c, o in exact:
        docs[c] = list(docs[o])
    for c, o in edited:
        docs[c] = list(docs[o])
        docs[c][len(docs[c]) // 2] = "edited"
    return docs, exact, edited


def spans_of(docs):
    """The text "w1 w2 ...\\n" per document with one span per word."""
    text, s, e, dt = bytearray(), [], [], [0]
    for d in docs:
        for w in d:
            s.append(len(text))
            text += w.encode()
            e.append(len(text))
            text += b" "
        text += b"\n"
        dt.append(len(s))
    return bytes(text), np.array(s, np.uint32), np.array(e, np.uint32), np.array(dt, np.uint64)


def test_host_chain_on_text():
    docs, exact, edited = planted_docs()
    text, s, e, dt = spans_of(docs)
    n, K, B, R = 5, 128, 32, 4
    sig, doc_n = J.minhash(text, s, e, dt, n, K, 1)
    keys = J.minhash_bands(sig, doc_n, B, R)
    m = 102  # the integer nearest 0.8 K
    pd, pa, po, npairs, st = J.neardup(keys, sig)
    wd, wa, wo, ws = NR.neardup(keys, sig, 64, m)
    assert pd.tobytes() == wd.tobytes() and pa.tobytes() == wa.tobytes() and po.tobytes() == wo.tobytes()
    assert st.tolist() == ws.tolist() and st[J.JB_ND_NTRUNC] == 0 and st[J.JB_ND_NENTRIES] == (len(docs) - 1) * B
    label = J.neardup_labels(po, pd)
    assert np.array_equal(label, NR.labels(wo, wd, len(docs)))
    pairs = {(int(pd[k]), j): int(pa[k]) for j in range(len(docs)) for k in range(int(po[j]), int(po[j + 1]))}
    for c, o in exact:  # byte-identical documents: equal signatures, so every band agrees and agree == K
        assert pairs[(min(c, o), max(c, o))] == K and label[c] == label[o] == min(label[c], o)
    assert pairs[(9, 25)] == K and label[9] == label[25] == 2
    assert label[3] == 3 and label[17] == 17 and (len(set(label.tolist())) == len(docs) - len(exact) - sum(
        1 for c, o in edited if label[c] == label[o]))
