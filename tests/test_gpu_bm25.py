"""GPU: BM25 search (jb_bm25_norms_device, jb_bm25_idf_device, jb_bm25_search_device, jb_index_set,
jb_search_batch; jb_bm25.hip) against bm25_ref.py's numpy restatement and the host rule on the cases of
bm25_cases.py, in both forms (JB_BM25_FORM, read at jb_open: one tokenizer per form), whose outputs must be the
same bytes.  Every output and the work buffer sit between canaries that must not change."""
import os
import subprocess
import threading

import numpy as np
import pytest

import bm25_cases as BC
import bm25_ref as BR
import jiebahip as J
import search_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = J.JB_BM25_TILE
NG = 64  # canary bytes on each side of every output and of the work buffer
FILL = 0x33
FORMS = [0, 1]  # JB_BM25_FORM
CASES = list(BC.all_cases())
assert T == BC.TILE


@pytest.fixture(scope="module")
def forms(mini_paths):
    """{form: a tokenizer opened with JB_BM25_FORM=form} (the knob is read at jb_open)."""
    old = os.environ.get("JB_BM25_FORM")
    tks = {}
    try:
        for f in FORMS:
            os.environ["JB_BM25_FORM"] = str(f)
            tks[f] = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    finally:
        if old is None:
            os.environ.pop("JB_BM25_FORM", None)
        else:
            os.environ["JB_BM25_FORM"] = old
    yield tks
    for tk in tks.values():
        tk.close()


def guarded(nbytes, fill):
    """A device buffer of nbytes between canaries: (tensor, pointer to the payload)."""
    import torch
    pad = (-nbytes) % 8
    t = torch.full((nbytes + pad + 2 * NG,), fill, dtype=torch.uint8, device="cuda")
    t[:NG] = 0x7A
    t[NG + nbytes:] = 0x7A
    assert (t.data_ptr() + NG) % 8 == 0
    return t, t.data_ptr() + NG


def payload(t, nbytes, what):
    b = t.cpu().numpy()
    assert (b[:NG] == 0x7A).all() and (b[NG + nbytes:] == 0x7A).all(), "written outside " + what
    return b[NG:NG + nbytes]


def _up(a, dtype, n, shift=0):
    """An allocation of exactly n entries (+ shift: the array then starts `shift` entries after a 16-byte
    boundary)."""
    import torch
    a = np.ascontiguousarray(a, dtype)[:n]
    held = np.concatenate([np.zeros(shift, dtype), a]).view(np.uint8)
    t = torch.from_numpy(held.copy() if len(held) else np.zeros(8, np.uint8)).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift * np.dtype(dtype).itemsize


def device(tk, c, topk, shift=0, work=None, alias=None, expect_error=None):
    """jb_bm25_search_device on a case -> (res_doc [nq, topk], res_score, res_n).  work = (missing bytes,
    misalignment) asks for a bad buffer; alias names an output to pass another array's pointer for."""
    import torch
    _, nm, wt = BR.inputs(c)
    nq, nd = len(c["q_off"]) - 1, c["ndocs"]
    hold = [_up(c["post_doc"], np.uint32, c["npost"], shift), _up(c["post_tf"], np.uint32, c["npost"], shift),
            _up(c["post_off"], np.uint64, c["nids"] + 1), _up(nm, np.float32, nd, shift),
            _up(wt, np.float32, c["nweights"], shift), _up(c["q_id"], np.uint32, c["q_cap"], shift),
            _up(c["q_off"], np.uint64, nq + 1)]
    p_pd, p_pt, p_po, p_nm, p_wt, p_qi, p_qo = [h[1] for h in hold]
    need = J.bm25_work_bytes(nq, nd, topk)
    wk, p_wk = guarded(need, 0x5B)
    rd, p_rd = guarded(nq * topk * 4, FILL)
    rs, p_rs = guarded(nq * topk * 8, FILL)
    rn, p_rn = guarded(nq * 4, FILL)
    st = torch.cuda.current_stream().cuda_stream
    wmiss, wmis = work or (0, 0)
    if alias == "res_doc":
        p_rd = p_qi
    if alias == "res_score":
        p_rs = p_po
    if alias == "res_n":
        p_rn = p_rd
    if alias == "work":
        p_rs = p_wk
    args = (p_pd, p_pt, p_po, c["npost"], c["nids"], p_nm, nd, p_wt, c["nweights"], c["k1"], p_qi, c["q_cap"], p_qo, nq,
            topk, p_rd, p_rs, p_rn, p_wk + wmis, need - wmiss, st)
    if expect_error is not None:
        with pytest.raises(J.JbError) as ei:
            tk.bm25_search_device(*args)
        assert ei.value.code == expect_error
        torch.cuda.synchronize()  # nothing was queued: every buffer holds its fill
        assert (payload(wk, need, "the work buffer") == 0x5B).all()
        for t, nb in ((rd, nq * topk * 4), (rs, nq * topk * 8), (rn, nq * 4)):
            assert (payload(t, nb, "an output") == FILL).all()
        return None
    tk.bm25_search_device(*args)
    torch.cuda.synchronize()
    payload(wk, need, "the work buffer")
    return (payload(rd, nq * topk * 4, "res_doc").copy().view(np.uint32).reshape(nq, topk),
            payload(rs, nq * topk * 8, "res_score").copy().view(np.uint64).reshape(nq, topk),
            payload(rn, nq * 4, "res_n").copy().view(np.uint32))


def host(c, topk):
    _, nm, wt = BR.inputs(c)
    return J.bm25_search(c["post_doc"], c["post_tf"], c["post_off"], nm, wt, c["k1"], c["q_id"], c["q_off"], topk,
                         npost=c["npost"], nids=c["nids"], ndocs=c["ndocs"], nweights=c["nweights"], q_cap=c["q_cap"])


def same(got, want, label):
    for g, w, name in zip(got, want, ("res_doc", "res_score", "res_n")):
        if g.tobytes() != np.ascontiguousarray(w).tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError(f"{label}: {name} differs at {len(bad)} places; first {bad[0].tolist()}: got "
                                 f"{g[tuple(bad[0])]} want {w[tuple(bad[0])]}")


# ---- 1. every case, both forms, every topk ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_cases(forms, c):
    for topk in c["topks"]:
        a, b = device(forms[0], c, topk), device(forms[1], c, topk)
        for x, y, name in zip(a, b, ("res_doc", "res_score", "res_n")):
            assert x.tobytes() == y.tobytes(), f"{c['label']} topk={topk}: the forms differ in {name}"
        same(a, BR.want(c, topk), f"{c['label']} topk={topk} against the reference")
        same(a, host(c, topk), f"{c['label']} topk={topk} against the host rule")
        n = a[2]
        for q in range(len(n)):  # the remaining slots
            assert (a[0][q, int(n[q]):] == J.JB_ID_UNK).all() and (a[1][q, int(n[q]):] == 0).all()


def test_ties_cross_the_tiles(forms):
    c = next(c for c in CASES if c["label"] == "ties")
    for f in FORMS:
        rd, rs, rn = device(forms[f], c, 64)
        assert rn[0] == 64 and rd[0].tolist() == list(range(64)) and len(set(rs[0].tolist())) == 1
        # a rare id: fewer than 40 of its documents lie in the first tile, so topk = 40 cuts the tie in the second
        lst = c["post_doc"][int(c["post_off"][3]):int(c["post_off"][4])]
        assert 40 < len(lst) < 64 and lst[39] >= T > lst[10]
        rd, rs, rn = device(forms[f], c, 40)
        assert rn[3] == 40 and np.array_equal(rd[3], lst[:40]) and len(set(rs[3].tolist())) == 1
        rd, rs, rn = device(forms[f], c, 64)
        assert rn[3] == len(lst) and np.array_equal(rd[3][:len(lst)], lst)


# ---- 2. misaligned array starts, run-to-run identity -----------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_starts(forms, shift):
    c = next(c for c in CASES if c["label"] == f"ndocs={T + 1}")
    for f in FORMS:
        same(device(forms[f], c, 10, shift=shift), BR.want(c, 10), f"shift={shift} form={f}")


def test_run_to_run(forms):
    c = next(c for c in CASES if c["label"] == f"ndocs={2 * T + 3}")
    for f in FORMS:
        a, b = device(forms[f], c, 64), device(forms[f], c, 64)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 3. norms and weights on the device ------------------------------------------------------------------------------
@pytest.mark.parametrize("label", [f"ndocs={T + 1}", "b=0", "b=1", "k1=0", "k1=64", "ndocs=1"])
def test_norms_and_weights(forms, label):
    import torch
    c = next(c for c in CASES if c["label"] == label)
    avg, nm, _ = BR.inputs(c)
    tk = forms[1]
    nd, nids = c["ndocs"], c["nids"]
    dl, p_dl = _up(c["doc_len"], np.uint32, nd, 1)
    po, p_po = _up(c["post_off"], np.uint64, nids + 1)
    on, p_on = guarded(nd * 4, FILL)
    ow, p_ow = guarded(nids * 4, FILL)
    st = torch.cuda.current_stream().cuda_stream
    tk.bm25_norms_device(p_dl, nd, c["k1"], c["b"], avg, p_on, st)
    tk.bm25_idf_device(p_po, nids, nd, p_ow, st)
    torch.cuda.synchronize()
    assert payload(on, nd * 4, "norm").tobytes() == nm.tobytes()
    assert payload(on, nd * 4, "norm").tobytes() == J.bm25_norms(c["doc_len"], c["k1"], c["b"], avg).tobytes()
    assert payload(ow, nids * 4, "weight").tobytes() == BR.idf(c["post_off"], nd).tobytes()
    for n in (1, 10 ** 9, (1 << 53) - 1):
        tk.bm25_idf_device(p_po, nids, n, p_ow, st)
        torch.cuda.synchronize()
        assert payload(ow, nids * 4, "weight").tobytes() == J.bm25_idf(c["post_off"], n).tobytes(), n
    for args, code in (((p_dl, nd, -1.0, 0.5, avg, p_on, st), J.JB_EINVAL), ((p_dl, nd, 1.2, 1.5, avg, p_on, st), J.JB_EINVAL),
                       ((p_dl, nd, 1.2, 0.5, 0.0, p_on, st), J.JB_EINVAL), ((p_dl, nd, 1.2, 0.5, float("nan"), p_on, st), J.JB_EINVAL),
                       ((p_dl, nd, 1.2, 0.5, avg, p_dl, st), J.JB_EINVAL)):
        with pytest.raises(J.JbError) as ei:
            tk.bm25_norms_device(*args)
        assert ei.value.code == code
    with pytest.raises(J.JbError) as ei:
        tk.bm25_idf_device(p_po, nids, 1 << 53, p_ow, st)
    assert ei.value.code == J.JB_ELIMIT


# ---- 4. refused calls queue nothing ----------------------------------------------------------------------------------
def test_refused_calls(forms):
    c = next(c for c in CASES if c["label"] == "ndocs=1")
    for f in FORMS:
        for alias in ("res_doc", "res_score", "res_n", "work"):
            device(forms[f], c, 10, alias=alias, expect_error=J.JB_EINVAL)
        device(forms[f], c, 10, work=(8, 0), expect_error=J.JB_EINVAL)
        device(forms[f], c, 10, work=(0, 4), expect_error=J.JB_EINVAL)
        device(forms[f], c, 0, expect_error=J.JB_EINVAL)
        device(forms[f], c, J.JB_KW_MAXK + 1, expect_error=J.JB_ELIMIT)
        bad = dict(c, k1=65.0, label="bad-k1")
        BR._CACHE[("in", "bad-k1")] = BR.inputs(c)
        device(forms[f], bad, 10, expect_error=J.JB_EINVAL)


def test_launch_counts(forms):
    """The number of launches depends on the arguments alone: form 1 queues k_bm25_tile and k_bm25_merge, form 0
    k_bm25_scatter, k_bm25_select and k_bm25_merge; without a document only the merge, without a query nothing."""
    by = {c["label"]: c for c in CASES}
    for f, names in ((1, {"k_bm25_tile": 1, "k_bm25_merge": 1}),
                     (0, {"k_bm25_scatter": 1, "k_bm25_select": 1, "k_bm25_merge": 1})):
        tk = forms[f]
        tk.profile(True)
        try:
            for label, want in ((f"ndocs={T + 1}", names), ("ties", names), ("ndocs=0", {"k_bm25_merge": 1}), ("nq=0", {})):
                tk.profile_reset()
                device(tk, by[label], 10)
                got = {k: v[1] for k, v in tk.profile_read().items() if k.startswith("k_bm25") and v[1]}
                assert got == want, (f, label, got)
        finally:
            tk.profile(False)


# ---- 5. the chain build_index -> set_index -> search on the mini fixtures --------------------------------------------
def chain_docs(seed=31, ndocs=90):
    rng = np.random.default_rng(seed)
    parts = ["今天", "天氣", "很好", "我", "昨天", "去", "上海", "交通", "大學", "這", "的", "一刹那", "，", "。", " ", "abc ", "2024 "]
    return ["".join(parts[int(rng.integers(0, len(parts)))] for _ in range(int(rng.integers(0, 40)))).encode()
            for _ in range(ndocs)]


KEYS = [k.encode() for k in ("今天", "天氣", "很好", "昨天", "上海", "交通", "大學", "的", "一刹那", "刹那", "abc", "2024", "absent")]
QUERIES = ["今天天氣很好", "上海交通大學", "", "abc abc 2024", "zzz 未知", "的", "昨天去上海 abc", "absent"]


def test_chain_build_set_search(forms):
    docs = chain_docs()
    want = {}
    for f in FORMS:
        tk = forms[f]
        tk.set_vocab(None)
        tk.clear_index()
        with pytest.raises(J.JbError) as ei:
            tk.search(QUERIES)
        assert ei.value.code == J.JB_EINVAL  # no vocabulary
        tk.set_vocab(KEYS)
        with pytest.raises(J.JbError) as ei:
            tk.search(QUERIES)
        assert ei.value.code == J.JB_EINVAL  # no index
        with pytest.raises(J.JbError) as ei:
            tk.index_info()
        assert ei.value.code == J.JB_EINVAL
        ix = tk.build_index([docs[:40], docs[40:]], hmm=True)
        po, pd, pt, dl, nd = ix
        tk.set_index(*ix)
        avg = BR.avgdl(dl)
        assert tk.index_info() == (nd, len(KEYS), len(pd), avg)
        # the reference: postings_batch of all documents at once, the reference's norms and weights, and the ids
        # of the plain cut of each query
        buf, off = R.batch_of(docs)
        qo, qd, qt, ql = tk.postings_batch(buf, off, True)
        assert np.array_equal(qo, po) and np.array_equal(qd, pd) and np.array_equal(qt, pt) and np.array_equal(ql, dl)
        nm, wt = BR.norms(dl, 1.2, 0.75, avg), BR.idf(po, nd)
        qids, qoff = [], [0]
        for q in QUERIES:
            qids += tk.CutIds(q, True)[1].tolist() if q else []
            qoff.append(len(qids))
        qi, qf = np.array(qids, np.uint32), np.array(qoff, np.uint64)
        for topk in (1, 10, 64):
            wd, ws, wn = BR.search(pd, pt, po, len(pd), len(KEYS), nm, nd, wt, len(KEYS), 1.2, qi, len(qi), qf, topk)
            got = tk.search(QUERIES, topk)
            assert got == [[(int(wd[q, r]), int(ws[q, r]) / 2.0 ** 24) for r in range(int(wn[q]))]
                           for q in range(len(QUERIES))], topk
        got = tk.search(QUERIES, 10)
        assert any(got) and not got[2] and not got[7]  # (the empty query; a key that is in no document)
        want[f] = got
        assert tk.search([], 5) == []
        # other parameters give other norms; an index of another vocabulary size is refused
        tk.set_index(po, pd, pt, dl, k1=2.0, b=0.0)
        nm2 = BR.norms(dl, 2.0, 0.0, avg)
        wd, ws, wn = BR.search(pd, pt, po, len(pd), len(KEYS), nm2, nd, wt, len(KEYS), 2.0, qi, len(qi), qf, 10)
        assert tk.search(QUERIES, 10) == [[(int(wd[q, r]), int(ws[q, r]) / 2.0 ** 24) for r in range(int(wn[q]))]
                                          for q in range(len(QUERIES))]
        tk.set_index(po[:-1], pd[:int(po[-2])], pt[:int(po[-2])], dl)
        with pytest.raises(J.JbError) as ei:
            tk.search(QUERIES)
        assert ei.value.code == J.JB_EINVAL
        for kw in (dict(k1=-1.0), dict(b=2.0)):
            with pytest.raises(J.JbError) as ei:
                tk.set_index(po, pd, pt, dl, **kw)
            assert ei.value.code == J.JB_EINVAL
        with pytest.raises(J.JbError) as ei:
            tk.set_index(po, pd, pt, np.zeros(nd, np.uint32))
        assert ei.value.code == J.JB_EINVAL  # an index without a token
        for bad in (0, J.JB_KW_MAXK + 1):
            with pytest.raises(J.JbError) as ei:
                tk.search(QUERIES, bad)
            assert ei.value.code == (J.JB_EINVAL if bad == 0 else J.JB_ELIMIT)
        tk.set_index(*ix)
        assert tk.search(QUERIES, 10) == got
    assert want[0] == want[1]


def test_two_threads_search_one_ctx(forms):
    tk = forms[1]
    docs = chain_docs(37, 70)
    tk.set_vocab(KEYS)
    tk.set_index(*tk.build_index([docs]))
    sets = (QUERIES, list(reversed(QUERIES)))
    want = [tk.search(s, 7) for s in sets]
    errs, res = [], {}

    def run(k):
        try:
            for _ in range(4):
                res[k] = tk.search(sets[k], 7)
        except BaseException as ex:  # noqa: BLE001 (reported below)
            errs.append(ex)

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    assert res[0] == want[0] and res[1] == want[1]


# ---- 6. the C++ mirror -----------------------------------------------------------------------------------------------
def test_cpp_consumer(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "cpp_bm25_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_bm25_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bm25 ok" in r.stdout, r.stderr + r.stdout
