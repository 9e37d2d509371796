"""GPU: postings (jb_postings_device, jb_postings_batch; jb_postings.hip) against postings_ref.py (numpy's stable
argsort) on CSRs the tests build themselves (postings_cases.py), in both forms of the scatter kernel
(JB_POSTINGS_FORM, read at jb_open: one tokenizer per form), whose outputs must be the same bytes.  Every
output and the work buffer sit between canaries that must not change."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import df_ref as DR
import jiebahip as J
import postings_cases as PC
import postings_ref as PR
import search_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = J.JB_POSTINGS_TILE
NG = 64  # canary bytes on each side of every output and of the work buffer
FILL = 0x33
FORMS = [0, 1]  # JB_POSTINGS_FORM
CASES = list(PC.all_cases())
assert T == PC.TILE


@pytest.fixture(scope="module")
def forms(mini_paths):
    """{form: a tokenizer opened with JB_POSTINGS_FORM=form} (the knob is read at jb_open)."""
    old = os.environ.get("JB_POSTINGS_FORM")
    tks = {}
    try:
        for f in FORMS:
            os.environ["JB_POSTINGS_FORM"] = str(f)
            tks[f] = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    finally:
        if old is None:
            os.environ.pop("JB_POSTINGS_FORM", None)
        else:
            os.environ["JB_POSTINGS_FORM"] = old
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


def _up(a, dtype, cap, shift):
    """An allocation of exactly cap entries (+ shift: the array then starts `shift` entries after a 16-byte
    boundary)."""
    import torch
    held = np.concatenate([np.full(shift, 3, dtype), np.ascontiguousarray(a, dtype)[:cap]])
    t = torch.from_numpy((held if len(held) else np.zeros(1, dtype)).view(np.int32 if dtype == np.uint32 else np.int64).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift * held.itemsize


def device(tk, c, pcap=None, shift=0, work=None, alias=None, expect_error=None):
    """jb_postings_device on a case -> (post_doc, post_tf, post_off, nposts): the first two hold the
    min(nposts, pcap) entries the call writes; what lies behind them must still hold the fill.  work = (missing
    bytes, misalignment) asks for a bad buffer; alias names an output to pass an input's pointer for."""
    import torch
    cap, nids, nd = c["cap"], c["nids"], len(c["term_off"]) - 1
    pcap = cap if pcap is None else pcap
    ti, p_ti = _up(c["term_id"], np.uint32, cap, shift)
    tc, p_tc = _up(c["term_cnt"], np.uint32, cap, shift)
    to, p_to = _up(c["term_off"], np.uint64, nd + 1, 0)
    tn = torch.tensor([c["nterms"]], dtype=torch.int64, device="cuda")
    need = J.postings_work_bytes(cap, nids, nd)
    wk, p_wk = guarded(need, 0x5B)
    pd, p_pd = guarded(pcap * 4, FILL)
    pt, p_pt = guarded(pcap * 4, FILL)
    po, p_po = guarded((nids + 1) * 8, FILL)
    pn, p_pn = guarded(8, FILL)
    st = torch.cuda.current_stream().cuda_stream
    wmiss, wmis = work or (0, 0)
    if alias == "post_doc":
        p_pd = p_ti
    if alias == "post_tf":
        p_pt = p_pd
    if alias == "post_off":
        p_po = p_to
    if alias == "nposts":
        p_pn = tn.data_ptr()
    args = (p_ti, p_tc, p_to, tn.data_ptr(), cap, nd, nids, c["doc_base"], p_pd, p_pt, pcap, p_po, p_pn, p_wk + wmis,
            need - wmiss, st)
    if expect_error is not None:
        with pytest.raises(J.JbError) as ei:
            tk.postings_device(*args)
        assert ei.value.code == expect_error
        torch.cuda.synchronize()  # nothing was queued: every buffer holds its fill
        assert (payload(wk, need, "the work buffer") == 0x5B).all()
        for t, nb in ((pd, pcap * 4), (pt, pcap * 4), (po, (nids + 1) * 8), (pn, 8)):
            assert (payload(t, nb, "an output") == FILL).all()
        return None
    tk.postings_device(*args)
    torch.cuda.synchronize()
    payload(wk, need, "the work buffer")
    n = int(payload(pn, 8, "nposts").copy().view(np.uint64)[0])
    off = payload(po, (nids + 1) * 8, "post_off").copy().view(np.uint64)
    w = min(n, pcap)
    outs = []
    for t, what in ((pd, "post_doc"), (pt, "post_tf")):
        b = payload(t, pcap * 4, what)
        assert (b[w * 4:] == FILL).all(), what + ": an entry at or past the count or pcap was written"
        outs.append(b[:w * 4].copy().view(np.uint32))
    return outs[0], outs[1], off, n


def want_of(c):
    return PR.postings(c["term_id"], c["term_cnt"], c["term_off"], c["nterms"], c["cap"], c["nids"], c["doc_base"])


def same(got, want, label, pcap=None):
    wd, wt, wo = want
    n = int(wo[-1])
    w = n if pcap is None else min(n, pcap)
    assert got[3] == n, f"{label}: nposts {got[3]}, want {n}"
    assert np.array_equal(got[2], wo), f"{label}: post_off differs"
    for g, x, name in ((got[0], wd, "post_doc"), (got[1], wt, "post_tf")):
        if not np.array_equal(g, x[:w]):
            bad = np.flatnonzero(g != x[:w])
            raise AssertionError(f"{label}: {name} differs at {len(bad)} positions; first {bad[0]}: got "
                                 f"{g[bad[:6]].tolist()} want {x[bad[:6]].tolist()}")


def both(forms, c, **kw):
    """The case on both forms: the outputs must be the same bytes; returns form 0's."""
    a, b = device(forms[0], c, **kw), device(forms[1], c, **kw)
    for x, y, name in zip(a[:3], b[:3], ("post_doc", "post_tf", "post_off")):
        assert x.tobytes() == y.tobytes(), f"{c['label']}: the forms differ in {name}"
    assert a[3] == b[3]
    return a


# ---- 1. hand-checked -------------------------------------------------------------------------------------------------
def test_hand_checked(forms):
    by = {c["label"]: c for c in PC.hand_checked()}
    for base in (0, 1000):
        pd, pt, po, n = both(forms, by[f"hand nids=10 base={base}"])
        assert n == 7 and po.tolist() == [0, 1, 2, 2, 2, 5, 5, 5, 5, 5, 7]
        assert (pd - base).tolist() == [2, 0, 0, 1, 2, 0, 2] and pt.tolist() == [5, 3, 1, 7, 4, 2, 6]
        pd, pt, po, n = both(forms, by[f"hand nids=12 base={base}"])
        assert n == 8 and po.tolist() == [0, 1, 2, 2, 2, 5, 5, 5, 5, 5, 7, 7, 8]
        assert (pd - base).tolist() == [2, 0, 0, 1, 2, 0, 2, 2] and pt.tolist() == [5, 3, 1, 7, 4, 2, 6, 8]
        pd, pt, po, n = both(forms, by[f"hand nids=1 base={base}"])
        assert n == 1 and po.tolist() == [0, 1] and (pd - base).tolist() == [2] and pt.tolist() == [5]
        pd, pt, po, n = both(forms, by[f"hand nids=0 base={base}"])
        assert n == 0 and po.tolist() == [0] and len(pd) == 0


# ---- 2 - 5. list lengths, digit edges, skew, stability; 7. form 0 against form 1 ---------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_cases(forms, c):
    same(both(forms, c), want_of(c), c["label"])


def test_stability(forms):
    for c in PC.stability():
        pd, pt, po, n = both(forms, c)
        assert n > 2 * T
        for t in range(c["nids"]):
            lst = pt[int(po[t]):int(po[t + 1])].astype(np.int64)
            assert (np.diff(lst) > 0).all(), "post_tf is ascending inside every list: input order is kept"


# ---- 6. counts and capacity ------------------------------------------------------------------------------------------
def test_counts_capacity_and_alignment(forms):
    for c in PC.counts_and_offsets():
        want = want_of(c)
        n = int(want[2][-1])
        for shift in (1, 2, 3):
            same(both(forms, c, shift=shift), want, f"{c['label']} shift={shift}")
        for pcap in (0, n // 2, n):
            same(both(forms, c, pcap=pcap), want, f"{c['label']} pcap={pcap}", pcap)


# ---- 7. run to run ---------------------------------------------------------------------------------------------------
def test_run_to_run(forms):
    c = [x for x in CASES if x["label"] == "zipf"][0]
    for f in FORMS:
        a, b = device(forms[f], c), device(forms[f], c)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_refused_calls_queue_nothing(forms):
    c = [x for x in CASES if x["label"] == "length 257"][0]
    tk = forms[0]
    device(tk, c, work=(1, 0), expect_error=J.JB_EINVAL)
    device(tk, c, work=(0, 4), expect_error=J.JB_EINVAL)
    for name in ("post_doc", "post_tf", "post_off", "nposts"):
        device(tk, c, alias=name, expect_error=J.JB_EINVAL)
    device(tk, dict(c, doc_base=0xFFFFFFFF - 3), expect_error=J.JB_ELIMIT)
    with pytest.raises(J.JbError) as ei:
        tk.postings_device(0, 0, 0, 0, 0, 1, 5, 0, 0, 0, 0, 0, 0, 0, 0)
    assert ei.value.code == J.JB_EINVAL
    with pytest.raises(J.JbError) as ei:
        tk.postings_device(8, 8, 8, 8, (1 << 32) - T, 1, 5, 0, 8, 8, 0, 8, 8, 8, 1 << 40)
    assert ei.value.code == J.JB_ELIMIT


def test_profile_lists_the_kernels(forms):
    c = [x for x in CASES if x["label"] == "digits nids=65536"][0]
    for f in FORMS:
        tk = forms[f]
        tk.profile(True)
        try:
            tk.profile_reset()
            same(device(tk, c), want_of(c), f"profiled form={f}")
            prof = tk.profile_read()
            # three passes for 17 bits: the launches depend on nids alone
            assert prof["k_post_hist"][1] == 3 and prof["k_post_scan"][1] == 3 and prof["k_post_scatter"][1] == 3
            assert prof["k_post_off"][1] == 1
        finally:
            tk.profile(False)


# ---- 8. the chain on the device --------------------------------------------------------------------------------------
def chain_docs(seed=23, ndocs=200):
    """Seeded documents over the mini dictionary's words, ASCII words w0 .. w11999 and punctuation; document 7
    holds 10,000 distinct ASCII words, so its row spans several tiles."""
    rng = np.random.default_rng(seed)
    parts = ["今天", "天氣", "很好", "我", "昨天", "去", "上海", "交通", "大學", "這", "的", "一刹那", "，", "。", " ", "abc", "2024"]
    docs = []
    for d in range(ndocs):
        n = int(rng.integers(0, 70))
        words = [parts[int(rng.integers(0, len(parts)))] if rng.random() < 0.6 else "w%d " % int(rng.integers(0, 12_000))
                 for _ in range(n)]
        if d == 7:
            words = ["w%d " % k for k in rng.permutation(12_000)[:10_000]]
        docs.append("".join(words).encode())
    return docs


def chain_keys():
    return ([k.encode() for k in ("今天", "天氣", "很好", "昨天", "上海", "交通", "大學", "的", "一刹那", "刹那", "abc", "2024")] +
            [b"w%d" % k for k in range(11_500)])


def run_chain(tk, buf, off, nids, rule=None):
    """search cut (-> filter) -> ids -> terms -> postings and df on one stream without a wait between.  Returns the
    CSR copied back, the postings and the df counters."""
    import torch
    nb, nd = int(off[-1]), len(off) - 1
    st = torch.cuda.current_stream().cuda_stream
    d_text = torch.from_numpy(np.concatenate([buf[:nb], np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64).copy()).cuda()
    cap = max(nb, 1)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")  # noqa: E731
    o_s, o_e, o_i, t_id, t_cnt = i32(cap), i32(cap), i32(cap), i32(cap), i32(cap)
    o_d, o_n, t_off, t_n = i64(nd + 1), i64(1), i64(nd + 1), i64(1)
    tk.cut_device_search_into(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, o_s.data_ptr(), o_e.data_ptr(), cap,
                              o_d.data_ptr(), o_n.data_ptr(), st)
    held = []
    if rule is not None:
        f_s, f_e, f_d, f_n, f_st = i32(cap), i32(cap), i64(nd + 1), i64(1), i64(5)
        fneed = J.filter_work_bytes(cap, nd)
        fwork = torch.empty(fneed, dtype=torch.uint8, device="cuda")
        tk.filter_device(d_text.data_ptr(), nb, o_s.data_ptr(), o_e.data_ptr(), o_d.data_ptr(), o_n.data_ptr(), cap, nd,
                         rule, f_s.data_ptr(), f_e.data_ptr(), 0, cap, f_d.data_ptr(), f_n.data_ptr(), f_st.data_ptr(),
                         fwork.data_ptr(), fneed, st)
        held = [o_s, o_e, o_d, o_n, fwork, f_st]
        o_s, o_e, o_d, o_n = f_s, f_e, f_d, f_n
    tk.ids_device(d_text.data_ptr(), nb, o_s.data_ptr(), o_e.data_ptr(), o_n.data_ptr(), cap, o_i.data_ptr(), st)
    need = J.terms_work_bytes(cap, nd)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    tk.terms_device(o_i.data_ptr(), cap, o_d.data_ptr(), o_n.data_ptr(), nd, t_id.data_ptr(), t_cnt.data_ptr(), cap,
                    t_off.data_ptr(), t_n.data_ptr(), work.data_ptr(), need, st)
    pneed = J.postings_work_bytes(cap, nids, nd)
    pwork = torch.empty(pneed, dtype=torch.uint8, device="cuda")
    p_d, p_t, p_o, p_n, d_df = i32(cap), i32(cap), i64(nids + 1), i64(1), i32(nids)
    tk.postings_device(t_id.data_ptr(), t_cnt.data_ptr(), t_off.data_ptr(), t_n.data_ptr(), cap, nd, nids, 0,
                       p_d.data_ptr(), p_t.data_ptr(), cap, p_o.data_ptr(), p_n.data_ptr(), pwork.data_ptr(), pneed, st)
    tk.df_device(t_id.data_ptr(), t_n.data_ptr(), cap, d_df.data_ptr(), nids, st)
    torch.cuda.synchronize()
    del held
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
    nt, n = int(u64(t_n)[0]), int(u64(p_n)[0])
    return (u32(t_id)[:nt], u32(t_cnt)[:nt], u64(t_off)), (u32(p_d)[:n], u32(p_t)[:n], u64(p_o), n), u32(d_df)


@pytest.mark.parametrize("filtered", [False, True])
def test_device_chain(forms, filtered):
    buf, off = R.batch_of(chain_docs())
    keys = chain_keys()
    nids = len(keys)
    rule = J.filter_rule(("other", "invalid"), 2, 0, False) if filtered else None
    got = {}
    for f in FORMS:
        forms[f].set_vocab(keys)
        csr, post, df = run_chain(forms[f], buf, off, nids, rule)
        assert int(csr[2][8] - csr[2][7]) > 2 * T, "one row spans several tiles"
        assert len(csr[0]) > 3 * T and (csr[0] >= nids).sum() == 0
        want = PR.postings(*csr, nids=nids)
        same(post, want, f"chain form={f} filtered={filtered}")
        assert np.array_equal(np.diff(post[2].astype(np.int64)), df), "the list lengths are jb_df_device's counters"
        assert np.array_equal(df, DR.df(csr[0], len(csr[0]), len(csr[0]), nids))
        for t in np.flatnonzero(df > 1)[:200]:
            assert (np.diff(post[0][int(post[2][t]):int(post[2][t + 1])].astype(np.int64)) > 0).all()
        got[f] = post
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[0][:3], got[1][:3]))
    if filtered:  # one-rune words are gone: "的" is in no list
        t = keys.index("的".encode())
        assert got[0][2][t] == got[0][2][t + 1]


# ---- 9. jb_postings_batch and build_index ----------------------------------------------------------------------------
def test_postings_batch_and_build_index(mini_paths):
    docs = chain_docs(29, 120)
    keys = chain_keys()
    nids = len(keys)
    tk = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    try:
        buf, off = R.batch_of(docs)
        with pytest.raises(J.JbError) as ei:
            tk.postings_batch(buf, off, True, nids=nids)
        assert ei.value.code == J.JB_EINVAL  # no vocabulary
        tk.set_vocab(keys)
        po, pd, pt, dl = tk.postings_batch(buf, off, True)
        assert len(po) == nids + 1 and int(po[-1]) == len(pd) == len(pt) > 2 * T
        # the reference: the plain cut's ids, counted per document
        s, e, dt = tk.cut_batch(buf, off, True)
        ids = tk.spans_ids(bytes(buf[:int(off[-1])]), s, e)
        assert np.array_equal(dl, np.diff(np.asarray(dt, np.int64)).astype(np.uint32)), "doc_len is the doc_tok differences"
        rows, cnts, roff = [], [], [0]
        for d in range(len(docs)):
            u, c = np.unique(ids[int(dt[d]):int(dt[d + 1])], return_counts=True)
            keep = u != 0xFFFFFFFF
            rows.append(u[keep])
            cnts.append(c[keep])
            roff.append(roff[-1] + int(keep.sum()))
        want = PR.postings(np.concatenate(rows).astype(np.uint32), np.concatenate(cnts).astype(np.uint32),
                           np.array(roff, np.uint64), nids=nids)
        same((pd, pt, po, len(pd)), want, "jb_postings_batch")
        # two batches with a running doc_base are one batch of all documents
        cut = 47
        ba, bb = R.batch_of(docs[:cut]), R.batch_of(docs[cut:])
        a = tk.postings_batch(*ba, True, 0)
        b = tk.postings_batch(*bb, True, cut)
        assert np.array_equal(np.concatenate([a[3], b[3]]), dl)
        for t in range(nids):
            one = np.concatenate([a[1][int(a[0][t]):int(a[0][t + 1])], b[1][int(b[0][t]):int(b[0][t + 1])]])
            assert np.array_equal(one, pd[int(po[t]):int(po[t + 1])]), t
        ipo, ipd, ipt, idl, ind = tk.build_index([[d for d in docs[:cut]], [], [d for d in docs[cut:]]], hmm=True)
        assert ind == len(docs) and np.array_equal(ipo, po) and np.array_equal(ipd, pd) and np.array_equal(ipt, pt)
        assert np.array_equal(idl, dl)
        # JB_ELIMIT at a short pcap, with *nposts right and post_off complete
        n = C.c_uint64()
        qo = np.zeros(nids + 1, np.uint64)
        qd, qt = np.full(100, 0xABABABAB, np.uint32), np.full(100, 0xABABABAB, np.uint32)
        rc = J.lib().jb_postings_batch(tk.h, buf.ctypes.data, off.ctypes.data, len(docs), 1, 0, 100, qo.ctypes.data, nids,
                                       qd.ctypes.data, qt.ctypes.data, C.byref(n), None)
        assert rc == J.JB_ELIMIT and n.value == len(pd) and np.array_equal(qo, po)
        assert (qd == 0xABABABAB).all() and (qt == 0xABABABAB).all()
        with pytest.raises(J.JbError) as ei:
            tk.postings_batch(buf, off, True, pcap=100)
        assert ei.value.code == J.JB_ELIMIT
        # concurrent calls from two threads take turns
        errs, res = [], {}

        def run(k):
            try:
                for _ in range(3):
                    res[k] = tk.postings_batch(*(ba if k == 0 else bb), True, 0 if k == 0 else cut)
            except BaseException as ex:  # noqa: BLE001 (reported below)
                errs.append(ex)

        th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not errs, errs
        for k, w in ((0, a), (1, b)):
            assert all(np.array_equal(x, y) for x, y in zip(res[k], w))
    finally:
        tk.close()


# ---- 10. the C++ mirror ----------------------------------------------------------------------------------------------
def test_cpp_consumer(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "cpp_postings_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_postings_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "postings ok" in r.stdout, r.stderr + r.stdout
