"""GPU: TextRank keywords (jb_textrank_device, jb_textrank_batch; jb_textrank.hip) against jb_textrank, the
host form of the rule, and against textrank_ref.py, bit for bit: ids, f32 score bits and kw_n.  Most tests
hand the kernels id lists and CSR rows they built themselves, in both forms of the push kernel
(JB_TR_WINDOW, read at jb_open: one tokenizer per form)."""
import os
import subprocess

import numpy as np
import pytest

import jiebahip as J
import search_ref as R
import synth
import terms_ref as TR
import textrank_cases as TC
import textrank_ref as KR
import vocab_ref as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNK = KR.UNK
GUARD = 0x7A7A7A7A
NG = 64  # canary words on each side of every output and of the work buffer
FORMS = [0, 1]  # JB_TR_WINDOW


def _dev(a, dtype, view=None):
    import torch
    a = np.ascontiguousarray(a, dtype)
    if len(a) == 0:
        a = np.zeros(1, dtype)
    return torch.from_numpy(a.view(view) if view is not None else a).cuda()


@pytest.fixture(scope="module")
def forms(mini_paths):
    """{form: a tokenizer opened with JB_TR_WINDOW=form} (the knob is read at jb_open)."""
    old = os.environ.get("JB_TR_WINDOW")
    tks = {}
    try:
        for f in FORMS:
            os.environ["JB_TR_WINDOW"] = str(f)
            tks[f] = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    finally:
        if old is None:
            os.environ.pop("JB_TR_WINDOW", None)
        else:
            os.environ["JB_TR_WINDOW"] = old
    yield tks
    for tk in tks.values():
        tk.close()


def guarded(n, fill, dtype):
    """A device array of n entries between two rows of NG canary words; fill is what the entries start as."""
    import torch
    t = torch.full((n + 2 * NG,), fill, dtype=dtype, device="cuda")
    t[:NG] = GUARD
    t[NG + n:] = GUARD
    return t


def intact(t, n):
    g = t.cpu().numpy().view(np.uint32)
    return (g[:NG] == GUARD).all() and (g[NG + n:] == GUARD).all()


def dev_textrank(tk, case, work_fill=0x5B, raw=False):
    """jb_textrank_device on the case's arrays -> (kw_id, kw_score, kw_n), or with raw the outputs' bytes.
    The id and term arrays are allocations of exactly ids_cap and cap entries; the outputs start as
    garbage, and they and the work buffer lie between canaries, which must not change."""
    import torch
    nd = len(case.doc_tok) - 1
    d_ids = _dev(case.ids[:case.ids_cap], np.uint32, np.int32)
    d_doc = _dev(case.doc_tok, np.uint64, np.int64)
    d_n = torch.tensor([case.ntok], dtype=torch.int64, device="cuda")
    d_tid = _dev(case.term_id[:case.cap], np.uint32, np.int32)
    d_toff = _dev(case.term_off, np.uint64, np.int64)
    d_keep = _dev(case.keep, np.uint8)
    nrec = nd * case.topk
    o_id, o_sc, o_n = guarded(nrec, 0x33333333, torch.int32), guarded(nrec, 0x33333333, torch.int32), \
        guarded(nd, 0x33333333, torch.int32)
    need = J.textrank_work_bytes(case.ids_cap, case.cap, nd)
    work = torch.full((need + 8 * NG,), work_fill, dtype=torch.uint8, device="cuda")  # (garbage between canaries)
    work[:4 * NG] = 0x7A
    work[4 * NG + need:] = 0x7A
    tk.textrank_device(d_ids.data_ptr(), case.ids_cap, d_doc.data_ptr(), d_n.data_ptr(), nd, d_tid.data_ptr(),
                       d_toff.data_ptr(), case.cap, d_keep.data_ptr(), len(case.keep), o_id.data_ptr() + 4 * NG,
                       o_sc.data_ptr() + 4 * NG, o_n.data_ptr() + 4 * NG, work.data_ptr() + 4 * NG, need, case.span,
                       case.iters, case.topk, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert intact(o_id, nrec) and intact(o_sc, nrec) and intact(o_n, nd), f"{case}: written outside an output"
    wb = work.cpu().numpy()
    assert (wb[:4 * NG] == 0x7A).all() and (wb[4 * NG + need:] == 0x7A).all(), f"{case}: written outside the work buffer"
    got = [t.cpu().numpy()[NG:NG + n] for t, n in ((o_id, nrec), (o_sc, nrec), (o_n, nd))]
    if raw:
        return b"".join(g.tobytes() for g in got)
    return (got[0].view(np.uint32).reshape(nd, case.topk), got[1].view(np.float32).reshape(nd, case.topk),
            got[2].view(np.uint32))


def host(case):
    return J.textrank(case.ids, case.doc_tok, case.term_id, case.term_off, case.keep, **case.args())


def check(tk, case, label):
    """device == reference == jb_textrank, bit for bit."""
    got = dev_textrank(tk, case)
    TC.same(got, case, label)
    TC.same(host(case), case, "jb_textrank")
    return got


# ---- 1. the host cases ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_host_cases(forms, form):
    for case in TC.host_cases():
        check(forms[form], case, f"form={form}")


@pytest.mark.parametrize("form", FORMS)
def test_zipf_documents(forms, form):
    for n, seed in TC.ZIPF[:2]:
        check(forms[form], TC.zipf_case(n, seed), f"form={form}")


# ---- 2. many small documents, one large one with a hot id ---------------------------------------------
@pytest.fixture(scope="module")
def tiny_docs():
    """5,000 documents of 0 to 8 tokens over 12 ids (one unkept, some unknown)."""
    rng = np.random.default_rng(107)
    docs = []
    for n in rng.integers(0, 9, 5000):
        d = rng.integers(0, 12, n).astype(np.uint32)
        d[rng.random(n) < 0.1] = UNK
        docs.append(d.tolist())
    keep = np.ones(12, np.uint8)
    keep[4] = 0
    return TC.Case("5000-tiny-documents", docs, keep, span=5, topk=5)


@pytest.fixture(scope="module")
def hot_doc():
    """One document of 20,000 tokens whose id 3 holds about 5 % of them: it spans many workgroups, which
    all add to one address."""
    rng = np.random.default_rng(109)
    d = (rng.zipf(1.3, 20_000) % 3000 + 10).astype(np.uint32)
    d[rng.random(20_000) < 0.05] = 3
    assert 800 < (d == 3).sum() < 1200
    return TC.Case("hot-id", [d.tolist()], np.ones(3010, np.uint8))


@pytest.mark.parametrize("form", FORMS)
def test_tiny_documents(forms, form, tiny_docs):
    got = check(forms[form], tiny_docs, f"form={form}")
    assert (got[2] == 0).sum() > 500 and (got[2] == 5).sum() > 100


@pytest.mark.parametrize("form", FORMS)
def test_hot_id(forms, form, hot_doc):
    got = check(forms[form], hot_doc, f"form={form}")
    assert 3 in got[0][0, :6]  # (the Zipf head holds more tokens than the hot id: it ranks among the first)


# ---- 3. boundaries ----------------------------------------------------------------------------------------
def boundary_docs(o):
    """Documents whose boundaries fall at 1024 + o (a chunk of the TextRank kernels), 4096 + o (a sort tile of
    jb_terms_device) and 5120 + o, each inside the windows of its neighbours; the second document spans
    three chunk boundaries itself."""
    rng = np.random.default_rng(113 + o)
    lens = [1024 + o, 3072, 1024, 300 - o]
    docs = []
    for n in lens:
        d = rng.integers(0, 25, n).astype(np.uint32)
        d[rng.random(n) < 0.15] = UNK
        docs.append(d.tolist())
    return docs


@pytest.fixture(scope="module")
def boundary_cases():
    keep = np.ones(25, np.uint8)
    keep[11] = 0
    return [TC.Case(f"boundary{o:+d}-span{span}", boundary_docs(o), keep, span=span, iters=3, topk=25)
            for o in (-1, 0, 1) for span in (5, 32)]


@pytest.mark.parametrize("form", FORMS)
def test_boundaries(forms, form, boundary_cases):
    """The CSR comes from jb_terms_device here, so that its tile boundary is the device's own."""
    import torch
    tk = forms[form]
    for case in boundary_cases:
        assert int(case.doc_tok[1]) in (1023, 1024, 1025) and int(case.doc_tok[2]) in (4095, 4096, 4097)
        n, nd = len(case.ids), len(case.doc_tok) - 1
        d_ids, d_doc = _dev(case.ids, np.uint32, np.int32), _dev(case.doc_tok, np.uint64, np.int64)
        d_n = torch.tensor([n], dtype=torch.int64, device="cuda")
        t_id, t_cnt = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        t_off, t_n = torch.zeros(nd + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        need = J.terms_work_bytes(n, nd)
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        tk.terms_device(d_ids.data_ptr(), n, d_doc.data_ptr(), d_n.data_ptr(), nd, t_id.data_ptr(), t_cnt.data_ptr(), n,
                        t_off.data_ptr(), t_n.data_ptr(), work.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        nt = int(t_n.cpu()[0])
        assert np.array_equal(t_id.cpu().numpy().view(np.uint32)[:nt], case.term_id)
        assert np.array_equal(t_off.cpu().numpy().view(np.uint64), case.term_off)
        check(tk, case, f"form={form}")


# ---- 4. determinism, the knob, the work buffer ---------------------------------------------------------------
def test_two_runs_and_both_forms_give_identical_bytes(forms, hot_doc, tiny_docs):
    """Whatever the work buffer held before, and whichever push kernel runs."""
    for case in (hot_doc, tiny_docs):
        runs = [dev_textrank(forms[f], case, work_fill=fill, raw=True) for f in FORMS for fill in (0x5B, 0xFF, 0x00)]
        assert all(r == runs[0] for r in runs[1:]), case


def test_a_bad_work_buffer_is_refused_with_nothing_queued(forms):
    import torch
    tk = forms[1]
    case = TC.Case("bad-work", [TC.HAND], TC.ALL)
    d_ids, d_doc = _dev(case.ids, np.uint32, np.int32), _dev(case.doc_tok, np.uint64, np.int64)
    d_n = torch.tensor([4], dtype=torch.int64, device="cuda")
    d_tid, d_toff = _dev(case.term_id, np.uint32, np.int32), _dev(case.term_off, np.uint64, np.int64)
    d_keep = _dev(case.keep, np.uint8)
    out = [torch.full((64,), 0x33333333, dtype=torch.int32, device="cuda") for _ in range(3)]
    need = J.textrank_work_bytes(4, 3, 1)
    work = torch.full((need + 64,), 0x5B, dtype=torch.uint8, device="cuda")

    def call(ptr, nwork, **kw):
        a = dict(span=5, iters=10, topk=20)
        a.update(kw)
        tk.textrank_device(d_ids.data_ptr(), 4, d_doc.data_ptr(), d_n.data_ptr(), 1, d_tid.data_ptr(), d_toff.data_ptr(),
                           3, d_keep.data_ptr(), 64, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ptr, nwork,
                           a["span"], a["iters"], a["topk"], torch.cuda.current_stream().cuda_stream)

    for ptr, nwork, kw, code in ((work.data_ptr() + 4, need, {}, J.JB_EINVAL), (work.data_ptr(), need - 1, {}, J.JB_EINVAL),
                                 (work.data_ptr(), 0, {}, J.JB_EINVAL), (0, need, {}, J.JB_EINVAL),
                                 (work.data_ptr(), need, {"span": 1}, J.JB_EINVAL),
                                 (work.data_ptr(), need, {"span": 33}, J.JB_ELIMIT),
                                 (work.data_ptr(), need, {"iters": 101}, J.JB_ELIMIT),
                                 (work.data_ptr(), need, {"topk": 65}, J.JB_ELIMIT)):
        with pytest.raises(J.JbError) as ei:
            call(ptr, nwork, **kw)
        assert ei.value.code == code, (nwork, kw)
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == 0x33333333).all() for o in out) and (work.cpu().numpy() == 0x5B).all()
    call(work.data_ptr(), need)  # and the good call runs
    torch.cuda.synchronize()
    assert out[2].cpu().numpy()[0] == 3


def test_profile_reports_the_kernels(forms):
    case = TC.Case("profiled", TC.mixed_docs()[0], TC.mixed_docs()[1], iters=7)
    for form in FORMS:
        tk = forms[form]
        tk.profile(True)
        try:
            tk.profile_reset()
            TC.same(dev_textrank(tk, case), case, f"profiled form={form}")
            prof = tk.profile_read()
            assert [prof[k][1] for k in ("k_tr_init", "k_tr_setup", "k_tr_count", "k_tr_step", "k_tr_push",
                                         "k_tr_final")] == [1, 1, 1, 7, 7, 1], prof
        finally:
            tk.profile(False)


# ---- 5. the real chain ----------------------------------------------------------------------------------------
def docs_of(buf, off):
    data = bytes(buf)
    return [data[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


@pytest.fixture(scope="module")
def corpus(syn_small):
    """About 200 KiB of generated documents, the 20k dictionary, and a vocabulary of half the distinct tokens
    of its hmm = 1 cut; keep holds the keys of two runes or more."""
    dp, ep, s = syn_small
    buf, off = s.corpus(synth.KIND_DOCS, 1700, target_bytes=200 << 10)[:2]
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
    data = bytes(buf)
    st, en, _ = tk.cut_batch(buf, off, True)
    toks = sorted({V.span_key(data, a, b) for a, b in zip(st.astype(np.int64).tolist(), en.astype(np.int64).tolist())})
    rng = np.random.default_rng(127)
    keys = [toks[i] for i in np.flatnonzero(rng.random(len(toks)) < 0.5)]
    tk.set_vocab(keys)
    keep = np.array([len(k.decode("utf-8", "replace")) >= 2 for k in keys], np.uint8)
    yield tk, buf, off, keys, keep
    tk.close()


@pytest.mark.parametrize("hmm", [False, True])
def test_the_real_chain(corpus, hmm):
    """cut_device -> ids_device -> terms_device -> textrank_device on one stream with one sync at the end,
    against the reference run on the ids copied back; then textrank_batch and Tokenizer.textrank."""
    import torch
    tk, buf, off, keys, keep = corpus
    nb, nd = int(off[-1]), len(off) - 1
    st = torch.cuda.current_stream().cuda_stream
    d_text = torch.from_numpy(np.frombuffer(bytes(buf[:nb]) + b"\0" * 64, np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    cap = max(nb, 1)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")  # noqa: E731
    o_s, o_e, o_i, t_id, t_cnt = i32(cap), i32(cap), i32(cap), i32(cap), i32(cap)
    o_d, o_n, t_off, t_n = i64(nd + 1), i64(1), i64(nd + 1), i64(1)
    need = J.terms_work_bytes(cap, nd)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    need2 = J.textrank_work_bytes(cap, cap, nd)
    work2 = torch.empty(need2, dtype=torch.uint8, device="cuda")
    d_keep = _dev(keep, np.uint8)
    k_id, k_sc, k_n = i32(nd * 20), i32(nd * 20), i32(nd)
    tk.cut_device_into(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, o_s.data_ptr(), o_e.data_ptr(), cap,
                       o_d.data_ptr(), o_n.data_ptr(), st)
    tk.ids_device(d_text.data_ptr(), nb, o_s.data_ptr(), o_e.data_ptr(), o_n.data_ptr(), cap, o_i.data_ptr(), st)
    tk.terms_device(o_i.data_ptr(), cap, o_d.data_ptr(), o_n.data_ptr(), nd, t_id.data_ptr(), t_cnt.data_ptr(), cap,
                    t_off.data_ptr(), t_n.data_ptr(), work.data_ptr(), need, st)
    tk.textrank_device(o_i.data_ptr(), cap, o_d.data_ptr(), o_n.data_ptr(), nd, t_id.data_ptr(), t_off.data_ptr(), cap,
                       d_keep.data_ptr(), len(keep), k_id.data_ptr(), k_sc.data_ptr(), k_n.data_ptr(), work2.data_ptr(),
                       need2, stream_ptr=st)
    torch.cuda.synchronize()
    ntok = int(o_n.cpu()[0])
    ids = o_i.cpu().numpy().view(np.uint32)[:ntok]
    doc_tok = o_d.cpu().numpy().view(np.uint64)
    assert ntok > 20_000 and nd > 5
    tid, _, toff = TR.terms(ids, doc_tok, ntok, ntok)
    want = KR.textrank(ids, doc_tok, tid, toff, keep)
    assert (want[2] == 20).sum() > nd // 2  # most documents have more than 20 nodes
    got = (k_id.cpu().numpy().view(np.uint32).reshape(nd, 20), k_sc.cpu().numpy().view(np.float32).reshape(nd, 20),
           k_n.cpu().numpy().view(np.uint32))
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"device chain hmm={hmm}"
    hst = J.textrank(ids, doc_tok, tid, toff, keep)
    for g, w in zip(hst, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"jb_textrank hmm={hmm}"
    bat = tk.textrank_batch(buf, off, hmm, keep)
    for g, w in zip(bat, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"jb_textrank_batch hmm={hmm}"
    ref = [[(keys[int(want[0][d, r])], float(want[1][d, r])) for r in range(int(want[2][d]))] for d in range(nd)]
    assert tk.textrank(docs_of(buf, off), keep, hmm=hmm, keys=keys) == ref
    # other arguments reach the kernels: span 2, 3 rounds, the 5 best
    want = KR.textrank(ids, doc_tok, tid, toff, keep, span=2, iters=3, topk=5)
    ref = [[(int(want[0][d, r]), float(want[1][d, r])) for r in range(int(want[2][d]))] for d in range(nd)]
    assert tk.textrank(docs_of(buf, off), keep, topK=5, span=2, iters=3, hmm=hmm) == ref


def test_batch_errors(mini_paths):
    tk = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    try:
        buf, off = R.batch_of([b"abc abc", b""])
        with pytest.raises(J.JbError) as ei:  # no vocabulary attached
            tk.textrank_batch(buf, off, False, [1])
        assert ei.value.code == J.JB_EINVAL
        tk.set_vocab([b"abc"])
        for kw, code in (({"span": 1}, J.JB_EINVAL), ({"span": 33}, J.JB_ELIMIT), ({"iters": 101}, J.JB_ELIMIT),
                         ({"topk": 0}, J.JB_EINVAL), ({"topk": 65}, J.JB_ELIMIT)):
            with pytest.raises(J.JbError) as ei:
                tk.textrank_batch(buf, off, False, [1], **kw)
            assert ei.value.code == code, kw
        kid, ksc, kn = tk.textrank_batch(buf, off, False, [1], topk=2)  # abc _ abc: a self loop
        assert kn.tolist() == [1, 0] and kid.tolist() == [[0, UNK], [UNK, UNK]] and ksc.tolist() == [[1.0, 0.0], [0.0, 0.0]]
        assert tk.textrank([], [1]) == []
        assert tk.textrank(["abc abc"], []) == [[]]  # an empty keep mask: nothing is kept
    finally:
        tk.close()


# ---- 6. C and C++ programs ------------------------------------------------------------------------------------
def test_c_and_cpp_consumers(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "c_abi_textrank")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_textrank.c"), "-L", lib,
                           "-ljiebahip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "textrank ok" in r.stdout, r.stdout + r.stderr
    # the program prints its records: they are the reference's for the ids in its comment
    case = TC.Case("c", [[0, 2, 1, UNK, UNK, 5, 3], [0, 0, 1]], [1, 1, 1, 1, 1, 0, 1], span=5, iters=10, topk=3)
    wid, wsc, wn = TC.want(case)
    lines = r.stdout.split("\n")
    for d in range(2):
        assert f"n {d} {wn[d]}" in lines, r.stdout
        for k in range(3):
            assert f"rec {d} {k} {wid[d, k]} {int(wsc[d, k:k + 1].view(np.uint32)[0]):08x}" in lines, r.stdout
    exe = str(tmp_path / "cpp_textrank_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_textrank_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "textrank ok" in r.stdout, r.stdout + r.stderr
