"""GPU: document frequencies and IDF weights (jb_df_device, jb_idf_device, jb_df_batch; jb_terms.hip)
against numpy (df_ref.py: np.bincount over the flat term list) and against jb_idf, the host form of the
rule.  Most tests hand the kernels term lists they built themselves, in both forms of the df kernel
(JB_DF_COMBINE, read at jb_open: one tokenizer per form)."""
import os
import subprocess
import threading

import numpy as np
import pytest

import df_ref as DR
import jiebahip as J
import oracle as O
import search_ref as R
import synth
import terms_ref as TR
import vocab_ref as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNK = TR.UNK
GUARD = 0x7A7A7A7A  # the canaries after the counters
NCANARY = 64
FORMS = [0, 1]  # JB_DF_COMBINE


def _dev(a, dtype, view=None):
    import torch
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(view) if view is not None else a).cuda()


@pytest.fixture(scope="module")
def forms(mini_paths):
    """{form: a tokenizer opened with JB_DF_COMBINE=form} (the knob is read at jb_open)."""
    old = os.environ.get("JB_DF_COMBINE")
    tks = {}
    try:
        for f in FORMS:
            os.environ["JB_DF_COMBINE"] = str(f)
            tks[f] = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    finally:
        if old is None:
            os.environ.pop("JB_DF_COMBINE", None)
        else:
            os.environ["JB_DF_COMBINE"] = old
    yield tks
    for tk in tks.values():
        tk.close()


def dev_df(tk, ids, ndf, nterms=None, cap=None, df0=None, shift=0, stream=None):
    """jb_df_device on a term list of the test's own -> df u32[ndf].  The id buffer is an allocation of
    exactly cap entries (+ shift: the list then starts `shift` entries after a 16-byte boundary); the
    counters start as df0 (zeros) and are followed by NCANARY canaries, which must not change."""
    import torch
    ids = np.asarray(ids, np.uint32)
    cap = len(ids) if cap is None else cap
    nterms = len(ids) if nterms is None else nterms
    held = np.concatenate([np.full(shift, 3, np.uint32), ids[:cap]])
    d_ids = _dev(held if len(held) else np.zeros(1, np.uint32), np.uint32, np.int32)
    assert d_ids.data_ptr() % 16 == 0
    d_n = torch.tensor([nterms], dtype=torch.int64, device="cuda")
    start = np.zeros(ndf, np.uint32) if df0 is None else np.asarray(df0, np.uint32)
    d_df = _dev(np.concatenate([start, np.full(NCANARY, GUARD, np.uint32)]), np.uint32, np.int32)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    tk.df_device(d_ids.data_ptr() + 4 * shift, d_n.data_ptr(), cap, d_df.data_ptr(), ndf, st)
    torch.cuda.synchronize()
    got = d_df.cpu().numpy().view(np.uint32)
    assert (got[ndf:] == GUARD).all(), "written at or past d_df[ndf]"
    return got[:ndf]


def same_df(got, want, label):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{label}: {len(bad)} counters differ; first id {bad[0]}: got {got[bad[:6]].tolist()} "
                             f"want {want[bad[:6]].tolist()}")


# ---- 1. hand-checked -------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_hand_checked(forms, form):
    # three documents: {1, 4, 9}, {4}, {0, 4, 9, 11}; ndf = 10, so id 11 is skipped
    term_id = [1, 4, 9, 4, 0, 4, 9, 11]
    assert dev_df(forms[form], term_id, 10).tolist() == [1, 1, 0, 0, 3, 0, 0, 0, 0, 2]
    assert dev_df(forms[form], term_id, 12).tolist() == [1, 1, 0, 0, 3, 0, 0, 0, 0, 2, 0, 1]
    assert dev_df(forms[form], term_id, 1).tolist() == [1]
    # ndf = 0: valid, nothing is added (the canaries say so)
    assert len(dev_df(forms[form], term_id, 0)) == 0


# ---- 2. list lengths ---------------------------------------------------------------------------------
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4097, 70_001]


@pytest.mark.parametrize("form", FORMS)
def test_list_lengths(forms, form):
    """Wave, workgroup and share edges and the tail; ids 256..299 and one 0xFFFFFFFF are skipped.  Each
    length also with the list starting 1, 2 and 3 entries after a 16-byte boundary."""
    rng = np.random.default_rng(61)
    for n in LENGTHS:
        ids = rng.integers(0, 300, n).astype(np.uint32)
        if n:
            ids[n // 2] = 0xFFFFFFFF
        want = DR.df(ids, n, n, 256)
        assert n < 300 or (want.sum() < n - 1 and (ids >= 256).sum() > 1)
        for shift in range(4):
            same_df(dev_df(forms[form], ids, 256, shift=shift), want, f"n={n} shift={shift} form={form}")


# ---- 3. contention and table collisions ---------------------------------------------------------
def colliding(n=20_000):
    """ids 3 + k * 2^j, j = 10..20: they share the low bits, so they collide in any power-of-two table."""
    js = np.arange(10, 21)
    pool = np.concatenate([3 + np.arange(1, 5, dtype=np.uint32) * (1 << j) for j in js]).astype(np.uint32)
    return pool[np.arange(n) % len(pool)]


@pytest.mark.parametrize("form", FORMS)
def test_contention_and_collisions(forms, form):
    tk = forms[form]
    # 5,000 one-term rows, all id 7
    got = dev_df(tk, np.full(5000, 7, np.uint32), 16)
    assert got[7] == 5000 and got.sum() == 5000
    ndf = 3 + 4 * (1 << 20) + 1
    ids = colliding()
    same_df(dev_df(tk, ids, ndf), DR.df(ids, len(ids), len(ids), ndf), f"collisions form={form}")
    rng = np.random.default_rng(67)
    mixed = np.concatenate([ids, rng.integers(0, 200, 20_000).astype(np.uint32)])
    rng.shuffle(mixed)
    want = DR.df(mixed, len(mixed), len(mixed), ndf)
    assert (want[:200] > 0).all()
    same_df(dev_df(tk, mixed, ndf), want, f"collisions among low ids form={form}")


def test_the_forms_agree(forms):
    rng = np.random.default_rng(71)
    ids = (rng.zipf(1.3, 50_000) % 5000).astype(np.uint32)
    a, b = dev_df(forms[0], ids, 4096), dev_df(forms[1], ids, 4096)
    same_df(a, b, "the two forms")
    same_df(a, DR.df(ids, len(ids), len(ids), 4096), "zipf")


# ---- 4. accumulation and an overflowed CSR ---------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_accumulation(forms, form):
    tk = forms[form]
    rng = np.random.default_rng(73)
    a, b = rng.integers(0, 500, 9000).astype(np.uint32), rng.integers(100, 700, 5001).astype(np.uint32)
    wa, wb = DR.df(a, len(a), len(a), 600), DR.df(b, len(b), len(b), 600)
    one = dev_df(tk, a, 600)
    two = dev_df(tk, b, 600, df0=one)
    same_df(two, wa + wb, f"two calls form={form}")
    same_df(dev_df(tk, a, 600, nterms=0, df0=two), wa + wb, f"*d_nterms = 0 form={form}")
    # counters near the top of u32 just add
    top = np.full(600, 0xFFFFFFFF, np.uint32) - wa
    assert (dev_df(tk, a, 600, df0=top) == 0xFFFFFFFF).all()


@pytest.mark.parametrize("form", FORMS)
def test_overflowed_csr(forms, form):
    """*d_nterms = cap + 1000: the list is read up to cap, the size of its allocation, and no further."""
    rng = np.random.default_rng(79)
    ids = rng.integers(0, 400, 12_000).astype(np.uint32)
    for cap in (0, 1, 5, 4096, 4099, 10_001):
        for shift in (0, 3):
            got = dev_df(forms[form], ids, 400, nterms=cap + 1000, cap=cap, shift=shift)
            same_df(got, DR.df(ids, cap + 1000, cap, 400), f"cap={cap} shift={shift} form={form}")
    # and the other way round: cap beyond the count
    same_df(dev_df(forms[form], ids, 400, nterms=777, cap=12_000), DR.df(ids, 777, 12_000, 400), "nterms < cap")


# ---- 5. jb_idf_device against jb_idf ---------------------------------------------------------------
IDF_DF = np.concatenate([np.arange(65536, dtype=np.uint32), np.array([2**31, 2**32 - 2, 2**32 - 1], np.uint32)])
IDF_NDOCS = [0, 1, 2, 73_443, 2**32 + 5, 2**53 - 2]
IDF_FILTERS = [(1, None, "null"), (0, None, "alternating"), (2, 5, "alternating"), (1000, None, "null"),
               (1, 0, "null"), (1, None, "zero")]


@pytest.mark.parametrize("ndocs", IDF_NDOCS)
def test_idf_device_is_jb_idf_bit_for_bit(forms, ndocs):
    """Pins the device logarithm and the f64 divide: every df 0..65535 and three large ones."""
    import torch
    tk = forms[1]
    n = len(IDF_DF)
    d_df = _dev(IDF_DF, np.uint32, np.int32)
    keeps = {"null": None, "zero": np.zeros(n, np.uint8), "alternating": (np.arange(n) & 1).astype(np.uint8)}
    st = torch.cuda.current_stream().cuda_stream
    for min_df, max_df, kname in IDF_FILTERS:
        keep = keeps[kname]
        want = J.idf(IDF_DF, ndocs, min_df, max_df, keep)
        d_keep = _dev(keep, np.uint8) if keep is not None else None
        d_w = torch.full((n + NCANARY,), float("nan"), dtype=torch.float32, device="cuda")
        tk.idf_device(d_df.data_ptr(), n, ndocs, d_w.data_ptr(), min_df, max_df,
                      d_keep.data_ptr() if d_keep is not None else 0, st)
        torch.cuda.synchronize()
        got = d_w.cpu().numpy()
        label = (ndocs, min_df, max_df, kname)
        assert np.isnan(got[n:]).all(), (label, "written past ndf")
        got = got[:n]
        assert not np.isnan(got).any(), (label, "a slot was not written")
        if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            raise AssertionError(f"{label}: {len(bad)} weights differ; first df={IDF_DF[bad[0]]}: got {got[bad[0]]!r} "
                                 f"want {want[bad[0]]!r}")
    # the errors are the host rule's
    with pytest.raises(J.JbError) as ei:
        tk.idf_device(d_df.data_ptr(), n, 2**53, d_w.data_ptr())
    assert ei.value.code == J.JB_ELIMIT
    with pytest.raises(J.JbError) as ei:
        tk.idf_device(0, n, 5, d_w.data_ptr())
    assert ei.value.code == J.JB_EINVAL
    tk.idf_device(0, 0, 5, 0)  # ndf = 0: valid


def test_profile_reports_the_kernels(forms):
    """With profiling on the calls take their timed variant, and jb_profile_read names both kernels."""
    import torch
    for form in FORMS:
        tk = forms[form]
        tk.profile(True)
        try:
            tk.profile_reset()
            ids = np.arange(5000, dtype=np.uint32) % 97
            same_df(dev_df(tk, ids, 100), DR.df(ids, 5000, 5000, 100), f"profiled form={form}")
            d_df = _dev(np.arange(100), np.uint32, np.int32)
            d_w = torch.zeros(100, dtype=torch.float32, device="cuda")
            tk.idf_device(d_df.data_ptr(), 100, 1000, d_w.data_ptr(), stream_ptr=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(d_w.cpu().numpy().view(np.uint32), J.idf(np.arange(100), 1000).view(np.uint32))
            prof = tk.profile_read()
            assert prof["k_df"][1] == 1 and prof["k_idf"][1] == 1, prof
        finally:
            tk.profile(False)


# ---- 6. end to end -----------------------------------------------------------------------------------
TOPK = 20


def make_vocab(o, batches):
    """A fixed-seed half of the distinct tokens of the oracle's hmm = 1 cut of the batches."""
    toks = set()
    for buf, off in batches:
        data = bytes(buf)
        s, e, _ = o.cut_batch(buf, off, True, nthreads=8)
        toks |= {V.span_key(data, a, b) for a, b in zip(s.astype(np.int64).tolist(), e.astype(np.int64).tolist())}
    toks = sorted(toks)
    rng = np.random.default_rng(83)
    return [toks[i] for i in np.flatnonzero(rng.random(len(toks)) < 0.5)]


def ref_csr(o, vocab, buf, off, hmm):
    s, e, d = o.cut_batch(buf, off, hmm, nthreads=8)
    ids = V.expect_ids(vocab, bytes(buf), np.asarray(s, np.int64).tolist(), np.asarray(e, np.int64).tolist())
    return TR.terms(ids, d, len(ids), len(ids))


def device_chain(tk, buf, off, hmm, d_df, ndf, stream=None):
    """cut -> ids -> terms -> df, queued on one stream without a host sync in between, into arrays of the
    call's own; d_df accumulates.  Returns the arrays, which must outlive the queued work."""
    import torch
    nb, nd = int(off[-1]), len(off) - 1
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    d_text = torch.from_numpy(np.frombuffer(bytes(buf[:nb]) + b"\0" * 64, np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    cap = max(nb, 1)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")  # noqa: E731
    o_s, o_e, o_i, t_id, t_cnt = i32(cap), i32(cap), i32(cap), i32(cap), i32(cap)
    o_d, o_n, t_off, t_n = i64(nd + 1), i64(1), i64(nd + 1), i64(1)
    need = J.terms_work_bytes(cap, nd)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    tk.cut_device_into(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, o_s.data_ptr(), o_e.data_ptr(), cap,
                       o_d.data_ptr(), o_n.data_ptr(), st)
    tk.ids_device(d_text.data_ptr(), nb, o_s.data_ptr(), o_e.data_ptr(), o_n.data_ptr(), cap, o_i.data_ptr(), st)
    tk.terms_device(o_i.data_ptr(), cap, o_d.data_ptr(), o_n.data_ptr(), nd, t_id.data_ptr(), t_cnt.data_ptr(), cap,
                    t_off.data_ptr(), t_n.data_ptr(), work.data_ptr(), need, st)
    tk.df_device(t_id.data_ptr(), t_n.data_ptr(), cap, d_df.data_ptr(), ndf, st)
    return (d_text, d_off, o_s, o_e, o_i, t_id, t_cnt, o_d, o_n, t_off, t_n, work)


def docs_of(buf, off):
    data = bytes(buf)
    return [data[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


@pytest.mark.parametrize("hmm", [False, True])
def test_end_to_end(syn_small, hmm):
    import torch
    dp, ep, s = syn_small
    batches = [s.corpus(synth.KIND_DOCS, 1300, target_bytes=1600 << 10)[:2],
               s.corpus(synth.KIND_DOCS, 1500, target_bytes=1400 << 10)[:2]]
    ndocs = sum(len(off) - 1 for _, off in batches)
    assert 150 <= ndocs <= 250  # (documents of about 15 KB)
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
    o = O.Oracle.from_files(dp, ep, 0)
    try:
        keys = make_vocab(o, batches)
        vocab = V.key_dict(keys)
        ndf = len(keys)
        tk.set_vocab(keys)
        csrs = [ref_csr(o, vocab, buf, off, hmm) for buf, off in batches]
        want = sum(DR.df(c[0], len(c[0]), len(c[0]), ndf).astype(np.int64) for c in csrs).astype(np.uint32)
        # frequent and rare ids, and (the vocabulary comes from the hmm = 1 cut) with hmm off absent ones
        assert want.max() > ndocs // 2 and (want == 1).any() and ((want == 0).any() or hmm)
        # the device chain over the two batches, one sync at the end
        d_df = torch.zeros(ndf + NCANARY, dtype=torch.int32, device="cuda")
        d_df[ndf:] = GUARD
        held = [device_chain(tk, buf, off, hmm, d_df, ndf) for buf, off in batches]
        torch.cuda.synchronize()
        got = d_df.cpu().numpy().view(np.uint32)
        assert (got[ndf:] == GUARD).all()
        same_df(got[:ndf], want, f"device chain hmm={hmm}")
        for h, c in zip(held, csrs):
            assert int(h[10].cpu()[0]) == len(c[0])
        # jb_df_batch over the same batches
        df = np.zeros(ndf, np.uint32)
        for buf, off in batches:
            tk.df_batch(buf, off, hmm, df)
        same_df(df, want, f"jb_df_batch hmm={hmm}")
        # fit_idf, then extract_tags with the fitted weights: the whole of TF-IDF
        keep = np.array([len(k.decode("utf-8", "replace")) >= 2 for k in keys], np.uint8)
        texts = [docs_of(buf, off) for buf, off in batches]
        for kw in ({}, {"min_df": 2, "max_df": ndocs // 2, "keep": keep}):
            w, fdf, fnd = tk.fit_idf(texts, hmm=hmm, **kw)
            same_df(fdf, want, "fit_idf's df")
            assert fnd == ndocs and w.dtype == np.float32 and len(w) == ndf
            wref = DR.idf(want, ndocs, kw.get("min_df", 1), kw.get("max_df", DR.NOMAX), kw.get("keep"))
            assert np.array_equal(w.view(np.uint32), wref.view(np.uint32)), kw
            assert (w > 0).sum() > 100
            for text, c in zip(texts, csrs):
                kid, ksc, kcn, kn = TR.keywords(c, wref, TOPK)
                ref = [[(int(kid[d, r]), float(ksc[d, r]), int(kcn[d, r])) for r in range(int(kn[d]))]
                       for d in range(len(text))]
                assert tk.extract_tags(text, w, topK=TOPK, hmm=hmm) == ref
    finally:
        tk.close()


# ---- 7. threads -----------------------------------------------------------------------------------------
def test_threads(syn_small):
    """4 threads, each with its own stream, arrays and counters, run the device chain on one ctx at once,
    3 rounds each into the same counters; every result is 3 x the reference."""
    import torch
    dp, ep, s = syn_small
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
    o = O.Oracle.from_files(dp, ep, 0)
    batches = [s.corpus(synth.KIND_DOCS, 190 + k, target_bytes=(96 + 32 * k) << 10)[:2] for k in range(4)]
    keys = make_vocab(o, batches[:1])
    vocab = V.key_dict(keys)
    ndf = len(keys)
    tk.set_vocab(keys)
    want = []
    for b in batches:
        c = ref_csr(o, vocab, *b, True)
        want.append(DR.df(c[0], len(c[0]), len(c[0]), ndf))
    errs = []

    def run(k):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                d_df = torch.zeros(ndf, dtype=torch.int32, device="cuda")
                held = [device_chain(tk, *batches[k], True, d_df, ndf, st.cuda_stream) for _ in range(3)]
                st.synchronize()
                same_df(d_df.cpu().numpy().view(np.uint32), 3 * want[k], f"thread {k}")
                del held
        except BaseException as e:  # noqa: BLE001 (reported below)
            errs.append(e)

    try:
        th = [threading.Thread(target=run, args=(k,)) for k in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not errs, errs
    finally:
        tk.close()


# ---- 8. C and C++ programs --------------------------------------------------------------------------------
# the documents and keys of tests/c_abi_df.c
C_DOCS = [b"abc abc \xe4\xbb\x8a\xe5\xa4\xa9", "abc \xff".encode("latin-1") + "今天天氣 这一刹那".encode(),
          "这一刹那 今天".encode(), b"", "刹那 abc".encode()]
C_KEYS = [k.encode() for k in ("abc", "今天", "�", "一刹那", "刹那", "这", "天天")]


def test_c_and_cpp_consumers(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "c_abi_df")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_df.c"), "-L", lib,
                           "-ljiebahip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "df ok" in r.stdout, r.stdout + r.stderr
    # the reference: the oracle's cut of the same documents, the dict over the same keys
    o = O.Oracle.from_files(mini_paths[0], mini_paths[1], 0)
    buf, off = R.batch_of(C_DOCS)
    c = ref_csr(o, V.key_dict(C_KEYS), buf, off, False)
    want_df = DR.df(c[0], len(c[0]), len(c[0]), len(C_KEYS))
    assert want_df.tolist() == [3, 3, 1, 2, 1, 2, 0]
    want_w = DR.idf(want_df, len(C_DOCS))
    lines = r.stdout.split("\n")
    assert f"ndocs {len(C_DOCS)}" in lines
    for i in range(len(C_KEYS)):
        assert f"df {i} {want_df[i]}" in lines, r.stdout
        assert f"weight {i} {int(want_w[i:i + 1].view(np.uint32)[0]):08x}" in lines, r.stdout
    exe = str(tmp_path / "cpp_df_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_df_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "df ok" in r.stdout, r.stdout + r.stderr
