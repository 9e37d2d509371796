"""GPU: MinHash signatures (jb_minhash_device, jb_minhash_bands_device, jb_minhash_batch; jb_minhash.hip) against
jb_minhash, the host form of the rule, bit for bit, and (for the small cases) against minhash_ref.py.  Most tests
hand the kernels spans and document offsets they built themselves, so the sketch is checked independently of
segmentation, in both forms of the signature kernel (JB_MH_FORM, read at jb_open: one tokenizer per form).  The
outputs and the work buffer lie between canaries that must not change."""
import os
import subprocess

import numpy as np
import pytest

import full_ref as F
import jiebahip as J
import minhash_ref as M
import oracle as O
import search_ref as R
import synth
import wc_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [0, 1]  # JB_MH_FORM
T = J.JB_MH_TILE  # tokens per workgroup of the staged form
NG = 64  # canary bytes on each side of every output and of the work buffer
MODES = [("cut", False), ("cut", True), ("search", False), ("search", True), ("full", False)]
MIXED = "english번역『하다』今天天氣很好，ステーションabc1231+1=2我昨天去上海*important*去"  # (test_gpu_ids.MIXED)
INVALID = b"\xff\xfe" + "中文".encode() + b"\x80abc\xe4\xb8"
TEXTS = [MIXED, INVALID, "这一刹那", MIXED, "今天天氣很好", "", "这一刹那的上海"]


def _open_forms(dp, ep):
    old = os.environ.get("JB_MH_FORM")
    tks = {}
    try:
        for f in FORMS:
            os.environ["JB_MH_FORM"] = str(f)
            tks[f] = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
    finally:
        if old is None:
            os.environ.pop("JB_MH_FORM", None)
        else:
            os.environ["JB_MH_FORM"] = old
    return tks


@pytest.fixture(scope="module")
def forms(mini_paths):
    """{form: a tokenizer opened with JB_MH_FORM=form} (the knob is read at jb_open)."""
    tks = _open_forms(*mini_paths)
    yield tks
    for tk in tks.values():
        tk.close()


@pytest.fixture(scope="module")
def syn_forms(syn_small):
    tks = _open_forms(syn_small[0], syn_small[1])
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


def device(tk, text, starts, ends, doc_tok, n, K, seed=1, ntok=None, cap=None, nbytes=None, work=None,
           expect_error=None, bands=None):
    """jb_minhash_device on host arrays: the span arrays are allocations of exactly cap entries, sig, doc_n and
    the work buffer lie between canaries.  work = (missing bytes, misalignment) asks for a bad buffer.  Returns
    (sig, doc_n), and the band keys too when bands = (B, R)."""
    import torch
    text = bytes(text)
    cap = len(starts) if cap is None else cap
    ntok = len(starts) if ntok is None else ntok
    nbytes = len(text) if nbytes is None else nbytes
    doc_tok = np.ascontiguousarray(doc_tok, np.uint64)
    nd = len(doc_tok) - 1
    d_text = torch.from_numpy(np.frombuffer(text + b"\0" * 64, np.uint8).copy()).cuda()
    d_s = torch.from_numpy(np.ascontiguousarray(starts, np.uint32)[:cap].view(np.int32).copy()).cuda() if cap else \
        torch.zeros(1, dtype=torch.int32, device="cuda")
    d_e = torch.from_numpy(np.ascontiguousarray(ends, np.uint32)[:cap].view(np.int32).copy()).cuda() if cap else \
        torch.zeros(1, dtype=torch.int32, device="cuda")
    d_tok = torch.from_numpy(doc_tok.view(np.int64).copy()).cuda()
    d_n = torch.tensor([ntok], dtype=torch.int64, device="cuda")
    need = J.minhash_work_bytes(cap, nd)
    nsig, ndn = nd * K * 4, nd * 4
    wk, p_wk = guarded(need, 0x5B)
    sg, p_sg = guarded(nsig, 0x33)
    dn, p_dn = guarded(ndn, 0x33)
    st = torch.cuda.current_stream().cuda_stream
    wmiss, wmis = work or (0, 0)
    args = (d_text.data_ptr(), nbytes, d_s.data_ptr(), d_e.data_ptr(), d_tok.data_ptr(), d_n.data_ptr(), cap, nd, n, K,
            seed, p_sg, p_dn, p_wk + wmis, need - wmiss, st)
    if expect_error is not None:
        with pytest.raises(J.JbError) as ei:
            tk.minhash_device(*args)
        assert ei.value.code == expect_error
        torch.cuda.synchronize()
        assert (payload(wk, need, "the work buffer") == 0x5B).all() and (payload(sg, nsig, "sig") == 0x33).all()
        return None
    tk.minhash_device(*args)
    keys = None
    if bands:
        B, R = bands
        ky, p_ky = guarded(nd * B * 8, 0x33)
        tk.minhash_bands_device(p_sg, p_dn, nd, K, B, R, p_ky, st)
    torch.cuda.synchronize()
    payload(wk, need, "the work buffer")
    sig = payload(sg, nsig, "sig").copy().view(np.uint32).reshape(nd, K)
    doc_n = payload(dn, ndn, "doc_n").copy().view(np.uint32)
    if bands:
        keys = payload(ky, nd * B * 8, "the band keys").copy().view(np.uint64).reshape(nd, B)
        return sig, doc_n, keys
    return sig, doc_n


def check(tks, text, s, e, dt, n, K, seed=1, ref=False, label="", **kw):
    """Both forms == jb_minhash (and minhash_ref when asked), bit for bit; returns the host's result."""
    host = J.minhash(text, s, e, dt, n, K, seed, **kw)
    if ref:
        r = M.minhash_ref(text, s, e, dt, n, K, seed, **kw)
        assert (host[0] == r[0]).all() and (host[1] == r[1]).all(), (label, "jb_minhash")
    for f in FORMS:
        sig, dn = device(tks[f], text, s, e, dt, n, K, seed, **kw)
        assert (dn == host[1]).all(), (label, f, n, K, dn[:8], host[1][:8])
        assert (sig == host[0]).all(), (label, f, n, K, np.argwhere(sig != host[0])[:4])
    return host


def words(ntok, seed, nkeys=60):
    rng = np.random.default_rng(seed)
    keys = [b"w%d" % i for i in range(nkeys)] + ["中文".encode(), b"\xff", b"x" * 30]
    return M.from_keys([keys[i] for i in rng.integers(0, len(keys), ntok)], gap=b" ")


# ---- 1. hand spans: document boundaries around the tile, halos, many tiny documents -------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_boundaries_around_the_tile(forms, n):
    """Document boundaries at tokens T - 1, T and T + 1, a document of 2T + n tokens (its halos cross two tile
    edges), and tokens before the first document and past the last."""
    ntok = 5 * T + 40
    text, s, e = words(ntok, 40 + n)
    for b in (T - 1, T, T + 1):
        dt = [3, b, b + 2 * T + n, b + 2 * T + n, ntok - 5]
        host = check(forms, text, s, e, dt, n, 64, label=f"b={b}")
        assert host[1].tolist() == [b - 3 - n + 1, 2 * T + 1, 0, ntok - 5 - (b + 2 * T + n) - n + 1]
    check(forms, text, s, e, [0, T - 1, T, T + 1, 2 * T, ntok], n, 65, label="one-token documents at the edge")


@pytest.mark.parametrize("K", [1, 64, 65, 128, 256])
def test_function_counts(forms, K):
    """One wave's worth of hash functions, one more than that, and the maximum; small cases against minhash_ref."""
    text, s, e = words(2 * T + 77, 50 + K)
    check(forms, text, s, e, [0, 10, 500, 500, T + 3, 2 * T + 77], 5, K, seed=K, label=f"K={K}")
    text, s, e = words(90, 60 + K)
    check(forms, text, s, e, [2, 30, 31, 33, 80], 3, K, seed=2 ** 64 - K, ref=True, label=f"K={K} ref")


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_many_tiny_documents(forms, n):
    """Several hundred documents of 0 to 3 tokens in one tile (m = 0, m < n and m = n among them), then longer ones."""
    rng = np.random.default_rng(70 + n)
    lens = rng.integers(0, 4, 700).tolist() + rng.integers(0, 3 * n + 2, 300).tolist() + [n, n - 1, n + 1, 0, 1]
    dt = np.cumsum([0] + lens).astype(np.uint64)
    text, s, e = words(int(dt[-1]) + 9, 80 + n, nkeys=12)
    host = check(forms, text, s, e, dt, n, 128, label=f"n={n}")
    m = np.array(lens)
    assert host[1].tolist() == np.where(m == 0, 0, np.where(m < n, 1, m - n + 1)).tolist()
    assert {0, 1}.issubset(set(host[1].tolist())) and int(dt[-1]) > T
    # equal tiny documents have equal rows, wherever they lie
    first = {}
    for d, (a, b) in enumerate(zip(dt[:-1].tolist(), dt[1:].tolist())):
        key = tuple(bytes(text[s[k]:e[k]]) for k in range(a, b))
        if key in first:
            assert (host[0][d] == host[0][first[key]]).all()
        first.setdefault(key, d)


def test_token_counts_and_caps(forms):
    """ntok on either side of cap (cap < *d_ntok is full mode's overflow), around the wave and the tile."""
    text, s, e = words(T + 300, 90)
    dt = [0, 7, 64, 65, 700, T, T + 1, T + 300]
    for ntok, cap in ((T + 300, T + 300), (T + 300, T - 1), (T + 300, 64), (10 ** 9, T + 1), (63, T + 300), (T, T + 300),
                      (1, 5), (0, T + 300), (T + 300, 0)):
        host = check(forms, text, s, e, dt, 3, 64, ntok=ntok, cap=cap, label=f"ntok={ntok} cap={cap}")
        nt = min(ntok, cap)
        ms = [max(0, min(dt[d + 1], nt) - min(dt[d], nt)) for d in range(len(dt) - 1)]
        assert host[1].tolist() == [0 if m == 0 else 1 if m < 3 else m - 2 for m in ms]
    check(forms, text, s, e, [0], 3, 64, label="no documents")
    check(forms, b"", [], [], [0, 0, 0], 2, 8, label="no tokens")


def test_bad_spans_and_long_keys(forms):
    """Reversed and empty spans, spans past the end, starts near 2^32; a 300-byte and a 70,000-byte alnum token
    (cut to 255 bytes: equal to each other where their first 255 bytes are)."""
    for seed in range(6):
        text, s, e, ntok, cap = W.random_case(seed, ntokens=T + 99, nbytes=4000)
        rng = np.random.default_rng(seed)
        dt = np.sort(rng.integers(0, T + 120, 9)).astype(np.uint64)
        check(forms, text, s, e, dt, 1 + seed, 64, ntok=ntok, cap=cap, label=f"seed={seed}")
    text, s, e, ntok, cap = W.random_case(3, ntokens=200, nbytes=900)
    check(forms, text, s, e, [0, 50, 50, 120, 200], 2, 32, ntok=ntok, cap=cap, ref=True, label="ref")
    big = b"a1" * 35_000
    toks = [b"x", big[:300], b"y", big, b"z", big[:255], b"q", big[:254] + b"!" + big[255:300]]
    text, s, e = M.from_keys(toks, gap=b" ")
    host = check(forms, text, s, e, np.arange(len(toks) + 1), 1, 64, ref=True, label="long keys")
    assert (host[0][1] == host[0][3]).all() and (host[0][1] == host[0][5]).all() and (host[0][1] != host[0][7]).any()
    check(forms, text, s, e, [0, len(toks)], 2, 64, label="long keys, one document")


@pytest.mark.parametrize("form", FORMS)
def test_decreasing_doc_tok(forms, form):
    """A contract check: the values are unspecified, nothing outside the outputs is written (every write index
    is a document index the search returned), and the documents the disorder does not touch are right."""
    text, s, e = words(2 * T + 50, 95)
    for dt in ([2 * T, T, 50, 0], [0, T + 7, T - 5, 2 * T, 30, 2 * T + 50], [5, 5, 3, 2 ** 40, 7, 9]):
        sig, dn = device(forms[form], text, s, e, dt, 3, 64)  # (the canaries are checked inside)
        assert sig.shape == (len(dt) - 1, 64)
    good = [0, 100, 300, T + 7, T - 5]
    sig, dn = device(forms[form], text, s, e, good, 3, 64)
    host = J.minhash(text, s, e, good[:4], 3, 64)
    assert (sig[:2] == host[0][:2]).all() and (dn[:2] == host[1][:2]).all()


def test_runs_are_identical(forms):
    text, s, e = words(3 * T + 11, 96)
    dt = [0, 9, T, T + 1, 3 * T + 11]
    runs = [device(forms[f], text, s, e, dt, 5, 128, seed=7) for f in (0, 1, 1, 0)]
    for sig, dn in runs[1:]:
        assert sig.tobytes() == runs[0][0].tobytes() and dn.tobytes() == runs[0][1].tobytes()


@pytest.mark.parametrize("form", FORMS)
def test_bad_buffers_and_limits(forms, form):
    tk = forms[form]
    text, s, e = words(300, 97)
    dt = [0, 100, 300]
    for kw in (dict(work=(8, 0)), dict(work=(0, 4)), dict(work=(0, 1))):
        device(tk, text, s, e, dt, 3, 64, expect_error=J.JB_EINVAL, **kw)
    for n, K, code in ((0, 64, J.JB_EINVAL), (3, 0, J.JB_EINVAL), (9, 64, J.JB_ELIMIT), (3, 257, J.JB_ELIMIT)):
        with pytest.raises(J.JbError) as ei:
            tk.minhash_device(8, 0, 8, 8, 8, 8, 0, 0, n, K, 1, 8, 8, 8, 256)
        assert ei.value.code == code
    with pytest.raises(J.JbError) as ei:
        tk.minhash_device(8, 2 ** 31, 8, 8, 8, 8, 0, 0, 3, 64, 1, 8, 8, 8, 256)
    assert ei.value.code == J.JB_ELIMIT
    with pytest.raises(J.JbError) as ei:
        tk.minhash_device(8, 8, 8, 8, 8, 8, 2 ** 32 - T, 0, 3, 64, 1, 8, 8, 8, 2 ** 40)
    assert ei.value.code == J.JB_ELIMIT
    for K, B, R, code in ((64, 0, 4, J.JB_EINVAL), (64, 4, 0, J.JB_EINVAL), (64, 9, 8, J.JB_EINVAL), (257, 1, 1, J.JB_ELIMIT)):
        with pytest.raises(J.JbError) as ei:
            tk.minhash_bands_device(8, 8, 1, K, B, R, 8)
        assert ei.value.code == code
    sig, dn = device(tk, text, s, e, dt, 3, 64)  # (and a good call still works)
    assert (sig == J.minhash(text, s, e, dt, 3, 64)[0]).all()


@pytest.mark.parametrize("form", FORMS)
def test_bands(forms, form):
    lens = [0, 40, 1, 40, 0, 7]
    dt = np.cumsum([0] + lens)
    text, s, e = words(int(dt[-1]), 98)
    for K, B, R in ((128, 16, 8), (128, 128, 1), (64, 1, 64), (65, 9, 7), (1, 1, 1)):
        sig, dn, keys = device(forms[form], text, s, e, dt, 2, K, bands=(B, R))
        want = J.minhash_bands(sig, dn, B, R)
        assert (keys == want).all() and (keys == M.bands_ref(sig, dn, B, R)).all(), (K, B, R)
        assert (keys[0] == M.NOKEY).all() and (keys[4] == M.NOKEY).all() and (keys[[1, 2, 3, 5]] != M.NOKEY).all()


def test_profile_lists_the_kernels(forms):
    tk = forms[1]
    text, s, e = words(2 * T, 99)
    tk.profile(True)
    try:
        tk.profile_reset()
        device(tk, text, s, e, [0, T, 2 * T], 3, 64, bands=(8, 8))
        prof = tk.profile_read()
    finally:
        tk.profile(False)
    for k in ("k_mh_init", "k_mh_hash", "k_mh_sig", "k_mh_bands"):
        assert prof[k][1] == 1, prof


# ---- 2. real cuts -------------------------------------------------------------------------------------------------
def _oracle_spans(o, buf, off, mode, hmm):
    if mode == "cut":
        return o.cut_batch(buf, off, hmm)
    if mode == "search":
        return R.expected(o, buf, off, hmm)
    return F.expected(o, buf[:int(off[-1])], off)


@pytest.fixture(scope="module")
def real_refs(mini_paths, syn_small):
    """{(dict, mode, hmm): jb_minhash over the oracle's spans}, and the two batches, computed once."""
    mini = R.batch_of(TEXTS)
    buf, off, _ = syn_small[2].corpus(synth.KIND_DOCS, 3, target_bytes=96 << 10)
    syn = (np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(off, np.uint64))
    out = {"mini": mini, "syn": syn}
    for name, (b, f), paths in (("mini", mini, mini_paths), ("syn", syn, syn_small[:2])):
        o = O.Oracle.from_files(paths[0], paths[1], 0)
        for mode, hmm in MODES:
            s, e, dt = _oracle_spans(o, b, f, mode, hmm)
            assert len(s) < 100_000
            out[name, mode, hmm] = J.minhash(bytes(b[:int(f[-1])]), s, e, dt, 5, 128, 11) + (s, e, dt)
    return out


@pytest.mark.parametrize("mode,hmm", MODES)
@pytest.mark.parametrize("name", ["mini", "syn"])
def test_real_cuts(forms, syn_forms, real_refs, name, mode, hmm):
    """jb_minhash_batch over a host batch, and jb_cut_device* -> jb_minhash_device on the device arrays, in every
    mode and both forms: the signatures of the oracle's tokens."""
    import torch
    want_sig, want_dn, rs, re_, rdt = real_refs[name, mode, hmm]
    buf, off = real_refs[name]
    nb, nd = int(off[-1]), len(off) - 1
    assert int(want_dn.sum()) > (20 if name == "mini" else 15_000)
    d_text = torch.from_numpy(np.concatenate([buf[:nb], np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for f in FORMS:
        tk = (forms if name == "mini" else syn_forms)[f]
        sig, dn = tk.minhash_batch(buf, off, hmm, 5, 128, 11, mode)
        assert (dn == want_dn).all() and (sig == want_sig).all(), (name, mode, hmm, f, "batch")
        # the device chain, queued on one stream without a wait between
        if mode == "cut":
            ps, pe, pt, pn = tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, st)
        elif mode == "search":
            ps, pe, pt, pn = tk.cut_device_search(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, st)
        else:
            ps, pe, pt, pn = tk.cut_device_full(d_text.data_ptr(), nb, d_off.data_ptr(), nd, st)
        cap = max(nb, 1)  # (the ctx-owned arrays hold nbytes spans; full mode's count may be larger: the clamp)
        need = J.minhash_work_bytes(cap, nd)
        wk = torch.empty(need, dtype=torch.uint8, device="cuda")
        d_sig = torch.zeros(nd * 128, dtype=torch.int32, device="cuda")
        d_dn = torch.zeros(nd, dtype=torch.int32, device="cuda")
        tk.minhash_device(d_text.data_ptr(), nb, ps, pe, pt, pn, cap, nd, 5, 128, 11, d_sig.data_ptr(), d_dn.data_ptr(),
                          wk.data_ptr(), need, st)
        torch.cuda.synchronize()
        # (a full-mode list longer than the ctx-owned arrays is clamped to them, by the rule's own clamp)
        c_sig, c_dn = (want_sig, want_dn) if len(rs) <= cap else \
            J.minhash(bytes(buf[:nb]), rs[:cap], re_[:cap], rdt, 5, 128, 11, ntok=len(rs), cap=cap)
        assert (d_dn.cpu().numpy().view(np.uint32) == c_dn).all(), (name, mode, hmm, f, "chain")
        assert (d_sig.cpu().numpy().view(np.uint32).reshape(nd, 128) == c_sig).all(), (name, mode, hmm, f, "chain")


def test_python_one_liner(forms):
    tk = forms[0]
    sig, dn = tk.minhash(TEXTS, n=2, K=64, seed=5)
    assert sig.shape == (len(TEXTS), 64) and sig.dtype == np.uint32 and dn.dtype == np.uint32
    assert (sig[0] == sig[3]).all() and dn[5] == 0 and (sig[5] == J.JB_MH_EMPTY).all()
    s2, d2 = forms[1].minhash(TEXTS, n=2, K=64, seed=5)
    assert sig.tobytes() == s2.tobytes() and dn.tobytes() == d2.tobytes()
    e, de = tk.minhash([], n=2, K=64)
    assert e.shape == (0, 64) and len(de) == 0
    with pytest.raises(ValueError):
        tk.minhash(TEXTS, mode="nope")
    with pytest.raises(J.JbError) as ei:
        tk.minhash(TEXTS, n=9)
    assert ei.value.code == J.JB_ELIMIT
    with pytest.raises(J.JbError) as ei:
        tk.minhash_batch(np.zeros(8, np.uint8), [0, 7, 3], True)
    assert ei.value.code == J.JB_EINVAL


def test_add_word_changes_the_signature(mini_paths):
    """One long-lived context: AddWord between two minhash calls changes the tokens, and the signature follows
    the oracle's new tokens."""
    tk = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    o = O.Oracle.from_files(mini_paths[0], mini_paths[1], 0)
    try:
        texts = ["今天天氣很好，我昨天去上海", "这一刹那", "今天天氣很好"]
        buf, off = R.batch_of(texts)
        text = bytes(buf[:int(off[-1])])

        def want():
            s, e, dt = o.cut_batch(buf, off, False)
            return J.minhash(text, s, e, dt, 2, 64, 3), len(s)

        (w0, d0), n0 = want()
        sig, dn = tk.minhash(texts, n=2, K=64, seed=3, hmm=False)
        assert (sig == w0).all() and (dn == d0).all()
        tk.AddWord("天氣", 10_000_000)
        o.add_term("天氣", 10_000_000)
        (w1, d1), n1 = want()
        assert n1 < n0 and (w1[0] != w0[0]).any() and (w1[1] == w0[1]).all()
        sig, dn = tk.minhash(texts, n=2, K=64, seed=3, hmm=False)
        assert (sig == w1).all() and (dn == d1).all()
    finally:
        tk.close()


def regrow_tokenizer(mini_paths):
    """A tokenizer over F.chain_dict(5) plus the mini dictionary, the smallest chain with a full-mode list longer than
    its text (test_ctx_model.py::test_the_regrow_case_is_the_smallest), and a batch of two such documents:
    (tk, buf, off, text).  A run of n >= 5 甲 has 4n - 10 spans in 3n bytes; with the second document's 𠀀 (one span,
    four bytes) runs of 11 give 69 spans in 70 bytes, runs of 12 give 77 in 76."""
    with open(mini_paths[0], encoding="utf-8") as f:
        d = f.read()
    tk = J.Tokenizer(J.make_config(dict_bytes=(F.chain_dict(5) + d).encode(), emit_path=mini_paths[1]))
    buf, off = R.batch_of([("甲" * 12).encode(), ("𠀀" + "甲" * 12).encode()])
    return tk, buf, off, bytes(buf[:int(off[-1])])


def test_minhash_batch_full_mode_regrow(mini_paths):
    """Full mode with more spans than bytes: jb_minhash_batch grows the span arrays and repeats the cut, twice over,
    and a plain-mode call that follows on the same context is not disturbed by it."""
    tf, buf, off, text = regrow_tokenizer(mini_paths)
    try:
        s, e, d = tf.cut_batch_full(buf, off)
        assert len(s) > int(off[-1])
        want_sig, want_dn = J.minhash(text, s, e, d, 2, 16, 5)
        assert int(want_dn.sum()) > 0
        for rep in range(2):
            sig, dn = tf.minhash_batch(buf, off, False, 2, 16, 5, "full")
            assert (dn == want_dn).all() and (sig == want_sig).all(), rep
        ps, pe, pd = tf.cut_batch(buf, off, False)
        assert len(ps) < len(s)
        plain_sig, plain_dn = J.minhash(text, ps, pe, pd, 2, 16, 5)
        sig, dn = tf.minhash_batch(buf, off, False, 2, 16, 5, "cut")
        assert (dn == plain_dn).all() and (sig == plain_sig).all()
    finally:
        tf.close()


def test_c_and_cpp_consumers(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "c_abi_minhash")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_minhash.c"), "-L", lib,
                           "-ljiebahip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "minhash ok" in r.stdout, r.stdout + r.stderr
    exe = str(tmp_path / "cpp_minhash_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_minhash_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "minhash ok" in r.stdout, r.stdout + r.stderr
