"""GPU: joined text (jb_join_device, jb_cut_batch_join; jb_join.hip) against jb_join, the host form of the
rule, and against join_ref.py, byte for byte.  Most tests hand the kernels spans they built themselves, so
the gather is checked independently of segmentation, in both forms of the write kernel (JB_JOIN_STAGE, read
at jb_open: one tokenizer per form).  Every output lies between canaries that must not change."""
import os
import subprocess

import numpy as np
import pytest

import codepoint_cases as CC
import jiebahip as J
import join_ref as JR
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [0, 1]  # JB_JOIN_STAGE
T, LONG = J.JB_JOIN_TILE, J.JB_JOIN_LONG
NG = 64  # canary bytes on each side of the output and of the work buffer
MODES = [("cut", False), ("cut", True), ("search", False), ("search", True), ("full", False)]


def _open_forms(dp, ep):
    old = os.environ.get("JB_JOIN_STAGE")
    tks = {}
    try:
        for f in FORMS:
            os.environ["JB_JOIN_STAGE"] = str(f)
            tks[f] = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
    finally:
        if old is None:
            os.environ.pop("JB_JOIN_STAGE", None)
        else:
            os.environ["JB_JOIN_STAGE"] = old
    return tks


@pytest.fixture(scope="module")
def forms(mini_paths):
    """{form: a tokenizer opened with JB_JOIN_STAGE=form} (the knob is read at jb_open)."""
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


def _dev(a, dtype, view):
    import torch
    a = np.ascontiguousarray(a, dtype)
    if len(a) == 0:
        a = np.zeros(1, dtype)
    return torch.from_numpy(a.view(view)).cuda()


def dev_join(tk, case, out_cap=None, shift=0, work=None, expect_error=None):
    """jb_join_device on the case's arrays -> (the out_cap bytes, out_doc_off, nout).  The span arrays are
    allocations of exactly cap entries; the output starts as 0x33 at d_out = an aligned address + shift, and it,
    the offsets and the work buffer lie between canaries.  out_cap None: room for the complete output.
    work = (missing bytes, misalignment) asks for a bad work buffer."""
    import torch
    nd = len(case.doc_tok) - 1
    if out_cap is None:
        out_cap = len(case.want()[0])
    d_text = torch.from_numpy(np.frombuffer(case.text + b"\0" * 64, np.uint8).copy()).cuda()
    d_s, d_e = _dev(case.starts[:case.cap], np.uint32, np.int32), _dev(case.ends[:case.cap], np.uint32, np.int32)
    d_doc = _dev(case.doc_tok, np.uint64, np.int64)
    d_n = torch.tensor([case.ntok], dtype=torch.int64, device="cuda")
    out = torch.full((out_cap + 2 * NG + 16,), 0x33, dtype=torch.uint8, device="cuda")
    base = NG + (-(out.data_ptr() + NG)) % 16 + shift if shift else NG
    out[:base] = 0x7A
    out[base + out_cap:] = 0x7A
    off = torch.full((nd + 1 + 16,), 0x3333333333333333, dtype=torch.int64, device="cuda")
    off[:8] = 0x7A7A
    off[8 + nd + 1:] = 0x7A7A
    nout = torch.full((3,), 0x7A7A, dtype=torch.int64, device="cuda")
    need = J.join_work_bytes(case.cap, nd)
    missing, misalign = work or (0, 0)
    wk = torch.full((need + 2 * NG + 8,), 0x5B, dtype=torch.uint8, device="cuda")
    wk[:NG] = 0x7A
    wk[NG + need:] = 0x7A
    args = (d_text.data_ptr(), case.nbytes, d_s.data_ptr(), d_e.data_ptr(), d_doc.data_ptr(), d_n.data_ptr(), case.cap,
            nd, case.sep, case.term, out.data_ptr() + base, out_cap, off.data_ptr() + 64, nout.data_ptr() + 8,
            wk.data_ptr() + NG + misalign, need - missing, torch.cuda.current_stream().cuda_stream)
    if expect_error is not None:
        with pytest.raises(J.JbError) as ei:
            tk.join_device(*args)
        assert ei.value.code == expect_error
    else:
        tk.join_device(*args)
    torch.cuda.synchronize()
    ob, fb, nb, wb = out.cpu().numpy(), off.cpu().numpy(), nout.cpu().numpy(), wk.cpu().numpy()
    assert (ob[:base] == 0x7A).all() and (ob[base + out_cap:] == 0x7A).all(), f"{case}: written outside d_out"
    assert (fb[:8] == 0x7A7A).all() and (fb[8 + nd + 1:] == 0x7A7A).all() and nb[0] == 0x7A7A and nb[2] == 0x7A7A, case
    assert (wb[:NG] == 0x7A).all() and (wb[NG + need:] == 0x7A).all(), f"{case}: written outside the work buffer"
    return ob[base:base + out_cap].tobytes(), fb[8:8 + nd + 1].astype(np.uint64), int(nb[1])


def check(tk, case, label, shift=0):
    """device == join_ref == jb_join, byte for byte; returns the device's bytes."""
    want, woff = case.want()
    got, off, nout = dev_join(tk, case, shift=shift)
    assert nout == len(want) and off.tolist() == woff, (label, case, nout, len(want))
    if got != want:
        bad = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"{label} {case}: byte {bad} of {len(want)}: got {got[max(0, bad - 16):bad + 16]!r} "
                             f"want {want[max(0, bad - 16):bad + 16]!r}")
    hout, hoff, hn = J.join(case.text, case.starts, case.ends, case.doc_tok, case.sep, case.term, ntok=case.ntok,
                            cap=case.cap, nbytes=case.nbytes)
    assert hn == nout and hoff.tolist() == woff and hout.tobytes() == want, (label, case, "jb_join")
    return got


def keyed(name, ntok, seed, sep=b" ", term=b"\n", maxdoc=400, maxkey=6, lead=b""):
    """ntok keys of 1 to maxkey bytes (some of them one invalid byte) in documents of 0 to maxdoc tokens."""
    rng = np.random.default_rng(seed)
    docs, left = [], ntok
    while left:
        n = min(left, int(rng.integers(0, maxdoc + 1)))
        doc = []
        for ln in rng.integers(1, maxkey + 1, n):
            doc.append(bytes([0x80 + int(rng.integers(0, 128))]) if rng.random() < 0.1 else
                       bytes(rng.integers(0x41, 0x5B, ln).astype(np.uint8)))
        docs.append(doc)
        left -= n
    return JR.from_keys(name, docs, sep, term, lead)


# ---- 1. hand spans: token counts around the tile, key lengths around JB_JOIN_LONG -------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ntok", [T - 1, T, T + 1, 3 * T + 7])
def test_token_counts(forms, form, ntok):
    check(forms[form], keyed(f"{ntok} tokens", ntok, ntok), f"form={form}")
    check(forms[form], keyed(f"{ntok} tokens, wide separators", ntok, ntok + 1, b"<-sep8->", b"\r\n!", maxdoc=40),
          f"form={form}")


@pytest.mark.parametrize("form", FORMS)
def test_key_lengths(forms, form):
    rng = np.random.default_rng(5)
    ones = lambda n: [bytes([0x61 + int(x)]) for x in rng.integers(0, 26, n)]
    for ln in (LONG - 1, LONG, LONG + 1):
        big = bytes(rng.integers(0x30, 0x3A, ln).astype(np.uint8))
        check(forms[form], JR.from_keys(f"a key of {ln} bytes", [ones(700) + [big] + ones(50), [big], [big, big] + ones(3)]),
              f"form={form}")
    big = bytes(rng.integers(0x30, 0x3A, 70_000).astype(np.uint8))
    check(forms[form], JR.from_keys("a key of 70,000 bytes", [ones(300), ones(700) + [big] + ones(900), ones(30)]),
          f"form={form}")


@pytest.mark.parametrize("form", FORMS)
def test_tile_larger_than_staging(forms, form):
    """2,400 keys of 20 to 40 bytes: a tile's output (about 60 KB) is several times the 24 KiB staged at once."""
    rng = np.random.default_rng(6)
    docs = [[bytes(rng.integers(0x61, 0x7B, int(n)).astype(np.uint8)) for n in rng.integers(20, 41, 300)]
            for _ in range(8)]
    check(forms[form], JR.from_keys("long tiles", docs, b"  ", b"\n\n"), f"form={form}")


@pytest.mark.parametrize("form", FORMS)
def test_output_alignments(forms, form):
    """A leading key of 0 to 15 bytes, and d_out itself at 0 to 15 bytes past a 16-byte boundary."""
    for a in range(16):
        lead = [[b"x" * a] if a else [], []]
        case = keyed(f"alignment {a}", 600, 40 + a, maxdoc=50)
        docs = JR.from_keys(f"alignment {a}", lead + [[case.text[s:e] for s, e in zip(case.starts[p:q], case.ends[p:q])]
                                                   for p, q in zip(case.doc_tok[:-1].astype(int), case.doc_tok[1:].astype(int))],
                            b" ", b"")
        check(forms[form], docs, f"form={form}", shift=(5 * a + 1) % 16)


@pytest.mark.parametrize("form", FORMS)
def test_invalid_byte_runs(forms, form):
    """Runs of invalid bytes, each a token of its own that triples."""
    rng = np.random.default_rng(7)
    text = rng.integers(0x80, 0x100, 5000).astype(np.uint8)
    text[rng.random(5000) < 0.2] = 0x2E
    s = np.arange(5000)
    case = JR.Case("invalid runs", text.tobytes(), s, s + 1, [0, 0, 1700, 1701, 4096, 5000], b"", b"\n")
    got = check(forms[form], case, f"form={form}")
    assert got.count(JR.REPL) == int((text >= 0x80).sum()) and got.decode("utf-8")


# ---- 2. malformed spans, clamps, empty documents --------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_malformed_spans_and_clamps(forms, form):
    for seed in range(24):
        check(forms[form], JR.random_case(seed), f"form={form}")
    for seed in (101, 102, 103):  # (the same over several tiles: ntok > cap, doc_tok past ntok)
        check(forms[form], JR.random_case(seed, ntokens=3 * T + 11 * seed, max_docs=40), f"form={form}")


@pytest.mark.parametrize("form", FORMS)
def test_empty_documents_at_tile_edges(forms, form):
    base = keyed("edges", 2 * T + 5, 9, maxdoc=10 ** 9)
    for cuts in ([0, 0, 0, T - 1, T - 1, T, T, T, T + 1, 2 * T, 2 * T, 2 * T + 5, 2 * T + 5, 2 * T + 5],
                 [0, 1, 1, T, 2 * T - 1, 2 * T - 1, 2 * T + 5], [3, T, T, 2 * T + 1]):
        case = JR.Case(f"cuts {cuts[:4]}", base.text, base.starts, base.ends, cuts, b", ", b";\n")
        check(forms[form], case, f"form={form}")


@pytest.mark.parametrize("form", FORMS)
def test_one_token_documents(forms, form):
    """5,000 documents of one token: more documents than a tile has tokens."""
    case = keyed("5000 documents", 5000, 11, maxdoc=1)
    docs = np.diff(case.doc_tok.astype(np.int64))
    assert (docs <= 1).all() and len(docs) >= 5000
    check(forms[form], case, f"form={form}")


# ---- 3. capacity and the work buffer ----------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_out_cap_truncation(forms, form):
    for case in (keyed("truncated", T + 300, 13, b" ", b"\r\n"), JR.random_case(7)):
        want, woff = case.want()
        for cap in JR.out_caps(len(want)) + [len(want) // 2, len(want) // 2 + 7]:
            for shift in (0, 3):
                got, off, nout = dev_join(forms[form], case, out_cap=cap, shift=shift)
                m = min(cap, len(want))
                assert nout == len(want) and off.tolist() == woff, (case, cap)
                assert got[:m] == want[:m] and got[m:] == b"\x33" * (cap - m), (case, cap)


@pytest.mark.parametrize("form", FORMS)
def test_bad_work_buffer(forms, form):
    case = keyed("work", 300, 15)
    n = len(case.want()[0])
    for work in ((8, 0), (0, 4), (0, 1)):
        got, off, nout = dev_join(forms[form], case, work=work, expect_error=J.JB_EINVAL)
        assert got == b"\x33" * n and (off == 0x3333333333333333).all() and nout == 0x7A7A  # (nothing was queued)


# ---- 4. the real chain ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(syn_small):
    buf, off, _ = syn_small[2].corpus(synth.KIND_DOCS, 3, target_bytes=960 << 10)
    assert int(off[-1]) <= 1 << 20
    return np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(off, np.uint64)


@pytest.fixture(scope="module")
def host_spans(syn_forms, corpus):
    """{(mode, hmm): (Case over the host spans of that mode, its reference)}, computed once."""
    buf, off = corpus
    tk = syn_forms[1]
    text = bytes(buf[:int(off[-1])])
    out = {}
    for mode, hmm in MODES:
        s, e, d = {"cut": lambda: tk.cut_batch(buf, off, hmm), "search": lambda: tk.cut_batch_search(buf, off, hmm),
                   "full": lambda: tk.cut_batch_full(buf, off)}[mode]()
        out[mode, hmm] = JR.Case(f"{mode} hmm={hmm}", text, s, e, d)
        out[mode, hmm].want()
    return out


def _chain(tk, corpus, mode, hmm, cap=None):
    """cut_device* of `mode`, then join_device on its device arrays -> (bytes, offsets, nout, ntok)."""
    import torch
    buf, off = corpus
    nb, nd = int(off[-1]), len(off) - 1
    d_text = torch.from_numpy(np.concatenate([buf[:nb], np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    if cap is not None:  # full mode into arrays of the test's own, shorter than the list
        d_s = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_e = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_d = torch.zeros(nd + 1, dtype=torch.int64, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        tk.cut_device_full_into(d_text.data_ptr(), nb, d_off.data_ptr(), nd, d_s.data_ptr(), d_e.data_ptr(), cap,
                                d_d.data_ptr(), d_n.data_ptr(), st)
        ps, pe, pd, pn = d_s.data_ptr(), d_e.data_ptr(), d_d.data_ptr(), d_n.data_ptr()
    else:
        cap = nb
        if mode == "cut":
            ps, pe, pd, pn = tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, st)
        elif mode == "search":
            ps, pe, pd, pn = tk.cut_device_search(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, st)
        else:
            ps, pe, pd, pn = tk.cut_device_full(d_text.data_ptr(), nb, d_off.data_ptr(), nd, st)
    ocap = 4 * nb
    out = torch.full((ocap + 2 * NG,), 0x33, dtype=torch.uint8, device="cuda")
    ooff = torch.zeros(nd + 1, dtype=torch.int64, device="cuda")
    nout = torch.zeros(1, dtype=torch.int64, device="cuda")
    need = J.join_work_bytes(cap, nd)
    wk = torch.empty(need, dtype=torch.uint8, device="cuda")
    tk.join_device(d_text.data_ptr(), nb, ps, pe, pd, pn, cap, nd, b" ", b"\n", out.data_ptr() + NG, ocap, ooff.data_ptr(),
                   nout.data_ptr(), wk.data_ptr(), need, st)
    torch.cuda.synchronize()
    n = int(nout.item())
    assert n <= ocap
    ob = out.cpu().numpy()
    assert (ob[:NG] == 0x33).all() and (ob[NG + n:] == 0x33).all()
    ntok = int(J.dev_to_host(pn, 8, np.uint64)[0])
    return ob[NG:NG + n].tobytes(), ooff.cpu().numpy().astype(np.uint64), n, ntok


@pytest.mark.parametrize("mode,hmm", MODES)
def test_real_chain(syn_forms, corpus, host_spans, mode, hmm):
    """cut_device / cut_device_search / cut_device_full, then join_device, in both forms and twice."""
    case = host_spans[mode, hmm]
    want, woff = case.want()
    assert len(case.starts) > 100_000
    runs = [_chain(syn_forms[f], corpus, mode, hmm) for f in (0, 1, 1, 0)]
    for got, off, n, ntok in runs:
        assert ntok == len(case.starts) and n == len(want) and off.tolist() == woff
        assert got == want
    assert want.decode("utf-8")  # (whole runes, ASCII or replaced bytes: valid UTF-8 in every mode)


def test_real_chain_full_short_arrays(syn_forms, corpus, host_spans):
    """Full mode into span arrays shorter than its list: the join clamps to the arrays, as jb_terms_device does."""
    case = host_spans["full", False]
    ntok = len(case.starts)
    cap = ntok // 2 + 17
    short = JR.Case("full, cap < ntok", case.text, case.starts[:cap], case.ends[:cap], case.doc_tok, ntok=ntok, cap=cap)
    want, woff = short.want()
    for f in FORMS:
        got, off, n, nt = _chain(syn_forms[f], corpus, "full", False, cap=cap)
        assert nt == ntok and n == len(want) and off.tolist() == woff and got == want


@pytest.mark.parametrize("mode,hmm", MODES)
def test_cut_batch_join(syn_forms, corpus, host_spans, mode, hmm):
    buf, off = corpus
    want, woff = host_spans[mode, hmm].want()
    for f in FORMS:
        for rep in range(2):
            out, ooff = syn_forms[f].cut_batch_join(buf, off, hmm, mode)
            assert ooff.tolist() == woff and out.tobytes() == want, (f, rep)
    # a sub-batch that does not start at 0, other delimiters
    a, b = 5, 25
    sub = host_spans[mode, hmm]
    k0, k1 = int(sub.doc_tok[a]), int(sub.doc_tok[b])
    w2, o2 = JR.join_ref(sub.text, sub.starts[k0:k1], sub.ends[k0:k1], sub.doc_tok[a:b + 1] - sub.doc_tok[a], b"\t", b"")
    out, ooff = syn_forms[1].cut_batch_join(buf, off[a:b + 1], hmm, J._MODES[mode], b"\t", b"")
    assert out.tobytes() == w2 and ooff.tolist() == o2


def test_cut_join(forms):
    tk = forms[1]
    texts = ["english번역『하다』今天天氣很好，ステーションabc1231+1=2我昨天去上海*important*去", b"\xff\xfe\xe4\xb8\xad\xe6\x96\x87\x80abc\xe4\xb8",
             "", "这一刹那", "   "]
    for mode, spans in (("cut", tk.cut_spans), ("search", tk.cut_search_spans), ("full", lambda t, h: tk.cut_full_spans(t))):
        for hmm in (False, True):
            for sep in (" ", "/", "，", ""):
                want = [sep.join(J.spans_to_tokens(t, *[x.tolist() for x in spans(t, hmm)])) for t in texts]
                assert tk.cut_join(texts, sep=sep, hmm=hmm, mode=mode) == want
    assert tk.cut_join(["这一刹那"], sep=" ", term="。", hmm=False, mode="search") == ["这 一刹 刹那 一刹那。"]
    assert tk.cut_join([]) == []
    out, off = tk.cut_batch_join(np.zeros(1, np.uint8), np.zeros(1, np.uint64), True)
    assert len(out) == 0 and off.tolist() == [0]


# ---- 5. every code point ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,hmm", [("cut", True), ("search", True), ("full", False)])
@pytest.mark.parametrize("name", ["D", "T", "M"])
def test_codepoint_sweep(syn_forms, name, mode, hmm):
    """The code-point sweep inputs through cut_batch_join: every document's output is strict UTF-8 and is the
    rule over the host spans of the same mode."""
    buf, off = {"D": CC.corpus_D, "T": CC.corpus_T, "M": CC.corpus_M}[name]()
    buf, off = np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(off, np.uint64)
    tk = syn_forms[1]
    out, ooff = tk.cut_batch_join(buf, off, hmm, mode, " ", "\n")
    s, e, d = {"cut": lambda: tk.cut_batch(buf, off, hmm), "search": lambda: tk.cut_batch_search(buf, off, hmm),
               "full": lambda: tk.cut_batch_full(buf, off)}[mode]()
    text = bytes(buf[:int(off[-1])])
    hout, hoff, hn = J.join(text, s, e, d, " ", "\n")
    assert hn == len(out) and ooff.tolist() == hoff.tolist() and out.tobytes() == hout.tobytes()
    raw = out.tobytes()
    raw.decode("utf-8")  # strict; and every document ends with its terminator, so each decodes on its own
    ends = ooff[1:].astype(np.int64)
    assert (out[ends - 1] == 0x0A).all() and (np.diff(ooff.astype(np.int64)) >= 1).all()
    if name != "M":  # (M has 235,904 documents: the Python statement of the rule on a share of them)
        assert JR.join_ref(text, s, e, d)[0] == raw
    else:
        k = int(d[20000])
        assert JR.join_ref(text, s[:k], e[:k], d[:20001])[0] == raw[:int(ooff[20000])]
    assert forms_equal(syn_forms[0], buf, off, hmm, mode, raw)


def forms_equal(tk0, buf, off, hmm, mode, raw):
    out0, _ = tk0.cut_batch_join(buf, off, hmm, mode, " ", "\n")
    return out0.tobytes() == raw


# ---- 6. the profile, errors, consumers -----------------------------------------------------------------------------
def test_profile_lists_the_kernels(forms):
    tk = forms[1]
    case = keyed("profile", 3 * T, 17)
    tk.profile(True)
    try:
        tk.profile_reset()
        dev_join(tk, case)
        prof = tk.profile_read()
    finally:
        tk.profile(False)
    for k in ("k_join_count", "k_join_scan", "k_join_doc", "k_join_write"):
        assert prof[k][1] == 1, prof


def test_batch_errors(forms, mini_paths):
    tk = forms[1]
    buf = np.frombuffer(b"abc def" + b"\0" * 16, np.uint8)
    with pytest.raises(J.JbError) as ei:
        tk.cut_batch_join(buf, [0, 7], True, 3)
    assert ei.value.code == J.JB_EINVAL
    with pytest.raises(ValueError):
        tk.cut_batch_join(buf, [0, 7], True, "nope")
    with pytest.raises(J.JbError) as ei:
        tk.cut_batch_join(buf, [0, 7, 3], True)
    assert ei.value.code == J.JB_EINVAL
    for sep, term in ((b"123456789", b""), (b"", b"123456789")):
        with pytest.raises(J.JbError) as ei:
            tk.cut_batch_join(buf, [0, 7], True, "cut", sep, term)
        assert ei.value.code == J.JB_ELIMIT
    # an input on which the reference panics (search_ref.PLAINW0_DICT): the cut's error passes through
    import search_ref as R
    bad = J.Tokenizer(J.make_config(dict_bytes=R.PLAINW0_DICT.encode(), emit_path=mini_paths[1]))
    try:
        t = "甲乙丙丁戊甲乙丙".encode()
        for mode in ("cut", "search"):
            with pytest.raises(J.JbError) as ei:
                bad.cut_batch_join(np.frombuffer(t + b"\0" * 16, np.uint8), [0, len(t)], False, mode)
            assert ei.value.code == J.JB_EPANIC
        assert bad.cut_join(["甲乙丙丁"], hmm=False) == [" ".join(bad.Cut("甲乙丙丁", False))]
    finally:
        bad.close()


def test_c_and_cpp_consumers(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "c_abi_join")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_join.c"), "-L", lib,
                           "-ljiebahip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "join ok" in r.stdout, r.stdout + r.stderr
    exe = str(tmp_path / "cpp_join_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_join_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "join ok" in r.stdout, r.stdout + r.stderr
