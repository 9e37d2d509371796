"""GPU: the token filter (jb_filter_device, jb_stopwords_set, jb_cut_batch_filter, jb_batch_filter_set;
jb_filter.hip) against jb_filter, the host form of the rule, exactly, on all six outputs, and (for the small
cases) against filter_ref.py.  Most tests hand the kernels spans and document offsets they built themselves, so
the filter is checked independently of segmentation.  Every output and the work buffer lie between canaries that
must not change, and entries at or past out_cap keep their fill."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_ref as FR
import full_ref as F
import jiebahip as J
import oracle as O
import search_ref as R
from filter_cases import LENGTH_PIECES, NEAR_KEYS, PIECES, RUNE_BOUNDS, STOP_KEYS, spans_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = J.JB_FILTER_TILE
NG = 64  # canary bytes on each side of every output and of the work buffer
FILL = 0x33
MODES = [("cut", False), ("cut", True), ("search", False), ("search", True), ("full", False)]
STOPS = STOP_KEYS + ["上海".encode(), b"w3", "今天".encode()]
RULE = J.filter_rule(("other", "invalid"), 2, 0, True)  # the idiom: no punctuation, no stop words, len(w) > 1


@pytest.fixture(scope="module")
def tk(mini_paths):
    t = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    t.set_stop_words(STOPS)
    yield t
    t.close()


@pytest.fixture(scope="module")
def stop():
    return J.Vocab(STOPS)


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


class Dev:
    """A span list on the device: the span arrays are allocations of exactly cap entries."""

    def __init__(self, text, starts, ends, doc_tok, ntok=None, cap=None, nbytes=None):
        import torch
        text = bytes(text)
        self.cap = len(starts) if cap is None else cap
        self.ntok = len(starts) if ntok is None else ntok
        self.nbytes = len(text) if nbytes is None else nbytes
        dt = np.ascontiguousarray(doc_tok, np.uint64)
        self.nd = len(dt) - 1
        self.text = torch.from_numpy(np.frombuffer(text + b"\0" * 64, np.uint8).copy()).cuda()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32)[:self.cap].view(np.int32).copy()).cuda() \
            if self.cap else torch.zeros(1, dtype=torch.int32, device="cuda")
        self.s, self.e = up(starts), up(ends)
        self.tok = torch.from_numpy(dt.view(np.int64).copy()).cuda()
        self.n = torch.tensor([self.ntok], dtype=torch.int64, device="cuda")


def device(tk, text, starts, ends, doc_tok, rule, ntok=None, cap=None, nbytes=None, out_cap=None, src=True, work=None,
           expect_error=None, keep=False):
    """jb_filter_device on host arrays -> (out_start, out_end, out_src or None, out_doc_tok, out_ntok, stats): the
    first three hold the min(out_ntok, out_cap) entries the call writes; what lies behind them must still hold
    the fill.  work = (missing bytes, misalignment) asks for a bad buffer.  keep: also return the device state."""
    import torch
    d = Dev(text, starts, ends, doc_tok, ntok, cap, nbytes)
    out_cap = d.cap if out_cap is None else out_cap
    need = J.filter_work_bytes(d.cap, d.nd)
    wk, p_wk = guarded(need, 0x5B)
    os_, p_os = guarded(out_cap * 4, FILL)
    oe, p_oe = guarded(out_cap * 4, FILL)
    osr, p_osr = guarded(out_cap * 4, FILL)
    odt, p_odt = guarded((d.nd + 1) * 8, FILL)
    on, p_on = guarded(8, FILL)
    ost, p_ost = guarded(40, FILL)
    st = torch.cuda.current_stream().cuda_stream
    wmiss, wmis = work or (0, 0)
    args = (d.text.data_ptr(), d.nbytes, d.s.data_ptr(), d.e.data_ptr(), d.tok.data_ptr(), d.n.data_ptr(), d.cap, d.nd,
            rule, p_os, p_oe, p_osr if src else 0, out_cap, p_odt, p_on, p_ost, p_wk + wmis, need - wmiss, st)
    if expect_error is not None:
        with pytest.raises(J.JbError) as ei:
            tk.filter_device(*args)
        assert ei.value.code == expect_error
        torch.cuda.synchronize()  # nothing was queued: every buffer holds its fill
        assert (payload(wk, need, "the work buffer") == 0x5B).all()
        for t, nb in ((os_, out_cap * 4), (oe, out_cap * 4), (osr, out_cap * 4), (odt, (d.nd + 1) * 8), (on, 8), (ost, 40)):
            assert (payload(t, nb, "an output") == FILL).all()
        return None
    tk.filter_device(*args)
    torch.cuda.synchronize()
    payload(wk, need, "the work buffer")
    n = int(payload(on, 8, "out_ntok").copy().view(np.uint64)[0])
    stats = payload(ost, 40, "stats").copy().view(np.uint64)
    dt = payload(odt, (d.nd + 1) * 8, "out_doc_tok").copy().view(np.uint64)
    w = min(n, out_cap)
    outs = []
    for t, what in ((os_, "out_start"), (oe, "out_end"), (osr, "out_src")):
        b = payload(t, out_cap * 4, what)
        assert (b[w * 4:] == FILL).all(), what + ": an entry at or past the count or out_cap was written"
        outs.append(b[:w * 4].copy().view(np.uint32))
    if not src:
        assert (payload(osr, out_cap * 4, "out_src") == FILL).all()
        outs[2] = None
    res = (outs[0], outs[1], outs[2], dt, n, stats)
    return res + ((d, os_, oe, odt, on, p_os, p_oe, p_odt, p_on),) if keep else res


def same(dev, host, label=""):
    """All six outputs of the device call == jb_filter's."""
    hs, he, hsrc, hdt, hn, hst = host
    w = len(dev[0])
    assert dev[4] == hn, (label, dev[4], hn)
    assert dev[5].tolist() == hst.tolist(), (label, dev[5], hst)
    assert dev[3].tolist() == hdt.tolist(), (label, np.argwhere(dev[3] != hdt)[:4])
    assert w == min(hn, len(hs)) and np.array_equal(dev[0], hs[:w]) and np.array_equal(dev[1], he[:w]), label
    if dev[2] is not None:
        assert np.array_equal(dev[2], hsrc[:w]), label
    assert int(hst[0]) == hn + int(hst[1:].sum())


def check(tk, stop, text, s, e, dt, rule=RULE, ref=False, label="", **kw):
    src = kw.pop("src", True)
    host = J.filter_spans(text, s, e, dt, rule, stop, **kw)
    if ref:
        r = FR.filter_ref(text, s, e, dt, rule.flags, rule.drop_classes, rule.min_runes, rule.max_runes, set(STOPS), **kw)
        w = len(r[0])
        assert (host[0][:w].tolist(), host[1][:w].tolist(), host[2][:w].tolist(), host[3].tolist(), host[4],
                host[5].tolist()) == r, (label, "jb_filter")
    same(device(tk, text, s, e, dt, rule, src=src, **kw), host, label)
    return host


POOL = [b"w%d" % i for i in range(40)] + ["中文".encode(), "今天".encode(), "的".encode(), "上海".encode(), b"\xff", b"x" * 30,
                                         "，".encode(), b"7", b"2024", b"!", "很好".encode(), b"abcdefghi", b"y" * 25]


def words(ntok, seed):
    rng = np.random.default_rng(seed)
    return spans_of([POOL[i] for i in rng.integers(0, len(POOL), ntok)], gap=b" ")


# ---- 1. the kernels against the host rule ------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 5])
def test_token_counts(tk, stop, nt):
    text, s, e = words(nt, 100 + nt)
    dt = sorted({0, nt // 3, nt // 2, nt})
    h = check(tk, stop, text, s, e, dt + [nt], ref=nt <= 65, label=nt)
    assert nt < 63 or (0 < h[4] < nt and h[5][2] > 0 and h[5][3] > 0 and h[5][4] > 0)
    check(tk, stop, text, s, e, [0, nt], J.filter_rule(), label=(nt, "keep all"))
    check(tk, stop, text, s, e, [0, nt], J.filter_rule(31), label=(nt, "drop all"))


def test_ntok_beyond_cap_and_below(tk, stop):
    text, s, e = words(T + 70, 7)
    n = len(s)
    for ntok, cap in ((n + 9, n), (2 ** 40, T), (n, T - 1), (65, n), (0, n), (n, 0)):
        h = check(tk, stop, text, s[:cap], e[:cap], [0, 10, T, n, n + 5], ntok=ntok, cap=cap, label=(ntok, cap))
        assert h[5][0] == min(ntok, cap)


def test_document_boundaries(tk, stop):
    """300 one-token documents and empty ones, with boundaries on word (64) and tile (2048) edges, entries beyond
    the list and tokens before the first document."""
    nt = 2 * T + 300
    text, s, e = words(nt, 8)
    edges = [3, 3, 63, 64, 64, 65, 127, 128, T - 1, T, T, T + 1, T + 64, 2 * T - 1, 2 * T, 2 * T]
    dt = edges + list(range(2 * T, nt + 1)) + [nt, nt + 1, 2 ** 63]
    h = check(tk, stop, text, s, e, dt, label="boundaries")
    assert len(dt) - 1 > 300 + 16 and int(h[3][-1]) == h[4]
    check(tk, stop, text, s, e, dt, J.filter_rule(), label="boundaries, keep all")
    check(tk, stop, text, s, e, [0], label="no document")
    check(tk, stop, text, s, e, [nt, T, 5, 0], label="decreasing")  # (every entry is computed on its own)


def test_out_cap_and_no_src(tk, stop):
    text, s, e = words(T + 200, 9)
    kept = J.filter_spans(text, s, e, [0, len(s)], RULE, stop)[4]
    assert kept > T // 4
    for oc in (0, kept - 1, kept):
        h = check(tk, stop, text, s, e, [0, 100, len(s)], out_cap=oc, label=oc)
        assert h[4] == kept
        check(tk, stop, text, s, e, [0, 100, len(s)], out_cap=oc, src=False, label=(oc, "no src"))


def test_bad_spans(tk, stop):
    rng = np.random.default_rng(10)
    text, s, e = words(T + 500, 10)
    s, e = np.array(s, np.int64), np.array(e, np.int64)
    n, nb = len(s), len(text)
    kind = rng.integers(0, 12, n)
    e = np.where(kind == 0, s, e)
    s, e = np.where(kind == 1, e, s), np.where(kind == 1, s, e)
    e = np.where(kind == 2, nb + 1 + rng.integers(0, 1000, n), e)
    s, e = np.where(kind == 3, 0xFFFFFFF0, s), np.where(kind == 3, 0xFFFFFFFF, e)
    s = np.where(kind == 4, rng.integers(0, nb, n), s)  # (overlapping, of any length)
    e = np.where(kind == 4, np.minimum(s + rng.integers(1, 40, n), nb), e)
    h = check(tk, stop, text, s, e, [0, 7, T, n], label="bad spans")
    assert h[5][1] > 300
    h = check(tk, stop, text, s, e, [0, n], nbytes=nb // 2, label="nbytes below the text")
    assert h[5][1] > n // 3
    h = check(tk, stop, b"", s, e, [0, n], nbytes=0, label="no text")
    assert h[5][1] == n and h[4] == 0


def test_classes(tk, stop):
    text, s, e = spans_of(PIECES)
    dt = [0, 4, len(s)]
    for cls in (1, 2, 4, 8, 16):
        h = check(tk, stop, text, s, e, dt, J.filter_rule(cls), ref=True, label=cls)
        assert h[5][2] > 0
        check(tk, stop, text, s, e, dt, J.filter_rule(31 & ~cls), ref=True, label=~cls)
    t = "中".encode()  # a Han rune cut short by e, a lone continuation byte
    h = check(tk, stop, t, [0, 0, 0, 1, 2], [3, 2, 1, 2, 3], [0, 5], J.filter_rule(("han",)), ref=True)
    assert h[2][:h[4]].tolist() == [1, 2, 3, 4]


@pytest.mark.parametrize("lo,hi", RUNE_BOUNDS)
def test_rune_bounds(tk, stop, lo, hi):
    text, s, e = spans_of(PIECES + LENGTH_PIECES)
    check(tk, stop, text, s, e, [0, len(s)], J.filter_rule((), lo, hi), ref=True, label=(lo, hi))


def test_stop_key_forms(tk, stop):
    text, s, e = spans_of(STOP_KEYS + NEAR_KEYS + STOP_KEYS)
    h = check(tk, stop, text, s, e, [0, 5, 5, len(s)], J.filter_rule((), 0, 0, True), ref=True)
    nk = len(STOP_KEYS)
    assert h[5][4] == 2 * nk + 2  # every key in its 8-byte, inline or pool form, and EF BF BD for \x80 and \xff
    assert h[2][:h[4]].tolist() == [k for k in range(nk, nk + len(NEAR_KEYS)) if NEAR_KEYS[k - nk] not in (b"\x80", b"\xff")]
    # the same keys at every alignment of the text
    for lead in (b"", b" ", b"  ", b"   "):
        t2, s2, e2 = spans_of(STOP_KEYS + NEAR_KEYS)
        check(tk, stop, lead + t2, [x + len(lead) for x in s2], [x + len(lead) for x in e2], [0, len(s2)],
              J.filter_rule((), 0, 0, True), ref=True, label=len(lead))


def test_two_runs_identical(tk, stop):
    text, s, e = words(3 * T + 5, 11)
    a = device(tk, text, s, e, [0, T, len(s)], RULE)
    b = device(tk, text, s, e, [0, T, len(s)], RULE)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_refused_calls_queue_nothing(tk, stop, mini_paths):
    text, s, e = words(100, 12)
    dt = [0, 100]
    device(tk, text, s, e, dt, RULE, work=(1, 0), expect_error=J.JB_EINVAL)
    device(tk, text, s, e, dt, RULE, work=(8, 4), expect_error=J.JB_EINVAL)
    device(tk, text, s, e, dt, J.jb_filter_rule(2, 0, 0, 0), expect_error=J.JB_EINVAL)
    device(tk, text, s, e, dt, J.jb_filter_rule(0, 32, 0, 0), expect_error=J.JB_EINVAL)
    device(tk, text, s, e, dt, J.jb_filter_rule(0, 0, 256, 0), expect_error=J.JB_ELIMIT)
    device(tk, text, s, e, dt, RULE, nbytes=2 ** 31, expect_error=J.JB_ELIMIT)
    device(tk, text, s, e, dt, None, expect_error=J.JB_EINVAL)
    t2 = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    try:  # JB_FILTER_STOP without a stop set
        assert t2.stop_words_size == -1
        device(t2, text, s, e, dt, RULE, expect_error=J.JB_EINVAL)
        same(device(t2, text, s, e, dt, J.filter_rule(("other",), 2)), J.filter_spans(text, s, e, dt, J.filter_rule(("other",), 2)))
    finally:
        t2.close()


def test_stop_set_replaced_and_removed(mini_paths):
    t = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    try:
        text, s, e = words(300, 13)
        dt = [0, 300]
        rule = J.filter_rule((), 0, 0, True)
        for keys in ([b"w1", b"w2"], [b"w3", "中文".encode(), b"x" * 30], []):
            t.set_stop_words(keys)
            assert t.stop_words_size == len(keys)
            h = J.filter_spans(text, s, e, dt, rule, J.Vocab(keys))
            same(device(t, text, s, e, dt, rule), h, keys)
            assert (h[5][4] > 0) == bool(keys)
        with pytest.raises(J.JbError):  # on an error the old set stays
            t.set_stop_words([b"dup", b"dup"])
        assert t.stop_words_size == 0
        t.set_vocab([b"w1"])  # independent of the id vocabulary
        assert t.stop_words_size == 0 and t.vocab_size == 1
        t.set_stop_words(None)
        assert t.stop_words_size == -1 and t.vocab_size == 1
        device(t, text, s, e, dt, rule, expect_error=J.JB_EINVAL)
    finally:
        t.close()


def test_profile_lists_the_kernels(tk):
    text, s, e = words(2 * T, 14)
    tk.profile(True)
    try:
        tk.profile_reset()
        device(tk, text, s, e, [0, T, 2 * T], RULE)
        prof = tk.profile_read()
    finally:
        tk.profile(False)
    for k in ("k_filt_mark", "k_filt_scan", "k_filt_write"):
        assert prof[k][1] == 1, prof
    assert sum(v[1] for v in prof.values()) == 3


# ---- 2. composition with the span list's consumers -----------------------------------------------------------------
def test_filter_then_join_wc_minhash(tk, stop):
    import torch
    text, s, e = words(T + 300, 15)
    n = len(s)
    dt = [0, 5, 5, T, n]
    nd = len(dt) - 1
    hs, he, _, hdt, hn, _ = J.filter_spans(text, s, e, dt, RULE, stop)
    res = device(tk, text, s, e, dt, RULE, keep=True)
    d, os_, oe, odt, on, p_os, p_oe, p_odt, p_on = res[6]
    st = torch.cuda.current_stream().cuda_stream
    nb, cap = len(text), n
    # joined text
    want, woff, wn = J.join(text, hs[:hn], he[:hn], hdt, b" ", b"\n")
    need = J.join_work_bytes(cap, nd)
    wk = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.zeros(wn + 8, dtype=torch.uint8, device="cuda")
    ooff = torch.zeros(nd + 1, dtype=torch.int64, device="cuda")
    nout = torch.zeros(1, dtype=torch.int64, device="cuda")
    tk.join_device(d.text.data_ptr(), nb, p_os, p_oe, p_odt, p_on, cap, nd, b" ", b"\n", out.data_ptr(), wn,
                   ooff.data_ptr(), nout.data_ptr(), wk.data_ptr(), need, st)
    torch.cuda.synchronize()
    assert int(nout[0]) == wn and out.cpu().numpy()[:wn].tobytes() == want.tobytes()
    assert ooff.cpu().numpy().view(np.uint64).tolist() == woff.tolist()
    assert b"\xef\xbf\xbd" not in want.tobytes() and b"\xef\xbc\x8c" not in want.tobytes() and b"w3" not in want.tobytes().split()
    # word counts
    wantc = J.wc_count(text, hs[:hn], he[:hn])
    nslots, pool = 1 << 10, 1 << 12
    ntable = J.wc_table_bytes(nslots, pool)
    tab = torch.zeros(ntable + 32, dtype=torch.uint8, device="cuda")
    p_tab = (tab.data_ptr() + 31) & ~31
    tk.wc_init_device(p_tab, ntable, nslots, pool, st)
    need = J.wc_work_bytes(cap)
    wk = torch.empty(need, dtype=torch.uint8, device="cuda")
    tk.wc_add_device(p_tab, ntable, d.text.data_ptr(), nb, p_os, p_oe, p_on, cap, wk.data_ptr(), need, st)
    got = tk.wc_read(p_tab, ntable, stream_ptr=st)
    assert got.keys == wantc.keys and got.counts.tolist() == wantc.counts.tolist() and got.tokens == hn
    assert (got.bad, got.dropped, got.collided) == (0, 0, 0)
    # MinHash
    wsig, wdn = J.minhash(text, hs[:hn], he[:hn], hdt, 3, 64, 5)
    need = J.minhash_work_bytes(cap, nd)
    wk = torch.empty(need, dtype=torch.uint8, device="cuda")
    sig = torch.zeros(nd * 64, dtype=torch.int32, device="cuda")
    dn = torch.zeros(nd, dtype=torch.int32, device="cuda")
    tk.minhash_device(d.text.data_ptr(), nb, p_os, p_oe, p_odt, p_on, cap, nd, 3, 64, 5, sig.data_ptr(), dn.data_ptr(),
                      wk.data_ptr(), need, st)
    torch.cuda.synchronize()
    assert (dn.cpu().numpy().view(np.uint32) == wdn).all()
    assert (sig.cpu().numpy().view(np.uint32).reshape(nd, 64) == wsig).all()


# ---- 3. real cuts ----------------------------------------------------------------------------------------------------
def synthetic_docs(seed, ndocs=40):
    """Seeded documents over the mini dictionary's runes, ASCII words and numbers, punctuation, kana and stray
    bytes."""
    rng = np.random.default_rng(seed)
    parts = ["今天", "天氣", "很好", "我", "昨天", "去", "上海", "交通", "大學", "這", "的", "一刹那", "量子力", "，", "。", "、", " ",
             "abc", "x86", "2024", "7", "*", "ステーション", "번역", "\n", "Hello", "中文"]
    raw = [b"\xff", b"\x80", b"\xe4\xb8"]
    docs = []
    for _ in range(ndocs):
        n = int(rng.integers(0, 60))
        docs.append(b"".join(raw[int(rng.integers(0, 3))] if rng.random() < 0.03 else parts[int(rng.integers(0, len(parts)))].encode()
                             for _ in range(n)))
    return docs


def _oracle_spans(o, buf, off, mode, hmm):
    if mode == "cut":
        return o.cut_batch(buf, off, hmm)
    if mode == "search":
        return R.expected(o, buf, off, hmm)
    return F.expected(o, buf[:int(off[-1])], off)


@pytest.fixture(scope="module")
def real(mini_paths):
    """The synthetic batch and, per mode, the oracle's spans, computed once."""
    buf, off = R.batch_of(synthetic_docs(16))
    o = O.Oracle.from_files(mini_paths[0], mini_paths[1], 0)
    out = {"batch": (buf, off)}
    for mode, hmm in MODES:
        out[mode, hmm] = _oracle_spans(o, buf, off, mode, hmm)
    return out


def _cut_device(tk, mode, hmm, d_text, nb, d_off, nd, st):
    if mode == "cut":
        return tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, st)
    if mode == "search":
        return tk.cut_device_search(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, st)
    return tk.cut_device_full(d_text.data_ptr(), nb, d_off.data_ptr(), nd, st)


def _filter_chain(tk, buf, off, mode, hmm, rule):
    """jb_cut_device* -> jb_filter_device on one stream without a wait between: (start, end, doc_tok, n, stats)."""
    import torch
    nb, nd = int(off[-1]), len(off) - 1
    d_text = torch.from_numpy(np.concatenate([buf[:nb], np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64).copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    ps, pe, pt, pn = _cut_device(tk, mode, hmm, d_text, nb, d_off, nd, st)
    cap = max(nb, 1)
    need = J.filter_work_bytes(cap, nd)
    wk = torch.empty(need, dtype=torch.uint8, device="cuda")
    os_ = torch.zeros(cap, dtype=torch.int32, device="cuda")
    oe = torch.zeros(cap, dtype=torch.int32, device="cuda")
    odt = torch.zeros(nd + 1, dtype=torch.int64, device="cuda")
    on = torch.zeros(1, dtype=torch.int64, device="cuda")
    ost = torch.zeros(5, dtype=torch.int64, device="cuda")
    tk.filter_device(d_text.data_ptr(), nb, ps, pe, pt, pn, cap, nd, rule, os_.data_ptr(), oe.data_ptr(), 0, cap,
                     odt.data_ptr(), on.data_ptr(), ost.data_ptr(), wk.data_ptr(), need, st)
    torch.cuda.synchronize()
    n = int(on[0])
    return (os_.cpu().numpy().view(np.uint32)[:n], oe.cpu().numpy().view(np.uint32)[:n], odt.cpu().numpy().view(np.uint64), n,
            ost.cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("mode,hmm", MODES)
def test_real_cuts(tk, stop, real, mode, hmm):
    """The cut of every mode, filtered on the device, is the host rule over the oracle's spans; jb_cut_batch_filter
    returns the same, and cut_filtered its words."""
    buf, off = real["batch"]
    s, e, dt = real[mode, hmm]
    text = bytes(buf[:int(off[-1])])
    hs, he, _, hdt, hn, hst = J.filter_spans(text, s, e, dt, RULE, stop)
    assert 100 < hn < len(s) and hst[2] > 0 and hst[3] > 0 and hst[4] > 0
    cs, ce, cdt, cn, cst = _filter_chain(tk, buf, off, mode, hmm, RULE)
    assert cn == hn and cst.tolist() == hst.tolist() and cdt.tolist() == hdt.tolist()
    assert np.array_equal(cs, hs[:hn]) and np.array_equal(ce, he[:hn])
    for rep in range(2):
        bs, be, bdt, bst, _ = tk.cut_batch_filter(buf, off, hmm, RULE, mode)
        assert np.array_equal(bs, cs) and np.array_equal(be, ce) and bdt.tolist() == cdt.tolist() and bst.tolist() == cst.tolist()
    docs = [bytes(buf[int(off[d]):int(off[d + 1])]) for d in range(len(off) - 1)]
    got = tk.cut_filtered(docs, stop=True, min_runes=2, mode=mode, hmm=hmm)
    want = [[text[hs[k]:he[k]].decode() for k in range(int(hdt[d]), int(hdt[d + 1]))] for d in range(len(docs))]
    assert got == want and not any(w in ("上海", "今天", "，") or len(w) < 2 for ws in got for w in ws)


def test_cut_batch_filter_cap_protocol(tk, stop, real):
    buf, off = real["batch"]
    nd = len(off) - 1
    full = tk.cut_batch_filter(buf, off, True, RULE, "cut")
    n = len(full[0])
    s, e = np.full(n - 1, 0xA5A5A5A5, np.uint32), np.full(n - 1, 0xA5A5A5A5, np.uint32)
    tok, cnt, stats = np.full(nd + 1, 77, np.uint64), C.c_uint64(), np.zeros(5, np.uint64)
    rc = J.lib().jb_cut_batch_filter(tk.h, buf.ctypes.data, off.ctypes.data, nd, 1, J.JB_MODE_CUT, C.byref(RULE),
                                     s.ctypes.data, e.ctypes.data, n - 1, tok.ctypes.data, C.byref(cnt), stats.ctypes.data)
    assert rc == J.JB_ELIMIT and cnt.value == n and stats.tolist() == full[3].tolist()
    assert (s == 0xA5A5A5A5).all() and (e == 0xA5A5A5A5).all() and (tok == 77).all()
    # no documents, an empty batch, a decreasing doc_off, an unknown mode
    s0, e0, t0, st0, _ = tk.cut_batch_filter(np.zeros(1, np.uint8), np.zeros(1, np.uint64), True, RULE)
    assert len(s0) == 0 and t0.tolist() == [0] and st0.tolist() == [0] * 5
    s0, e0, t0, st0, _ = tk.cut_batch_filter(np.zeros(1, np.uint8), np.zeros(3, np.uint64), True, RULE)
    assert len(s0) == 0 and t0.tolist() == [0, 0, 0]
    with pytest.raises(J.JbError) as ei:
        tk.cut_batch_filter(buf, [0, 7, 3], True, RULE)
    assert ei.value.code == J.JB_EINVAL
    with pytest.raises(ValueError):
        tk.cut_batch_filter(buf, off, True, RULE, "nope")
    assert tk.cut_filtered([]) == []


def test_cut_batch_filter_full_mode_regrow(mini_paths):
    """Full mode with more spans than bytes (F.chain_dict(12) on 甲 x 200): the call grows the kept span arrays and
    repeats the cut, then filters the longer list."""
    tf = J.Tokenizer(J.make_config(dict_bytes=F.chain_dict(12).encode(), emit_path=mini_paths[1]))
    try:
        docs = [("甲" * 200).encode(), ("𠀀，" + "甲" * 150).encode()]
        buf, off = R.batch_of(docs)
        s, e, d = tf.cut_batch_full(buf, off)
        assert len(s) > int(off[-1])
        text = bytes(buf[:int(off[-1])])
        rule = J.filter_rule(("other",), 2, 7)
        hs, he, _, hdt, hn, hst = J.filter_spans(text, s, e, d, rule)
        assert 0 < hn < len(s) and hst[3] > 0
        for rep in range(2):
            bs, be, bdt, bst, _ = tf.cut_batch_filter(buf, off, False, rule, "full")
            assert np.array_equal(bs, hs[:hn]) and np.array_equal(be, he[:hn])
            assert bdt.tolist() == hdt.tolist() and bst.tolist() == hst.tolist()
    finally:
        tf.close()


# ---- 4. the batch filter ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,hmm", [("cut", True), ("search", False), ("full", False)])
def test_batch_filter(mini_paths, stop, real, mode, hmm):
    """With a batch filter set, jb_cut_batch_join, jb_wc_batch and jb_minhash_batch equal the host rules over the
    filtered oracle spans; cleared, they return byte for byte what they returned before it was set."""
    import torch
    t = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    try:
        t.set_stop_words(STOPS)
        buf, off = real["batch"]
        s, e, dt = real[mode, hmm]
        text = bytes(buf[:int(off[-1])])
        nslots, pool = 1 << 10, 1 << 12
        ntable = J.wc_table_bytes(nslots, pool)
        tab = torch.zeros(ntable + 32, dtype=torch.uint8, device="cuda")
        p_tab = (tab.data_ptr() + 31) & ~31

        def run():
            out, ooff = t.cut_batch_join(buf, off, hmm, mode, b" ", b"\n")
            t.wc_init_device(p_tab, ntable, nslots, pool)
            t.wc_batch(buf, off, hmm, p_tab, ntable, mode)
            wc = t.wc_read(p_tab, ntable)
            sig, dn = t.minhash_batch(buf, off, hmm, 3, 64, 5, mode)
            return (out.tobytes(), ooff.tobytes(), wc.keys, wc.counts.tobytes(), wc.tokens, sig.tobytes(), dn.tobytes())

        def want(fs, fe, fdt):
            out, ooff, _ = J.join(text, fs, fe, fdt, b" ", b"\n")
            wc = J.wc_count(text, fs, fe)
            sig, dn = J.minhash(text, fs, fe, fdt, 3, 64, 5)
            return (out.tobytes(), ooff.tobytes(), wc.keys, wc.counts.tobytes(), wc.tokens, sig.tobytes(), dn.tobytes())

        before = run()
        assert before == want(s, e, dt)
        t.set_batch_filter(("other", "invalid"), 2, 0, True)
        hs, he, _, hdt, hn, _ = J.filter_spans(text, s, e, dt, RULE, stop)
        filtered = run()
        assert filtered == want(hs[:hn], he[:hn], hdt) and filtered != before
        t.set_batch_filter(("han",))  # a second rule replaces the first
        hs, he, _, hdt, hn, _ = J.filter_spans(text, s, e, dt, J.filter_rule(("han",)))
        assert run() == want(hs[:hn], he[:hn], hdt)
        t.clear_batch_filter()
        assert run() == before
        # a rule that asks for a stop set that is not there fails the batch call, and clearing restores it
        t.set_stop_words(None)
        t.set_batch_filter(stop=True)
        with pytest.raises(J.JbError) as ei:
            t.cut_batch_join(buf, off, hmm, mode)
        assert ei.value.code == J.JB_EINVAL
        with pytest.raises(J.JbError):
            t.set_batch_filter(min_runes=256)
        t.clear_batch_filter()
        assert t.cut_batch_join(buf, off, hmm, mode, b" ", b"\n")[0].tobytes() == before[0]
    finally:
        t.close()


def test_batch_filter_after_full_mode_regrow(mini_paths):
    """A batch whose full-mode list is longer than the text has bytes (F.chain_dict(5) over the mini dictionary,
    test_ctx_model.py::test_the_regrow_case_is_the_smallest; 77 spans in 76 bytes): the cut's regrow, then the batch filter,
    then jb_cut_batch_join, jb_wc_batch and jb_minhash_batch's own step equal the host rules over the filtered
    full-mode spans; with the filter cleared, over all of them."""
    import torch
    with open(mini_paths[0], encoding="utf-8") as f:
        d = f.read()
    t = J.Tokenizer(J.make_config(dict_bytes=(F.chain_dict(5) + d).encode(), emit_path=mini_paths[1]))
    try:
        buf, off = R.batch_of([("甲" * 12).encode(), ("𠀀" + "甲" * 12).encode()])
        text = bytes(buf[:int(off[-1])])
        s, e, dt = t.cut_batch_full(buf, off)
        assert len(s) > int(off[-1])
        nslots, pool = 1 << 10, 1 << 12
        ntable = J.wc_table_bytes(nslots, pool)
        tab = torch.zeros(ntable + 32, dtype=torch.uint8, device="cuda")
        p_tab = (tab.data_ptr() + 31) & ~31

        def run():
            out, ooff = t.cut_batch_join(buf, off, False, "full", b" ", b"\n")
            t.wc_init_device(p_tab, ntable, nslots, pool)
            t.wc_batch(buf, off, False, p_tab, ntable, "full")
            wc = t.wc_read(p_tab, ntable)
            sig, dn = t.minhash_batch(buf, off, False, 2, 16, 5, "full")
            return (out.tobytes(), ooff.tobytes(), wc.keys, wc.counts.tobytes(), wc.tokens, sig.tobytes(), dn.tobytes())

        def want(fs, fe, fdt):
            out, ooff, _ = J.join(text, fs, fe, fdt, b" ", b"\n")
            wc = J.wc_count(text, fs, fe)
            sig, dn = J.minhash(text, fs, fe, fdt, 2, 16, 5)
            return (out.tobytes(), ooff.tobytes(), wc.keys, wc.counts.tobytes(), wc.tokens, sig.tobytes(), dn.tobytes())

        # (every token here is Han, so the first rule keeps none of the longer list; the second keeps the words of
        # two runes and more)
        seen = []
        for rule, some in (((("han",), 2, 0), False), (((), 2, 0), True)):
            t.set_batch_filter(*rule)
            hs, he, _, hdt, hn, _ = J.filter_spans(text, s, e, dt, J.filter_rule(*rule))
            assert hn < len(s) and (hn > 0) == some
            seen.append(run())
            assert seen[-1] == want(hs[:hn], he[:hn], hdt)
        t.clear_batch_filter()
        plain = run()
        assert plain == want(s, e, dt) and plain not in seen and seen[0] != seen[1]
    finally:
        t.close()


def test_c_and_cpp_consumers(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "c_abi_filter")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_filter.c"), "-L", lib,
                           "-ljiebahip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "filter ok" in r.stdout, r.stdout + r.stderr
    exe = str(tmp_path / "cpp_filter_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_filter_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "filter ok" in r.stdout, r.stderr + r.stdout
