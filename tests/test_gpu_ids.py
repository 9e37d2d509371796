"""GPU: token ids (jb_vocab_set, jb_ids_device, jb_spans_ids; kernel k_ids) against a Python dict over
the token bytes, vocab.get(key, UNK).  Most tests hand the kernel spans they built themselves, so the
lookup is checked independently of segmentation."""
import os
import subprocess
import threading

import numpy as np
import pytest

import full_ref as F
import jiebahip as J
import oracle as O
import search_ref as R
import synth
import vocab_ref as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(J.JB_DICT_TXT, 0), (J.JB_DICT_PREFIX, J.JIEBA_SIZE)]
UNK = V.UNK
U = -1  # (UNK in the hand-written lists below)
MIXED = "english번역『하다』今天天氣很好，ステーションabc1231+1=2我昨天去上海*important*去"  # test_gpu_full.EDGE_TEXTS
INVALID = b"\xff\xfe" + "中文".encode() + b"\x80abc\xe4\xb8"


def _pad(text):
    return np.frombuffer(bytes(text) + b"\0" * 64, np.uint8).copy()


def _u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def dev_ids(tk, text, starts, ends, nbytes=None, ntok=None, cap=None, fill=-7, extra=0):
    """jb_ids_device on spans of the test's own: the whole ids array (cap + extra entries, pre-filled)."""
    import torch
    nbytes = len(text) if nbytes is None else nbytes
    n = len(starts)
    ntok = n if ntok is None else ntok
    cap = n if cap is None else cap
    d_text = torch.from_numpy(_pad(text)).cuda()
    d_s, d_e = _u32(starts), _u32(ends)
    d_n = torch.tensor([ntok], dtype=torch.int64, device="cuda")
    d_ids = torch.full((max(cap, n) + extra + 1,), fill, dtype=torch.int32, device="cuda")
    tk.ids_device(d_text.data_ptr(), nbytes, d_s.data_ptr(), d_e.data_ptr(), d_n.data_ptr(), cap, d_ids.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_ids.cpu().numpy()


def _same(got, want, label):
    got, want = np.asarray(got).astype(np.uint32), np.asarray(want).astype(np.uint32)
    assert len(got) == len(want), (label, len(got), len(want))
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{label}: {len(bad)} of {len(want)} ids differ; first #{bad[0]}: "
                             f"got {got[bad[:6]].tolist()} want {want[bad[:6]].tolist()}")


@pytest.fixture(scope="module")
def mini(mini_paths):
    tk = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    yield tk
    tk.close()


# ---- 1. hand-checked ids ---------------------------------------------------------------------
HAND_VOCAB = ["abc", "中", "def", "今天", "天", "，", "ー", "abc1231", "1", "我", "上海", "important", "*", "�",
              "一刹那", "刹那", "天天", "english", "번", b"\xff", "去", "这"]
# mini_dict.txt, hmm off.  Tokens, by mode (search differs from cut only in the last text, full in the
# last two):
#   abc|中|文|def
#   english|번|역|『|하|다|』|今天|天|氣|很|好|，|ス|テ|ー|シ|ョ|ン|abc1231|+|1|=|2|我|昨天|去|上海|*|important|*|去
#     (full: 今天|天天 instead of 今天|天)
#   (\xff\xfe: a block without an alnum byte has no tokens) 中|文|�|abc|�|�
#   这|一刹那     search: 这|一刹|刹那|一刹那     full: 这|一刹|一刹那|刹那
HAND = [
    ("abc 中文 def", {"cut": [0, 1, U, 2], "search": [0, 1, U, 2], "full": [0, 1, U, 2]}),
    (MIXED, {m: [17, 18, U, U, U, U, U, 3, 16 if m == "full" else 4, U, U, U, 5, U, U, 6, U, U, U, 7, U, 8, U, U, 9, U,
                 20, 10, 12, 11, 12, 20] for m in ("cut", "search", "full")}),
    (INVALID, {m: [1, U, 13, 0, 13, 13] for m in ("cut", "search", "full")}),
    ("这一刹那", {"cut": [21, 14], "search": [21, U, 15, 14], "full": [21, U, 14, 15]}),
]


def _batch_ids(tk, texts, mode):
    buf, off = R.batch_of(texts)
    s, e, d = {"cut": lambda: tk.cut_batch(buf, off, False), "search": lambda: tk.cut_batch_search(buf, off, False),
               "full": lambda: tk.cut_batch_full(buf, off)}[mode]()
    return tk.spans_ids(buf, s, e), d


def test_hand_checked_ids(mini):
    tk = mini
    tk.set_vocab(HAND_VOCAB)
    assert tk.vocab_size == len(HAND_VOCAB)
    for mode in ("cut", "search", "full"):
        for text, want in HAND:
            toks, ids = tk.CutIds(text, False, mode)
            assert ids.dtype == np.uint32 and len(toks) == len(ids)
            _same(ids, np.array(want[mode], np.int64), f"CutIds {mode} {text[:12]!r}")
        ids, d = _batch_ids(tk, [t for t, _ in HAND], mode)
        _same(ids, np.array(sum((w[mode] for _, w in HAND), []), np.int64), f"batch {mode}")
        assert d.tolist() == np.cumsum([0] + [len(w[mode]) for _, w in HAND]).tolist()
    # without "�" the invalid bytes are unknown; the 1-byte key \xff never matches anything
    tk.set_vocab([k for k in HAND_VOCAB if k != "�"])
    _, ids = tk.CutIds(INVALID, False)
    _same(ids, np.array([1, U, U, 0, U, U], np.int64), "no U+FFFD key")
    tk.set_vocab([b"\xff", b"\x80", b"\xe4", "abc"])
    _, ids = tk.CutIds(INVALID, False)
    _same(ids, np.array([U, U, U, 3, U, U], np.int64), "one-byte keys >= 0x80")
    text = b"\xffabc\xff"
    _same(dev_ids(tk, text, [0, 1, 4, 0], [1, 4, 5, 4])[:4], np.array([U, 3, U, U], np.int64), "\\xff spans")
    with pytest.raises(ValueError):
        tk.CutIds("abc", False, "nope")
    tk.set_vocab(None)


# ---- 2. identity on built spans --------------------------------------------------------------
@pytest.fixture(scope="module")
def ident(mini):
    keys = V.identity_keys()
    text = b"".join(keys)
    ends = np.cumsum([len(k) for k in keys]).astype(np.int64)
    starts = ends - np.array([len(k) for k in keys], np.int64)
    mini.set_vocab(keys)
    yield mini, keys, V.key_dict(keys), text, starts, ends
    mini.set_vocab(None)


def test_identity_on_built_spans(ident):
    tk, keys, d, text, s, e = ident
    n = len(keys)
    assert tk.vocab_size == n and len(text) > 4 << 20
    assert {int(x) & 15 for x in s[:5000]} == set(range(16))  # every start alignment mod 16
    # every key is found at its own index, except the 128 one-byte keys >= 0x80: as a span such a byte
    # is an invalid UTF-8 byte, whose key is EF BF BD (not in this vocabulary)
    ident_ids = np.arange(n, dtype=np.uint32)
    high = np.array([len(k) == 1 and k[0] >= 0x80 for k in keys])
    assert int(high.sum()) == 128
    ident_ids[high] = UNK
    _same(V.expect_ids(d, text, s.tolist(), e.tolist()), ident_ids, "the dict itself")
    _same(tk.spans_ids(text, s, e), ident_ids, "jb_spans_ids")
    _same(dev_ids(tk, text, s, e)[:n], ident_ids, "jb_ids_device")
    nb = len(text)
    for label, s2, e2 in (("end - 1", s, e - 1), ("start + 1", s + 1, e), ("17 extra bytes", s, np.minimum(e + 17, nb))):
        want = V.expect_ids(d, text, s2.tolist(), e2.tolist())
        assert (want == UNK).sum() > n * 9 // 10  # (near misses; one-byte remainders can be keys)
        _same(dev_ids(tk, text, s2, e2)[:n], want, f"jb_ids_device, {label}")
        _same(tk.spans_ids(text, s2, e2), want, f"jb_spans_ids, {label}")


# ---- 3. spans the kernel must not trust ------------------------------------------------------
def test_untrusted_spans(mini):
    tk = mini
    big, mid = b"a" * 100_000, b"Q7" * 150
    longest = b"m" * 40
    keys = [b"abc", b"xyz", longest, b"a"]
    tk.set_vocab(keys)
    text = b"abc " + big + b" " + mid + b" " + longest + b"m xyz"
    nb = len(text)
    p_big, p_mid = 4, 4 + len(big) + 1
    p_long = p_mid + len(mid) + 1
    spans = [
        (0, 3, 0),                              # a key
        (2, 2, U), (3, 2, U), (nb, 0, U),       # start == end, start > end
        (nb - 3, nb + 1, U), (0, nb + 1, U),    # end == nbytes + 1
        (0xFFFFFFF0, 0xFFFFFFFF, U), (5, 0xFFFFFFFF, U),
        (nb - 3, nb, 1),                        # ends exactly at nbytes, in the vocabulary
        (p_big, p_big + len(big), U),           # a 100,000-byte alnum token
        (p_mid, p_mid + len(mid), U),           # a 300-byte one
        (p_long, p_long + 40, 2),               # exactly maxlen bytes
        (p_long, p_long + 41, U),               # maxlen + 1
        (p_big, p_big + 1, 3),
    ]
    s = np.array([a for a, _, _ in spans], np.uint32)
    e = np.array([b for _, b, _ in spans], np.uint32)
    want = np.array([w for _, _, w in spans], np.int64)
    _same(dev_ids(tk, text, s, e)[:len(spans)], want, "untrusted spans")
    # the plain cut of this text has the long tokens themselves
    toks, ids = tk.CutIds(text, False)
    assert toks == ["abc", big.decode(), mid.decode(), (longest + b"m").decode(), "xyz"]
    _same(ids, np.array([0, U, U, U, 1], np.int64), "long alnum tokens")
    # host spans: empty and reversed ones are unknown, the covered range may start anywhere
    _same(tk.spans_ids(text, [nb - 3, 7, 9, p_long], [nb, 7, 8, p_long + 40]), np.array([1, U, U, 2], np.int64),
          "host spans")
    assert len(tk.spans_ids(text, [], [])) == 0
    with pytest.raises(J.JbError) as ei:
        tk.ids_device(16, 1 << 31, 16, 16, 16, 1, 16)
    assert ei.value.code == J.JB_ELIMIT
    tk.set_vocab(None)


# ---- 4. count and capacity ---------------------------------------------------------------------
def test_count_and_capacity(mini, mini_paths):
    import torch
    tk = mini
    keys = [b"k%d" % i for i in range(1000)]
    tk.set_vocab(keys)
    order = np.random.default_rng(5).permutation(1000)
    text = b" ".join(keys[i] for i in order)
    e = np.cumsum([len(keys[i]) + 1 for i in order]) - 1
    s = e - np.array([len(keys[i]) for i in order])
    n = 1000
    got = dev_ids(tk, text, s, e, ntok=700, cap=n, extra=300)  # *d_ntok = n < cap
    _same(got[:700], order[:700], "count below the capacity")
    assert (got[700:] == -7).all()
    got = dev_ids(tk, text, s, e, ntok=n, cap=n // 2, extra=300)  # cap = n // 2
    _same(got[:n // 2], order[:n // 2], "capacity below the count")
    assert (got[n // 2:] == -7).all()
    assert (dev_ids(tk, text, s, e, ntok=0) == -7).all()
    assert (dev_ids(tk, b"", s[:0], e[:0], nbytes=0, ntok=0, cap=0, extra=8) == -7).all()
    assert (dev_ids(tk, text, s, e, ntok=n, cap=0) == -7).all()
    # full mode: more spans than bytes (F.chain_dict(12) on 甲 x 200), capacity = nbytes for both calls
    tf = J.Tokenizer(J.make_config(dict_bytes=F.chain_dict(12).encode(), emit_path=mini_paths[1]))
    with open(mini_paths[1], "rb") as f:
        o = O.Oracle(F.chain_dict(12).encode(), f.read(), J.JB_DICT_TXT, 0)
    try:
        buf, off = R.batch_of(["甲" * 200])
        ws, we, _ = F.expected(o, buf, off)
        nb = int(off[-1])
        assert len(ws) > nb
        words = ["甲" * k for k in range(1, 13)]
        vocab = {w.encode(): i for i, w in enumerate(words[::2])}
        tf.set_vocab(words[::2])
        want = V.expect_ids(vocab, bytes(buf), ws.astype(np.int64).tolist(), we.astype(np.int64).tolist(), nb)
        assert 0 < (want[:nb] != UNK).sum() < nb
        dev = torch.device("cuda:0")
        d_text = torch.from_numpy(_pad(bytes(buf[:nb]))).to(dev)
        d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
        stream = torch.cuda.current_stream().cuda_stream
        guard = 64
        o_s = torch.full((nb + guard,), -7, dtype=torch.int32, device=dev)
        o_e = torch.full((nb + guard,), -7, dtype=torch.int32, device=dev)
        o_i = torch.full((nb + guard,), -7, dtype=torch.int32, device=dev)
        o_d = torch.zeros(2, dtype=torch.int64, device=dev)
        o_n = torch.zeros(1, dtype=torch.int64, device=dev)
        tf.cut_device_full_into(d_text.data_ptr(), nb, d_off.data_ptr(), 1, o_s.data_ptr(), o_e.data_ptr(), nb,
                                o_d.data_ptr(), o_n.data_ptr(), stream)
        tf.ids_device(d_text.data_ptr(), nb, o_s.data_ptr(), o_e.data_ptr(), o_n.data_ptr(), nb, o_i.data_ptr(), stream)
        torch.cuda.synchronize()
        assert int(o_n.cpu()[0]) == len(ws) > nb
        got = o_i.cpu().numpy()
        _same(got[:nb], want[:nb], "full-mode overflow")  # exactly cap ids, and the right ones
        assert (got[nb:] == -7).all()
    finally:
        tf.close()
        tk.set_vocab(None)


# ---- 5. corpus, all modes -----------------------------------------------------------------------
def corpus_vocab(o, dict_path, buf, off):
    """Every second of the sorted distinct tokens of the oracle's hmm = 1 cut, and every second
    dictionary word (those not among the tokens taken)."""
    data = bytes(buf)
    s, e, _ = o.cut_batch(buf, off, True, nthreads=8)
    toks = sorted({V.span_key(data, a, b) for a, b in zip(s.astype(np.int64).tolist(), e.astype(np.int64).tolist())})
    keys = toks[::2]
    seen = set(keys)
    with open(dict_path, encoding="utf-8") as f:
        words = [ln.split(" ")[0].encode() for ln in f if ln.strip()]
    for w in words[::2]:
        if w and w not in seen:
            seen.add(w)
            keys.append(w)
    return keys, len(toks)


def want_ids(vocab, buf, s, e):
    """The dict applied to reference spans; the found share must make the check mean something."""
    data = bytes(buf)
    want = V.expect_ids(vocab, data, np.asarray(s, np.int64).tolist(), np.asarray(e, np.int64).tolist())
    share = float((want != UNK).mean())
    return want, share


def _fetch_ids(tk, ptrs, args, stream):
    import torch
    ps, pe, pd, pn = ptrs
    nb = args[1]
    d_ids = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
    tk.ids_device(args[0], nb, ps, pe, pn, nb, d_ids.data_ptr(), stream)
    torch.cuda.synchronize()
    tk.device_status(stream)
    n = int(J.dev_to_host(pn, 8, np.uint64)[0])
    assert n <= nb
    got = d_ids.cpu().numpy()
    assert (got[n:] == -7).all()
    return got[:n]


@pytest.mark.parametrize("kind,size", KINDS)
@pytest.mark.parametrize("hmm", [False, True])
def test_corpus_all_modes(syn_small, kind, size, hmm):
    import torch
    dp, ep, s = syn_small
    buf, off = s.corpus(synth.KIND_DOCS, 1000, target_bytes=256 << 10)[:2]
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep, kind=kind, size_override=size))
    o = O.Oracle.from_files(dp, ep, kind, size)
    try:
        keys, ndistinct = corpus_vocab(o, dp, buf, off)
        vocab = V.key_dict(keys)
        tk.set_vocab(keys)
        nb, nd = int(off[-1]), len(off) - 1
        d_text = torch.from_numpy(np.ascontiguousarray(buf[:nb + 16])).cuda()
        d_text = torch.cat([d_text, torch.zeros(64, dtype=torch.uint8, device="cuda")])
        d_off = torch.from_numpy(off.astype(np.int64)).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        args = (d_text.data_ptr(), nb, d_off.data_ptr(), nd)
        ps, pe, _ = o.cut_batch(buf, off, hmm, nthreads=8)
        refs = {"cut": (ps, pe), "search": R.expected(o, buf, off, hmm)[:2], "full": F.expected(o, buf, off)[:2]}
        calls = {"cut": lambda: tk.cut_device(*args, hmm, stream), "search": lambda: tk.cut_device_search(*args, hmm, stream),
                 "full": lambda: tk.cut_device_full(*args, stream)}
        for mode in ("cut", "search", "full"):
            want, share = want_ids(vocab, buf, *refs[mode])
            print(f"kind={kind} hmm={hmm} {mode}: {len(want)} tokens, {ndistinct} distinct (hmm=1 cut), "
                  f"found share {share:.3f}")
            assert 0.25 <= share <= 0.75, (mode, share)
            _same(_fetch_ids(tk, calls[mode](), args, stream), want, f"kind={kind} hmm={hmm} {mode}")
        # the host path on the library's own spans
        gs, ge, _ = tk.cut_batch(buf, off, hmm)
        _same(tk.spans_ids(buf, gs, ge), want_ids(vocab, buf, *refs["cut"])[0], "jb_spans_ids on a host batch")
    finally:
        tk.close()


# ---- 6. vocabulary lifecycle -------------------------------------------------------------------
def test_vocabulary_lifecycle(mini_paths):
    tk = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    try:
        text = "今天天氣很好abc"
        b = text.encode()
        s, e = tk.cut_spans(text, False)
        assert J.spans_to_tokens(text, s.tolist(), e.tolist()) == ["今天", "天", "氣", "很", "好", "abc"]
        assert tk.vocab_size == -1
        with pytest.raises(J.JbError) as ei:  # no vocabulary: both id calls refuse
            tk.spans_ids(text, s, e)
        assert ei.value.code == J.JB_EINVAL
        with pytest.raises(J.JbError) as ei:
            dev_ids(tk, b, s, e)
        assert ei.value.code == J.JB_EINVAL
        tk.set_vocab([])  # an empty one: all unknown
        assert tk.vocab_size == 0
        _same(tk.spans_ids(text, s, e), np.full(6, U, np.int64), "empty vocabulary, host")
        _same(dev_ids(tk, b, s, e)[:6], np.full(6, U, np.int64), "empty vocabulary, device")
        A, B = ["今天", "abc", "好"], ["天", "好", "很", "今天天"]
        tk.set_vocab(A)
        _same(tk.spans_ids(text, s, e), np.array([0, U, U, U, 2, 1], np.int64), "A")
        tk.set_vocab(B)
        assert tk.vocab_size == 4
        _same(tk.spans_ids(text, s, e), np.array([U, 0, U, 2, 1, U], np.int64), "B only")
        _same(dev_ids(tk, b, s, e)[:6], np.array([U, 0, U, 2, 1, U], np.int64), "B only, device")
        tk.set_vocab(A)
        with pytest.raises(J.JbError) as ei:  # a failing set leaves A attached
            tk.set_vocab(["很", "x", "很"])
        assert ei.value.code == J.JB_EINVAL and tk.vocab_size == 3
        with pytest.raises(J.JbError) as ei:
            tk.set_vocab(["很", b"y" * 256])
        assert ei.value.code == J.JB_ELIMIT and tk.vocab_size == 3
        _same(tk.spans_ids(text, s, e), np.array([0, U, U, U, 2, 1], np.int64), "A after a failed set")
        # AddWord changes the spans, not the vocabulary
        tk.AddWord("天氣", 1_000_000)
        toks, ids = tk.CutIds(text, False)
        assert toks == ["今", "天", "天氣", "很", "好", "abc"] or toks == ["今天", "天氣", "很", "好", "abc"]
        want = {"今天": 0, "abc": 1, "好": 2}
        _same(ids, np.array([want.get(t, U) for t in toks], np.int64), "A after AddWord")
        assert tk.vocab_size == 3 and toks != ["今天", "天", "氣", "很", "好", "abc"]
        tk.set_vocab(None)
        assert tk.vocab_size == -1
    finally:
        tk.close()


# ---- 7. threads ---------------------------------------------------------------------------------
def test_threads(syn_small):
    """4 threads, each with its own stream and arrays: jb_cut_device_into then jb_ids_device, 3 rounds;
    every result equals the single-threaded one."""
    import torch
    dp, ep, s = syn_small
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
    o = O.Oracle.from_files(dp, ep, 0)
    batches = [s.corpus(synth.KIND_DOCS, 80 + k, target_bytes=(96 + 32 * k) << 10)[:2] for k in range(4)]
    keys, _ = corpus_vocab(o, dp, *batches[0])
    vocab = V.key_dict(keys)
    tk.set_vocab(keys)
    errs = []

    def run(k, out):
        try:
            buf, off = batches[k]
            nb, nd = int(off[-1]), len(off) - 1
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                d_text = torch.from_numpy(_pad(bytes(buf[:nb]))).cuda()
                d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
                o_s = torch.empty(nb + 1, dtype=torch.int32, device="cuda")
                o_e = torch.empty(nb + 1, dtype=torch.int32, device="cuda")
                o_i = torch.empty(nb + 1, dtype=torch.int32, device="cuda")
                o_d = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
                o_n = torch.zeros(1, dtype=torch.int64, device="cuda")
                for rep in range(3):
                    o_i.fill_(-7)
                    tk.cut_device_into(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, o_s.data_ptr(),
                                       o_e.data_ptr(), nb + 1, o_d.data_ptr(), o_n.data_ptr(), st.cuda_stream)
                    tk.ids_device(d_text.data_ptr(), nb, o_s.data_ptr(), o_e.data_ptr(), o_n.data_ptr(), nb + 1,
                                  o_i.data_ptr(), st.cuda_stream)
                    st.synchronize()
                    n = int(o_n.item())
                    got = o_i.cpu().numpy()
                    assert (got[n:] == -7).all()
                    out.append(got[:n].copy())
        except Exception as e:  # noqa: BLE001 (reported below)
            errs.append(e)

    try:
        single = []
        for k in range(4):
            r = []
            run(k, r)
            assert not errs, errs
            ws, we, _ = o.cut_batch(*batches[k], True, nthreads=8)
            _same(r[0], want_ids(vocab, batches[k][0], ws, we)[0], f"single-threaded {k}")
            single.append(r[0])
        outs = [[] for _ in range(4)]
        th = [threading.Thread(target=run, args=(k, outs[k])) for k in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not errs, errs
        for k in range(4):
            assert len(outs[k]) == 3
            for rep in range(3):
                _same(outs[k][rep], single[k], f"thread {k} round {rep}")
    finally:
        tk.close()


# ---- 8. C and C++ programs ------------------------------------------------------------------------
def test_c_and_cpp_consumers(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "c_abi_ids")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_ids.c"), "-L", lib,
                           "-ljiebahip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ids ok" in r.stdout, r.stdout + r.stderr
    exe = str(tmp_path / "cpp_ids_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_ids_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ids ok" in r.stdout, r.stdout + r.stderr
