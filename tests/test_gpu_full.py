"""GPU: full mode (jb_cut_*_full, jieba's cut_all) against the expected output built from the oracle
(tests/full_ref.py: the literal jieba loop over Oracle.build_dag), exact equality of spans and doc_tok."""
import os
import subprocess

import numpy as np
import pytest

import full_ref as F
import jiebahip as J
import oracle as O
import search_ref as R
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(J.JB_DICT_TXT, 0), (J.JB_DICT_PREFIX, J.JIEBA_SIZE)]


def _cmp(got, want, label):
    gs, ge, gd = got
    ws, we, wd = want
    if not (np.array_equal(gs, ws) and np.array_equal(ge, we)):
        n = min(len(gs), len(ws))
        bad = int(np.argmax((gs[:n] != ws[:n]) | (ge[:n] != we[:n]))) if n and not (
            np.array_equal(gs[:n], ws[:n]) and np.array_equal(ge[:n], we[:n])) else n
        raise AssertionError(f"{label}: {len(gs)} vs {len(ws)} spans; first diff #{bad}: "
                             f"gpu={list(zip(gs[bad:bad + 6].tolist(), ge[bad:bad + 6].tolist()))} "
                             f"want={list(zip(ws[bad:bad + 6].tolist(), we[bad:bad + 6].tolist()))}")
    assert np.array_equal(gd, wd), label


def _cmp_batch(tk, o, texts, label, blocks=None):
    buf, off = R.batch_of(texts)
    want = F.expected(o, buf, off, blocks)
    _cmp(tk.cut_batch_full(buf, off), want, label)
    return want


def _open(dict_bytes, emit_path, kind, size):
    tk = J.Tokenizer(J.make_config(dict_bytes=dict_bytes, emit_path=emit_path, kind=kind, size_override=size))
    with open(emit_path, "rb") as f:
        o = O.Oracle(dict_bytes, f.read(), kind, size)
    return tk, o


@pytest.fixture(scope="module")
def small(syn_small):
    dp, ep, s = syn_small
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
    o = O.Oracle.from_files(dp, ep, 0)
    yield tk, o, s
    tk.close()


@pytest.fixture(scope="module")
def corpus(syn_small):
    return syn_small[2].corpus(synth.KIND_DOCS, 1000, target_bytes=256 << 10)[:2]


@pytest.mark.parametrize("kind,size", KINDS)
def test_hand_worked_examples(mini_paths, kind, size):
    for dict_text, cases in F.EXAMPLES:
        tk, o = _open(dict_text.encode(), mini_paths[1], kind, size)
        try:
            for text, want in cases:
                assert tk.CutAll(text) == want, (text, kind)
            _cmp_batch(tk, o, [t for t, _ in cases], f"examples kind={kind}")
        finally:
            tk.close()


EDGE_TEXTS = [
    "", " ", "中", "中文", "abc 中文 def", "abcd 1234", "x", "中a文b丁",
    "english번역『하다』今天天氣很好，ステーションabc1231+1=2我昨天去上海*important*去",
    "　全角空格　中文　abc x\u0085y z",
    "𠀀𠀁𠀂中𪜀文",
    "㐀㐁㐂一二三㐃",
    b"\xff\xfe" + "中文".encode() + b"\x80abc\xe4\xb8",
    "中文".encode() + b"\xed\xa0\x80\xc0\xaf\xf4\x90\x80\x80" + "文".encode() + b"\xe0\x80\xaf",
    "⺀⺙⺛⻳⼀⿕々〇〡〩〸〻豈鶴侮頻𖿰𖿱",
    "〆ゝ中ー文",
    "丁" * 300, "一㐀丁" * 50,
    "a" * 6141 + "丁" * 343, "a" * 6143 + "丁" * 400,  # tokens across a k_zh group edge
    "一丁㐀中文" * 700,  # a long block (k_long)
    "，".join(["中文"] * 2000),
]


def test_edge_texts(small):
    tk, o, s = small
    bl = F.Blocks(o)
    for t in EDGE_TEXTS:
        b = t.encode("utf-8") if isinstance(t, str) else t
        buf, off = R.batch_of([b])
        ws, we, _ = F.expected(o, buf, off, bl)
        gs, ge = tk.cut_full_spans(b)
        assert np.array_equal(gs, ws) and np.array_equal(ge, we), repr(t[:40])
    _cmp_batch(tk, o, EDGE_TEXTS, "edge texts as a batch", bl)
    _cmp_batch(tk, o, ["", "", ""], "empty documents")
    gs, ge, gd = tk.cut_batch_full(np.zeros(16, np.uint8), np.zeros(1, np.uint64))  # an empty batch
    assert len(gs) == 0 and len(ge) == 0 and gd.tolist() == [0]


def _chain_words(dict_text, nmin=12):
    """The longest word of each of the overflow recipe's nested chains, those of at least nmin runes."""
    best = {}
    for ln in dict_text.splitlines():
        w = ln.split(" ")[0]
        if len(w) >= nmin and len(w) > len(best.get(w[:4], "")):
            best[w[:4]] = w
    return list(best.values())


def _pins(word, k):
    """Block ends inside `word` after k runes: a document end whose continuation opens the next document,
    and one ASCII byte."""
    return [word, word[:k], word[k:], "x" + word[:k], word[k:] + "y", word[:k] + "a" + word[k:], word]


def test_block_end_pins(mini_paths, syn_small):
    """A dictionary word must not be found across a document end or a non-Han byte: by the records
    (DICT_A), by the trie walk of zero records (the overflow dictionary) and with plainw == 0."""
    for kind, size in KINDS:
        tk, o = _open(F.DICT_A.encode(), mini_paths[1], kind, size)
        try:
            texts = _pins("甲乙丙丁", 2) + _pins("甲乙丙丁", 1) + _pins("甲乙丙丁", 3)
            want = _cmp_batch(tk, o, texts, f"pins kind={kind}")
            assert tk.CutAll("甲乙a丙丁") == ["甲乙", "a", "丙丁"]
            buf, off = R.batch_of(["x甲乙", "丙丁y"])
            gs, ge, gd = tk.cut_batch_full(buf, off)
            assert O.spans_to_tokens(bytes(buf), gs.astype(np.int64), ge.astype(np.int64)) == ["x", "甲乙", "丙丁", "y"]
            assert gd.tolist() == [0, 2, 4] and len(want[0]) > 20
        finally:
            tk.close()
    dict_text, _ = R.overflow_recipe()
    words = _chain_words(dict_text)
    assert len(words) >= 15
    for kind, size in KINDS:
        tk, o = _open(dict_text.encode(), syn_small[1], kind, size)
        try:
            bl = F.Blocks(o)
            texts = []
            for w in words:
                texts += _pins(w, len(w) // 2) + _pins(w, 3) + _pins(w, 9)
            _cmp_batch(tk, o, texts, f"zero-record pins kind={kind}", bl)
            # (the head of a chain has an edge per prefix that is a word, up to the first absent prefix
            # under JB_DICT_TXT: a record cannot hold more than four, or one longer than eight runes)
            assert bl.stats["zero_like"] >= len(words) // 2, bl.stats
        finally:
            tk.close()
    tk, o = _open(R.PLAINW0_DICT.encode(), mini_paths[1], J.JB_DICT_TXT, 0)
    try:
        assert o.size == -73
        texts = _pins("甲乙丙丁", 2) + _pins("甲乙丙丁", 1) + _pins("甲乙丙丁", 3) + ["x甲乙丙丁，乙丙丁", "丁丁丁丁丁丁甲乙"]
        _cmp_batch(tk, o, texts, "plainw == 0 pins")
        assert tk.CutAll("甲乙丙丁") == F.expected_text(o, "甲乙丙丁") and len(tk.CutAll("甲乙丙丁")) > 2
    finally:
        tk.close()


# Cut takes 甲|乙|丙|丁 and 子|丑|寅|卯 (the singles are frequent, the words rare), so the word of 甲
# reaches over the following plain tokens: 乙, 丙 and 丁 are tokens of their own whose look-back finds 甲.
# In the second family 丑 has a word of its own (丑寅), which is then the nearest for 寅 and 卯.
LOOK_DICT = ("甲 1000\n乙 1000\n丙 1000\n丁 1000\n甲乙 0\n甲乙丙 0\n甲乙丙丁 1\n己 1000\n"
             "子 1000\n丑 1000\n寅 1000\n卯 1000\n子丑 0\n子丑寅 0\n子丑寅卯 1\n丑寅 1\n")


def test_look_back_pins(mini_paths):
    for kind, size in KINDS:
        tk, o = _open(LOOK_DICT.encode(), mini_paths[1], kind, size)
        try:
            if kind == J.JB_DICT_TXT:  # (with the prefix dictionary's size Cut keeps the two words whole)
                assert o.cut("甲乙丙丁丁子丑寅卯", False) == list("甲乙丙丁丁子丑寅卯")
            assert tk.CutAll("甲乙丙丁丁戊") == ["甲乙丙丁", "丁", "戊"]
            assert tk.CutAll("子丑寅卯卯") == ["子丑寅卯", "丑寅", "卯", "卯"]  # (丑寅 ends before the first 卯)
            bl = F.Blocks(o)
            for nfill in range(4084, 4098):  # the token tile (4,096 plain tokens) ends at each rune of the two words
                texts = ["x " * nfill + "甲乙丙丁丁戊己子丑寅卯卯" + " y" * 5000, "乙丙丁"]
                buf, off = R.batch_of(texts)
                assert len(o.cut_batch(buf, off, False)[0]) > 2 * 4096
                _cmp(tk.cut_batch_full(buf, off), F.expected(o, buf, off, bl), f"tile edge nfill={nfill} kind={kind}")
            # runs of singles longer than maxlen (4) behind a word, of runes inside and outside the dictionary
            _cmp_batch(tk, o, ["甲乙丙丁" + "戊" * 20, "甲乙丙丁" + "丁" * 20, "甲乙" + "己" * 9 + "甲乙丙丁己己己己己己",
                               "戊" * 11 + "甲乙丙丁"], f"singles kind={kind}", bl)
        finally:
            tk.close()


def test_look_back_past_eight_runes(mini_paths):
    """A word of twelve runes that Cut does not take (its runes are frequent, the word rare; its proper
    prefixes have frequency 0): its first rune's record cannot hold an edge of twelve runes, so it is a
    zero record, and the single-rune tokens behind it find it up to eleven runes back."""
    word = "子丑寅卯辰巳午未申酉戌亥"
    # (twelve singles cost 12 log(1/12) whatever their frequency; the word, 1 in 1.2e15, costs more)
    dict_text = ("".join(f"{r} {10 ** 14}\n" for r in word) + "".join(f"{word[:k]} 0\n" for k in range(2, 12)) +
                 f"{word} 1\n")
    tk, o = _open(dict_text.encode(), mini_paths[1], J.JB_DICT_TXT, 0)
    try:
        assert o.cut(word + "子", False) == list(word + "子")
        assert tk.CutAll(word + "子") == [word, "子"]
        assert tk.CutAll(word[:11] + "子") == list(word[:11] + "子")  # (no word: every rune alone)
        bl = F.Blocks(o)
        texts = ["x " * k + word + "子" + word[:11] + "，" + word[3:] + word for k in (0, 5, 20, 4090)]
        texts += [word[:k] + "a" + word[k:] + word for k in (1, 6, 11)] + [word[:6], word[6:] + "子"]
        _cmp_batch(tk, o, texts, "a word of twelve runes", bl)
    finally:
        tk.close()


@pytest.mark.parametrize("kind,size", KINDS)
def test_corpus(syn_small, corpus, kind, size):
    dp, ep, _ = syn_small
    buf, off = corpus
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep, kind=kind, size_override=size))
    o = O.Oracle.from_files(dp, ep, kind, size)
    try:
        bl = F.Blocks(o)
        want = F.expected(o, buf, off, bl)
        # (a kernel that copies the plain spans, or drops nothing, cannot pass)
        assert bl.stats["multi"] >= 10000 and bl.stats["dropped"] >= 1000, bl.stats
        for rep in range(2):  # (the second call replays the graph)
            _cmp(tk.cut_batch_full(buf, off), want, f"corpus kind={kind} call {rep}")
        assert tk.last_stats()["tokens"] == len(o.cut_batch(buf, off, False, nthreads=8)[0])  # the plain counts
    finally:
        tk.close()


@pytest.mark.parametrize("kind,size", KINDS)
def test_overflowed_records(syn_small, kind, size):
    """Runes with more than 4 edges or an edge longer than 8 runes have the record 0: their words
    come from the trie walk."""
    dict_text, texts = R.overflow_recipe()
    tk, o = _open(dict_text.encode(), syn_small[1], kind, size)
    try:
        bl = F.Blocks(o)
        _cmp_batch(tk, o, texts, f"overflow kind={kind}", bl)
        assert bl.stats["zero_like"] >= 200, bl.stats
    finally:
        tk.close()


def test_expansion_past_the_byte_count(mini_paths):
    """More spans than bytes: the host call returns them all; the device call writes the first `cap`,
    counts all of them and reports JB_ELIMIT; the ctx is fine afterwards."""
    import torch
    tk, o = _open(F.chain_dict(12).encode(), mini_paths[1], J.JB_DICT_TXT, 0)
    try:
        text = "甲" * 200
        buf, off = R.batch_of([text, "x", text])
        want = F.expected(o, buf, off)
        nb, nd = int(off[-1]), len(off) - 1
        assert len(want[0]) > 3 * nb
        _cmp(tk.cut_batch_full(buf, off), want, "host")
        assert len(tk.CutAll(text)) == sum(min(11, 199 - i) for i in range(200))
        dev = torch.device("cuda:0")
        d_text = torch.from_numpy(np.array(buf)).to(dev)
        d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
        stream = torch.cuda.current_stream().cuda_stream
        cap, guard = 64, 32
        o_s = torch.full((cap + guard,), -7, dtype=torch.int32, device=dev)
        o_e = torch.full((cap + guard,), -7, dtype=torch.int32, device=dev)
        o_d = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
        o_n = torch.zeros(1, dtype=torch.int64, device=dev)
        tk.cut_device_full_into(d_text.data_ptr(), nb, d_off.data_ptr(), nd, o_s.data_ptr(), o_e.data_ptr(), cap,
                                o_d.data_ptr(), o_n.data_ptr(), stream)
        torch.cuda.synchronize()
        with pytest.raises(J.JbError) as ei:
            tk.device_status(stream)
        assert ei.value.code == J.JB_ELIMIT
        assert int(o_n.cpu()[0]) == len(want[0])
        assert np.array_equal(o_d.cpu().numpy().view(np.uint64), want[2])
        assert np.array_equal(o_s[:cap].cpu().numpy().view(np.uint32), want[0][:cap].astype(np.uint32))
        assert np.array_equal(o_e[:cap].cpu().numpy().view(np.uint32), want[1][:cap].astype(np.uint32))
        assert bool((o_s[cap:] == -7).all()) and bool((o_e[cap:] == -7).all())  # nothing past the capacity
        assert tk.last_stats()["tokens"] == len(o.cut_batch(buf, off, False)[0])
        # the ctx-owned arrays hold nbytes spans: the same report
        ps, pe, pd, pn = tk.cut_device_full(d_text.data_ptr(), nb, d_off.data_ptr(), nd, stream)
        torch.cuda.synchronize()
        with pytest.raises(J.JbError) as ei:
            tk.device_status(stream)
        assert ei.value.code == J.JB_ELIMIT
        assert int(J.dev_to_host(pn, 8, np.uint64)[0]) == len(want[0])
        assert np.array_equal(J.dev_to_host(ps, 4 * nb, np.uint32), want[0][:nb].astype(np.uint32))
        # a following plain call is fine and correct
        plain = o.cut_batch(buf, off, False)
        ps, pe, pd, pn = tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, False, stream)
        torch.cuda.synchronize()
        tk.device_status(stream)
        n = int(J.dev_to_host(pn, 8, np.uint64)[0])
        _cmp((J.dev_to_host(ps, 4 * n, np.uint32), J.dev_to_host(pe, 4 * n, np.uint32),
              J.dev_to_host(pd, 8 * (nd + 1), np.uint64)), plain, "plain after the overflow")
        # arrays of the reported size take the whole list
        n = len(want[0])
        o_s = torch.zeros(n, dtype=torch.int32, device=dev)
        o_e = torch.zeros(n, dtype=torch.int32, device=dev)
        tk.cut_device_full_into(d_text.data_ptr(), nb, d_off.data_ptr(), nd, o_s.data_ptr(), o_e.data_ptr(), n,
                                o_d.data_ptr(), o_n.data_ptr(), stream)
        torch.cuda.synchronize()
        tk.device_status(stream)
        _cmp((o_s.cpu().numpy().view(np.uint32), o_e.cpu().numpy().view(np.uint32),
              o_d.cpu().numpy().view(np.uint64)), want, "device into, full size")
    finally:
        tk.close()


def test_device_api_and_graphs(small, corpus):
    """Plain, search and full calls alternating on one ctx and the same buffers: each replays its own
    graph, and each result is its own."""
    import torch
    tk, o, s = small
    buf, off = corpus
    nb, nd = int(off[-1]), len(off) - 1
    dev = torch.device("cuda:0")
    d_text = torch.from_numpy(np.array(buf)).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    plain = o.cut_batch(buf, off, False, nthreads=8)
    plain_h = o.cut_batch(buf, off, True, nthreads=8)
    srch = R.expand(o, buf, *plain_h)
    full = F.expected(o, buf, off)
    assert len(full[0]) <= nb  # (this corpus fits the ctx-owned arrays)

    def fetch(ps, pe, pd, pn):
        n = int(J.dev_to_host(pn, 8, np.uint64)[0])
        return J.dev_to_host(ps, 4 * n, np.uint32), J.dev_to_host(pe, 4 * n, np.uint32), J.dev_to_host(
            pd, 8 * (nd + 1), np.uint64)

    def check(label, ntok):
        torch.cuda.synchronize()
        tk.device_status(stream)
        assert tk.last_stats()["tokens"] == ntok, label

    args = (d_text.data_ptr(), nb, d_off.data_ptr(), nd)
    for rep in range(3):
        _cmp(fetch(*tk.cut_device_full(*args, stream)), full, f"full {rep}")
        check(f"full {rep}", len(plain[0]))
        _cmp(fetch(*tk.cut_device(*args, True, stream)), plain_h, f"plain {rep}")
        check(f"plain {rep}", len(plain_h[0]))
        _cmp(fetch(*tk.cut_device_search(*args, True, stream)), srch, f"search {rep}")
        check(f"search {rep}", len(plain_h[0]))
    o_s = torch.zeros(nb, dtype=torch.int32, device=dev)
    o_e = torch.zeros(nb, dtype=torch.int32, device=dev)
    o_d = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    o_n = torch.zeros(1, dtype=torch.int64, device=dev)
    for rep in range(2):
        tk.cut_device_full_into(*args, o_s.data_ptr(), o_e.data_ptr(), nb, o_d.data_ptr(), o_n.data_ptr(), stream)
        check(f"into {rep}", len(plain[0]))
        n = int(o_n.cpu()[0])
        _cmp((o_s[:n].cpu().numpy().view(np.uint32), o_e[:n].cpu().numpy().view(np.uint32),
              o_d.cpu().numpy().view(np.uint64)), full, f"device into {rep}")


def test_several_devices(syn_small, monkeypatch):
    """Two devices (JB_DEVICE_WRAP maps them onto the one GPU): a documents corpus, then its first
    document alone, which is one document split at Han-run starts."""
    dp, ep, s = syn_small
    monkeypatch.setenv("JB_DEVICE_WRAP", "1")
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep, ndevices=2))
    monkeypatch.delenv("JB_DEVICE_WRAP")
    o = O.Oracle.from_files(dp, ep, 0)
    try:
        buf, off, _ = s.corpus(synth.KIND_DOCS, 42, target_bytes=512 << 10)
        bl = F.Blocks(o)
        _cmp(tk.cut_batch_full(buf, off), F.expected(o, buf, off, bl), "two devices")
        _cmp(tk.cut_batch_full(buf, off[:2]), F.expected(o, buf, off[:2], bl), "one document over two devices")
    finally:
        tk.close()


def test_c_consumer(mini_paths, tmp_path):
    """A C99 program on the full-mode entry points, and the C++ mirror's CutAll."""
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "c_abi_full")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_full.c"), "-L", lib,
                           "-ljiebahip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "full ok" in r.stdout, r.stdout + r.stderr
    exe = str(tmp_path / "cpp_full_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_full_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    dp = tmp_path / "dict.txt"
    dp.write_text(F.DICT_B, encoding="utf-8")
    r = subprocess.run([exe, str(dp), mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "full ok" in r.stdout, r.stdout + r.stderr
