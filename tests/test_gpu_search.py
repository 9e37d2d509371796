"""GPU: search mode (jb_cut_*_search) against the expected output built from the oracle
(tests/search_ref.py), exact equality of spans and doc_tok."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

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


def _cmp_batch(tk, o, buf, off, hmm, label, grams=None):
    want = R.expected(o, buf, off, hmm, grams=grams)
    _cmp(tk.cut_batch_search(buf, off, hmm), want, label)
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
def test_hand_checked_examples(mini_paths, kind, size):
    with open(mini_paths[0], "rb") as f:
        mini = f.read()
    for dict_text, cases in R.EXAMPLES:
        tk, o = _open(mini if dict_text is None else dict_text.encode(), mini_paths[1], kind, size)
        try:
            for hmm in (False, True):
                for text, want in cases:
                    assert tk.CutForSearch(text, hmm) == want, (text, kind, hmm)
                buf, off = R.batch_of([t for t, _ in cases])
                _cmp_batch(tk, o, buf, off, hmm, f"examples kind={kind} hmm={hmm}")
        finally:
            tk.close()


EDGE_TEXTS = [
    "", " ", "中", "中文", "abc 中文 def",
    "english번역『하다』今天天氣很好，ステーションabc1231+1=2我昨天去上海*important*去",
    "　全角空格　中文　abc x\u0085y z",
    "𠀀𠀁𠀂中𪜀文",
    "㐀㐁㐂一二三㐃",
    b"\xff\xfe" + "中文".encode() + b"\x80abc\xe4\xb8",
    "中文".encode() + b"\xed\xa0\x80\xc0\xaf\xf4\x90\x80\x80" + "文".encode() + b"\xe0\x80\xaf",
    "⺀⺙⺛⻳⼀⿕々〇〡〩〸〻豈鶴侮頻𖿰𖿱",
    "〆ゝ中ー文",
    "a1+1=2 中文 x　y",
    "丁" * 300, "一㐀丁" * 50,
    "a" * 6141 + "丁" * 343, "a" * 6143 + "丁" * 400,  # tokens across a k_zh group edge
    ("中文。" * 900) + "丁" * 3000 + ("，中文" * 900),
    "一丁㐀中文" * 700,  # a long block (k_long)
    "，".join(["中文"] * 4000),
]


@pytest.mark.parametrize("hmm", [False, True])
def test_edge_texts(small, hmm):
    tk, o, s = small
    g = R.Grams(o)
    for t in EDGE_TEXTS:
        b = t.encode("utf-8") if isinstance(t, str) else t
        buf, off = R.batch_of([b])
        ws, we, _ = R.expected(o, buf, off, hmm, nthreads=1, grams=g)
        gs, ge = tk.cut_search_spans(b, hmm)
        assert np.array_equal(gs, ws) and np.array_equal(ge, we), repr(t[:40])
    buf, off = R.batch_of(EDGE_TEXTS)
    _cmp_batch(tk, o, buf, off, hmm, f"edge texts as a batch hmm={hmm}", g)


def test_random_mixed_script(small):
    tk, o, s = small
    rng = random.Random(2)
    alphabet = [chr(c) for c in range(0x4E00, 0x4E00 + 3000, 3)] + ["㐀", "㒐", "a", "Z", "9", " ", "，", "。",
                                                                    "　", "ス", "한", " ", "\n", "𠀀"]
    texts = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 80))) for _ in range(2000)]
    assert "" in texts
    buf, off = R.batch_of(texts)
    g = R.Grams(o)
    for hmm in (False, True):
        _cmp_batch(tk, o, buf, off, hmm, f"mixed hmm={hmm}", g)


def _gram_counts(buf, off, o, hmm):
    """(grams, 3-rune grams) of the expected output."""
    ps, pe, pd = o.cut_batch(buf, off, hmm, nthreads=8)
    xs, xe, _ = R.expand(o, buf, ps, pe, pd)
    data = bytes(buf)
    n = n3 = k = 0  # (the spans before a token's own span are its grams)
    for a, b in zip(ps.tolist(), pe.tolist()):
        while not (int(xs[k]) == a and int(xe[k]) == b):
            n += 1
            n3 += len(data[int(xs[k]):int(xe[k])].decode("utf-8")) == 3
            k += 1
        k += 1
    assert k == len(xs)
    return n, n3


@pytest.mark.parametrize("hmm", [False, True])
@pytest.mark.parametrize("kind,size", KINDS)
def test_corpus(syn_small, corpus, kind, size, hmm):
    dp, ep, _ = syn_small
    buf, off = corpus
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep, kind=kind, size_override=size))
    o = O.Oracle.from_files(dp, ep, kind, size)
    try:
        n, n3 = _gram_counts(buf, off, o, hmm)
        assert n >= 1000 and n3 >= 100, (n, n3)  # (a kernel that emits nothing cannot pass)
        for rep in range(2):  # (the second call replays the pipeline's graph)
            _cmp_batch(tk, o, buf, off, hmm, f"corpus kind={kind} hmm={hmm} call {rep}")
    finally:
        tk.close()


_NO_GRAPH = """
import sys
sys.path[:0] = [{tests!r}, {oracle!r}, {gen!r}, {py!r}]
import numpy as np
import jiebahip as J, oracle as O, search_ref as R, synth
dp, ep = sys.argv[1:3]
s = synth.Synth(nwords=20_000)
buf, off, _ = s.corpus(synth.KIND_DOCS, 1000, target_bytes=256 << 10)
tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
o = O.Oracle.from_files(dp, ep, 0)
for rep in range(2):
    for hmm in (False, True):
        gs, ge, gd = tk.cut_batch_search(buf, off, hmm)
        ws, we, wd = R.expected(o, buf, off, hmm)
        assert np.array_equal(gs, ws) and np.array_equal(ge, we) and np.array_equal(gd, wd), (rep, hmm)
tk.close()
print("ok", len(ws))
"""


def test_corpus_without_graphs(syn_small):
    """The corpus once more with JB_GRAPH=0 (read once per process, so in a child process)."""
    dp, ep, _ = syn_small
    code = _NO_GRAPH.format(tests=os.path.join(ROOT, "tests"), oracle=os.path.join(ROOT, "oracle"),
                            gen=os.path.join(ROOT, "gen"), py=os.path.join(ROOT, "jieba-go_amd", "python"))
    env = dict(os.environ, JB_GRAPH="0")
    r = subprocess.run([sys.executable, "-c", code, dp, ep], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


@pytest.mark.parametrize("kind,size", KINDS)
def test_overflowed_records(syn_small, kind, size):
    """Runes with more than 4 edges or an edge longer than 8 runes have the record 0: their grams
    come from the trie walk."""
    dict_text, texts = R.overflow_recipe()
    tk, o = _open(dict_text.encode(), syn_small[1], kind, size)
    try:
        buf, off = R.batch_of(texts)
        data = bytes(buf)
        g = R.Grams(o)
        for hmm in (False, True):
            ps, pe, pd = o.cut_batch(buf, off, hmm, nthreads=8)
            nover, dags = 0, {}
            for a, b in zip(ps.tolist(), pe.tolist()):
                tok = data[a:b]
                gr = g.of_token(tok) if b - a >= 9 and tok[0] >= 0x80 else []
                if not gr:
                    continue
                if tok not in dags:
                    # (the token's own DAG: a subset of its Han run's, so this count is a lower bound)
                    dag = o.build_dag(tok)
                    pos, p = {}, 0
                    for i, ch in enumerate(tok.decode("utf-8")):
                        pos[p] = i
                        p += len(ch.encode("utf-8"))
                    dags[tok] = {q for q, i in pos.items() if len(dag[i]) > 4 or max(dag[i]) - i > 8}
                nover += sum(1 for x, _ in gr if x in dags[tok])
            assert nover >= 100, nover
            _cmp(tk.cut_batch_search(buf, off, hmm), R.expand(o, buf, ps, pe, pd, g),
                 f"overflow kind={kind} hmm={hmm}")
    finally:
        tk.close()


def test_plainw_zero(mini_paths):
    """A dictionary whose size is negative: every record is zero, every gram comes from the walk."""
    tk, o = _open(R.PLAINW0_DICT.encode(), mini_paths[1], J.JB_DICT_TXT, 0)
    try:
        assert o.size == -73
        for hmm in (False, True):
            for text in ("甲乙丙丁", "x甲乙丙丁，乙丙丁"):
                assert tk.CutForSearch(text, hmm) == R.expected_text(o, text, hmm), text
            assert len(tk.CutForSearch("甲乙丙丁", hmm)) > 1
            bad = "甲乙丙丁戊甲乙丙"
            with pytest.raises(RuntimeError):
                o.cut(bad, hmm)
            with pytest.raises(J.JbError) as ei:
                tk.Cut(bad, hmm)
            assert ei.value.code == J.JB_EPANIC
            with pytest.raises(J.JbError) as ei:
                tk.CutForSearch(bad, hmm)
            assert ei.value.code == J.JB_EPANIC
    finally:
        tk.close()


def test_device_api_and_graphs(small, corpus):
    """jb_cut_device_search / _into on torch-owned buffers; plain and search calls alternating on the
    same buffers each replay their own graph and leave no state behind."""
    import torch
    tk, o, s = small
    buf, off = corpus
    nb, nd = int(off[-1]), len(off) - 1
    dev = torch.device("cuda:0")
    d_text = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    hmm = True
    plain = o.cut_batch(buf, off, hmm, nthreads=8)
    want = R.expand(o, buf, *plain)

    def fetch(ps, pe, pd, pn):
        n = int(J.dev_to_host(pn, 8, np.uint64)[0])
        return J.dev_to_host(ps, 4 * n, np.uint32), J.dev_to_host(pe, 4 * n, np.uint32), J.dev_to_host(
            pd, 8 * (nd + 1), np.uint64)

    def check(label):
        torch.cuda.synchronize()
        tk.device_status(stream)
        assert tk.last_stats()["tokens"] == len(plain[0]), label

    _cmp(fetch(*tk.cut_device_search(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, stream)), want, "device")
    check("device")
    o_s = torch.zeros(nb, dtype=torch.int32, device=dev)
    o_e = torch.zeros(nb, dtype=torch.int32, device=dev)
    o_d = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    o_n = torch.zeros(1, dtype=torch.int64, device=dev)
    tk.cut_device_search_into(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, o_s.data_ptr(), o_e.data_ptr(), nb,
                              o_d.data_ptr(), o_n.data_ptr(), stream)
    check("into")
    n = int(o_n.cpu()[0])
    _cmp((o_s[:n].cpu().numpy().view(np.uint32), o_e[:n].cpu().numpy().view(np.uint32),
          o_d.cpu().numpy().view(np.uint64)), want, "device into")
    with pytest.raises(J.JbError) as ei:
        tk.cut_device_search_into(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, o_s.data_ptr(), o_e.data_ptr(),
                                  nb - 1, o_d.data_ptr(), o_n.data_ptr(), stream)
    assert ei.value.code == J.JB_EINVAL
    for rep in range(3):
        _cmp(fetch(*tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, stream)), plain, f"plain {rep}")
        check(f"plain {rep}")
        _cmp(fetch(*tk.cut_device_search(d_text.data_ptr(), nb, d_off.data_ptr(), nd, hmm, stream)), want,
             f"search {rep}")
        check(f"search {rep}")


def test_several_devices(syn_small, monkeypatch):
    """Two devices (JB_DEVICE_WRAP maps them onto the one GPU): a documents corpus, then its first
    document alone, which is one document split at Han-run starts."""
    dp, ep, s = syn_small
    monkeypatch.setenv("JB_DEVICE_WRAP", "1")
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep, ndevices=2))
    monkeypatch.delenv("JB_DEVICE_WRAP")
    o = O.Oracle.from_files(dp, ep, 0)
    try:
        buf, off, _ = s.corpus(synth.KIND_DOCS, 42, target_bytes=6 << 20)
        g = R.Grams(o)
        _cmp_batch(tk, o, buf, off, True, "two devices", g)
        _cmp_batch(tk, o, buf, off[:2], True, "one document over two devices", g)
    finally:
        tk.close()


def test_c_consumer(mini_paths, tmp_path):
    """A C99 program on the search entry points, and the C++ mirror's CutForSearch."""
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "c_abi_search")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_search.c"), "-L", lib,
                           "-ljiebahip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "search ok" in r.stdout, r.stdout + r.stderr
    exe = str(tmp_path / "cpp_search_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_search_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    dp = tmp_path / "dict.txt"
    dp.write_text(R.EXAMPLES[0][0], encoding="utf-8")
    r = subprocess.run([exe, str(dp), mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "search ok" in r.stdout, r.stdout + r.stderr
