"""CPU: jb_wc_count, the host form of the word-count rule (jieba-go_amd/csrc/jb_wc.cpp), against wc_ref.py:
keys, counts, order and totals, exactly; the size helpers, jb_wc_fp and the limits.  The cuts come from the
oracle and the mode references over tests/golden/mini_dict.txt.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest

import codepoint_cases as CC
import full_ref as F
import jiebahip as J
import oracle as O
import search_ref as R
import wc_ref as W

MIXED = "english번역『하다』今天天氣很好，ステーションabc1231+1=2我昨天去上海*important*去"  # (test_gpu_ids.MIXED)
INVALID = b"\xff\xfe" + "中文".encode() + b"\x80abc\xe4\xb8"
TEXTS = [MIXED, INVALID, "这一刹那", MIXED, "今天天氣很好", "", "这一刹那的上海"]
NEW = ["jb_wc_table_bytes", "jb_wc_work_bytes", "jb_wc_fp", "jb_wc_init_device", "jb_wc_add_device", "jb_wc_read",
       "jb_wc_result_free", "jb_wc_count", "jb_wc_batch", "jb_device_alloc", "jb_device_free"]


def test_exports():
    L = J.lib()
    for name in NEW:
        assert name in J.EXPORTS and hasattr(L, name), name


def check(text, s, e, ntok=None, cap=None, **kw):
    ref = W.wc_ref(text, s, e, ntok, cap, **kw)
    got = J.wc_count(text, s, e, ntok=ntok, cap=cap, **kw)
    assert W.same(got, ref) is None, W.same(got, ref)
    return got, ref


def _spans(o, buf, off, mode, hmm):
    if mode == "cut":
        return o.cut_batch(buf, off, hmm)
    if mode == "search":
        return R.expected(o, buf, off, hmm)
    return F.expected(o, buf[:int(off[-1])], off)


@pytest.mark.parametrize("mode,hmm", [("cut", False), ("cut", True), ("search", False), ("search", True), ("full", False)])
def test_mini_dictionary_cuts(mini_paths, mode, hmm):
    o = O.Oracle.from_files(mini_paths[0], mini_paths[1], 0)
    buf, off = R.batch_of(TEXTS)
    s, e, _ = _spans(o, buf, off, mode, hmm)
    got, ref = check(bytes(buf[:int(off[-1])]), s, e)
    assert got.tokens == len(s) > 60 and got.bad == 0 and got.long == 0
    c = dict(zip(got.keys, got.counts.tolist()))
    assert c[W.REPL] == 3 and c["上海".encode()] == 3 and c[b"english"] == 2 and c["今天".encode()] == 3
    assert c.get("一刹".encode(), 0) == (0 if mode == "cut" else 2)
    assert int(got.counts.sum()) == got.tokens


@pytest.mark.parametrize("name", ["D", "T", "M"])
def test_codepoint_inputs(mini_paths, name):
    """Every code point and malformed sequence through the plain cut: invalid bytes are keyed as U+FFFD."""
    buf, off = {"D": CC.corpus_D, "T": CC.corpus_T, "M": CC.corpus_M}[name]()
    buf, off = np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(off, np.uint64)
    if name == "M":
        off = off[:12_001]  # (235,904 documents: a share of them keeps the Python statement quick)
    o = O.Oracle.from_files(mini_paths[0], mini_paths[1], 0)
    s, e, _ = o.cut_batch(buf, off, True)
    got, ref = check(bytes(buf[:int(off[-1])]), s, e)
    assert got.bad == 0 and got.long == 0 and got.tokens == len(s) > 400
    for k in got.keys:
        k.decode("utf-8")  # every key is whole runes, or U+FFFD for an invalid byte
    if name != "D":
        assert W.REPL in got.keys


def test_malformed_span_lists():
    kinds = set()
    for seed in range(300):
        text, s, e, ntok, cap = W.random_case(seed)
        got, ref = check(text, s, e, ntok, cap)
        kinds.add((ntok > cap, ntok < cap, got.bad > 0, got.long > 0))
        assert int(got.counts.sum()) + got.bad + got.long == got.tokens == min(ntok, cap)
        assert got.dropped == 0 and got.collided == 0
        if seed % 10 == 0:
            check(text, s, e, ntok, cap, min_count=2)
            check(text, s, e, ntok, cap, max_keys=3)
            check(text, s, e, ntok, cap, min_count=3, max_keys=2)
    assert all(any(k[i] for k in kinds) for i in range(4))


def test_order_and_filters():
    toks = [b"b", b"ab", b"a", b"abc", b"b", b"a", b"\xff", b"\xc3\xa9", b"abc", b"z" * 255, b"z" * 254, b"ab", b"a"]
    text, s, e = W.from_keys(toks, gap=b" ")
    got, _ = check(text, s, e)
    # by count, then by bytes with a proper prefix first; bytes compare unsigned (\xc3 before \xef, after "z")
    assert got.keys == [b"a", b"ab", b"abc", b"b", b"z" * 254, b"z" * 255, b"\xc3\xa9", W.REPL]
    assert got.counts.tolist() == [3, 2, 2, 2, 1, 1, 1, 1]
    assert J.wc_count(text, s, e, min_count=2).keys == [b"a", b"ab", b"abc", b"b"]
    assert J.wc_count(text, s, e, min_count=4).keys == []
    assert J.wc_count(text, s, e, max_keys=2).keys == [b"a", b"ab"]
    assert J.wc_count(text, s, e, min_count=2, max_keys=9).keys == [b"a", b"ab", b"abc", b"b"]
    r = J.wc_count(text, s, e, min_count=0, max_keys=1)
    assert r.keys == [b"a"] and r.tokens == len(toks)  # (the totals do not depend on the filters)
    # a key of 256 bytes is long, whatever it holds; an empty and a reversed span are bad
    text, s, e = W.from_keys([b"q" * 256, b"\xff" * 256, b"q"])
    r = J.wc_count(text, np.append(s, [5, 9]), np.append(e, [5, 2]))
    assert r.keys == [b"q"] and r.long == 2 and r.bad == 2 and r.tokens == 5


def test_empty_inputs():
    for text, s, e, kw in ((b"", [], [], {}), (b"abc", [], [], {}), (b"abc", [0], [3], dict(ntok=0)),
                           (b"abc", [0], [3], dict(cap=0)), (b"", [0], [1], {})):
        r = J.wc_count(text, s, e, **kw)
        assert r.keys == [] and len(r.counts) == 0 and r.tokens == (1 if text == b"" and len(s) else 0)
        assert r.bad == r.tokens


def test_size_helpers():
    prev = 0
    for nslots in (0, 1, 8, 9, 16, 1000, 1024, 1025, 2 ** 20, 2 ** 30, 2 ** 30 + 1, 2 ** 40, 2 ** 63, 2 ** 64 - 1):
        w = J.wc_table_bytes(nslots, 100)
        assert w > 0 and w >= prev, nslots
        prev = w
    prev = 0
    for pool in (0, 1, 255, 256, 257, 2 ** 20, 2 ** 32, 2 ** 48, 2 ** 64 - 1):
        w = J.wc_table_bytes(1024, pool)
        assert w > 0 and w >= prev, pool
        prev = w
    assert J.wc_table_bytes(8, 0) == J.wc_table_bytes(0, 0) == 256 + 8 * 48
    assert J.wc_table_bytes(1024, 25) >= 256 + 1024 * 48 + 25
    prev = 0
    for ntok in (0, 1, 63, 64, 65, 10 ** 6, 2 ** 32 - 257, 2 ** 40, 2 ** 64 - 1):
        w = J.wc_work_bytes(ntok)
        assert w > 0 and w >= prev and (ntok > 2 ** 60 or w >= 4 * ntok), ntok
        prev = w


def test_fingerprint_is_the_vocabulary_hash():
    """jb_wc_fp is jb_vocab_hash (what jb_vocab_lookup and k_ids probe with), narrowed: wc_ref.vocab_hash
    restates it, and a vocabulary of the same keys finds each of them by it."""
    rng = np.random.default_rng(3)
    keys = {bytes(rng.integers(1, 256, int(n)).astype(np.uint8)) for n in rng.integers(1, 256, 400)}
    keys |= {b"a", b"a" * 8, b"a" * 9, b"a" * 16, b"a" * 17, b"a" * 24, b"a" * 25, b"a" * 255, W.REPL, "中文".encode()}
    keys = sorted(keys)
    for k in keys:
        assert J.wc_fp(k) == (W.vocab_hash(k) or 1), k
        for bits in (1, 4, 17, 32, 63):
            f = J.wc_fp(k, bits)
            assert f == W.fp(k, bits) and 1 <= f < (1 << bits) or (bits == 1 and f == 1), (k, bits)
    v = J.Vocab(keys)
    try:
        assert [v.lookup(k) for k in keys] == list(range(len(keys)))
    finally:
        v.close()
    L = J.lib()
    assert L.jb_wc_fp(None, 3, 64) == 0 and L.jb_wc_fp(b"abc", 0, 64) == 0 and L.jb_wc_fp(b"a" * 256, 256, 64) == 0
    assert L.jb_wc_fp(b"abc", 3, 0) == 0 and L.jb_wc_fp(b"abc", 3, 65) == 0


def test_limits():
    L = J.lib()
    r = J.jb_wc_result()
    s, e = np.array([0], np.uint32), np.array([3], np.uint32)
    assert L.jb_wc_count(b"abc", 3, s.ctypes.data, e.ctypes.data, 1, 1, 1, 0, C.byref(r)) == J.JB_OK and r.nkeys == 1
    L.jb_wc_result_free(C.byref(r))
    assert not r.keys and not r.key_off and not r.counts and r.nkeys == 0
    L.jb_wc_result_free(C.byref(r))  # (twice is fine)
    L.jb_wc_result_free(None)
    assert L.jb_wc_count(b"abc", 3, s.ctypes.data, e.ctypes.data, 1, 1, 1, 0, None) == J.JB_EINVAL
    assert L.jb_wc_count(None, 3, s.ctypes.data, e.ctypes.data, 1, 1, 1, 0, C.byref(r)) == J.JB_EINVAL
    assert L.jb_wc_count(b"abc", 3, None, e.ctypes.data, 1, 1, 1, 0, C.byref(r)) == J.JB_EINVAL
    assert L.jb_wc_count(b"abc", 3, s.ctypes.data, None, 1, 1, 1, 0, C.byref(r)) == J.JB_EINVAL
    assert L.jb_wc_count(b"abc", 2 ** 31, s.ctypes.data, e.ctypes.data, 1, 1, 1, 0, C.byref(r)) == J.JB_ELIMIT
    assert b"2 GiB" in L.jb_last_error()
    # null is fine where the length is 0
    assert L.jb_wc_count(None, 0, s.ctypes.data, e.ctypes.data, 1, 1, 1, 0, C.byref(r)) == J.JB_OK and r.nbad == 1
    L.jb_wc_result_free(C.byref(r))
    assert L.jb_wc_count(b"abc", 3, None, None, 7, 0, 1, 0, C.byref(r)) == J.JB_OK and r.ntokens == 0
    L.jb_wc_result_free(C.byref(r))
