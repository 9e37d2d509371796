"""GPU: term counts and keywords (jb_terms_device, jb_keywords_device, jb_keywords_batch; jb_terms.hip)
against numpy (terms_ref.py: np.unique per document, np.lexsort over (id, -score)).  Most tests hand the
kernels id arrays and CSRs they built themselves, so counting and ranking are checked independently of
segmentation and lookup."""
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
import terms_ref as TR
import vocab_ref as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(J.JB_DICT_TXT, 0), (J.JB_DICT_PREFIX, J.JIEBA_SIZE)]  # (those of test_gpu_ids.py)
UNK = TR.UNK
T = J.JB_TERMS_TILE
GUARD = 0x7A7A7A7A  # what the output arrays hold before a call


def test_tile_constant_follows_the_code():
    # the work buffer holds two 8-byte entries per token of whole tiles: it grows by 16 T from T to T + 1
    assert 16 * T <= J.terms_work_bytes(T + 1, 1) - J.terms_work_bytes(T, 1) < 16 * T + 4096
    assert J.terms_work_bytes(1, 1) == J.terms_work_bytes(T, 1)


def _dev(a, dtype, view=None):
    import torch
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(view) if view is not None else a).cuda()


def dev_terms(tk, ids, doc_tok, ntok=None, ids_cap=None, cap=None, extra=64, nwork=None, stream=None):
    """jb_terms_device on an id list of the test's own -> (term_id, term_cnt: the whole arrays, cap + extra
    entries pre-filled with GUARD; term_off; nterms)."""
    import torch
    ids = np.asarray(ids, np.uint32)
    ids_cap = len(ids) if ids_cap is None else ids_cap
    ntok = len(ids) if ntok is None else ntok
    cap = ids_cap if cap is None else cap
    nd = len(doc_tok) - 1
    d_ids = _dev(ids if len(ids) else np.zeros(1, np.uint32), np.uint32, np.int32)
    d_tok = _dev(doc_tok, np.uint64, np.int64)
    d_n = torch.tensor([ntok], dtype=torch.int64, device="cuda")
    o_id = torch.full((cap + extra,), GUARD, dtype=torch.int32, device="cuda")
    o_cnt = torch.full((cap + extra,), GUARD, dtype=torch.int32, device="cuda")
    o_off = torch.full((nd + 1 + 8,), -7, dtype=torch.int64, device="cuda")
    o_n = torch.full((1 + 8,), -7, dtype=torch.int64, device="cuda")
    need = J.terms_work_bytes(ids_cap, nd)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    tk.terms_device(d_ids.data_ptr(), ids_cap, d_tok.data_ptr(), d_n.data_ptr(), nd, o_id.data_ptr(), o_cnt.data_ptr(),
                    cap, o_off.data_ptr(), o_n.data_ptr(), work.data_ptr(), need if nwork is None else nwork, st)
    torch.cuda.synchronize()
    off, n = o_off.cpu().numpy(), o_n.cpu().numpy()
    assert (off[nd + 1:] == -7).all() and (n[1:] == -7).all()
    return (o_id.cpu().numpy().view(np.uint32), o_cnt.cpu().numpy().view(np.uint32), off[:nd + 1].astype(np.uint64),
            int(n[0]))


def check_terms(got, want, cap, label):
    gid, gcnt, goff, gn = got
    wid, wcnt, woff = want
    assert gn == len(wid) == int(woff[-1]), (label, gn, len(wid))
    assert np.array_equal(goff, woff), (label, "term_off", np.flatnonzero(goff != woff)[:5])
    k = min(cap, len(wid))
    for name, g, w in (("term_id", gid, wid), ("term_cnt", gcnt, wcnt)):
        if not np.array_equal(g[:k], w[:k]):
            bad = np.flatnonzero(g[:k] != w[:k])
            raise AssertionError(f"{label}: {len(bad)} of {k} {name} differ; first #{bad[0]}: got "
                                 f"{g[bad[:6]].tolist()} want {w[bad[:6]].tolist()}")
        assert (g[k:] == GUARD).all(), (label, name, "written at or past the capacity")


def dev_keywords(tk, csr, weights, topk, cap=None, exact=False):
    """jb_keywords_device on a CSR of the test's own -> (kw_id, kw_score, kw_cnt, kw_n).  exact: the term
    arrays are allocations of exactly cap entries."""
    import torch
    tid, tcnt, off = csr
    nd = len(off) - 1
    cap = len(tid) if cap is None else cap
    pad = 0 if exact else 16
    d_id = _dev(np.concatenate([tid[:cap], np.full(pad, 12345, np.uint32)]) if cap + pad else np.zeros(1, np.uint32),
                np.uint32, np.int32)
    d_cnt = _dev(np.concatenate([tcnt[:cap], np.full(pad, 99, np.uint32)]) if cap + pad else np.zeros(1, np.uint32),
                 np.uint32, np.int32)
    d_off = _dev(off, np.uint64, np.int64)
    w = np.asarray(weights, np.float32)
    d_w = _dev(w if len(w) else np.zeros(1, np.float32), np.float32)
    o_id = torch.full((nd * topk + 8,), GUARD, dtype=torch.int32, device="cuda")
    o_sc = torch.full((nd * topk + 8,), -3.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((nd * topk + 8,), GUARD, dtype=torch.int32, device="cuda")
    o_n = torch.full((nd + 8,), GUARD, dtype=torch.int32, device="cuda")
    tk.keywords_device(d_id.data_ptr(), d_cnt.data_ptr(), d_off.data_ptr(), nd, cap, d_w.data_ptr(), len(w), topk,
                       o_id.data_ptr(), o_sc.data_ptr(), o_cnt.data_ptr(), o_n.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    a, s, c, n = (x.cpu().numpy() for x in (o_id, o_sc, o_cnt, o_n))
    m = nd * topk
    assert (a[m:] == GUARD).all() and (s[m:] == -3.0).all() and (c[m:] == GUARD).all() and (n[nd:] == GUARD).all()
    return (a[:m].view(np.uint32).reshape(nd, topk), s[:m].reshape(nd, topk), c[:m].view(np.uint32).reshape(nd, topk),
            n[:nd].view(np.uint32))


def check_keywords(got, want, label):
    """Every slot of every row, bit for bit (the scores as their u32 patterns), the padding included."""
    for name, g, w in zip(("kw_id", "kw_score", "kw_cnt", "kw_n"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert g.shape == w.shape, (label, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{label}: {len(bad)} {name} entries differ; first at {bad[0].tolist()}: got "
                                 f"{g[tuple(bad[0])]} want {w[tuple(bad[0])]}")


@pytest.fixture(scope="module")
def mini(mini_paths):
    tk = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    yield tk
    tk.close()


def device_chain(tk, buf, off, hmm, weights, topk, mode="cut", stream=None):
    """cut -> ids -> terms -> keywords, all queued on one stream without a host sync in between (into
    arrays of the test's own) -> ((term_id, term_cnt, term_off), (kw_id, kw_score, kw_cnt, kw_n))."""
    import torch
    nb, nd = int(off[-1]), len(off) - 1
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    d_text = torch.from_numpy(np.frombuffer(bytes(buf[:nb]) + b"\0" * 64, np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    cap = max(nb, 1)
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device="cuda")  # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")  # noqa: E731
    o_s, o_e, o_i, t_id, t_cnt = i32(cap), i32(cap), i32(cap), i32(cap, GUARD), i32(cap, GUARD)
    o_d, o_n, t_off, t_n = i64(nd + 1), i64(1), i64(nd + 1), i64(1)
    k_id, k_cnt, k_n = i32(nd * topk, GUARD), i32(nd * topk, GUARD), i32(nd, GUARD)
    k_sc = torch.full((nd * topk,), -3.0, dtype=torch.float32, device="cuda")
    w = np.asarray(weights, np.float32)
    d_w = torch.from_numpy(w).cuda()
    need = J.terms_work_bytes(cap, nd)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    a = (d_text.data_ptr(), nb, d_off.data_ptr(), nd)
    if mode == "cut":
        tk.cut_device_into(*a, hmm, o_s.data_ptr(), o_e.data_ptr(), cap, o_d.data_ptr(), o_n.data_ptr(), st)
    elif mode == "search":
        tk.cut_device_search_into(*a, hmm, o_s.data_ptr(), o_e.data_ptr(), cap, o_d.data_ptr(), o_n.data_ptr(), st)
    else:
        tk.cut_device_full_into(*a, o_s.data_ptr(), o_e.data_ptr(), cap, o_d.data_ptr(), o_n.data_ptr(), st)
    tk.ids_device(d_text.data_ptr(), nb, o_s.data_ptr(), o_e.data_ptr(), o_n.data_ptr(), cap, o_i.data_ptr(), st)
    tk.terms_device(o_i.data_ptr(), cap, o_d.data_ptr(), o_n.data_ptr(), nd, t_id.data_ptr(), t_cnt.data_ptr(), cap,
                    t_off.data_ptr(), t_n.data_ptr(), work.data_ptr(), need, st)
    tk.keywords_device(t_id.data_ptr(), t_cnt.data_ptr(), t_off.data_ptr(), nd, cap, d_w.data_ptr(), len(w), topk,
                       k_id.data_ptr(), k_sc.data_ptr(), k_cnt.data_ptr(), k_n.data_ptr(), st)
    torch.cuda.synchronize()
    n = int(t_n.cpu()[0])
    off_h = t_off.cpu().numpy().astype(np.uint64)
    assert n == int(off_h[-1]) <= cap
    csr = (t_id.cpu().numpy().view(np.uint32)[:n], t_cnt.cpu().numpy().view(np.uint32)[:n], off_h)
    kw = (k_id.cpu().numpy().view(np.uint32).reshape(nd, topk), k_sc.cpu().numpy().reshape(nd, topk),
          k_cnt.cpu().numpy().view(np.uint32).reshape(nd, topk), k_n.cpu().numpy().view(np.uint32))
    return csr, kw


# ---- 1. hand-checked -------------------------------------------------------------------------------
MIXED = "english번역『하다』今天天氣很好，ステーションabc1231+1=2我昨天去上海*important*去"
INVALID = b"\xff\xfe" + "中文".encode() + b"\x80abc\xe4\xb8"
HAND_VOCAB = ["abc", "中", "def", "今天", "天", "，", "ー", "abc1231", "1", "我", "上海", "important", "*", "�",
              "一刹那", "刹那", "天天", "english", "번", b"\xff", "去", "这"]
# mini_dict.txt, hmm off; the tokens and their ids are those of test_gpu_ids.py:
#   abc|中|文|def                                  0 1 U 2
#   english|번|역|『|하|다|』|今天|天|氣|很|好|，|ス|テ|ー|シ|ョ|ン|abc1231|+|1|=|2|我|昨天|去|上海|*|important|*|去
#                                                17 18 U U U U U 3 4 U U U 5 U U 6 U U U 7 U 8 U U 9 U 20 10 12 11 12 20
#   中|文|�|abc|�|�                               1 U 13 0 13 13
#   这|一刹那                                      21 14
HAND_TEXTS = ["abc 中文 def", MIXED, INVALID, "这一刹那"]
HAND_TERMS = [
    [(0, 1), (1, 1), (2, 1)],
    [(3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1), (9, 1), (10, 1), (11, 1), (12, 2), (17, 1), (18, 1), (20, 2)],
    [(0, 1), (1, 1), (13, 3)],
    [(14, 1), (21, 1)],
]
#               abc  中  def  今天 天 ，  ー abc1231 1  我  上海 important *    �   一刹那 刹那 天天 english 번 \xff 去   这
HAND_WEIGHTS = [1.0, 0, 1.5, 2.0, 0, 0, 0, 3.0,    0, 0, 2.5, 1.0,      0.75, 0.5, 4.0,  1.0, 1.0, 1.0,   0, 1.0, 0.5, -1.0]
# topK = 5.  Text 2: "*" x 2 = 1.5, then important, english and 去 x 2 tie at 1.0: the lowest id, 11, is kept
HAND_TAGS = [
    [(2, 1.5, 1), (0, 1.0, 1)],
    [(7, 3.0, 1), (10, 2.5, 1), (3, 2.0, 1), (12, 1.5, 2), (11, 1.0, 1)],
    [(13, 1.5, 3), (0, 1.0, 1)],
    [(14, 4.0, 1)],
]


def test_hand_checked(mini):
    tk = mini
    tk.set_vocab(HAND_VOCAB)
    try:
        buf, off = R.batch_of(HAND_TEXTS)
        csr, kw = device_chain(tk, buf, off, False, HAND_WEIGHTS, 5)
        tid, tcnt, toff = csr
        assert toff.tolist() == np.cumsum([0] + [len(t) for t in HAND_TERMS]).tolist()
        assert tid.tolist() == [i for t in HAND_TERMS for i, _ in t]
        assert tcnt.tolist() == [c for t in HAND_TERMS for _, c in t]
        kid, ksc, kcn, kn = kw
        assert kn.tolist() == [len(t) for t in HAND_TAGS]
        for d, tags in enumerate(HAND_TAGS):
            pad = 5 - len(tags)
            assert kid[d].tolist() == [i for i, _, _ in tags] + [UNK] * pad
            assert ksc[d].tolist() == [s for _, s, _ in tags] + [0.0] * pad
            assert kcn[d].tolist() == [c for _, _, c in tags] + [0] * pad
        assert tk.extract_tags(HAND_TEXTS, HAND_WEIGHTS, topK=5, hmm=False) == HAND_TAGS
        keyed = tk.extract_tags(HAND_TEXTS[:1], HAND_WEIGHTS, topK=1, hmm=False, keys=HAND_VOCAB)
        assert keyed == [[("def", 1.5, 1)]]
        assert tk.extract_tags([], HAND_WEIGHTS) == []
        assert tk.extract_tags(["", "abc"], HAND_WEIGHTS, topK=2) == [[], [(0, 1.0, 1)]]
        tk.set_vocab(None)
        with pytest.raises(J.JbError) as ei:  # the host call needs a vocabulary
            tk.extract_tags(HAND_TEXTS, HAND_WEIGHTS)
        assert ei.value.code == J.JB_EINVAL
    finally:
        tk.set_vocab(None)


# ---- 2. documents against tiles ------------------------------------------------------------------
def tile_batch():
    rng = np.random.default_rng(41)
    parts = []

    def rnd(n):
        x = rng.integers(0, 300, n).astype(np.uint32)
        x[rng.random(n) < 0.1] = UNK
        return x

    lens = [0, 0,               # empty documents at the start
            T - 1, 1,           # the second one ends at a tile edge
            T,                  # starts and ends at a tile edge
            0, 0, 0,            # empty documents at a tile edge
            T + 1, 2 * T, 2 * T + 1, 3 * T - 1,
            9 * T + 5,          # at least 9 tiles
            0, 0,               # between two long documents
            5 * T]              # one id: its count is summed over the tiles
    for n in lens:
        parts.append(rnd(n))
    parts[-1][:] = 77
    parts.append(np.arange(3 * T + 7, 0, -1, dtype=np.uint32) + 1000)   # all distinct, descending
    parts.append(np.full(50, UNK, np.uint32))                           # all unknown
    parts.append(np.array([0xFFFFFFFE, 0, 5, 0xFFFFFFFE, 0, 0], np.uint32))
    parts += [np.zeros(0, np.uint32)] * 3                               # empty documents at the end
    doc_tok = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
    assert int(doc_tok[4]) == T and int(doc_tok[5]) == 2 * T            # the tile edges claimed above
    return np.concatenate(parts), doc_tok


def test_documents_against_tiles(mini):
    ids, doc_tok = tile_batch()
    want = TR.terms(ids, doc_tok, len(ids), len(ids))
    assert want[1][int(want[2][15])] == 5 * T and int(want[2][16]) - int(want[2][15]) == 1  # (the one-id document)
    check_terms(dev_terms(mini, ids, doc_tok), want, len(ids), "tiles")
    # the same list shifted by one token: no document meets a tile edge where it did
    ids2 = np.concatenate([np.array([9], np.uint32), ids])
    tok2 = np.concatenate([[0], doc_tok + np.uint64(1)]).astype(np.uint64)
    check_terms(dev_terms(mini, ids2, tok2), TR.terms(ids2, tok2, len(ids2), len(ids2)), len(ids2), "tiles + 1")


def test_many_tiny_documents(mini):
    rng = np.random.default_rng(43)
    lens = rng.integers(0, 21, 10_000)
    doc_tok = np.cumsum(np.concatenate([[0], lens])).astype(np.uint64)
    ids = rng.integers(0, 50, int(doc_tok[-1])).astype(np.uint32)
    ids[rng.random(len(ids)) < 0.05] = UNK
    check_terms(dev_terms(mini, ids, doc_tok), TR.terms(ids, doc_tok, len(ids), len(ids)), len(ids), "tiny documents")


def test_count_width(mini):
    """One document of 2^24 + 3 tokens of one id: the count is exact as u32, and the score is the f32
    product of the rounded count."""
    big = 2**24 + 3
    ids = np.full(big + 10, 7, np.uint32)
    ids[:4] = [3, 7, 3, 9]
    ids[-6:] = [7, 7, 1, 1, 1, 2]
    doc_tok = np.array([0, 4, 4 + big, big + 10], np.uint64)
    want = (np.array([3, 7, 9, 7, 1, 2, 7], np.uint32), np.array([2, 1, 1, big, 3, 1, 2], np.uint32),
            np.array([0, 3, 4, 7], np.uint64))
    got = dev_terms(mini, ids, doc_tok, cap=64)
    check_terms(got, want, 64, "2^24 + 3")
    w = np.zeros(10, np.float32)
    w[7], w[1] = 0.3, 1.0
    kw = dev_keywords(mini, want, w, 2)
    check_keywords(kw, TR.keywords(want, w, 2), "2^24 + 3 keywords")
    assert kw[1][1, 0].view(np.uint32) == (np.float32(big) * np.float32(0.3)).view(np.uint32) and kw[2][1, 0] == big


# ---- 3. bounds and capacity ------------------------------------------------------------------------
def test_bounds_of_the_token_list(mini):
    rng = np.random.default_rng(47)
    n = 3 * T + 100
    ids = rng.integers(0, 40, n).astype(np.uint32)
    doc_tok = np.array([0, 10, T + 5, T + 5, 2 * T + 50, 3 * T, n], np.uint64)
    for ntok, ids_cap in ((n + 5000, 2 * T + 60), (n, 2 * T + 50), (2 * T + 7, n), (T + 5, n), (0, n), (n, 0)):
        want = TR.terms(ids, doc_tok, ntok, ids_cap)
        got = dev_terms(mini, ids, doc_tok, ntok=ntok, ids_cap=ids_cap, cap=n)
        check_terms(got, want, n, f"ntok={ntok} ids_cap={ids_cap}")


def test_capacity(mini):
    ids, doc_tok = tile_batch()
    want = TR.terms(ids, doc_tok, len(ids), len(ids))
    nterms = len(want[0])
    runs = [dev_terms(mini, ids, doc_tok, cap=cap, extra=T + 64) for cap in (0, 1, nterms - 1, nterms)]
    for cap, got in zip((0, 1, nterms - 1, nterms), runs):
        check_terms(got, want, cap, f"cap={cap}")  # (nothing at or past cap changes)
        assert np.array_equal(got[2], runs[0][2]) and got[3] == runs[0][3] == nterms


def test_work_buffer_one_byte_short(mini):
    ids = np.arange(100, dtype=np.uint32)
    doc_tok = np.array([0, 100], np.uint64)
    with pytest.raises(J.JbError) as ei:
        dev_terms(mini, ids, doc_tok, nwork=J.terms_work_bytes(100, 1) - 1)
    assert ei.value.code == J.JB_EINVAL and "jb_terms_work_bytes" in str(ei.value)


# ---- 4. keywords on hand-built CSRs ---------------------------------------------------------------
def built_csr(topk, seed=53, nw=120_000):
    """Documents with 0, 1, topk - 1, topk, topk + 1, 63, 64, 65 and 100,003 terms; weights mostly from
    {0.5, 1, 2}, so most scores tie, with 0, -1, NaN and +Inf among them and ids past the table."""
    rng = np.random.default_rng(seed)
    w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), nw)
    special = rng.choice(nw, 4000, replace=False)
    w[special[:1000]], w[special[1000:2000]], w[special[2000:3000]] = 0.0, -1.0, np.nan
    w[special[3000:3010]] = np.inf
    sizes = [0, 1, max(topk - 1, 0), topk, topk + 1, 63, 64, 65, 100_003, 5]
    tid, tcnt = [], []
    for k, n in enumerate(sizes):
        i = np.sort(rng.choice(nw + 2000, n, replace=False)).astype(np.uint32)  # (some ids >= nweights)
        if k == len(sizes) - 1:
            i = np.array([3, 7, nw + 5, 0xFFFFFFF0, 0xFFFFFFFE], np.uint32)
        tid.append(i)
        tcnt.append(rng.integers(1, 4, n).astype(np.uint32))
    off = np.cumsum([0] + sizes).astype(np.uint64)
    return (np.concatenate(tid), np.concatenate(tcnt), off), w


@pytest.mark.parametrize("topk", [1, 20, J.JB_KW_MAXK])
def test_keywords_on_built_csrs(mini, topk):
    csr, w = built_csr(topk)
    want = TR.keywords(csr, w, topk)
    assert want[3].tolist()[:8] != [0] * 8 and int(want[3][8]) == topk
    with np.errstate(invalid="ignore"):
        assert np.isinf(want[1][8]).any() or topk < 3  # (+Inf scores lead the big document)
    check_keywords(dev_keywords(mini, csr, w, topk), want, f"topk={topk}")
    # no weights: every row is padding
    check_keywords(dev_keywords(mini, csr, np.zeros(0, np.float32), topk), TR.keywords(csr, np.zeros(0), topk), "no weights")


def test_keywords_on_an_overflowed_csr(mini):
    """term_off describes more terms than the arrays hold: the documents whose range passes cap get
    kw_n = 0, and nothing is read past cap (the arrays are allocations of exactly cap entries)."""
    csr, w = built_csr(20)
    tid, tcnt, off = csr
    for cap in (int(off[8]) + 1000, int(off[8]), int(off[5]) + 1, 0):
        inside = off[1:] <= cap
        want = list(TR.keywords(csr, w, 20))
        want[0][~inside], want[1][~inside], want[2][~inside], want[3][~inside] = UNK, 0.0, 0, 0
        assert (~inside).any()
        check_keywords(dev_keywords(mini, csr, w, 20, cap=cap, exact=True), want, f"overflow cap={cap}")


def test_topk_limits(mini):
    csr, w = built_csr(20)
    for topk, code in ((0, J.JB_EINVAL), (J.JB_KW_MAXK + 1, J.JB_ELIMIT)):
        with pytest.raises(J.JbError) as ei:
            dev_keywords(mini, csr, w, topk)
        assert ei.value.code == code


# ---- 5. end to end ------------------------------------------------------------------------------------
TOPK = 20


def half_vocab(o, buf, off):
    """A fixed-seed half of the distinct tokens of the oracle's hmm = 1 cut, and weights from {0, 0.5, 1, 2}."""
    data = bytes(buf)
    s, e, _ = o.cut_batch(buf, off, True, nthreads=8)
    toks = sorted({V.span_key(data, a, b) for a, b in zip(s.astype(np.int64).tolist(), e.astype(np.int64).tolist())})
    rng = np.random.default_rng(59)
    keys = [toks[i] for i in np.flatnonzero(rng.random(len(toks)) < 0.5)]
    w = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], np.float32), len(keys))
    return keys, w


def ref_keywords(vocab, w, buf, spans, topk):
    s, e, d = spans
    ids = V.expect_ids(vocab, bytes(buf), np.asarray(s, np.int64).tolist(), np.asarray(e, np.int64).tolist())
    assert 0.2 < float((ids == UNK).mean()) < 0.9  # (unknown tokens occur)
    csr = TR.terms(ids, d, len(ids), len(ids))
    return csr, TR.keywords(csr, w, topk)


@pytest.mark.parametrize("kind,size", KINDS)
@pytest.mark.parametrize("hmm", [False, True])
def test_end_to_end(syn_small, kind, size, hmm):
    dp, ep, s = syn_small
    buf, off = s.corpus(synth.KIND_DOCS, 1200, target_bytes=1 << 20)[:2]
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep, kind=kind, size_override=size))
    o = O.Oracle.from_files(dp, ep, kind, size)
    try:
        keys, w = half_vocab(o, buf, off)
        vocab = V.key_dict(keys)
        tk.set_vocab(keys)
        refs = {"cut": o.cut_batch(buf, off, hmm, nthreads=8), "search": R.expected(o, buf, off, hmm),
                "full": F.expected(o, buf, off)}
        for mode in ("cut", "search", "full"):
            wcsr, wkw = ref_keywords(vocab, w, buf, refs[mode], TOPK)
            if mode == "cut":  # the reference itself: a document with more than topk candidates, a tie at the cut
                ncand = [int((w[wcsr[0][int(a):int(b)]] > 0).sum()) for a, b in zip(wcsr[2][:-1], wcsr[2][1:])]
                assert max(ncand) > TOPK
                full_rows = TR.keywords(wcsr, w, TOPK + 1)
                assert ((full_rows[3] > TOPK) & (full_rows[1][:, TOPK - 1] == full_rows[1][:, TOPK])).any()
            csr, kw = device_chain(tk, buf, off, hmm, w, TOPK, mode)
            n = len(wcsr[0])
            check_terms((csr[0], csr[1], csr[2], len(csr[0])), wcsr, n, f"terms kind={kind} hmm={hmm} {mode}")
            check_keywords(kw, wkw, f"keywords kind={kind} hmm={hmm} {mode}")
        wkw = ref_keywords(vocab, w, buf, refs["cut"], TOPK)[1]
        check_keywords(tk.keywords_batch(buf, off, hmm, w, TOPK), wkw, f"jb_keywords_batch kind={kind} hmm={hmm}")
    finally:
        tk.close()


# ---- 6. threads -----------------------------------------------------------------------------------------
def test_threads(syn_small):
    """4 threads, each with its own stream, arrays and work buffer, run the device chain on one ctx at
    once, 3 rounds each; every result is the reference's."""
    import torch
    dp, ep, s = syn_small
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
    o = O.Oracle.from_files(dp, ep, 0)
    batches = [s.corpus(synth.KIND_DOCS, 90 + k, target_bytes=(96 + 32 * k) << 10)[:2] for k in range(4)]
    keys, w = half_vocab(o, *batches[0])
    vocab = V.key_dict(keys)
    tk.set_vocab(keys)
    want = [ref_keywords(vocab, w, b[0], o.cut_batch(*b, True, nthreads=8), TOPK) for b in batches]
    errs = []

    def run(k):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for rep in range(3):
                    csr, kw = device_chain(tk, *batches[k], True, w, TOPK, "cut", st.cuda_stream)
                    check_terms((csr[0], csr[1], csr[2], len(csr[0])), want[k][0], len(csr[0]), f"thread {k}")
                    check_keywords(kw, want[k][1], f"thread {k} round {rep}")
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


# ---- 7. C and C++ programs --------------------------------------------------------------------------------
def test_c_and_cpp_consumers(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "c_abi_keywords")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_keywords.c"), "-L", lib,
                           "-ljiebahip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "keywords ok" in r.stdout, r.stdout + r.stderr
    exe = str(tmp_path / "cpp_keywords_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_keywords_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "keywords ok" in r.stdout, r.stdout + r.stderr
