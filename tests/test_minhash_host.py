"""CPU: jb_minhash, jb_minhash_params and jb_minhash_bands, the host form of the MinHash rule
(jieba-go_amd/csrc/jb_minhash.cpp), against minhash_ref.py, exactly; the size helper and the limits; the rule's
properties, and one statistical check of the estimate against the shingle sets' Jaccard similarity.  The cuts
come from the oracle and the mode references over tests/golden/mini_dict.txt.  No kernel is launched here."""
import math

import numpy as np
import pytest

import full_ref as F
import jiebahip as J
import minhash_ref as M
import oracle as O
import search_ref as R
import wc_ref as W

MIXED = "english번역『하다』今天天氣很好，ステーションabc1231+1=2我昨天去上海*important*去"  # (test_gpu_ids.MIXED)
INVALID = b"\xff\xfe" + "中文".encode() + b"\x80abc\xe4\xb8"
TEXTS = [MIXED, INVALID, "这一刹那", MIXED, "今天天氣很好", "", "这一刹那的上海"]
NEW = ["jb_minhash_work_bytes", "jb_minhash_params", "jb_minhash", "jb_minhash_bands", "jb_minhash_device",
       "jb_minhash_bands_device", "jb_minhash_batch"]


def test_exports():
    L = J.lib()
    for name in NEW:
        assert name in J.EXPORTS and hasattr(L, name), name
    assert (J.JB_MH_MAXN, J.JB_MH_MAXK, J.JB_MH_TILE, J.JB_MH_EMPTY, J.JB_MH_NOKEY) == (
        M.MAXN, M.MAXK, M.TILE, M.EMPTY, M.NOKEY)


def check(text, s, e, doc_tok, n, K, seed=1, **kw):
    ref = M.minhash_ref(text, s, e, doc_tok, n, K, seed, **kw)
    got = J.minhash(text, s, e, doc_tok, n, K, seed, **kw)
    assert got[0].dtype == np.uint32 and got[0].shape == ref[0].shape
    assert (got[1] == ref[1]).all(), (n, K, got[1], ref[1])
    assert (got[0] == ref[0]).all(), (n, K, np.argwhere(got[0] != ref[0])[:4])
    return got


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
    s, e, dt = _spans(o, buf, off, mode, hmm)
    text = bytes(buf[:int(off[-1])])
    assert len(s) > 60
    for n in range(1, 9):
        for K in (1, 7, 128, 256):
            sig, dn = check(text, s, e, dt, n, K)
            m = np.diff(np.asarray(dt, np.int64))
            assert dn.tolist() == [0 if x == 0 else 1 if x < n else x - n + 1 for x in m.tolist()]
            assert (sig[0] == sig[3]).all() and dn[5] == 0 and (sig[5] == M.EMPTY).all()  # MIXED twice, "" once
            assert (sig[dn > 0] != M.EMPTY).any()


def test_params():
    for seed in (0, 1, 2 ** 63, 2 ** 64 - 1, 0x1234567890ABCDEF):
        for K in (1, 2, 7, 256):
            a, b = J.minhash_params(seed, K)
            ra, rb = M.params(seed, K)
            assert a.tolist() == ra and b.tolist() == rb
            assert all(x & 1 for x in a.tolist())
    # the well-known first outputs of splitmix64 from state 0: a_0 is the first (made odd), b_0 the second
    a, b = J.minhash_params(0, 1)
    assert int(a[0]) == 0xE220A8397B1DCDAF | 1 and int(b[0]) == 0x6E789E6AA1B965F4


def test_key_lengths():
    """Keys of every length at which the hash takes another path; bytes past 255 do not count."""
    rng = np.random.default_rng(5)
    keys = [bytes(rng.integers(0x30, 0x3A, ln).astype(np.uint8)) for ln in (1, 8, 9, 16, 17, 24, 25, 255, 256, 300)]
    long_a = keys[-1]
    long_b = long_a[:255] + bytes(x ^ 1 for x in long_a[255:])  # differs only after byte 255 (index >= 255)
    long_c = long_a[:254] + bytes([long_a[254] ^ 1]) + long_a[255:]  # differs at byte 254
    toks = keys + [long_b, long_c]
    text, s, e = M.from_keys(toks, gap=b"-")
    s, e = np.append(s, [3]).astype(np.uint32), np.append(e, [3]).astype(np.uint32)  # and a key of length 0
    nt = len(s)
    dt = np.arange(nt + 1, dtype=np.uint64)  # one token per document, n = 1: a row is a function of t alone
    sig, dn = check(text, s, e, dt, 1, 64)
    assert (dn == 1).all()
    t = M.token_hashes(text, s.tolist(), e.tolist(), nt)
    assert t[-1] == M.fin(M.mix(M.init(0), 0))
    ia, ib, ic = len(keys) - 1, len(keys), len(keys) + 1
    assert t[ia] == t[ib] and (sig[ia] == sig[ib]).all()
    assert t[ia] != t[ic] and (sig[ia] != sig[ic]).any()
    assert len(set(t)) == nt - 1
    for k in toks[:8]:  # up to 255 bytes the hash is the vocabulary's (wc_ref restates it for 1 .. 255 bytes)
        assert M.key_hash(k) == W.vocab_hash(k)


def test_invalid_byte_is_replacement_character():
    text = b"\xffab\xef\xbf\xbd\x80"
    s, e = np.array([0, 3, 6, 1], np.uint32), np.array([1, 6, 7, 2], np.uint32)
    sig, dn = check(text, s, e, np.arange(5, dtype=np.uint64), 1, 32)
    assert (sig[0] == sig[1]).all() and (sig[0] == sig[2]).all() and (sig[0] != sig[3]).any()


def test_bad_spans_hash_as_the_empty_key():
    text = b"abcdef"
    s = np.array([2, 4, 5, 0xFFFFFFF0, 0, 6], np.uint32)
    e = np.array([2, 3, 9, 0xFFFFFFFF, 7, 6], np.uint32)
    sig, dn = check(text, s, e, np.arange(7, dtype=np.uint64), 1, 16)
    assert all((sig[i] == sig[0]).all() for i in range(6))
    t = M.token_hashes(text, s.tolist(), e.tolist(), 6)
    assert set(t) == {M.key_hash(b"")}
    # the same under a smaller nbytes: a span that was good is bad now
    s2, e2 = np.array([0, 0], np.uint32), np.array([3, 5], np.uint32)
    sig, _ = check(text, s2, e2, np.arange(3, dtype=np.uint64), 1, 16, nbytes=4)
    assert (sig[1] != sig[0]).any() and (sig[1] == J.minhash(b"", [0], [0], [0, 1], 1, 16, nbytes=0)[0][0]).all()


def test_malformed_span_lists():
    kinds = set()
    for seed in range(120):
        text, s, e, ntok, cap = W.random_case(seed)
        rng = np.random.default_rng(1000 + seed)
        nd = int(rng.integers(0, 9))
        dt = np.sort(rng.integers(0, len(s) + 4, nd + 1)).astype(np.uint64)
        n, K = int(rng.integers(1, 9)), int(rng.choice([1, 7, 64, 128, 256]))
        _, dn = check(text, s, e, dt, n, K, seed, ntok=ntok, cap=cap)
        kinds.add((ntok > cap, ntok < cap, bool((dn == 0).any()), bool((dn == 1).any()), bool((dn > 1).any())))
    assert all(any(k[i] for k in kinds) for i in range(5))


def test_document_shapes():
    """m = 0, m < n, m = n and m = n + 1; tokens before the first document and past the last."""
    toks = [b"w%d" % i for i in range(30)]
    text, s, e = M.from_keys(toks, gap=b" ")
    n = 4
    dt = np.array([3, 3, 5, 9, 14, 14, 20], np.uint64)  # m = 0, 2, 4, 5, 0, 6; tokens 0-2 and 20-29 are of no document
    sig, dn = check(text, s, e, dt, n, 64)
    assert dn.tolist() == [0, 1, 1, 2, 0, 3]
    assert (sig[0] == M.EMPTY).all() and (sig[4] == M.EMPTY).all()
    # the tokens of no document do not count: other bytes there, the same rows
    toks2 = [b"zz"] * 3 + toks[3:20] + [b"q"] * 10
    text2, s2, e2 = M.from_keys(toks2, gap=b" ")
    sig2, dn2 = check(text2, s2, e2, dt, n, 64)
    assert (sig2 == sig).all() and (dn2 == dn).all()
    # a short document's one shingle is over its own width: [w3 w4] is not the start of [w3 w4 w5 w6]
    a, _ = check(text, s, e, np.array([3, 5], np.uint64), n, 64)
    b, _ = check(text, s, e, np.array([3, 7], np.uint64), n, 64)
    assert (a != b).any()
    # ntok and cap on either side of the arrays
    for ntok, cap in ((30, 12), (12, 30), (0, 30), (30, 0), (99, 30), (17, 17)):
        dtc = np.array([0, 4, 11, 16, 30], np.uint64)
        _, dnc = check(text, s[:cap], e[:cap], dtc, n, 8, ntok=ntok, cap=cap)
        nt = min(ntok, cap)
        ms = [max(0, min(int(dtc[d + 1]), nt) - min(int(dtc[d]), nt)) for d in range(4)]
        assert dnc.tolist() == [0 if m == 0 else 1 if m < n else m - n + 1 for m in ms]


def test_rows_depend_on_their_own_document_only():
    rng = np.random.default_rng(11)
    vocab = [b"k%d" % i for i in range(50)]
    docs = [[vocab[i] for i in rng.integers(0, 50, int(m))] for m in (40, 0, 3, 40, 17, 1)]
    docs[3] = list(docs[0])

    def run(ds):
        toks = [t for d in ds for t in d]
        text, s, e = M.from_keys(toks, gap=b" ")
        dt = np.cumsum([0] + [len(d) for d in ds]).astype(np.uint64)
        return check(text, s, e, dt, 3, 128, seed=9)

    sig, dn = run(docs)
    assert (sig[0] == sig[3]).all() and dn[0] == dn[3] == 38  # equal documents at different places: equal rows
    other = [docs[0], [b"x"] * 5, docs[2], docs[3], [b"y", b"z"], docs[5]]
    sig2, _ = run(other)
    for d in (0, 2, 3, 5):
        assert (sig2[d] == sig[d]).all()
    assert (sig2[4] != sig[4]).any()
    assert (J.minhash(*M.from_keys(docs[0], gap=b" "), [0, 40], 3, 128, 10)[0] != sig[0]).any()  # another seed


def test_bands():
    rng = np.random.default_rng(12)
    sig = rng.integers(0, 2 ** 32, (6, 128), dtype=np.uint64).astype(np.uint32)
    sig[2] = 7  # equal values in every row of every band
    sig[4] = sig[1]
    dn = np.array([3, 1, 9, 0, 1, 2], np.uint32)
    for B, R in ((1, 1), (16, 8), (32, 4), (128, 1), (1, 128), (5, 7)):
        keys = J.minhash_bands(sig, dn, B, R)
        assert keys.dtype == np.uint64 and keys.shape == (6, B)
        assert (keys == M.bands_ref(sig, dn, B, R)).all(), (B, R)
        assert (keys[3] == M.NOKEY).all() and (keys[[0, 1, 2, 4, 5]] != M.NOKEY).all()
        assert (keys[4] == keys[1]).all()
        assert len(set(keys[2].tolist())) == B  # the band's number is part of its key
    # a band's key depends on its number and its rows alone (the slots past B * R are unused)
    assert (J.minhash_bands(sig, dn, 4, 8)[:, :4] == J.minhash_bands(sig, dn, 16, 8)[:, :4]).all()


def test_size_helper():
    prev = 0
    for ntok in (0, 1, 31, 32, 33, 1023, 1024, 1025, 10 ** 6, 2 ** 32 - 1025, 2 ** 40, 2 ** 63, 2 ** 64 - 1):
        w = J.minhash_work_bytes(ntok, 10)
        assert w > 0 and w >= prev and (ntok > 2 ** 59 or w >= 8 * ntok), ntok
        prev = w
    prev = 0
    for nd in (0, 1, 255, 256, 257, 10 ** 6, 2 ** 32 - 1):
        w = J.minhash_work_bytes(5000, nd)
        assert w > 0 and w >= prev, nd
        prev = w


def test_limits():
    L = J.lib()
    text = b"abc def"
    s, e = np.array([0, 4], np.uint32), np.array([3, 7], np.uint32)
    dt = np.array([0, 2], np.uint64)
    sig, dn = np.zeros(256, np.uint32), np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data

    def call(text=text, nbytes=7, s=p(s), e=p(e), dt=p(dt), ntok=2, cap=2, nd=1, n=2, K=4, sg=p(sig), d=p(dn)):
        return L.jb_minhash(text, nbytes, s, e, dt, ntok, cap, nd, n, K, 1, sg, d)

    assert call() == J.JB_OK and dn[0] == 1
    for kw in (dict(text=None), dict(s=None), dict(e=None), dict(dt=None), dict(sg=None), dict(d=None), dict(n=0),
               dict(K=0)):
        assert call(**kw) == J.JB_EINVAL, kw
    for kw in (dict(n=9), dict(K=257), dict(nbytes=2 ** 31), dict(cap=2 ** 32 - 1024)):
        assert call(**kw) == J.JB_ELIMIT, kw
    assert b"2^32" in L.jb_last_error()
    assert call(n=8, K=256) == J.JB_OK
    # null is fine where the capacity is 0
    assert call(text=None, nbytes=0) == J.JB_OK and dn[0] == 1  # (two bad spans: one shingle of two empty keys)
    assert call(s=None, e=None, cap=0) == J.JB_OK and dn[0] == 0
    assert call(sg=None, d=None, nd=0) == J.JB_OK
    a, b = np.zeros(256, np.uint64), np.zeros(256, np.uint64)
    assert L.jb_minhash_params(1, 256, p(a), p(b)) == J.JB_OK
    assert L.jb_minhash_params(1, 0, p(a), p(b)) == J.JB_EINVAL
    assert L.jb_minhash_params(1, 4, None, p(b)) == J.JB_EINVAL and L.jb_minhash_params(1, 4, p(a), None) == J.JB_EINVAL
    assert L.jb_minhash_params(1, 257, p(a), p(b)) == J.JB_ELIMIT
    keys = np.zeros(256, np.uint64)
    assert L.jb_minhash_bands(p(sig), p(dn), 1, 8, 2, 4, p(keys)) == J.JB_OK
    for K, B, R in ((8, 0, 4), (8, 2, 0), (0, 1, 1), (8, 3, 3), (8, 9, 1), (8, 1, 9), (256, 2 ** 31, 2)):
        assert L.jb_minhash_bands(p(sig), p(dn), 1, K, B, R, p(keys)) == J.JB_EINVAL, (K, B, R)
    assert L.jb_minhash_bands(p(sig), p(dn), 1, 257, 1, 1, p(keys)) == J.JB_ELIMIT
    assert L.jb_minhash_bands(None, p(dn), 1, 8, 2, 4, p(keys)) == J.JB_EINVAL
    assert L.jb_minhash_bands(p(sig), None, 1, 8, 2, 4, p(keys)) == J.JB_EINVAL
    assert L.jb_minhash_bands(p(sig), p(dn), 1, 8, 2, 4, None) == J.JB_EINVAL
    assert L.jb_minhash_bands(None, None, 0, 8, 2, 4, None) == J.JB_OK


def test_estimate_tracks_the_jaccard_similarity():
    """Three seeded pairs of about 2,000 tokens, K = 256: the share of equal slots lies within 4 standard
    deviations, sd = sqrt(J (1 - J) / K), of the Jaccard similarity J of the two shingle sets, which the test
    computes from the tokens itself.  (Slots are near-independent Bernoulli(J) draws; the inputs are fixed by
    seed, so the outcome is too.)"""
    K = 256
    for pair, (n, change) in enumerate(((1, 0.30), (3, 0.08), (5, 0.03))):
        rng = np.random.default_rng(700 + pair)
        vocab = [b"w%d" % i for i in range(3000)]
        da = [vocab[i] for i in rng.integers(0, 3000, 2000)]
        db = [vocab[int(rng.integers(0, 3000))] if rng.random() < change else t for t in da]
        text, s, e = M.from_keys(da + db, gap=b" ")
        sig, dn = J.minhash(text, s, e, [0, 2000, 4000], n, K, seed=pair + 1)
        sa = {tuple(da[i:i + n]) for i in range(2000 - n + 1)}
        sb = {tuple(db[i:i + n]) for i in range(2000 - n + 1)}
        jac = len(sa & sb) / len(sa | sb)
        est = float((sig[0] == sig[1]).mean())
        sd = math.sqrt(jac * (1 - jac) / K)
        print(f"n={n} J={jac:.4f} estimate={est:.4f} |diff|/sd={abs(est - jac) / sd:.2f}")
        assert 0.2 < jac < 0.9 and dn.tolist() == [2000 - n + 1] * 2
        assert abs(est - jac) <= 4 * sd, (n, jac, est, sd)
