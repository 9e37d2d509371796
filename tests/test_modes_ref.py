"""CPU: tests/modes_ref.py (replicated and joined expected outputs, the piece rule) against the
references computed directly on the repeated text.  No kernel is launched here."""
import numpy as np

import full_ref as F
import modes_ref as M
import oracle as O
import search_ref as R
import synth
import vocab_ref as V

BASE = [
    "今天天氣很好，abc 中文 def", "", "english번역『하다』ステーション1+1=2", b"\xff\xfe" + "中文".encode() + b"\x80abc\xe4\xb8",
    "𠀀𠀁𠀂中𪜀文", "", "x " * 7, "中文".encode() + b"\xed\xa0\x80\xc0\xaf\xf4\x90\x80\x80" + "文".encode() + b"\xe0\x80\xaf", "丁" * 40,
]


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.uint64 and np.array_equal(g, w)


def test_replicate_and_join_equal_the_direct_references(syn_small):
    dp, ep, s = syn_small
    o = O.Oracle.from_files(dp, ep, 0)
    cb, co, _ = s.corpus(synth.KIND_DOCS, 1000, target_bytes=24 << 10)
    docs = [bytes(cb[int(a):int(b)]) for a, b in zip(co[:-1], co[1:])]
    base = BASE[:4] + docs[:10] + BASE[4:] + docs[10:]
    assert "" in base and any(isinstance(t, bytes) for t in base)
    buf, off = R.batch_of(base)
    nb = int(off[-1])
    buf3, off3 = R.batch_of(base * 3)
    part = M.Part(o, buf=buf, off=off)
    for hmm in (False, True):
        want = R.expected(o, buf, off, hmm)
        assert len(want[0]) > len(o.cut_batch(buf, off, hmm)[0]) > 1000  # (there are grams)
        _same(M.replicate(want, nb, 3), R.expected(o, buf3, off3, hmm))
        _same(M.replicate(part.want("search", hmm), nb, 3), R.expected(o, buf3, off3, hmm))
        _same(M.replicate(part.want("cut", hmm), nb, 3), o.cut_batch(buf3, off3, hmm))
        _same(M.replicate(want, nb, 1), want)
    wf = F.expected(o, buf, off)
    _same(M.replicate(wf, nb, 3), F.expected(o, buf3, off3))
    _same(part.want("full"), wf)
    # parts of different texts laid end to end, and an exact token count
    fill = M.filler_part(o, 5)
    b = M.Batch([(fill, 2), (part, 2), (fill, 1)])
    texts = ["x " * 5] * 2 + base * 2 + ["x " * 5]
    bufj, offj = R.batch_of(texts)
    assert np.array_equal(b.off, offj) and np.array_equal(b.buf[:b.nbytes], bufj[:int(offj[-1])])
    for hmm in (False, True):
        _same(b.want("search", hmm), R.expected(o, bufj, offj, hmm))
        _same(b.want("cut", hmm), o.cut_batch(bufj, offj, hmm))
        assert b.ntok(hmm) == len(o.cut_batch(bufj, offj, hmm)[0])
    _same(b.want("full"), F.expected(o, bufj, offj))
    cpart = M.Part(o, buf=cb, off=co)
    assert cpart.ndocs >= 2
    for target in (cpart.ntok() - 5, 3 * cpart.ntok() + 4096 + 17):
        e = M.exact_batch(o, cpart, target, False, 0.6, fill_doc=4096)
        plain = o.cut_batch(e.buf, e.off, False)
        assert len(plain[0]) == target and e.han_tokens() * 3 >= target
        _same(e.want("cut"), plain)
        _same(e.want("full"), F.expected(o, e.buf, e.off))
        _same(e.want("search"), R.expected(o, e.buf, e.off, False))
    # ids: a token's id depends on its bytes alone
    s1, e1, _ = wf
    s3, e3, _ = M.replicate(wf, nb, 3)
    data, data3 = bytes(buf), bytes(buf3)
    keys = sorted({V.span_key(data, a, b) for a, b in zip(s1.astype(np.int64).tolist(), e1.astype(np.int64).tolist())})[::2]
    vocab = V.key_dict(keys)
    ids = V.expect_ids(vocab, data, s1.astype(np.int64).tolist(), e1.astype(np.int64).tolist(), nb)
    assert 0 < (ids == V.UNK).sum() < len(ids)
    assert np.array_equal(M.replicate_ids(ids, 3), V.expect_ids(vocab, data3, s3.astype(np.int64).tolist(),
                                                               e3.astype(np.int64).tolist(), 3 * nb))
    o.close()


def test_pieces_rule():
    off = np.array([0, 10, 20, 35, 35, 100, 104, 110], np.uint64)
    assert M.pieces(off, 20) == [(0, 2), (2, 4), (4, 5), (5, 7)]  # (a longer document is a piece of its own)
    assert M.pieces(off, 1000) == [(0, 7)]
    assert M.pieces(off[3:], 4) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert M.pieces(off[:1], 4) == []
