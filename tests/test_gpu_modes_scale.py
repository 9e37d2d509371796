"""GPU: search mode, full mode and token ids at the geometries the plain path is tested at.

test_gpu_search.py, test_gpu_full.py and test_gpu_ids.py check what the passes compute; here the same
passes run where their indexing changes: past 256 token tiles (the second level of the tile scan) and at
exact tile counts, with more than 2^24 full-mode spans (the 64-bit sums), through the host pipeline in
pieces (output sets reused, a piece run twice, a batch that starts inside its buffer, pinned input, one
document split over pieces), past one trip of k_ids' grid, behind every form of the plain pipeline, and
at the edges of the passes' own constants (kSrchFastN, tile4 at text-tile edges, full_back's fast form).
Every expected value comes from the oracle (O.Oracle, search_ref, full_ref, vocab_ref), the large ones
through modes_ref's replication of documents, which test_modes_ref.py checks on the CPU; every coverage
condition (token counts, spans in tiles of index 256 and up, piece counts, ...) is asserted from the
reference or the device properties, never from the library.

Not tested: more than 2^32 full-mode spans in one list (the smallest input is tens of MB of runes with
many edges each) and more than 65,536 token tiles (256 x 256: hundreds of MB), where the third level of
the scan would be needed.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import full_ref as F
import jiebahip as J
import modes_ref as M
import oracle as O
import search_ref as R
import synth
import test_gpu_full as TF
import test_gpu_search as TS
import vocab_ref as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(J.JB_DICT_TXT, 0), (J.JB_DICT_PREFIX, J.JIEBA_SIZE)]
MODES = [("search", False), ("search", True), ("full", False)]
TILE = 4096  # kSrchTile: plain tokens per token tile; also kTileBytes, the bytes of a text tile
X4 = "\U00020000"  # a 4-byte Han rune


def _cmp(got, want, label):
    gs, ge, gd = got
    ws, we, wd = want
    if not (np.array_equal(gs, ws) and np.array_equal(ge, we)):
        n = min(len(gs), len(ws))
        ne = (np.asarray(gs[:n], np.uint64) != np.asarray(ws[:n], np.uint64)) | (
            np.asarray(ge[:n], np.uint64) != np.asarray(we[:n], np.uint64))
        bad = int(np.argmax(ne)) if ne.any() else n
        raise AssertionError(f"{label}: {len(gs)} vs {len(ws)} spans; first diff #{bad}: "
                             f"gpu={list(zip(gs[bad:bad + 6].tolist(), ge[bad:bad + 6].tolist()))} "
                             f"want={list(zip(ws[bad:bad + 6].tolist(), we[bad:bad + 6].tolist()))}")
    assert np.array_equal(gd, wd), label


def _open_env(env, oracle=True, ndevices=1, **kw):
    """A tokenizer opened under `env` (the switches are read at jb_open), and its oracle.
    kw: dict_path / dict_bytes, emit_path, kind, size_override."""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        tk = J.Tokenizer(J.make_config(ndevices=ndevices, **kw))
    if not oracle:
        return tk, None
    kind, size = kw.get("kind", J.JB_DICT_TXT), kw.get("size_override", 0)
    if "dict_path" in kw:
        return tk, O.Oracle.from_files(kw["dict_path"], kw["emit_path"], kind, size)
    with open(kw["emit_path"], "rb") as f:
        return tk, O.Oracle(kw["dict_bytes"], f.read(), kind, size)


def _host(tk, mode, hmm, buf, off):
    return tk.cut_batch_full(buf, off) if mode == "full" else tk.cut_batch_search(buf, off, hmm)


def _single(tk, mode, hmm, text):
    return tk.cut_full_spans(text) if mode == "full" else tk.cut_search_spans(text, hmm)


class DevBatch:
    """A batch in torch-owned device memory (64 zero bytes after the text)."""

    def __init__(self, buf, off):
        import torch
        self.nb, self.nd = int(off[-1]), len(off) - 1
        text = np.zeros(self.nb + 64, np.uint8)
        text[:self.nb] = np.asarray(buf, np.uint8)[:self.nb]
        self.text = torch.from_numpy(text).cuda()
        self.off = torch.from_numpy(np.asarray(off, np.uint64).astype(np.int64)).cuda()
        self.args = (self.text.data_ptr(), self.nb, self.off.data_ptr(), self.nd)
        self.stream = torch.cuda.current_stream().cuda_stream


def _device(tk, mode, hmm, db):
    """cut_device_search / cut_device_full: the ctx-owned arrays -> ((starts, ends, doc_tok), count)."""
    import torch
    if mode == "full":
        ps, pe, pd, pn = tk.cut_device_full(*db.args, db.stream)
    elif mode == "search":
        ps, pe, pd, pn = tk.cut_device_search(*db.args, hmm, db.stream)
    else:
        ps, pe, pd, pn = tk.cut_device(*db.args, hmm, db.stream)
    torch.cuda.synchronize()
    tk.device_status(db.stream)
    n = int(J.dev_to_host(pn, 8, np.uint64)[0])
    assert n <= db.nb
    return (J.dev_to_host(ps, 4 * n, np.uint32), J.dev_to_host(pe, 4 * n, np.uint32),
            J.dev_to_host(pd, 8 * (db.nd + 1), np.uint64)), n


GUARD = 64


def _device_into(tk, mode, hmm, db, cap, status=True):
    """The _into forms on arrays of cap entries followed by guard words: ((starts, ends, doc_tok), count).
    Nothing may be written past min(count, cap), nor behind doc_tok and the count."""
    import torch
    o_s = torch.full((cap + GUARD,), -7, dtype=torch.int32, device="cuda")
    o_e = torch.full((cap + GUARD,), -7, dtype=torch.int32, device="cuda")
    o_d = torch.full((db.nd + 1 + GUARD,), -7, dtype=torch.int64, device="cuda")
    o_n = torch.full((1 + GUARD,), -7, dtype=torch.int64, device="cuda")
    outs = (o_s.data_ptr(), o_e.data_ptr(), cap, o_d.data_ptr(), o_n.data_ptr(), db.stream)
    if mode == "full":
        tk.cut_device_full_into(*db.args, *outs)
    else:
        tk.cut_device_search_into(*db.args, hmm, *outs)
    torch.cuda.synchronize()
    if status:
        tk.device_status(db.stream)
    n = int(o_n[0].item())
    m = min(n, cap)
    assert bool((o_s[m:] == -7).all()) and bool((o_e[m:] == -7).all()), "spans written past the count or the capacity"
    assert bool((o_d[db.nd + 1:] == -7).all()) and bool((o_n[1:] == -7).all())
    return (o_s[:m].cpu().numpy().view(np.uint32), o_e[:m].cpu().numpy().view(np.uint32),
            o_d[:db.nd + 1].cpu().numpy().view(np.uint64)), n


@pytest.fixture(scope="module")
def small(syn_small):
    dp, ep, s = syn_small
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
    o = O.Oracle.from_files(dp, ep, 0)
    yield tk, o, s
    tk.close()


@pytest.fixture(scope="module")
def caches(small):
    """The references' caches (dictionary lookups, spans per block text), shared by the module."""
    return R.Grams(small[1]), F.Blocks(small[1])


@pytest.fixture(scope="module")
def corpus(small, caches):
    """The 256 KiB corpus of test_gpu_search.py / test_gpu_full.py with its references."""
    buf, off = small[2].corpus(synth.KIND_DOCS, 1000, target_bytes=256 << 10)[:2]
    return M.Part(small[1], buf=buf, off=off, grams=caches[0], blocks=caches[1])


# ---- A. past 256 token tiles, and the tile-count edges ------------------------------------------
T256 = 256 * TILE  # 1,048,576 plain tokens: 256 token tiles
BIG = 2 * T256 + 300 * TILE + 77
# plain tokens -> the corpus's share of them (the rest are "x " units; at least a third are Han tokens)
COUNTS = {TILE: 0.6, TILE + 1: 0.6, T256: 0.4, T256 + 1: 0.9, BIG: 0.4}


def _spans_from_token(b, plain, want, t, mode):
    """Of the tokens at and after the first document that starts at plain token t or later: the grams
    (search), the spans of more than one rune (full).  A lower bound of those in token tiles >= t / TILE."""
    pd, md = plain[2].astype(np.int64), want[2].astype(np.int64)
    j = int(np.searchsorted(pd, t, side="left"))
    if mode == "search":
        return (len(want[0]) - int(md[j])) - (len(plain[0]) - int(pd[j]))
    s, e = want[0][int(md[j]):].astype(np.int64), want[1][int(md[j]):].astype(np.int64)
    return int(((e - s >= 6) & (b.buf[s] >= 0xE0)).sum())


@pytest.mark.parametrize("mode,hmm", MODES)
@pytest.mark.parametrize("count", list(COUNTS))
def test_token_tile_counts(small, corpus, count, mode, hmm):
    """Batches of an exact plain-token count: one tile and one more token; 256 tiles (tile 255 is the last
    and writes the total, tile 256 returns); 256 tiles and one token (k_sup's first sum, pf_load's sn = 1,
    r = 0); and past 2 x 256 + 300 tiles (sn = 2, r > 0).  The batch of 256 tiles is under 4 MiB (k_tok1),
    the larger ones over it (k_tok + k_doc_tok).  Device API, ctx-owned arrays and the _into forms."""
    tk, o, s = small
    b = M.exact_batch(o, corpus, count, hmm, COUNTS[count])
    plain, want = b.want("cut", hmm), b.want(mode, hmm)
    assert len(plain[0]) == count == b.ntok(hmm) and 3 * b.han_tokens(hmm) >= count
    assert len(want[0]) <= b.nbytes
    if count == T256:
        assert 1 << 20 < b.nbytes < 4 << 20  # (the second level's launch, and k_tok1)
    if count > T256:
        assert b.nbytes > 4 << 20
    if count == BIG:  # real spans behind both sums of k_sup: a wrong second-level prefix moves them
        for tile in (256, 512):
            assert _spans_from_token(b, plain, want, tile * TILE, mode) >= 1000
    db = DevBatch(b.buf, b.off)
    got, n = _device(tk, mode, hmm, db)
    assert n == len(want[0])
    _cmp(got, want, f"{mode} hmm={hmm} {count} tokens")
    assert tk.last_stats()["tokens"] == count
    got, n = _device_into(tk, mode, hmm, db, db.nb)
    assert n == len(want[0])
    _cmp(got, want, f"{mode} hmm={hmm} {count} tokens, into")
    assert tk.last_stats()["tokens"] == count


# ---- B. more than 2^24 full-mode spans ------------------------------------------------------------
def _spans_before_token(b, t):
    """The full-mode spans of the whole documents that end at or before plain token t: a lower bound of the
    spans before token t."""
    pd, md = b.want("cut")[2].astype(np.int64), b.want("full")[2].astype(np.int64)
    return int(md[int(np.searchsorted(pd, t, side="right")) - 1])


@pytest.mark.parametrize("layout", ["filler first", "chains first"])
def test_full_mode_past_2_24_spans(mini_paths, layout):
    """The 64-bit sums: F.chain_dict(12) on documents of 甲 x 200 (17 plain tokens and 2,134 spans each).
    Filler first: 257 token tiles of "x ", then 8,300 chain documents, so that more than 2^24 spans lie
    before the last token tile (7.1 MB of text, 18.8 M spans).  Chains first: 7,700 chain documents and
    filler in the first 256 token tiles, which then hold more than 2^24 spans, and 600 chain documents in
    the tiles behind them: only then does one thread of k_full_write carry a value of 2^24 or more
    (sup[0]), so that wg_sum64's middle limb is not zero.  (A single tile's count stays below 2^24 with any
    dictionary in reach, so k_sup64's own middle limb stays zero.)
    Then a capacity of 64: the first 64 spans, nothing past them, the complete count and doc_tok,
    JB_ELIMIT, and a clean plain cut afterwards."""
    import torch
    tk, o = _open_env({}, dict_bytes=F.chain_dict(12).encode(), emit_path=mini_paths[1])
    try:
        chain = M.Part(o, texts=["甲" * 200])
        per = len(chain.want("full")[0])
        assert chain.nbytes == 600 and chain.ntok() == 17 and per == 2134
        fill = M.filler_part(o, TILE)
        if layout == "filler first":
            b = M.Batch([(fill, 257), (chain, 8300)])
        else:
            b = M.Batch([(chain, 7700), (fill, 225), (chain, 600)])
        want, plain = b.want("full"), b.want("cut")
        nplain = len(plain[0])
        assert nplain == b.ntok() > T256 + 2 * TILE
        last0 = (nplain - 1) // TILE * TILE  # the last token tile's first token
        assert _spans_before_token(b, last0) > 1 << 24
        if layout == "chains first":
            assert _spans_before_token(b, T256) >= 1 << 24  # sup[0]
            assert len(want[0]) - _spans_before_token(b, T256 + TILE) >= 100 * per  # real spans behind it
        db = DevBatch(b.buf, b.off)
        n = len(want[0])
        got, cnt = _device_into(tk, "full", False, db, n)
        assert cnt == n
        _cmp(got, want, "more than 2^24 spans")
        assert tk.last_stats()["tokens"] == nplain
        got, cnt = _device_into(tk, "full", False, db, 64, status=False)
        with pytest.raises(J.JbError) as ei:
            tk.device_status(db.stream)
        assert ei.value.code == J.JB_ELIMIT
        assert cnt == n and np.array_equal(got[2], want[2])
        assert np.array_equal(got[0], want[0][:64]) and np.array_equal(got[1], want[1][:64])
        got, cnt = _device(tk, "cut", False, db)
        assert cnt == nplain
        _cmp(got, plain, "plain after the overflow")
        del got, db
        torch.cuda.empty_cache()
    finally:
        tk.close()


# ---- C. the host pipeline in pieces -----------------------------------------------------------------
PIECE = 256 << 10


@pytest.fixture(scope="module")
def pieces_tk(syn_small):
    dp, ep, s = syn_small
    tk, _ = _open_env({"JB_PIECE_KIB": "256"}, oracle=False, dict_path=dp, emit_path=ep)
    yield tk
    tk.close()


@pytest.fixture(scope="module")
def corpus2m(small, caches):
    buf, off = small[2].corpus(synth.KIND_DOCS, 2000, target_bytes=2 << 20)[:2]
    return M.Part(small[1], buf=buf, off=off, grams=caches[0], blocks=caches[1])


@pytest.mark.parametrize("mode,hmm", MODES)
def test_pipeline_in_pieces(pieces_tk, corpus2m, mode, hmm):
    """2 MiB in pieces of 256 KiB: the three output sets are reused and the stager waits for collections.
    Twice (graph replay), from a batch that starts inside its buffer, and from pinned memory."""
    tk, p = pieces_tk, corpus2m
    buf, off = p._padded(), p.off
    assert len(M.pieces(off, PIECE)) >= 7
    want, plain = p.want(mode, hmm), p.want("cut", hmm)
    for rep in range(2):
        _cmp(_host(tk, mode, hmm, buf, off), want, f"{mode} hmm={hmm} in pieces, call {rep}")
        assert tk.last_stats()["tokens"] == len(plain[0])  # summed over the pieces
    # documents 5 .. of the same buffer: the spans are offsets into the buffer, doc_tok starts at 0
    k, kp = int(want[2][5]), int(plain[2][5])
    assert int(off[5]) > 0 and len(M.pieces(off[5:], PIECE)) >= 7
    sub = (want[0][k:], want[1][k:], want[2][5:] - np.uint64(k))
    _cmp(_host(tk, mode, hmm, buf, off[5:]), sub, f"{mode} hmm={hmm} in pieces, from document 5")
    assert tk.last_stats()["tokens"] == len(plain[0]) - kp
    hb = J.HostBuffer(len(buf))
    try:
        hb.array[:] = buf
        _cmp(_host(tk, mode, hmm, hb.array, off), want, f"{mode} hmm={hmm} in pieces, pinned input")
        _cmp(_host(tk, mode, hmm, hb.array, off[5:]), sub, f"{mode} hmm={hmm} in pieces, pinned, from document 5")
    finally:
        hb.free()


def _short_doc(nbytes):
    """An ordinary document of exactly nbytes bytes for the chain dictionary: fewer spans than bytes."""
    unit = "abc 甲甲甲 de1, "
    k = nbytes // len(unit.encode())
    return unit * k + "y" * (nbytes - k * len(unit.encode()))


def _piece_docs(nlong):
    """Documents of exactly one piece (262,144 bytes): nlong documents of 甲 x 4000 among short ones."""
    docs = ["甲" * 4000, _short_doc(TILE)] + ["甲" * 4000] * (nlong - 1) if nlong else []
    left = PIECE - sum(len(d.encode()) for d in docs)
    while left > TILE:
        docs.append(_short_doc(TILE))
        left -= TILE
    docs.append(_short_doc(left))
    assert sum(len(d.encode()) for d in docs) == PIECE
    return docs


def test_full_mode_second_run_inside_a_pipeline(mini_paths):
    """A piece whose full-mode list outgrows its output set is run again from the collecting thread: as
    the first piece, as a middle one on the output set that the first one's second run enlarged (pieces 0
    and 3), and as the last one, with ordinary pieces between them."""
    tk, o = _open_env({"JB_PIECE_KIB": "256"}, dict_bytes=F.chain_dict(12).encode(), emit_path=mini_paths[1])
    try:
        bl = F.Blocks(o)
        kinds = {n: M.Part(o, texts=_piece_docs(n), blocks=bl) for n in (0, 12, 21)}
        order = [12, 0, 0, 21, 0, 12]
        b = M.Batch([(kinds[n], 1) for n in order])
        pcs = M.pieces(b.off, PIECE)
        want = b.want("full")
        wd = want[2].astype(np.int64)
        assert len(pcs) == len(order) and [int(b.off[d1] - b.off[d0]) for d0, d1 in pcs] == [PIECE] * len(order)
        cap = [PIECE + 4] * 3  # the output sets: the largest piece's bytes + 4, then what a second run needed + 4
        twice = []
        for k, (d0, d1) in enumerate(pcs):
            n = int(wd[d1] - wd[d0])
            assert (n > PIECE + 4) == (order[k] > 0)
            if n > cap[k % 3]:
                twice.append(k)
                cap[k % 3] = n + 4
        assert twice == [0, 3, 5]
        for rep in range(2):  # (the second call finds the sets large enough)
            _cmp(_host(tk, "full", False, b.buf, b.off), want, f"second runs inside a pipeline, call {rep}")
            assert tk.last_stats()["tokens"] == b.ntok()
    finally:
        tk.close()


@pytest.fixture(scope="module")
def long_doc(small, caches):
    """One punctuated document of 300,000 runes (about 900 KB), alone and between two short documents."""
    tk, o, s = small
    buf, off, _ = s.corpus(synth.KIND_LONG_PUNCT, 77, target_runes=300_000)
    doc = bytes(buf[:int(off[-1])])
    assert len(off) == 2 and len(doc) > 3 * PIECE
    return (M.Part(o, texts=[doc], grams=caches[0], blocks=caches[1]),
            M.Part(o, texts=["短文本，中文 abc", doc, "中文"], grams=caches[0], blocks=caches[1]))


@pytest.mark.parametrize("mode,hmm", MODES)
def test_one_document_over_pieces(pieces_tk, long_doc, mode, hmm):
    """A document longer than a piece is cut into units at Han-run starts (jb_split_points' rule); the
    reference is computed on the whole document."""
    for p in long_doc:
        _cmp(_host(pieces_tk, mode, hmm, p._padded(), p.off), p.want(mode, hmm), f"{mode} hmm={hmm} {p.ndocs} documents")
        assert pieces_tk.last_stats()["tokens"] == p.ntok(hmm)


def test_one_document_over_two_devices_full(syn_small, long_doc):
    dp, ep, _ = syn_small
    tk, _ = _open_env({"JB_DEVICE_WRAP": "1", "JB_PIECE_KIB": "256"}, oracle=False, ndevices=2, dict_path=dp,
                      emit_path=ep)
    try:
        for p in long_doc:
            _cmp(_host(tk, "full", False, p._padded(), p.off), p.want("full"), f"two devices, {p.ndocs} documents")
    finally:
        tk.close()


# ---- D. k_ids past one grid trip --------------------------------------------------------------------
@pytest.fixture(scope="module")
def ids_base(mini_paths):
    """The identity keys as vocabulary and text; base spans (the keys' own, end - 1, start + 1) with
    their expected ids, computed once: every test list indexes into them."""
    import torch
    tk = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    keys = V.identity_keys()
    d = V.key_dict(keys)
    text = b"".join(keys)
    e = np.cumsum([len(k) for k in keys]).astype(np.int64)
    s = e - np.array([len(k) for k in keys], np.int64)
    bs, be = np.concatenate([s, s, s + 1]), np.concatenate([e, e - 1, e])
    ids = V.expect_ids(d, text, bs.tolist(), be.tolist())
    tk.set_vocab(keys)
    d_text = torch.from_numpy(np.frombuffer(text + b"\0" * 64, np.uint8).copy()).cuda()
    yield tk, text, d_text, bs, be, ids, len(keys)
    tk.close()


def _ids_list(base, n, seed):
    """n spans: two thirds the keys' own, a third near misses, shuffled -> (starts, ends, expected ids)."""
    tk, text, d_text, bs, be, ids, nk = base
    rng = np.random.default_rng(seed)
    idx = np.where(rng.random(n) < 2 / 3, rng.integers(0, nk, n), rng.integers(nk, 3 * nk, n))
    return bs[idx], be[idx], ids[idx]


def _run_ids(base, s, e, ntok, cap, extra=512):
    import torch
    tk, text, d_text = base[:3]
    d_s = torch.from_numpy(np.ascontiguousarray(s, np.uint32).view(np.int32)).cuda()
    d_e = torch.from_numpy(np.ascontiguousarray(e, np.uint32).view(np.int32)).cuda()
    d_n = torch.tensor([ntok], dtype=torch.int64, device="cuda")
    d_ids = torch.full((max(cap, len(s)) + extra,), -7, dtype=torch.int32, device="cuda")
    tk.ids_device(d_text.data_ptr(), len(text), d_s.data_ptr(), d_e.data_ptr(), d_n.data_ptr(), cap, d_ids.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_ids.cpu().numpy()


def _same_ids(got, want, label):
    got, want = np.asarray(got).view(np.uint32), np.asarray(want, np.uint32)
    assert len(got) == len(want), (label, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (f"{label}: {len(bad)} of {len(want)} ids differ; first #{bad[0]}: got {got[bad[:6]].tolist()} "
                           f"want {want[bad[:6]].tolist()}")


TRIPS = {"trip": lambda t: t, "trip + 1": lambda t: t + 1, "2 * trip - 1": lambda t: 2 * t - 1,
         "2 * trip + 255": lambda t: 2 * t + 255, "3 * trip + 77": lambda t: 3 * t + 77}


@pytest.mark.parametrize("expr", list(TRIPS))
def test_ids_past_one_grid_trip(ids_base, expr):
    """k_ids' grid is ncu * 8 workgroups of 256 spans: lists that end with the first trip, one span into the
    second, at its end, and in the third and fourth, with the span loads one trip ahead.  Then a capacity
    and a count inside the second trip: exactly that many ids, nothing behind them."""
    import torch
    trip = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    n = TRIPS[expr](trip)
    assert n >= trip and (not expr.startswith("3") or n > 3 * trip) and (expr != "2 * trip + 255" or n > 2 * trip)
    s, e, want = _ids_list(ids_base, n, len(expr))
    assert 0.3 <= float((want == V.UNK).mean()) <= 0.4  # a third unknown
    got = _run_ids(ids_base, s, e, n, n)
    _same_ids(got[:n], want, f"n = {expr}")
    assert (got[n:] == -7).all()
    inside = trip + min(1000, n - trip - 1) if n > trip + 1 else n - 1  # inside the second trip where there is one
    assert inside < n and (n <= trip + 1 or inside > trip)
    got = _run_ids(ids_base, s, e, n, inside)
    _same_ids(got[:inside], want[:inside], f"n = {expr}, cap = {inside}")
    assert (got[inside:] == -7).all()
    got = _run_ids(ids_base, s, e, inside, n)
    _same_ids(got[:inside], want[:inside], f"n = {expr}, count = {inside}")
    assert (got[inside:] == -7).all()
    if expr == "3 * trip + 77":
        tk, text = ids_base[:2]
        _same_ids(tk.spans_ids(text, s, e), want, "jb_spans_ids on the largest list")


# ---- E. the passes behind every pipeline form -----------------------------------------------------------
FORMS = [{"JB_ZH_WIDE": "1"}, {"JB_NZ_FUSE_MIB": "0"}, {"JB_ZH_GROUP": "1024"}, {"JB_ZH_GROUP": "6144"},
         {"JB_MW_SPLIT": "0"}, {"JB_MW_SPLIT": "1"}, {"JB_MW_SPLIT": "2"}, {"JB_TOK1": "0"}, {"JB_SMALL": "0"}]


def _junk_then_4byte():
    """test_long_block_4byte_rune_after_junk's batches: long blocks that fill every record slot, then
    blocks with a 4-byte rune in the same slots."""
    rng = random.Random(11)
    pool = [chr(c) for c in range(0x4E00, 0x4E00 + 2000)]
    han = "".join(rng.choice(pool) for _ in range(12000))
    return [han[:6000], han[6000:]], [han[:1500] + X4 + han[1502:6000], X4 + han[6002:12000]]


def _edge_texts():
    seen, out = set(), []
    for t in TS.EDGE_TEXTS + TF.EDGE_TEXTS + ["中文" * 1500 + X4 + "中文" * 1500]:  # (a long block on k_long_dp's general path)
        b = t.encode("utf-8") if isinstance(t, str) else t
        if b not in seen:
            seen.add(b)
            out.append(b)
    return out


@pytest.fixture(scope="module")
def form_parts(small, caches, corpus):
    o = small[1]
    junk, with4 = _junk_then_4byte()
    kw = dict(grams=caches[0], blocks=caches[1])
    return [("corpus", corpus), ("edge texts", M.Part(o, texts=_edge_texts(), **kw)),
            ("junk", M.Part(o, texts=junk, **kw)), ("4-byte runes after junk", M.Part(o, texts=with4, **kw))]


@pytest.mark.parametrize("env", FORMS, ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_passes_behind_pipeline_forms(syn_small, form_parts, env):
    """The passes read erec, lanemask, tile_cnt, tile4, tok_start and doc_tok, which every form of the plain
    pipeline writes in its own way."""
    dp, ep, _ = syn_small
    tk, _ = _open_env(env, oracle=False, dict_path=dp, emit_path=ep)
    try:
        for label, p in form_parts:  # (junk, then the 4-byte runes in the workspace it filled)
            for mode, hmm in (("search", True), ("full", False)):
                _cmp(_host(tk, mode, hmm, p._padded(), p.off), p.want(mode, hmm), f"{env} {mode} {label}")
                assert tk.last_stats()["tokens"] == p.ntok(hmm)
        edge = form_parts[1][1]
        for mode, hmm in (("search", True), ("full", False)):  # each edge text alone
            ws, we, wd = (x.astype(np.int64) for x in edge.want(mode, hmm))
            for j in range(edge.ndocs):
                a, b = int(edge.off[j]), int(edge.off[j + 1])
                gs, ge = _single(tk, mode, hmm, edge.buf[a:b].tobytes())
                assert np.array_equal(gs, ws[wd[j]:wd[j + 1]] - a) and np.array_equal(ge, we[wd[j]:wd[j + 1]] - a), (
                    env, mode, j)
    finally:
        tk.close()


@pytest.fixture(scope="module")
def long_blocks(syn_small):
    dict_text, texts = M.long_blocks_recipe()
    with open(syn_small[1], "rb") as f:
        o = O.Oracle(dict_text.encode(), f.read(), J.JB_DICT_TXT, 0)
    p = M.Part(o, texts=texts)
    # (what makes the recipe worth running here: tokens past kSrchFastN runes, and runes with up to 19 words)
    plain = p.want("cut", True)
    assert int(((plain[1] - plain[0]) > 3 * 32).sum()) >= 100
    assert len(p.want("full")[0]) > 3 * p.ntok() and len(p.want("search", True)[0]) > p.ntok(True) + 100
    return dict_text.encode(), p


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("spec", ["0", "2", "3"])
def test_passes_behind_long_block_forms(syn_small, long_blocks, spec, fused):
    """test_long_blocks_many's batch: the records of long blocks come from k_long_*, by the exact chain (0),
    with planted wrong choices (2), by the decided chain (3); as one launch and as separate ones."""
    dict_bytes, p = long_blocks
    tk, _ = _open_env({"JB_LONG_SPEC": spec, "JB_LONG_FUSED": fused}, oracle=False, dict_bytes=dict_bytes,
                      emit_path=syn_small[1])
    try:
        for mode, hmm in MODES:
            _cmp(_host(tk, mode, hmm, p._padded(), p.off), p.want(mode, hmm), f"spec={spec} fused={fused} {mode} hmm={hmm}")
            assert tk.last_stats()["long_blocks"] >= 6 and tk.last_stats()["tokens"] == p.ntok(hmm)
    finally:
        tk.close()


_NO_GRAPH = """
import sys
sys.path[:0] = [{tests!r}, {oracle!r}, {gen!r}, {py!r}]
import numpy as np
import jiebahip as J, oracle as O, full_ref as F, synth
dp, ep = sys.argv[1:3]
s = synth.Synth(nwords=20_000)
buf, off, _ = s.corpus(synth.KIND_DOCS, 1000, target_bytes=256 << 10)
tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
o = O.Oracle.from_files(dp, ep, 0)
ws, we, wd = F.expected(o, buf, off)
for rep in range(2):
    gs, ge, gd = tk.cut_batch_full(buf, off)
    assert np.array_equal(gs, ws) and np.array_equal(ge, we) and np.array_equal(gd, wd), rep
    gs, ge, gd = tk.cut_batch(buf, off, True)
tk.close()
print("ok", len(ws))
"""


def test_full_mode_without_graphs(syn_small):
    """The corpus in full mode with JB_GRAPH=0 (read once per process, so in a child process)."""
    dp, ep, _ = syn_small
    code = _NO_GRAPH.format(tests=os.path.join(ROOT, "tests"), oracle=os.path.join(ROOT, "oracle"),
                            gen=os.path.join(ROOT, "gen"), py=os.path.join(ROOT, "jieba-go_amd", "python"))
    env = dict(os.environ, JB_GRAPH="0")
    r = subprocess.run([sys.executable, "-c", code, dp, ep], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


# ---- F. edges of the passes' own constants ------------------------------------------------------------------
def _dict_of(words, singles_freq=1, word_freq=10 ** 7, sub_freq=2, rare=()):
    """A dictionary in which Cut keeps each of `words` whole: every prefix is a key (frequency 0: the trie
    walk goes on through it), every rune a word (the gate on the first rune), every 2- and 3-rune
    substring a word, the words themselves by far the likeliest.  rare: words of frequency 1 that Cut
    does not take and full mode emits."""
    d = {}
    for w in list(words) + list(rare):
        for k in range(1, len(w)):
            d.setdefault(w[:k], 0)
    for w in rare:
        d[w] = 1
    for w in words:
        for ch in w:
            d[ch] = singles_freq
    for w in words:
        for L in (2, 3):
            for i in range(len(w) - L + 1):
                d[w[i:i + L]] = sub_freq
    for w in words:
        d[w] = word_freq
    return "".join(f"{k} {v}\n" for k, v in d.items())


FASTN = [3, 4, 5, 31, 32, 33, 34, 64, 255]  # runes: around kSrchFastN = 32, and the longest word


def _fastn_words():
    """The words of FASTN runes, every rune in one word only; then words of 12 runes (their first rune's record
    overflows: its grams come from the trie walk) with a 4-byte rune first, second and third."""
    runes = iter(chr(c) for c in range(0x4E00, 0x4E00 + sum(FASTN) + 3 * 11))
    words = ["".join(next(runes) for _ in range(n)) for n in FASTN]
    for k in range(3):
        w = "".join(next(runes) for _ in range(11))
        words.append(w[:k] + chr(0x20000 + k) + w[k:])
    return words


@pytest.mark.parametrize("kind,size", KINDS)
def test_tokens_around_the_fast_forms_length(mini_paths, kind, size):
    """Tokens of 3 .. 255 runes whose every 2- and 3-rune substring is a word: srch_masks takes those of up
    to kSrchFastN = 32 runes, srch_grams the longer ones; the first and last grams are at the masks' ends.
    Each word alone, behind 0 .. 15 bytes of ASCII (every alignment of its records), and in a batch."""
    words = _fastn_words()
    dict_text = _dict_of(words)
    tk, o = _open_env({}, dict_bytes=dict_text.encode(), emit_path=mini_paths[1], kind=kind, size_override=size)
    try:
        g, bl = R.Grams(o), F.Blocks(o)
        for w in words:
            for hmm in (False, True):
                assert o.cut(w, hmm) == [w], (len(w), hmm)
            n = len(w)
            assert len(g.of_token(w.encode())) == (n - 1) + (n - 2 if n > 3 else 0)  # every substring is a gram
        texts = ["a" * k + w for w in words for k in range(16)]
        p = M.Part(o, texts=texts + ["，".join(words), "".join(words)], grams=g, blocks=bl)
        for mode, hmm in MODES:
            ws, we, wd = (x.astype(np.int64) for x in p.want(mode, hmm))
            for j, t in enumerate(texts):
                gs, ge = _single(tk, mode, hmm, t)
                a = int(p.off[j])
                assert np.array_equal(gs, ws[wd[j]:wd[j + 1]] - a) and np.array_equal(ge, we[wd[j]:wd[j + 1]] - a), (
                    mode, hmm, len(t), j % 16)
            _cmp(_host(tk, mode, hmm, p._padded(), p.off), p.want(mode, hmm), f"kind={kind} {mode} hmm={hmm} batch")
    finally:
        tk.close()


# tile4 (does a 4,096-byte text tile hold a 4-byte Han rune?) is read for two tiles per decision: those of
# s and e - 1 (srch_masks), of s and min(e + 23, nbytes - 1) (full_token), of p - 24 and p - 1 (full_back).
EDGE_WORDS = ["甲乙", "丙丁戊己", "子丑寅卯辰巳午未", "丙" + X4 + "戊己", "子丑寅" + X4 + "辰巳午未"]  # 2, 4, 8 runes
# three 4-byte runes: such a token's length is a multiple of three again, which srch_masks takes for a stride
X3 = "\U00020001\U00020002\U00020003"
EDGE_WORDS3 = ["庚" + X3, "辛癸" + X3 + "申"]
DOC = 2 * TILE  # every sweep document is two text tiles long: its token sits around the edge between them


def _at(end, head, tail=""):
    """A document of DOC bytes: ASCII, then `head` ending at byte `end` of the document, then `tail`."""
    hb, tb = head.encode(), tail.encode()
    pre = end - len(hb)
    assert pre > 0 and end + len(tb) < DOC
    return b"a" * pre + hb + tb + b" " + b"b" * (DOC - end - len(tb) - 1)


def _junk(o, word, ndocs, blocks=None):
    """ndocs documents of DOC bytes, each one Han run of `word` repeated: run before a sweep, it leaves a
    record in every slot, also in those that are no rune's in the sweep's documents (erec is not cleared)."""
    k = DOC // len(word.encode())
    doc = word * k + "a" * (DOC - k * len(word.encode()))
    return M.Batch([(M.Part(o, texts=[doc], blocks=blocks), ndocs)])


def test_tile4_at_text_tile_edges(mini_paths):
    """A token that ends at each of the bytes -27 .. +3 around a text-tile edge, with a 4-byte Han rune just
    before it, inside it, and 1 .. 8 runes behind it in the same Han block; tokens with three 4-byte runes
    whose first rune alone lies before the edge.  Each run follows a batch that left a record in every slot."""
    # (rare words from a token's last rune across the runes behind it to the 4-byte rune: in full mode their
    # spans start inside the token, and their ends depend on the 4-byte rune's width)
    across = [w[-1] + "壬" * (k - 1) + X4 for w in EDGE_WORDS[:3] for k in range(1, 8)]
    dict_text = _dict_of(EDGE_WORDS + EDGE_WORDS3 + ["壬", X4], rare=across)
    tk, o = _open_env({}, dict_bytes=dict_text.encode(), emit_path=mini_paths[1])
    try:
        for w in EDGE_WORDS + EDGE_WORDS3:
            assert o.cut(w, False) == [w] == o.cut(w, True)
            assert len(w.encode()) % 3 == (0 if w in EDGE_WORDS[:3] + EDGE_WORDS3 else 1)
        docs, ends = [], []
        for w in EDGE_WORDS[:3]:
            for d in range(-27, 4):
                docs.append(_at(TILE + d, w))
                docs.append(_at(TILE + d, X4 + w))
                docs += [_at(TILE + d, w, "壬" * (k - 1) + X4) for k in range(1, 9)]
                ends += [TILE + d] * 10
        for w in EDGE_WORDS[3:]:
            for d in range(-27, 4):
                docs.append(_at(TILE + d, w))
                ends.append(TILE + d)
        for w in EDGE_WORDS3:  # (up to the token's first rune alone before the edge, its 4-byte runes behind it)
            for d in range(-27, len(w.encode())):
                docs.append(_at(TILE + d, w))
                ends.append(TILE + d)
        bl = F.Blocks(o)
        p = M.Part(o, texts=docs, grams=R.Grams(o), blocks=bl)
        junk = _junk(o, EDGE_WORDS[2], len(docs), bl)
        assert all(len(t) == DOC for t in docs)
        for hmm in (False, True):  # (from the reference: a plain token ends at the byte the document was built for)
            pe, pd = p.want("cut", hmm)[1].astype(np.int64), p.want("cut", hmm)[2].astype(np.int64)
            for j, end in enumerate(ends):
                assert j * DOC + end in pe[pd[j]:pd[j + 1]], (j, end, hmm)
        assert len(p.want("search")[0]) > p.ntok() + 2 * len(docs) and len(p.want("full")[0]) > p.ntok() + 2 * len(docs)
        fs, fe, fd = (x.astype(np.int64) for x in p.want("full"))
        over = sum(bool(((fs[fd[j]:fd[j + 1]] < j * DOC + end) & (fe[fd[j]:fd[j + 1]] > j * DOC + end)).any())
                   for j, end in enumerate(ends))
        assert over >= 3 * 31 * 7  # documents with a full-mode span from inside the token to past its end
        for mode, hmm in MODES:
            _cmp(_host(tk, "full", False, junk.buf, junk.off), junk.want("full"), "a record in every slot")
            _cmp(_host(tk, mode, hmm, p._padded(), p.off), p.want(mode, hmm), f"tile edges {mode} hmm={hmm}")
    finally:
        tk.close()


def _look_back_dict(words):
    """Words that Cut does not take: their runes are frequent, the words rare, their prefixes keys of
    frequency 0 (test_look_back_past_eight_runes' recipe).  In full mode the word is emitted at its first
    rune, and each later rune, a plain token of its own, looks back for it."""
    d = {}
    for w in words:
        for k in range(2, len(w)):
            d.setdefault(w[:k], 0)
    for w in words:
        for ch in w:
            d[ch] = 10 ** 16
    for w in words:
        d[w] = 1
    return "".join(f"{k} {v}\n" for k, v in d.items())


G12, G8 = "子丑寅卯辰巳午未申酉戌亥", "甲乙丙丁戊己庚辛"  # a zero record (12 runes), a record (8)
BACK_WORDS = [G12, G8] + [G12[:k] + X4 + G12[k + 1:] for k in (0, 3, 6, 10)] + [G8[:k] + X4 + G8[k + 1:] for k in (1, 6)]


def test_full_back_at_text_tile_edges_and_byte_32(mini_paths):
    """full_back: a rune without words whose covering word starts 1 .. 11 runes back, at every byte around a
    text-tile edge (its fast form reads tile4 of p - 24 and p - 1) and, at the head of a batch, around
    p = 32, where the fast form begins; with a 4-byte rune among the runes it steps over."""
    tk, o = _open_env({}, dict_bytes=_look_back_dict(BACK_WORDS).encode(), emit_path=mini_paths[1])
    try:
        bl, g = F.Blocks(o), R.Grams(o)
        for w in BACK_WORDS:
            assert o.cut(w + w[0], False) == list(w + w[0])
            assert F.expected_text(o, w + w[0], bl) == [w, w[0]]  # (every later rune is covered, the rune behind is not)
        docs = []
        for w in BACK_WORDS:  # the word's runes, and the uncovered rune behind it, at every byte around the edge
            n = len(w.encode())
            docs += [_at(TILE + d, w, w[0] + w[:5]) for d in range(-27, n + 4)]
        p = M.Part(o, texts=docs, grams=g, blocks=bl)
        junk = _junk(o, G8, len(docs), bl)
        jw = junk.want("full")
        assert int((jw[1] - jw[0] == 24).sum()) >= 300 * len(docs)  # (its records have words)
        # (from the reference: single-rune tokens of full mode's plain cut start at every byte near the edge)
        ps, pe = (x.astype(np.int64) for x in p.want("cut")[:2])
        one = ps[(pe - ps <= 4) & (p.buf[ps] >= 0xE0)] % DOC - TILE
        assert set(one[(one >= -27) & (one <= 3)].tolist()) == set(range(-27, 4))
        for mode, hmm in MODES:
            _cmp(_host(tk, "full", False, junk.buf, junk.off), junk.want("full"), "a record in every slot")
            _cmp(_host(tk, mode, hmm, p._padded(), p.off), p.want(mode, hmm), f"full_back at tile edges {mode} hmm={hmm}")
        # the head of a batch: the word starts at bytes 0 .. 35, so that its runes' tokens start at 29 .. 35 too
        for w in BACK_WORDS:
            for k in range(36):
                t = "a" * k + w + w[0] + w[:5]
                for mode, hmm in (("search", False), ("full", False)):
                    want = F.expected_text(o, t, bl) if mode == "full" else R.expected_text(o, t, hmm)
                    gs, ge = _single(tk, mode, hmm, t)
                    assert J.spans_to_tokens(t, gs.tolist(), ge.tolist()) == want, (mode, k, w)
    finally:
        tk.close()
