"""GPU: every code point and every class of malformed sequence through each cut path, bit-exact.

The device asks "valid UTF-8? \\p{Han}? IsSpace?" in eight separately written places (k_mark_walk's fast
loop, dec_lead + han_cp, han_rune, the re-decode of Han starts, k_small's own phase, the three copies of
the non-Han cutter, full_w / srch_rune, and jb_row's pagemap route).  codepoint_cases' corpora reach all of
them: S (one document per scalar value), D (24 consecutive scalars per document), M (235,904 malformed
four-byte sequences), T (runes cut by a document end), L (a Han run that ends at a 4 KiB tile end, followed
by bytes the lookahead must not take for a rune) and E (a dictionary, an emission table and texts over the
rare Han ranges).  Every expected value comes from the oracle or the mode references (modes_ref,
search_ref, full_ref, vocab_ref); test_codepoint_cases.py pins the oracle itself to an independent model
on the same corpora.  The tokenizers are opened once per module.
"""
import numpy as np
import pytest

import codepoint_cases as CC
import full_ref as F
import modes_ref as M
import oracle as O
import search_ref as R
import vocab_ref as V
from test_gpu_parity import ZH_FORMS, _pair_env

pytestmark = pytest.mark.gpu

FORMS = list(ZH_FORMS)
HMM = [False, True]
MODES = [("search", False), ("search", True), ("full", False)]
RARE_KEYS = ["⺀", "⻳", "⼀", "々", "〇", "〡", "〻", "㐀", "䶿", "鿼", "豈", "𖿰", "𠀀", "𱍊"]
VOCAB_KEYS = ["�", "一", "丁一", "丁一丁"] + RARE_KEYS


class Set:
    """One dictionary's tokenizers (one per form of ZH_FORMS, and one with JB_SMALL=0) and its oracle, with
    the references of each corpus computed once."""

    def __init__(self, dp, ep):
        self.tk = {}
        for form, env in ZH_FORMS.items():
            self.tk[form], self.o = _pair_env(dp, ep, env)
        self.tk["pipeline"], _ = _pair_env(dp, ep, {"JB_SMALL": "0"})
        self.grams, self.blocks = R.Grams(self.o), F.Blocks(self.o)
        self.parts = {}

    def part(self, name, corpus):
        if name not in self.parts:
            buf, off = corpus
            self.parts[name] = M.Part(self.o, buf=buf, off=off, grams=self.grams, blocks=self.blocks)
        return self.parts[name]

    def close(self):
        for t in self.tk.values():
            t.close()


@pytest.fixture(scope="module")
def corp():
    L = CC.corpus_L()
    c = {"S0": CC.corpus_S(0), "S7": CC.corpus_S(7), "D": CC.corpus_D(), "M": CC.corpus_M(), "T": CC.corpus_T(),
         "L": L[:2]}
    c["DM1"] = CC.one_document(*CC.concat([c["D"], c["M"]]))
    c["Lcases"] = L[2]
    c["Scount"] = CC.scalar_token_counts(CC.all_scalars())
    return c


@pytest.fixture(scope="module")
def syn(syn_small):
    s = Set(syn_small[0], syn_small[1])
    yield s
    s.close()


@pytest.fixture(scope="module")
def lset(mini_paths, tmp_path_factory):
    dp = str(tmp_path_factory.mktemp("cp_L") / "dict.txt")
    with open(dp, "w", encoding="utf-8") as f:
        f.write(CC.dict_L())
    s = Set(dp, mini_paths[1])
    yield s
    s.close()


@pytest.fixture(scope="module")
def eset(tmp_path_factory):
    dp, ep, words = CC.files_E(str(tmp_path_factory.mktemp("cp_E")))
    s = Set(dp, ep)
    s.words = words
    s.corpus = CC.corpus_E(words)
    yield s
    s.close()


def _cmp(got, want, label, buf=None):
    gs, ge, gd = got
    ws, we, wd = want
    if not (np.array_equal(gs, ws) and np.array_equal(ge, we)):
        n = min(len(gs), len(ws))
        ne = (np.asarray(gs[:n], np.uint64) != np.asarray(ws[:n], np.uint64)) | (
            np.asarray(ge[:n], np.uint64) != np.asarray(we[:n], np.uint64))
        bad = int(np.argmax(ne)) if ne.any() else n
        lo = int(min(gs[bad] if len(gs) > bad else 0, ws[bad] if len(ws) > bad else 0))
        ctx = bytes(np.asarray(buf)[max(0, lo - 24):lo + 40]) if buf is not None else b""
        raise AssertionError(f"{label}: {len(gs)} vs {len(ws)} spans; first diff #{bad} near byte {lo}: {ctx!r}; "
                             f"gpu={list(zip(gs[bad:bad + 6].tolist(), ge[bad:bad + 6].tolist()))} "
                             f"want={list(zip(ws[bad:bad + 6].tolist(), we[bad:bad + 6].tolist()))}")
    assert np.array_equal(gd, wd), label


def _plain(s, form, name, corpus, hmm):
    buf, off = corpus
    want = s.part(name, corpus).want("cut", hmm)
    _cmp(s.tk[form].cut_batch(buf, off, hmm), want, f"{name} {form} hmm={hmm}", buf)


# ---- the pipeline -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmm", HMM)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shift", [0, 7])
def test_pipeline_scalars(syn, corp, shift, form, hmm):
    """S: every scalar value as a document of its own, at every lane offset and tile position.  The
    per-document token count against the closed form first, so that a failure names the code point."""
    buf, off = corp[f"S{shift}"]
    gs, ge, gd = syn.tk[form].cut_batch(buf, off, hmm)
    got = np.diff(gd.astype(np.int64))[1 if shift else 0:]
    bad = np.flatnonzero(got != corp["Scount"])
    cps = CC.all_scalars()
    assert len(bad) == 0, (f"{len(bad)} code points with a wrong token count, the first: " +
                           ", ".join(f"U+{int(cps[k]):04X} {int(got[k])} for {int(corp['Scount'][k])}" for k in bad[:8]))
    _cmp((gs, ge, gd), syn.part(f"S{shift}", corp[f"S{shift}"]).want("cut", hmm), f"S shift={shift} {form} hmm={hmm}", buf)


@pytest.mark.parametrize("hmm", HMM)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["D", "M", "T"])
def test_pipeline(syn, corp, name, form, hmm):
    _plain(syn, form, name, corp[name], hmm)


@pytest.mark.parametrize("hmm", HMM)
@pytest.mark.parametrize("form", FORMS)
def test_pipeline_lookahead(lset, corp, form, hmm):
    """L under its own dictionary: bytes after a tile's last Han rune that are no rune give no edge."""
    _plain(lset, form, "L", corp["L"], hmm)


@pytest.mark.parametrize("hmm", HMM)
def test_one_document(syn, corp, hmm):
    """D and M as a single document: the blocks merge across the former boundaries."""
    assert len(corp["DM1"][1]) == 2 and int(corp["DM1"][1][1]) == int(corp["D"][1][-1]) + int(corp["M"][1][-1])
    _plain(syn, "auto", "DM1", corp["DM1"], hmm)


# ---- k_small ------------------------------------------------------------------------------------------------
def _small(s, name, corpus, min_small):
    """The corpus in batches of at most 4,096 bytes and 4,096 documents, one call each, against slices of
    the oracle's result for the whole corpus and the pipeline's counters (JB_SMALL=0)."""
    buf, off = corpus
    tk, tp = s.tk["auto"], s.tk["pipeline"]
    batches = CC.small_batches(buf, off)
    o64 = off.astype(np.int64)
    nsmall = sum(1 for a, b in batches if o64[b] - o64[a] <= 4096)
    assert nsmall >= min_small, (name, nsmall)
    for hmm in HMM:
        ws, we, wd = s.part(name, corpus).want("cut", hmm)
        for a, b in batches:
            k0, k1 = int(wd[a]), int(wd[b])
            want = (ws[k0:k1], we[k0:k1], wd[a:b + 1] - np.uint64(k0))
            label = f"{name} documents {a}..{b} hmm={hmm}"
            _cmp(tk.cut_batch(buf, off[a:b + 1], hmm), want, label, buf)
            st = tk.last_stats()
            assert st["tokens"] == k1 - k0, label
            if o64[b] - o64[a] <= 4096:  # (a longer batch took the pipeline in both)
                _cmp(tp.cut_batch(buf, off[a:b + 1], hmm), want, label + " pipeline", buf)
                sp = tp.last_stats()
                for k in ("tokens", "blocks", "zh_blocks"):
                    assert st[k] == sp[k], (label, k, st, sp)


@pytest.mark.parametrize("name,min_small", [("D", 190), ("M", 1000), ("T", 1)])
def test_small_batches(syn, corp, name, min_small):
    _small(syn, name, corp[name], min_small)


def test_small_batches_lookahead(lset, corp):
    _small(lset, "L", corp["L"], 20)


# ---- search mode, full mode, ids --------------------------------------------------------------------------
def _full_want(s, name, corpus):
    """full_ref.expected's loop with one split buffer for all documents (M has 235,904)."""
    key = ("full", name)
    if key not in s.parts:
        buf, off = corpus
        data = bytes(np.asarray(buf, np.uint8)[:int(off[-1])])
        o = [int(x) for x in off]
        out = np.zeros(3 * (2 * max(np.diff(o).max(), 1) + 2), np.uint64)
        split = O.lib().or_split_text
        xs, xe, xd = [], [], [0]
        for a, b in zip(o[:-1], o[1:]):
            doc = data[a:b]
            n = split(doc, b - a, 0, out.ctypes.data)
            v = out[:3 * n].tolist()
            for i in range(n):
                x, y, han = v[3 * i], v[3 * i + 1], v[3 * i + 2]
                blk = doc[x:y]
                for p, q in (s.blocks.of_han(blk) if han else s.blocks.of_non(blk)):
                    xs.append(a + x + p)
                    xe.append(a + x + q)
            xd.append(len(xs))
        s.parts[key] = (np.array(xs, np.uint64), np.array(xe, np.uint64), np.array(xd, np.uint64))
    return s.parts[key]


def _mode(s, name, corpus, mode, hmm):
    buf, off = corpus
    tk = s.tk["auto"]
    if mode == "full":
        want = _full_want(s, name, corpus)
        if name == "T":  # (the short loop is full_ref's own)
            _cmp(want, s.part(name, corpus).want("full"), "full_ref")
        got = tk.cut_batch_full(buf, off)
    else:
        want = s.part(name, corpus).want("search", hmm)
        got = tk.cut_batch_search(buf, off, hmm)
    _cmp(got, want, f"{name} {mode} hmm={hmm}", buf)
    return got


@pytest.mark.parametrize("mode,hmm", MODES)
@pytest.mark.parametrize("name", ["D", "M", "T"])
def test_modes(syn, corp, name, mode, hmm):
    _mode(syn, name, corp[name], mode, hmm)


@pytest.mark.parametrize("mode,hmm", MODES)
def test_modes_lookahead(lset, corp, mode, hmm):
    """L in search and full mode.  Full mode emits the words that start at the run's last 丁 (丁一 and
    丁一丁, or 丁𠀀 and 丁𠀀丁, or 丁文) only after the three valid tails; after every other tail that 丁
    stands alone."""
    buf, off = corp["L"]
    gs, ge, _ = _mode(lset, "L", corp["L"], mode, hmm)
    if mode != "full":
        return
    gs, ge = gs.astype(np.int64), ge.astype(np.int64)
    nvalid = 0
    for d, tail, end in corp["Lcases"]:
        got = sorted(ge[gs == end - 3].tolist())
        t = tail.decode("utf-8", "replace")
        if t in ("一", "𠀀"):
            want = [end + len(tail), end + len(tail) + 3]
        elif t == "文":
            want = [end + 3]
        else:
            want = [end]
        nvalid += len(want) > 1 or t == "文"
        assert got == want, (d, tail, end, got, want)
    assert nvalid == 3 * 2 * len(CC.L_ENDS)


@pytest.mark.parametrize("name", ["D", "M", "T", "L"])
def test_ids(syn, lset, corp, name):
    """The id lookup over the plain tokens: a 1-byte span with a byte >= 0x80 maps to the U+FFFD key, and
    nothing else does but the key's own bytes."""
    s = lset if name == "L" else syn
    buf, off = corp[name]
    tk = s.tk["auto"]
    tk.set_vocab(VOCAB_KEYS)
    try:
        vocab = V.key_dict([k.encode() for k in VOCAB_KEYS])
        data = bytes(np.asarray(buf, np.uint8)[:int(off[-1])])
        nfffd = 0
        for hmm in HMM:
            ws, we, _ = s.part(name, corp[name]).want("cut", hmm)
            want = V.expect_ids(vocab, data, ws.tolist(), we.tolist())
            got = tk.spans_ids(np.asarray(buf, np.uint8), ws, we)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (name, hmm, [(int(ws[k]), int(we[k]), int(got[k]), int(want[k])) for k in bad[:8]])
            b8, a64, n64 = np.asarray(buf, np.uint8), ws.astype(np.int64), (we - ws).astype(np.int64)
            one = (n64 == 1) & (b8[a64] >= 0x80)
            whole = (n64 == 3) & (b8[a64] == 0xEF) & (b8[a64 + 1] == 0xBF) & (b8[a64 + 2] == 0xBD)
            assert np.array_equal(want == 0, one | whole)
            nfffd += int(one.sum())
        if name in ("M", "T"):
            assert nfffd >= 100
    finally:
        tk.set_vocab(None)


# ---- E: words, emissions and texts over the rare ranges -------------------------------------------------------
def test_rare_corpus_is_not_hollow(eset):
    """From the oracle alone: at least 500 distinct dictionary words of two or more runes and at least 100
    distinct four-byte runes among the tokens, every Han range's end points in the pool, and tokens on
    both sides of the HMM."""
    buf, off = eset.corpus
    data = bytes(buf[:int(off[-1])])
    pool = set(CC.pool_E())
    assert all(chr(lo) in pool and chr(hi) in pool for lo, hi in CC.HAN)
    assert 2500 <= len(eset.words) <= 3500 and len(off) - 1 == 301
    for hmm in HMM:
        ws, we, _ = eset.part("E", eset.corpus).want("cut", hmm)
        toks = {data[a:b] for a, b in zip(ws.tolist(), we.tolist())}
        words = {t.decode() for t in toks if len(t) >= 5 and t.decode("utf-8", "replace") in eset.words}
        assert len([w for w in words if len(w) >= 2]) >= 500, len(words)
        four = {ch for t in toks for ch in t.decode("utf-8", "replace") if ord(ch) >= 0x10000}
        assert len(four) >= 100, len(four)


@pytest.mark.parametrize("hmm", HMM)
@pytest.mark.parametrize("form", FORMS)
def test_rare_pipeline(eset, form, hmm):
    _plain(eset, form, "E", eset.corpus, hmm)


def test_rare_small_batches(eset):
    _small(eset, "E", eset.corpus, 100)


@pytest.mark.parametrize("mode,hmm", MODES)
def test_rare_modes(eset, mode, hmm):
    got = _mode(eset, "E", eset.corpus, mode, hmm)
    plain = eset.part("E", eset.corpus).want("cut", hmm)
    assert len(got[0]) > len(plain[0]) + 1000  # (grams and overlapping words do come out)
