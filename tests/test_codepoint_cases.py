"""CPU: the checker itself at every range edge and byte class, and the corpora the GPU sweep relies on.

The oracle (or_split_text, or_cut_nonzh, Oracle.cut_batch without the HMM) must equal codepoint_cases'
independent model, token for token, on S', D, M, T and L; jb_common.h's jb_decode, jb_is_han and
jb_is_space, built into tests/host/rune_check.cpp, must equal it on every malformed sequence and valid
encoding under every `lim`, and on every value; the same program runs clean under AddressSanitizer and
UndefinedBehaviorSanitizer.  The corpus properties test_gpu_codepoints.py depends on are asserted here
from the corpora themselves.
"""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import codepoint_cases as CC
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLES = "丁 5\n"  # no word of two runes: without the HMM every Han rune is a token, whatever it is


@pytest.fixture(scope="module")
def corpora():
    L = CC.corpus_L()
    return {"S'": CC.corpus_Sprime(), "D": CC.corpus_D(), "M": CC.corpus_M(), "T": CC.corpus_T(), "L": L[:2]}


@pytest.fixture(scope="module")
def singles(mini_paths):
    with open(mini_paths[1], "rb") as f:
        return O.Oracle(SINGLES, f.read(), 0)


def test_counts():
    assert len(CC.all_scalars()) == 1_112_064
    sp = CC.sprime_scalars()
    assert len(sp) == 213_606 == len(np.unique(sp)) and bool(np.all(np.diff(sp.astype(np.int64)) > 0))
    assert not bool(np.any((sp >= 0xD800) & (sp < 0xE000)))
    buf, off = CC.corpus_S()
    assert len(off) - 1 == 1_112_064 and 20 << 20 < int(off[-1]) < 22 << 20
    assert sorted(set(np.diff(off).tolist())) == [13, 15, 17, 19]
    # the documents are what the recipe says, by Python's own encoder (a sample of each width, both ends)
    for k in (0, 0x41, 0x7F, 0x80, 0x7FF, 0x800, 0xD7FF, 0xD800, 0xFFFF - 0x800, 0x10000 - 0x800, 1_112_063):
        c = chr(int(CC.all_scalars()[k]))
        assert bytes(buf[int(off[k]):int(off[k + 1])]) == ("，" + c + "，中a" + c + "b").encode(), hex(ord(c))
    buf7, off7 = CC.corpus_Sprime(7)
    assert int(off7[1]) == 7 and bytes(buf7[:7]) == b"x" * 7 and len(off7) - 2 == 213_606
    b0, o0 = CC.corpus_Sprime()
    assert np.array_equal(buf7[7:7 + int(o0[-1])], b0[:int(o0[-1])])
    seqs = CC.malformed_seqs()
    assert seqs.shape == (235_904, 4)
    for r in (0x4000, 0x4FFF, 0x9000, 0x9FFF & ~0x3F | 0x3F):  # overlong encodings of Han values are among them
        if CC.is_han(r):
            assert bool(np.any(np.all(seqs == np.frombuffer(CC.overlong4(r), np.uint8), axis=1))), hex(r)
    assert CC.is_han(0x4000) and CC.is_han(0x4FFF) and CC.is_han(0x9000)
    assert len(CC.corpus_M()[1]) - 1 == 235_904
    assert len(CC.corpus_D()[1]) - 1 == (213_606 + 23) // 24
    assert 38 <= len(CC.T_RUNES) == len(set(CC.T_RUNES)) <= 42
    assert len(CC.corpus_T()[1]) - 1 == 2 * sum(CC.width_of(r) - 1 for r in CC.T_RUNES)


def test_sprime_lane_offsets_and_tile_crossings(corpora):
    """Every offset 0..15 of c in its 16-byte chunk, for each width; at least 200 documents astride a 4 KiB
    tile edge for the widths 3 and 4, c itself (either copy) astride one at least 50 times.  (The 1,920
    two-byte scalars fill 28,800 bytes, seven tile edges in all: for width 2, a document astride every one
    of those edges.)"""
    buf, off = corpora["S'"]
    o = off.astype(np.int64)
    ln = np.diff(o)
    for w in (2, 3, 4):
        d = np.flatnonzero(ln == 11 + 2 * w)
        first, second = o[d] + 3, o[d] + 3 + w + 7
        assert set((first % 16).tolist()) == set(range(16)) == set((second % 16).tolist()), w
        astride = sum(int(np.count_nonzero((p // CC.TILE) != ((p + w - 1) // CC.TILE))) for p in (first, second))
        docs_astride = int(np.count_nonzero((o[d] // CC.TILE) != ((o[d + 1] - 1) // CC.TILE)))
        if w > 2:
            assert docs_astride >= 200 and astride >= 50, (w, astride, docs_astride)
        else:
            assert docs_astride == int(o[d[-1] + 1] - 1) // CC.TILE - int(o[d[0]]) // CC.TILE >= 7


def test_lookahead_layout():
    """L from its offsets: the run's last 丁 ends at each listed offset against the tile, for every tail,
    with the document starting in that tile and in the tile before; the first three tiles are used."""
    buf, off, cases = CC.corpus_L()
    data = bytes(buf[:int(off[-1])])
    run = ("丁" * CC.L_RUN).encode()
    seen, tiles = set(), set()
    for d, tail, _ in cases:
        a, b = int(off[d]), int(off[d + 1])
        doc = data[a:b]
        p = doc.index("，".encode())
        assert doc[:p] == b"f" * p and doc[p + 3:p + 3 + len(run)] == run
        end = a + p + 3 + len(run)  # one past the last 丁 of the run
        assert doc[p + 3 + len(run):] == tail + "丁丁文".encode()
        (e,) = [x for x in CC.L_ENDS if (end - x) % CC.TILE == 0]
        t = (end - e) // CC.TILE    # the tile the offset is counted in: the one the run's last 丁 starts in
        assert t == (end - 3) // CC.TILE
        where = a // CC.TILE - t
        assert where in (0, -1)
        seen.add((tail, e, where))
        tiles.add(t)
    assert seen == {(t, e, w) for t in CC.L_TAILS for e in CC.L_ENDS for w in (0, -1)}
    assert {0, 1, 2} <= tiles
    assert len(CC.L_TAILS) == 15 == len(set(CC.L_TAILS))


def _oracle_split(doc, out):
    n = O.lib().or_split_text(doc, len(doc), 0, out.ctypes.data)
    v = out[:3 * n].tolist()
    return [(v[3 * i], v[3 * i + 1], bool(v[3 * i + 2])) for i in range(n)]


def _oracle_nonzh(doc, s, e):
    n = O.lib().or_cut_nonzh(doc, len(doc), s.ctypes.data, e.ctypes.data, len(s))
    return list(zip(s[:n].tolist(), e[:n].tolist()))


@pytest.mark.parametrize("name", ["S'", "D", "M", "T", "L"])
def test_oracle_equals_model(corpora, singles, name):
    buf, off = corpora[name]
    docs = CC.docs_of(buf, off)
    cap = max(len(d) for d in docs) + 2
    out, s, e = np.zeros(3 * (2 * cap + 2), np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    bad = []
    ms, me, md = [], [], [0]
    base = [int(x) for x in off]
    for k, d in enumerate(docs):
        blocks = CC.split_blocks(d)
        if _oracle_split(d, out) != blocks:
            bad.append(("split", k, d))
        if _oracle_nonzh(d, s, e) != CC.cut_nonzh(d):
            bad.append(("nonzh", k, d))
        for x, y in CC.cut_singles(d, blocks):
            ms.append(base[k] + x)
            me.append(base[k] + y)
        md.append(len(ms))
    assert not bad, (len(bad), bad[:5])
    gs, ge, gd = singles.cut_batch(buf, off, False, nthreads=8)
    diff = int(np.count_nonzero(gd != np.array(md, np.uint64)))
    assert diff == 0 and np.array_equal(gs, np.array(ms, np.uint32)) and np.array_equal(ge, np.array(me, np.uint32)), \
        (name, diff)


def test_scalar_token_counts_closed_form(singles):
    """The closed form the GPU test names a code point by, against the oracle on all of S."""
    buf, off = CC.corpus_S()
    for hmm in (False, True):
        gd = singles.cut_batch(buf, off, hmm, nthreads=8, want_spans=False)[2]
        got = np.diff(gd.astype(np.int64))
        want = CC.scalar_token_counts(CC.all_scalars())
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, [hex(int(CC.all_scalars()[k])) for k in bad[:10]]


# ---- jb_common.h's rules as a program -------------------------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "jieba-go_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "host", "rune_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def rune_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("rune")
    return _build(tmp, "rune_check", ["-O2"]), _build(tmp, "rune_check_san", SAN), tmp


@pytest.fixture(scope="module")
def words(rune_check):
    """M and every valid encoding as 4-byte words (zero bytes after a shorter encoding), and the file of
    them that rune_check reads."""
    valid = []
    for w, c in CC._width_groups(CC.all_scalars()):
        enc = np.zeros((len(c), 4), np.uint8)
        enc[:, :w] = CC.encode_np(c)
        valid.append(enc)
    valid = np.concatenate(valid)
    # the encodings are Python's own: one strict decode of them all gives the scalars back
    text = b"".join(bytes(row[:w]) for row, w in ((valid[k], CC.width_of(int(c))) for k, c in
                                                  enumerate(CC.all_scalars()[:70000].tolist())))
    assert [ord(ch) for ch in text.decode("utf-8")] == CC.all_scalars()[:70000].tolist()
    four = valid[valid[:, 0] >= 0xF0]
    assert four.tobytes().decode("utf-8") == "".join(map(chr, range(0x10000, 0x110000)))
    allw = np.ascontiguousarray(np.concatenate([CC.malformed_seqs(), valid]))
    path = str(rune_check[2] / "words.bin")
    allw.view("<u4").tofile(path)
    return allw, path


def _expected_decode(allw):
    """The model under lim = 1..4: (n, 8) of rune, width pairs."""
    n = len(allw)
    out = np.zeros((n, 8), np.int64)
    cache = {}
    data = allw.tobytes()
    for k in range(n):
        key = data[4 * k:4 * k + 4]
        v = cache.get(key)
        if v is None:
            v = []
            for lim in (1, 2, 3, 4):
                v += CC.decode(key[:lim])
            cache[key] = v
        out[k] = v
    return out


def test_rune_check_equals_model(rune_check, words):
    allw, path = words
    r = subprocess.run([rune_check[0], "decode", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.loadtxt(io.StringIO(r.stdout), dtype=np.int64)
    assert got.shape == (len(allw), 8)
    want = _expected_decode(allw)
    bad = np.flatnonzero(np.any(got != want, axis=1))
    assert len(bad) == 0, (len(bad), [(allw[k].tobytes().hex(), got[k].tolist(), want[k].tolist()) for k in bad[:5]])
    r = subprocess.run([rune_check[0], "classes"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    cls = np.loadtxt(io.StringIO(r.stdout), dtype=np.int64)
    assert cls.shape == (0x110001, 3)
    han = np.array([CC.is_han(c) for c in range(0x110001)])
    sp = np.array([CC.is_space(c) for c in range(0x110001)])
    al = np.array([c < 0x80 and c in CC.ALNUM for c in range(0x110001)])
    for name, g, w in (("han", cls[:, 0], han), ("space", cls[:, 1], sp), ("alnum", cls[:, 2], al)):
        bad = np.flatnonzero(g.astype(bool) != w)
        assert len(bad) == 0, (name, [hex(int(k)) for k in bad[:10]])
    assert int(han.sum()) == sum(hi - lo + 1 for lo, hi in CC.HAN) and int(sp.sum()) == 25


def test_rune_check_under_asan_ubsan(rune_check, words):
    """The same program built with the sanitizers, run as a program of its own: clean, same output."""
    plain = subprocess.run([rune_check[0], "decode", words[1]], capture_output=True, timeout=600)
    for args in (["decode", words[1]], ["classes"]):
        r = subprocess.run([rune_check[1], *args], capture_output=True, timeout=600, env=ENV)
        assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
        if args[0] == "decode":
            assert r.stdout == plain.stdout
