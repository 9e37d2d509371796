"""k_mark_walk's instruction-issue cuts, path by path: the walk
trip's 32-bit record halves and wave-uniform refill, the dump-slot stores of a lane's seven
slots, the 32-bit document mask, the run-links loop.  Every case is cut through
jb_cut_device and compared span for span with the oracle, with JB_MW_SPLIT at its default
and forced to 1 (two workgroups per tile, each walking half of the entries).

The inputs are the smallest that reach each path; before any kernel runs, each case checks
on the bytes and on the oracle's DAG that the input really holds what it is named for."""
import random

import numpy as np
import pytest

import jiebahip as J
import oracle as O
import synth

pytestmark = pytest.mark.gpu

TILE = 4096          # kTileBytes
LANE = 16            # bytes per lane
LA_RUNES = 8         # kLA: lookahead entries past the tile end
REC_IDX_MAX = (1 << 14) - 2  # kRecIdxMax

SPLITS = {"default": {}, "split1": {"JB_MW_SPLIT": "1"}}


def _r(base, n):
    return "".join(chr(base + i) for i in range(n))


POOL = [chr(0x4E00 + i) for i in range(200)]
W8, W9, W12 = _r(0x5000, 8), _r(0x5010, 9), _r(0x5020, 12)  # words whose only other edge is the first rune's own
W40 = _r(0x5100, 40)                                         # ... and a walk of more trips than a 32-bit shift has bits
R4, R5 = _r(0x5040, 4), _r(0x5050, 5)                       # every prefix a word: 4 and 5 words start at the first rune
D = chr(0x5060)                                              # D, DD, DDD are words: every rune of a D run walks
SIZE = 60101967                                              # (the prefix form takes its size from the caller)
NFILL = 17000                                                # two-rune words, each with a weight of its own


def _dict_lines():
    rng = random.Random(3)
    lines = [f"{W8[0]} 11", f"{W8} 12", f"{W9[0]} 13", f"{W9} 14", f"{W12[0]} 15", f"{W12} 16",
             f"{W40[0]} 17", f"{W40} 18"]
    lines += [f"{R4[:k]} {20 + k}" for k in range(1, 5)] + [f"{R5[:k]} {30 + k}" for k in range(1, 6)]
    lines += [f"{D * k} {40 + k}" for k in range(1, 4)]
    lines += [f"{c} {100 + i}" for i, c in enumerate(POOL)]  # (a rune with count 0 has its single edge only, :468-471)
    pairs = [a + b for a in POOL for b in POOL]
    rng.shuffle(pairs)
    fill = pairs[:NFILL]
    lines += [f"{w} {1000 + 3 * i}" for i, w in enumerate(fill)]
    return lines, fill


@pytest.fixture(scope="module")
def issue_dict(tmp_path_factory, syn_small):
    lines, fill = _dict_lines()
    dp = tmp_path_factory.mktemp("mw_issue") / "dict.txt"
    dp.write_text("\n".join(lines) + "\n", encoding="utf-8")
    # (the prefix-dictionary form: every prefix of a word is a key, so walks go through them)
    o = O.Oracle.from_files(str(dp), syn_small[1], J.JB_DICT_PREFIX, SIZE)
    freqs = {int(ln.split()[1]) for ln in lines}
    # more distinct weights than a record's 14-bit field holds: with every fill word in the
    # text, the weight indices kRecIdxMax and kRecIdxMax + 1 are both walked
    assert len(freqs) > REC_IDX_MAX + 2
    yield str(dp), syn_small[1], o, fill
    o.close()


@pytest.fixture(scope="module", params=list(SPLITS))
def pair(issue_dict, request):
    dp, ep, o, fill = issue_dict
    with pytest.MonkeyPatch.context() as mp:
        for k, v in SPLITS[request.param].items():
            mp.setenv(k, v)
        tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep, kind=J.JB_DICT_PREFIX, size_override=SIZE))
    yield tk, o, fill
    tk.close()


def _batch(docs):
    bs = [d.encode("utf-8") if isinstance(d, str) else d for d in docs]
    off = np.zeros(len(bs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs) + b"\0" * 64, np.uint8), off


def _cut_device(tk, buf, off, hmm):
    import torch
    nbytes = int(off[-1])
    d_text = torch.from_numpy(np.array(buf)).cuda()
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    ps, pe, pd, pn = tk.cut_device(d_text.data_ptr(), nbytes, d_off.data_ptr(), len(off) - 1, bool(hmm), stream)
    tk.device_status(stream)
    n = int(J.dev_to_host(pn, 8, np.uint64)[0])
    return (J.dev_to_host(ps, 4 * n, np.uint32), J.dev_to_host(pe, 4 * n, np.uint32),
            J.dev_to_host(pd, 8 * len(off), np.uint64))


def _check(tk, o, docs, label):
    buf, off = _batch(docs)
    for hmm in (False, True):
        gs, ge, gd = _cut_device(tk, buf, off, hmm)
        os_, oe, od = o.cut_batch(buf, off, hmm, nthreads=8)
        assert len(gs) == len(os_) and np.array_equal(gs, os_) and np.array_equal(ge, oe), (label, hmm)
        assert np.array_equal(gd, od), (label, hmm)


# ---- what the bytes hold, lane by lane (a lane's window is [p0 - 4, p0 + 20)) -----------------

def _lane_leads(b):
    """Lead bytes (>= 0xC0) in each lane's window indices 0..19."""
    a = np.frombuffer(b, np.uint8)
    lead = np.concatenate([np.zeros(4, bool), a >= 0xC0, np.zeros(LANE + 4, bool)])
    return [int(lead[p0:p0 + 20].sum()) for p0 in range(0, len(a), LANE)]


def _lane_han_starts(text):
    """Han rune starts in each lane's own 16 bytes (the text is valid UTF-8, one document)."""
    n = len(text.encode("utf-8"))
    cnt = [0] * ((n + LANE - 1) // LANE)
    pos = 0
    for ch in text:
        c = ord(ch)
        if (0x4E00 <= c <= 0x9FFC or 0x3400 <= c <= 0x4DBF or c in (0x3005, 0x3007) or 0x3021 <= c <= 0x3029
                or 0x3038 <= c <= 0x303B or 0x2E80 <= c <= 0x2FFF or 0xF900 <= c <= 0xFAFF or c >= 0x20000):
            cnt[pos // LANE] += 1
        pos += len(ch.encode("utf-8"))
    return cnt


def _dag_edges(o, run):
    """(start rune, length) of every DAG edge of a Han run."""
    return [(i, e - i) for i, ends in o.build_dag(run).items() for e in ends]


def _fill_run(fill, rng, nrunes):
    s = "".join(rng.choice(fill) for _ in range(nrunes // 2 + 1))
    return s[:nrunes]


# ---- the cases ------------------------------------------------------------------------------

def test_seven_and_eight_leads(pair):
    """A lane with exactly 7 leads (all in the unrolled loop) and one with 8 (the 8th goes to
    the general decode), at every alignment."""
    tk, o, fill = pair
    rng = random.Random(1)
    text = "".join("a" * s + _fill_run(fill, rng, 40) + "，" + "é中" * 12 + "é" * 14 + "x" for s in range(16))
    leads = _lane_leads(text.encode())
    assert 7 in leads and 8 in leads and max(leads) >= 10
    assert len(text.encode()) <= 3 * TILE
    _check(tk, o, [text], "7 and 8 leads")


@pytest.mark.parametrize("rune", ["\U00020000", "々", "〇", "⺀", "豈"])
def test_redecode_refills_slots(pair, rune):
    """Han starts the fast loop does not take (a 4-byte rune, the U+3000 page, the rare
    ranges): the lane decodes all of its starts again."""
    tk, o, fill = pair
    rng = random.Random(2)
    text = "".join("a" * s + _fill_run(fill, rng, 4) + rune + _fill_run(fill, rng, 5) + "，" for s in range(16))
    starts = _lane_han_starts(text)
    lanes_with = [starts[p // LANE] for p in (len(text[:i].encode()) for i, ch in enumerate(text) if ch == rune)]
    assert len(lanes_with) == 16 and max(lanes_with) >= 4  # the rune shares lanes with ordinary starts
    probe = POOL[0] + rune + POOL[1]  # the oracle takes it as Han: one block with its neighbours
    assert O.split_text("a" + probe + "a") == [(b"a", False), (probe.encode(), True), (b"a", False)]
    _check(tk, o, [text], f"redecode U+{ord(rune):04X}")


def test_zero_one_six_starts_in_a_wave(pair):
    """Lanes with 0, 1 and 6 Han starts in one wave: the dump-slot stores and the ranks."""
    tk, o, fill = pair
    rng = random.Random(4)
    text = "a" * 16 + "a" * 6 + POOL[5] + "a" * 7 + _fill_run(fill, rng, 11) + "b" * 15
    text += "".join("c" * s + _fill_run(fill, rng, 7) + "，" for s in range(1, 12))
    starts = _lane_han_starts(text)[:64]
    assert starts[0] == 0 and starts[1] == 1 and starts[2] == 6 and {2, 3, 4, 5} <= set(starts)
    _check(tk, o, [text], "0, 1 and 6 starts")


def test_document_starts_at_every_window_position(pair):
    """A document start at each of a window's 20 positions (every residue of the start mod 16
    puts it at two of them), sequences cut by a boundary, and batches that end inside a
    lane's window at every residue: the 32-bit document mask."""
    tk, o, fill = pair
    rng = random.Random(5)
    docs = []
    for j in range(48):
        docs.append(_fill_run(fill, rng, 1 + j % 7).encode() + b"a" * (j % 3))
    docs += [POOL[1].encode()[:2], POOL[1].encode()[2:] + POOL[2].encode(), b"\xf0\xa0\x80", b"\x80" + POOL[3].encode()]
    _, off = _batch(docs)
    assert {int(x) % 16 for x in off[1:-1]} == set(range(16))
    _check(tk, o, docs, "document starts")
    tail = _fill_run(fill, rng, 12).encode()
    ends = set()
    for cut in range(len(tail) - 16, len(tail)):
        d = docs + [b"xy" + tail[:cut]]
        ends.add(int(_batch(d)[1][-1]) % 16)
        _check(tk, o, d, f"batch end {cut}")
    assert ends == set(range(16))


@pytest.mark.parametrize("past", [1, 13, 14, 20])
@pytest.mark.parametrize("phase", [0, 1, 2])
def test_run_across_tile_end(pair, past, phase):
    """A Han run whose last rune of the tile ends at the tile end or 1-2 bytes past it, with
    `past` runes after it: the lookahead chain, kEntEdge, and record 0 for a walk that goes
    on past the lookahead (the 12-rune word starts at the tile's last rune)."""
    tk, o, fill = pair
    rng = random.Random(6)
    m = 24                                  # runes of the run that start in the tile
    last = TILE - 3 + phase                 # byte of the tile's last rune
    s0 = last - 3 * (m - 1)
    # the tile's last rune and the runes past it: a two-rune word across the end, or the 12-rune one
    tail = rng.choice(fill) if past == 1 else (W12 + W8 + W9)[:1 + past]
    run = _fill_run(fill, rng, m - 9) + W8 + tail
    text = "a" * s0 + run + "，" + _fill_run(fill, rng, 6)
    b = text.encode()
    assert b[last] >= 0xE0 and len(b) <= 3 * TILE
    pos = [s0 + 3 * i for i in range(len(run))]
    edges = _dag_edges(o, run)
    crossing = [(i, n) for i, n in edges if pos[i] < TILE <= pos[i + n - 1]]
    assert crossing, "no DAG edge crosses the tile end"
    if past >= 11:  # the whole 12-rune word: an edge that ends past the kLA lookahead entries
        assert any(pos[i] < TILE and i + n - 1 > (m - 1) + LA_RUNES for i, n in edges)
    _check(tk, o, [text], f"tile end past={past} phase={phase}")


def test_long_edges_and_many_words(pair):
    """Edges of 8 runes (the last a record holds) and 9 (record 0); a rune with 4 words
    starting at it (a full record) and one with 5 (record 0)."""
    tk, o, fill = pair
    for run, want in ((W8, (8, None)), (W9, (9, None)), (R4, (None, 4)), (R5, (None, 5))):
        dag = o.build_dag(run)
        if want[0]:
            assert want[0] in [e - 0 for e in dag[0]]
        else:
            assert len(dag[0]) == want[1]
    text = "".join("a" * s + W8 + "，" + W9 + "。" + R4 + "，" + R5 + "x" + W8 + R4 + W9 + R5 + "，" for s in range(16))
    _check(tk, o, [text], "edge lengths and word counts")


def test_walk_longer_than_the_length_bit(pair):
    """A walk of 39 trips through prefixes that are keys without being words: the edge length is
    kept as a mask bit doubled every trip, which must saturate, not shift out to the value that
    means "this lane has no walk" (a walk dropped there leaves the sort's scratch value as its
    record)."""
    tk, o, fill = pair
    assert (0, 40) in _dag_edges(o, W40) and all(o.get(W40[:k]) == 0 for k in range(2, 40))
    text = "".join("a" * s + W40 + "，" + W40[:35] + "。" for s in range(0, 16, 3))
    _check(tk, o, [text], "walk of 39 trips")


def test_weight_index_limit(pair):
    """Every fill word once: more than 2^14 distinct weights, so the indices kRecIdxMax (the
    last that fits a record) and kRecIdxMax + 1 (record 0) are both walked."""
    tk, o, fill = pair
    assert len(set(fill)) == NFILL > REC_IDX_MAX + 2
    text = "，".join(fill)
    _check(tk, o, [text], "weight index limit")


def test_empty_and_full_walk_lists(pair):
    """A tile none of whose entries walks (single Han runes between commas) and one where
    every entry does (a run of a rune whose 1-, 2- and 3-fold are words)."""
    tk, o, fill = pair
    lone = (POOL[7] + "，") * (TILE // 6 + 8)
    assert all(n == 1 for _, n in _dag_edges(o, POOL[7]))
    run = D * (TILE // 3 + 40)
    dag = o.build_dag(run)
    assert all(len(dag[i]) == 3 for i in range(TILE // 3 + 1))
    _check(tk, o, [lone], "empty walk list")
    _check(tk, o, [run], "every entry walks")
    _check(tk, o, [lone[:TILE], run], "both")


@pytest.mark.parametrize("split", list(SPLITS))
def test_plainw_zero(tmp_path, mini_paths, split, monkeypatch):
    """A dictionary of size < 0 (DevImage::plainw == 0): every record is 0, no entry walks."""
    dp = tmp_path / "dict.txt"
    dp.write_text("中 5\n文 1\n中文 -20\n天氣 2\n", encoding="utf-8")
    for k, v in SPLITS[split].items():
        monkeypatch.setenv(k, v)
    tk = J.Tokenizer(J.make_config(dict_path=str(dp), emit_path=mini_paths[1]))
    o = O.Oracle.from_files(str(dp), mini_paths[1], 0)
    try:
        assert o.size < 0
        docs = ["中文上海天氣很好" * 60, "中" * 40 + "，" + "文中" * 30, "abc 中文 def", "一丁㐀中文" * 200]
        assert sum(len(d.encode()) for d in docs) > TILE  # past one tile
        _check(tk, o, docs, "plainw == 0")
    finally:
        tk.close()
        o.close()


@pytest.mark.parametrize("split", list(SPLITS))
def test_docs_slice(syn_full, split, monkeypatch):
    """One 4 MiB slice of the headline corpus (C_syn documents on D_syn)."""
    dp, ep, s = syn_full
    for k, v in SPLITS[split].items():
        monkeypatch.setenv(k, v)
    tk = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
    o = O.Oracle.from_files(dp, ep, 0)
    try:
        buf, off, _ = s.corpus(synth.KIND_DOCS, 4242, target_bytes=4 << 20)
        buf = np.concatenate([np.asarray(buf)[:int(off[-1])], np.zeros(64, np.uint8)])
        for hmm in (False, True):
            gs, ge, gd = _cut_device(tk, buf, off, hmm)
            os_, oe, od = o.cut_batch(buf, off, hmm, nthreads=8)
            assert np.array_equal(gs, os_) and np.array_equal(ge, oe) and np.array_equal(gd, od), hmm
    finally:
        tk.close()
        o.close()
