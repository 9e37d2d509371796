"""CPU: the shadow model and the op generator of tests/ctx_model.py, which test_gpu_sequences.py runs against
the library.  The seeds that file uses must contain every transition between calls the sequences exist for;
the model's own rules (the suggested frequency, which added words buildDag can reach) are checked against the
oracle and the hand-worked examples."""
import hashlib
import os

import numpy as np
import pytest

import ctx_model as M
import full_ref as F
import join_ref as JR
import search_ref as R
import test_gpu_sequences as T
import wc_ref as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def syn(syn_small):
    dp, ep, s = syn_small
    with open(dp, "rb") as f:
        d = f.read()
    with open(ep, "rb") as f:
        e = f.read()
    return d, e, s, M.make_batch(s, M.VOCAB_SOURCE)


@pytest.fixture(scope="module")
def mini():
    with open(os.path.join(GOLDEN, "mini_dict.txt"), encoding="utf-8") as f:
        d = f.read()
    with open(os.path.join(GOLDEN, "mini_emit.json"), "rb") as f:
        e = f.read()
    return d if d.endswith("\n") else d + "\n", e


# ---- the generator ------------------------------------------------------------------------------------------
def specs_of(ops):
    return [op[4] if op[0] == "cut" else op[2] for op in ops if op[0] == "cut" or op[0] in M.BATCH_OPS]


@pytest.mark.parametrize("seed", M.SEEDS)
def test_seed_covers_every_transition(seed):
    ops = M.gen_ops(seed, M.NSTEPS)
    assert len(ops) == M.NSTEPS and ops == M.gen_ops(seed, M.NSTEPS)  # (plain tuples, the same every time)
    c = M.coverage(ops)
    assert set(c["kinds"]) == set(M.OPS) and all(v >= 3 for v in c["kinds"].values()), c["kinds"]
    assert set(c["classes"]) == set(M.CLASSES) and all(v >= 2 for v in c["classes"].values()), c["classes"]
    for name in ("add_then_every_mode", "grow_then_repeat", "tiny_plain_host_after_add"):
        assert c[name], name
    for k in M.BATCH_OPS:
        assert c[k + ":large_then_tiny"] and c[k + ":tiny_then_large"], k
    assert M.covered(ops)
    assert sum(1 for op in ops if op[0] == "add_word") == 3  # (each one rebuilds the 20k image)
    for op in ops:
        assert op[0] in M.OPS
        if op[0] == "cut":
            assert op[1] in M.MODES and op[3] in M.ROUTES and op[4][0] in M.CLASSES and not (op[1] == "full" and op[2])


def test_the_condition_is_one():
    """Most seeds miss something: the condition the seeds are held to can fail."""
    missed = [s for s in range(1, 60) if not M.covered(M.gen_ops(s, M.NSTEPS))]
    assert len(missed) > 20 and not set(missed) & set(M.SEEDS)


@pytest.mark.parametrize("seed", M.SEEDS)
def test_size_classes_hold_for_the_real_batches(syn, seed):
    """The classes are promises about bytes and documents: checked on the batches make_batch builds."""
    s = syn[2]
    top = 0
    seen = {}
    for sp in specs_of(M.gen_ops(seed, M.NSTEPS)):
        b = seen.get(sp) or M.make_batch(s, sp)
        cls = sp[0]
        assert b.nbytes <= M.MAX_BYTES and len(b.buf) == int(b.off[-1]) + 64 and not b.buf[int(b.off[-1]):].any()
        if cls == "tiny":
            assert 0 < b.nbytes <= M.SMALL_MAX and b.ndocs <= M.SMALL_MAX
        elif cls == "small":
            assert 6 << 10 <= b.nbytes <= 60 << 10
        elif cls == "grow" and sp not in seen:
            assert b.nbytes > top, (sp, b.nbytes, top)
        elif cls == "large":
            assert b.nbytes > 64 << 10
        elif cls == "manydocs":
            assert b.ndocs > M.WORK_MIN_DOCS and np.diff(b.off.astype(np.int64)).max() <= 8
        elif cls == "empty":
            assert b.nbytes == 0 and b.ndocs > 0
        elif cls == "offset":
            assert int(b.off[0]) > 0 and b.nbytes > M.SMALL_MAX
            t, o = b.rel()
            assert int(o[0]) == 0 and bytes(t[:b.nbytes]) == bytes(b.buf[int(b.off[0]):int(b.off[-1])])
        seen[sp] = b
        top = max(top, b.nbytes)


# ---- the model ----------------------------------------------------------------------------------------------
def test_suggested_frequency_is_the_references_formula(mini):
    """tokenizer.go:589-614 on the mini dictionary, as test_add_word (test_gpu_parity.py) restates it."""
    d, e = mini
    m = M.Model(d.encode(), e)
    for word in ("很好", "天氣", "今天天氣", "量子力學", "甲乙"):
        pieces = m.o.cut(word, False)
        dsize = float(m.o.size)
        f = 1.0
        for p in pieces:
            v = m.o.get(p)
            f *= float(v if v is not None else 1) / dsize
        want = max(int(f * dsize) + 1, m.o.get(word) or 1)
        assert m.suggest(word) == (want, pieces)
    size0, pieces = m.o.size, m.o.cut("很好", False)
    got = m.add_word("很好", 0)
    assert got == m.o.get("很好") >= 1 and m.o.size == size0 + got
    assert m.last_tokens == len(pieces)  # (the library cuts the word to suggest a frequency: its last cut)
    assert m.version == 1 and m.add_word("天氣", 500) == 500 and m.o.get("天氣") == 500 and m.version == 2


def test_reachable_words_become_edges_and_others_do_not(mini):
    d, e = mini
    m = M.Model((F.chain_dict(4) + d).encode(), e)
    assert m.reachable("甲" * 5) and not m.is_edge("甲" * 5)
    m.add_word("甲" * 5, 9)
    assert m.is_edge("甲" * 5) and m.o.build_dag("甲" * 5)[0] == [1, 2, 3, 4, 5]
    assert not m.reachable("甲" * 7)  # (甲 x 6 is no key: AddWord adds no prefixes, tokenizer.go:475-478, 580-585)
    m.add_word("甲" * 7, 9)
    assert not m.is_edge("甲" * 7) and m.o.get("甲" * 7) == 9 and m.o.build_dag("甲" * 7)[0] == [1, 2, 3, 4, 5]
    assert not m.reachable("乙甲")  # (the gate on the first rune, :468-471)
    m.add_word("乙甲", 9)
    assert not m.is_edge("乙甲")


def test_fresh_caches_after_add_word(mini):
    """search_ref.Grams and full_ref.Blocks cache dictionary lookups: the model must not keep them."""
    d, e = mini
    m = M.Model((F.chain_dict(4) + d).encode(), e)
    b = M.from_texts(("t",), ["甲" * 6 + "，一刹那"])
    before = [m.cut(b, mode, False) for mode in M.MODES]
    m.add_word("甲" * 5, 10 ** 6)
    after = [m.cut(b, mode, False) for mode in M.MODES]
    for (ws, we, _), mode in zip(after, M.MODES):
        want = (m.o.cut_batch(b.buf, b.off, False) if mode == "plain" else
                R.expected(m.o, b.buf, b.off, False, grams=R.Grams(m.o)) if mode == "search" else
                F.expected(m.o, b.buf, b.off, F.Blocks(m.o)))
        assert np.array_equal(ws, want[0]) and np.array_equal(we, want[1]), mode
    assert any(len(x[0]) != len(y[0]) or not np.array_equal(x[0], y[0]) for x, y in zip(before, after))
    assert m.last_tokens == len(m.o.cut_batch(b.buf, b.off, False)[0])  # (full mode reports the plain counts)


def test_the_model_gives_the_hand_worked_examples(mini):
    d, e = mini
    for dict_text, cases in F.EXAMPLES:
        m = M.Model(dict_text.encode(), e)
        for text, want in cases:
            b = M.from_texts((text,), ["x", text])
            s, en, dt = m.cut(b, "full", False)
            k = int(dt[1])
            assert [bytes(b.buf[int(x):int(y)]).decode() for x, y in zip(s[k:], en[k:])] == want
    for dict_text, cases in R.EXAMPLES:
        m = M.Model((dict_text if dict_text is not None else d).encode(), e)
        for text, want in cases:
            b = M.from_texts((text,), ["x", text])
            s, en, dt = m.cut(b, "search", True)
            k = int(dt[1])
            assert [bytes(b.buf[int(x):int(y)]).decode() for x, y in zip(s[k:], en[k:])] == want


def test_the_scripted_words_are_reachable(mini, syn):
    """Every word the scripted GPU sequences add is one buildDag reaches (Driver.add_word asserts it again on
    the GPU): here without one, with the same dictionaries."""
    d, e = mini
    for lines in (F.chain_dict(8), "甲 100\n" + "".join(f"{'甲' * k} 0\n" for k in range(2, 8)) + f"{'甲' * 8} 108\n"):
        m = M.Model(T.reach_dict(d, lines).encode(), e)
        for n, w in T.FAM.items():
            assert not m.reachable(w)
            for word, f in (("甲" * n, 100 + n), (w[:2], T.FAM2), (w, 1)):
                assert m.reachable(word), word
                m.add_word(word, f)
                assert m.is_edge(word), word
            assert m.o.cut(w + w[0], False) == list(w + w[0])
            assert F.expected_text(m.o, w + w[0], m.blocks) == [w[:2], w, w[0]]
    m = M.Model((F.chain_dict(4) + d).encode(), e)
    assert m.o.build_dag("甲" * 9)[0] == [1, 2, 3, 4] and m.reachable("甲" * 5)
    dd, ee, s, source = syn
    m = M.Model(dd, ee, source=source)
    words = [m.pick_word(k) for k in range(3)]
    assert len(set(words)) == 3
    for w in words:
        assert len(w) == 2 and m.o.get(w) is None and m.reachable(w)
        m.add_word(w, 10_000_000)
        assert m.is_edge(w)


def test_vocabularies_and_the_batch_references(syn):
    """Vocabulary 1 is smaller than vocabulary 0 and has a longer longest key; the chain's references are
    not trivial on the source batch (ids found, terms counted, keywords and TextRank records present)."""
    d, e, s, source = syn
    m = M.Model(d, e, source=source)
    v0, v1 = m.vocab_keys(0), m.vocab_keys(1)
    assert len(v1) < len(v0) and max(map(len, v1)) > max(map(len, v0)) and len(set(v0)) == len(v0)
    m.set_vocab(v0)
    ids, dt, (tid, tcnt, toff) = m.chain(source, True)
    assert (ids != M.UNK).mean() > 0.3 and int(tcnt.sum()) == int((ids != M.UNK).sum()) and m.last_tokens == len(ids)
    kid, ksc, kcn, kn = m.keywords(source, True, 5)
    assert kn.max() == 5 and (ksc[:, 0] >= ksc[:, 1]).all()
    wid, wsc, wn = m.textrank(source, True)
    assert wn.max() == 20 and (wsc[wn > 0, 0] == 1.0).all()
    assert int(m.df(source, True, len(v0)).sum()) == len(tid)
    empty = M.make_batch(s, ("empty", 0, 5))
    assert not m.keywords(empty, True, 5)[3].any() and not m.textrank(empty, True)[2].any() and m.last_tokens == 0


# ---- the second op set: joined text, character offsets and word counts ----------------------------------------
# sha256 of repr(gen_ops(seed, NSTEPS)) as the generator stood before the second op set was added to it
GEN_OPS_SHA256 = {6: "dbb491204aa6d7c0e47d29cbffc113e6ed20584375669a2e5ec25294b5cc13ac",
                  24: "f4bd3acd9e1cb17938a8825cd0331432a8befcef127aae940e204975d26bd9e0",
                  38: "39ec05dccbafa37d6332ac1101168226393eb0ae1ceb7d7ffe78616cba87387d"}


@pytest.mark.parametrize("seed", M.SEEDS)
def test_the_first_op_set_is_what_it_was(seed):
    ops = M.gen_ops(seed, M.NSTEPS)
    assert hashlib.sha256(repr(ops).encode()).hexdigest() == GEN_OPS_SHA256[seed]
    assert all(op[0] in M.OPS for op in ops)


@pytest.mark.parametrize("seed", M.SEEDS2)
def test_seed2_covers_every_transition(seed):
    ops = M.gen_ops2(seed, M.NSTEPS2)
    assert len(ops) == M.NSTEPS2 and ops == M.gen_ops2(seed, M.NSTEPS2)
    c = M.coverage2(ops)
    assert set(c["kinds"]) == set(M.OPS2) and all(v >= 3 for v in c["kinds"].values()), c["kinds"]
    assert sum(1 for op in ops if op[0] == "cut") >= 14
    assert set(c["classes"]) == set(M.CLASSES) and all(v >= 2 for v in c["classes"].values()), c["classes"]
    for name in ("add_then_every_mode", "grow_then_repeat", "tiny_plain_host_after_add", "wc_around_add",
                 "charspans_inplace_on_ctx_arrays", "charspans_reuse_too_small"):
        assert c[name], name
    for k in M.ALL_BATCH_OPS:
        assert c[k + ":large_then_tiny"] and c[k + ":tiny_then_large"], k
    for k in M.NEW_BATCH_OPS:
        assert c[k + ":after_old"], k
    for k in M.BATCH_OPS:
        assert c[k + ":after_new"], k
    assert M.covered2(ops)
    assert sum(1 for op in ops if op[0] == "add_word") == 3
    seps = {x for op in ops if op[0] in ("join", "join_batch") for x in op[-2:]}
    assert seps <= set(JR.SEPS) and {len(x) for x in JR.SEPS} == {0, 1, 3, 8}
    for op in ops:
        assert op[0] in M.OPS2
        if op[0] in M.NEW_BATCH_OPS:
            assert op[1] in M.MODES and not (op[1] == "full" and op[2]) and M.spec_at(op) == op[3]
        if op[0] in ("charspans", "charspans_batch"):
            assert op[-2] in M.UNITS and op[-1] in (True, False)


def test_the_second_condition_is_one():
    """Most seeds miss something of the second set too, and each new condition is missed by some seed."""
    missed = [s for s in range(1, 60) if not M.covered2(M.gen_ops2(s, M.NSTEPS2))]
    assert len(missed) > 20 and not set(missed) & set(M.SEEDS2)
    names = set()
    for s in range(1, 200):
        names |= {k for k, v in M.coverage2(M.gen_ops2(s, M.NSTEPS2)).items() if k not in ("kinds", "classes") and not v}
    assert {"wc_around_add", "charspans_inplace_on_ctx_arrays", "charspans_reuse_too_small"} <= names
    assert {k + ":after_old" for k in M.NEW_BATCH_OPS} | {k + ":after_new" for k in M.BATCH_OPS} <= names


def test_dev_state_follows_the_cutting_calls():
    b = ("tiny", 0, 1)
    ops = [("join", b"", b""), ("cut", "plain", True, "device", b), ("ids", "host"), ("charspans", "rune", True),
           ("wc_read",), ("cut", "plain", True, "host", b), ("cut", "full", False, "device_into", b), ("set_vocab", 1),
           ("wc_batch", "plain", True, b), ("cut", "search", True, "device", b), ("add_word", 0, 5), ("last_stats",)]
    assert M.dev_state(ops) == [None, None, "device", "device", "device", "device", None, "device_into", "device_into",
                                None, "device", None]
    assert M.coverage2(ops)["charspans_inplace_on_ctx_arrays"]
    assert not M.coverage2(ops[:1] + ops[4:])["charspans_inplace_on_ctx_arrays"]


@pytest.mark.parametrize("seed", M.SEEDS2)
def test_size_classes_hold_for_the_second_set(syn, seed):
    s = syn[2]
    top, seen = 0, {}
    for op in M.gen_ops2(seed, M.NSTEPS2):
        if op[0] != "cut" and op[0] not in M.ALL_BATCH_OPS:
            continue
        sp = M.spec_at(op)
        b = seen.get(sp) or M.make_batch(s, sp)
        cls = sp[0]
        assert b.nbytes <= M.MAX_BYTES and len(b.buf) == int(b.off[-1]) + 64 and not b.buf[int(b.off[-1]):].any()
        if cls == "tiny":
            assert 0 < b.nbytes <= M.SMALL_MAX and b.ndocs <= M.SMALL_MAX
        elif cls == "small":
            assert 6 << 10 <= b.nbytes <= 60 << 10
        elif cls == "grow" and sp not in seen:
            assert b.nbytes > top, (sp, b.nbytes, top)
        elif cls == "large":
            assert b.nbytes > 64 << 10
        elif cls == "manydocs":
            assert b.ndocs > M.WORK_MIN_DOCS
        elif cls == "empty":
            assert b.nbytes == 0 and b.ndocs > 0
        elif cls == "offset":
            assert int(b.off[0]) > 0 and b.nbytes > M.SMALL_MAX
        seen[sp] = b
        top = max(top, b.nbytes)


def fits(m, sizes):
    """The condition on a table: at most a quarter of the slots and half of the pool, from the model alone."""
    nkeys, nbytes = m.wc_size()
    assert 0 < nkeys <= sizes[0] // 4 and nbytes <= sizes[1] // 2, (nkeys, nbytes, sizes)
    assert m.wc_long == 0  # (no key past 255 bytes: every token is counted)


@pytest.mark.parametrize("seed", M.SEEDS2)
def test_no_random_sequence_fills_its_table(syn, seed):
    """The sequence through the model alone: the table the GPU test uses is never what limits it, the reused
    span arrays are too small at least once and a cut is repeated after an in-place charspans."""
    dr = T.dry_20k(syn)
    dr.set_vocab(dr.m.vocab_keys(0))
    for op in M.gen_ops2(seed, M.NSTEPS2):
        dr.run(op)
    fits(dr.m, (M.WC_NSLOTS, M.WC_POOL))
    assert dr.too_small >= 1 and dr.restored >= 1
    assert sum(dr.m.wc.values()) + dr.m.wc_bad == dr.m.wc_tokens > 0


def test_no_script_fills_its_table(syn, mini):
    d, e = mini
    for script, dr, sizes in ((T.script_arenas, T.dry_20k(syn), (M.WC_NSLOTS, M.WC_POOL)),
                              (T.script_regrow, T.dry_text(T.regrow_dict(d), e), (M.WC_NSLOTS, M.WC_POOL)),
                              (T.script_same_shape, T.dry_20k(syn), T.SAME_SHAPE_TABLE),
                              (T.script_wc_life, T.dry_20k(syn), (M.WC_NSLOTS, M.WC_POOL))):
        script(dr)
        fits(dr.m, sizes)


def test_the_regrow_case_is_the_smallest(mini):
    """REGROW_K and REGROW_N: the first chain, and for it the first run of 甲, whose full-mode list is longer than
    the text has bytes."""
    d, e = mini
    first = None
    for k in range(2, T.REGROW_K + 1):
        m = M.Model((F.chain_dict(k) + d).encode(), e)
        for n in range(1, 40):
            b = M.from_texts(("run", k, n), ["甲" * n])
            if len(m.cut(b, "full", False, count=False)[0]) > b.nbytes:
                first = first or (k, n)
                break
    assert first == (T.REGROW_K, T.REGROW_N)


def test_the_model_gives_the_references_hand_cases(mini):
    """Model.join, charspans and wc_batch on the hand-worked cases of test_join_host.py and test_wc_host.py, and
    charspans against Python's own str: a broken model fails here, not on the GPU."""
    import test_join_host as TJ
    import test_wc_host as TW
    d, e = mini
    m = M.Model(d.encode(), e)
    b = M.from_texts(("hand",), TJ.TEXTS)
    for mode, lib_mode in (("plain", "cut"), ("search", "search"), ("full", "full")):
        out, off = m.join(b, mode, False, b" ", b"\n")
        assert out == "".join(h + "\n" for h in TJ.HAND[lib_mode]).encode()
        assert off == np.cumsum([0] + [len(h.encode()) + 1 for h in TJ.HAND[lib_mode]]).tolist()
        assert m.join(b, mode, False, "／".encode(), b"")[0].decode() == "".join(h.replace(" ", "／") for h in TJ.HAND[lib_mode])
        assert m.last_tokens == len(m.cut(b, "plain", False, count=False)[0])
    valid = M.from_texts(("valid",), ["x", TJ.MIXED, "", "a中𠀀b😀é", "这一刹那"])
    for mode in M.MODES:
        s, en, dt = m.cut(valid, mode, False, count=False)
        for unit in M.UNITS:
            cs, ce, tok, un = m.charspans(valid, mode, False, unit)
            assert np.array_equal(tok, dt) and len(cs) == len(s)
            for k in range(valid.ndocs):
                u = bytes(valid.buf[int(valid.off[k]):int(valid.off[k + 1])]).decode()
                u16 = u.encode("utf-16-le")
                assert un[k] == (len(u) if unit == "rune" else len(u16) // 2)
                for t in range(int(dt[k]), int(dt[k + 1])):
                    piece = bytes(valid.buf[int(s[t]):int(en[t])]).decode()
                    assert (u[cs[t]:ce[t]] if unit == "rune" else u16[2 * cs[t]:2 * ce[t]].decode("utf-16-le")) == piece
    for mode, hmm in (("plain", False), ("plain", True), ("search", True), ("full", False)):
        m2 = M.Model(d.encode(), e)
        b2 = M.from_texts(("wc",), TW.TEXTS)
        m2.wc_batch(b2, mode, hmm)
        r = m2.wc_result()
        c = dict(zip(r.keys, r.counts))
        assert c[W.REPL] == 3 and c["上海".encode()] == 3 and c[b"english"] == 2 and c["今天".encode()] == 3
        assert c.get("一刹".encode(), 0) == (0 if mode == "plain" else 2) and r.bad == r.long == 0
        assert sum(r.counts) == r.tokens == len(m2.cut(b2, mode, hmm, count=False)[0])
        assert r.counts == sorted(r.counts, reverse=True)
        m2.wc_batch(b2, mode, hmm)  # (the table is added to)
        assert m2.wc_result().keys == r.keys and m2.wc_result().counts == [2 * x for x in r.counts]
    # a word added between two batches changes the later cut, never the earlier counts
    m3 = M.Model((F.chain_dict(4) + d).encode(), e)
    b3 = M.from_texts(("add",), ["甲" * 5])
    m3.wc_batch(b3, "plain", False)
    before = dict(m3.wc)
    m3.add_word("甲" * 5, 10 ** 6)
    m3.wc_batch(b3, "plain", False)
    assert m3.wc[("甲" * 5).encode()] == 1 and ("甲" * 5).encode() not in before
    assert all(m3.wc[k] == v for k, v in before.items())
