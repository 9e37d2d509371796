"""CPU: the shadow model and the op generator of tests/ctx_model.py, which test_gpu_sequences.py runs against
the library.  The seeds that file uses must contain every transition between calls the sequences exist for;
the model's own rules (the suggested frequency, which added words buildDag can reach) are checked against the
oracle and the hand-worked examples."""
import hashlib
import math
import os
import re

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


# ---- the third op set: MinHash, the caller's filter, postings, search, near-duplicates and collocations ----------
# sha256 of repr(gen_ops2(seed, NSTEPS2)) as the generator stood before the third op set was added beside it
GEN_OPS2_SHA256 = {1308: "40f44ae112f0761c19bd50445d8d275e284e0de5c56d5050e069efb8d4fcd75b",
                   1931: "39196e08b9c46a70043f9ac8281e9517a31bb4a9516ab6b827da2eeebdc57b09",
                   3045: "986182bc17790cd98c0933707823030a39aef6a9fc09d4dc9f7f15855bdff232"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", M.SEEDS2)
def test_the_second_op_set_is_what_it_was(seed):
    ops = M.gen_ops2(seed, M.NSTEPS2)
    assert hashlib.sha256(repr(ops).encode()).hexdigest() == GEN_OPS2_SHA256[seed]
    assert all(op[0] in M.OPS2 for op in ops)


CONDITIONS3 = (["filter_replaced", "stop_set_replaced_under_a_rule", "every_kind_under_a_filter", "filtered_kinds_after_the_clear",
                "search_around_add", "vocab_replaced_under_an_index", "colloc_around_add", "neardup_with_copies",
                "neardup_without"] +
               [k + t for k in M.NEWEST_BATCH_OPS for t in (":large_then_tiny", ":tiny_then_large", ":after_older")] +
               [k + ":after_newest" for k in M.ALL_BATCH_OPS] + ["full_mode_then:" + k for k in M.HANDOVER_OPS])


def test_there_are_seeds():
    assert len(M.SEEDS3) == 3 and len(set(M.SEEDS3)) == 3


@pytest.mark.parametrize("seed", M.SEEDS3)
def test_seed3_covers_every_transition(seed):
    ops = M.gen_ops3(seed, M.NSTEPS3)
    assert len(ops) == M.NSTEPS3 and ops == M.gen_ops3(seed, M.NSTEPS3)
    c = M.coverage3(ops)
    assert set(c) == set(CONDITIONS3) | {"kinds"}  # (every condition the issue lists is one coverage3 reports)
    assert set(c["kinds"]) == set(M.OPS3) and all(v >= 1 for v in c["kinds"].values()), c["kinds"]
    for name in CONDITIONS3:
        assert c[name], name
    assert M.covered3(ops)
    assert sum(1 for op in ops if op[0] == "add_word") == 2  # (each one rebuilds the 20k image)
    for op in ops:
        assert op[0] in M.OPS3
        if op[0] in M.ALL_BATCH_OPS3:
            assert M.spec_at3(op)[0] in M.CLASSES + ("large", "dups", "queries")
        if op[0] in ("minhash_batch", "filter_batch"):
            assert op[1] in M.MODES and not (op[1] == "full" and op[2])
        if op[0] == "search_batch":
            assert op[2][0] == "queries"


def test_the_third_condition_is_one():
    """Many seeds miss something of the third set, none of them is used, and each of its conditions on the order of
    the calls is missed by some seed."""
    missed = [s for s in range(1, 60) if not M.covered3(M.gen_ops3(s, M.NSTEPS3))]
    assert len(missed) > 20 and not set(missed) & set(M.SEEDS3)
    names = set()
    for s in range(1, 400):
        names |= {k for k, v in M.coverage3(M.gen_ops3(s, M.NSTEPS3)).items() if k != "kinds" and not v}
    assert {"vocab_replaced_under_an_index", "search_around_add", "colloc_around_add"} <= names
    assert {"full_mode_then:" + k for k in M.HANDOVER_OPS} <= names
    assert {k + t for k in ("filter_batch", "postings_batch", "search_batch") for t in (":large_then_tiny", ":tiny_then_large")} <= names
    # a sequence without its filter's clear, and one whose stop set stays, miss theirs
    ops = M.gen_ops3(M.SEEDS3[0], M.NSTEPS3)
    assert not M.covered3([op for op in ops if op[0] != "clear_filter"])
    assert not M.coverage3([op for op in ops if op != ("set_stop", 1)])["stop_set_replaced_under_a_rule"]
    assert not M.coverage3([op for op in ops if op[0] != "set_filter" or M.RULES[op[1]].stop])["filter_replaced"]
    assert not M.coverage3([op for op in ops if op[0] != "minhash_batch" or op[3][0] != "dups"])["neardup_with_copies"]


def front_options(source):
    """{entry point: whether its front runs the ctx's batch filter}, read from jb_batch.cpp: per extern "C" function
    the third field of the FrontOpts it hands batch_front (a braced list in the call, or `const FrontOpts o{...}`
    before it); a function that goes through batch_chain runs none."""
    parts = re.split(r'^extern "C" \w[\w ]*?\b(jb_\w+)\(', source, flags=re.M)
    out = {}
    for name, body in zip(parts[1::2], parts[2::2]):
        if "batch_chain(" in body:
            out[name] = False
            continue
        m = re.search(r"\bbatch_front\(ctx, who, ordinal, \w+, \w+, \w+, nb, (\{[^{}]*\}|o), \[&\]", body)
        if not m:
            continue
        opts = m.group(1)
        if opts == "o":
            d = re.search(r"const FrontOpts o(\{[^{}]*\});", body)
            assert d, f"{name}: batch_front takes `o`, and no `const FrontOpts o{{...}};` is in sight"
            opts = d.group(1)
        fields = [f.strip() for f in opts[1:-1].split(",")]
        assert len(fields) >= 2 and (len(fields) < 3 or fields[2] in ("true", "false")), f"{name}: FrontOpts {opts}"
        out[name] = len(fields) >= 3 and fields[2] == "true"
    return out


def test_the_filter_table_is_the_sources():
    with open(os.path.join(ROOT, "jieba-go_amd", "csrc", "jb_batch.cpp"), encoding="utf-8") as f:
        found = front_options(f.read())
    assert set(M.ENTRY_POINTS) == set(M.FILTERED) == set(M.ALL_BATCH_OPS3)
    missing = sorted(set(M.ENTRY_POINTS.values()) - set(found))
    assert not missing, f"jb_batch.cpp no longer matches the parser's pattern for {missing}"
    assert {k: found[M.ENTRY_POINTS[k]] for k in M.FILTERED} == M.FILTERED
    # (and the parser tells the two apart on text of its own)
    probe = ('extern "C" int jb_a(jb_ctx* ctx) {\n    return batch_front(ctx, who, ordinal, text, doc_off, ndocs, nb, {mode, hmm, true}, '
             '[&](Front& f) -> int { return 0; });\n}\nextern "C" int jb_b(jb_ctx* ctx) {\n    const FrontOpts o{mode, hmm, false, '
             'nullptr, 0};\n    return batch_front(ctx, who, ordinal, text, doc_off, ndocs, nb, o, [&](Front& f) -> int { return 0; });\n}\n'
             'extern "C" int jb_c(jb_ctx* ctx) {\n    return batch_chain(ctx, who, text, doc_off, ndocs, hmm, 0, [&]() {});\n}\n'
             'extern "C" int jb_d(jb_ctx* ctx) {\n    return batch_front(ctx, who, ordinal, text, doc_off, ndocs, nb, {mode, hmm}, [&](Front& f) '
             '-> int { return 0; });\n}\n')
    assert front_options(probe) == {"jb_a": True, "jb_b": False, "jb_c": False, "jb_d": False}


def test_hand_worked_minhash_under_a_filter(mini):
    """Two documents that differ in one ASCII word: other signatures until a rule drops the class."""
    import minhash_ref as MR
    d, e = mini
    m = M.Model(d.encode(), e)
    b = M.from_texts(("mh",), ["今天天氣很好abc我去上海", "今天天氣很好xyz我去上海"])
    words = ["今天", "天氣", "很", "好", "abc", "我", "去", "上海"]
    s, en, _ = m.cut(b, "plain", True)
    assert [bytes(b.buf[int(x):int(y)]).decode() for x, y in zip(s, en)] == words + [w.replace("abc", "xyz") for w in words]
    sig, dn = m.minhash(b, "plain", True, 2, 16, 1)
    assert dn.tolist() == [7, 7] and not np.array_equal(sig[0], sig[1]) and m.last_tokens == 16
    m.set_filter(M.rule(("alnum",)))
    fsig, fdn = m.minhash(b, "plain", True, 2, 16, 1)
    assert fdn.tolist() == [6, 6] and np.array_equal(fsig[0], fsig[1]) and not np.array_equal(fsig[0], sig[0])
    assert m.last_tokens == 16  # (jb_last_stats describes the cut, not what the filter kept)
    # the same from the seven words alone, one span each
    text, ks, ke = MR.from_keys([w.encode() for w in words if w != "abc"])
    hand, hn = MR.minhash_ref(text, ks, ke, [0, 7], 2, 16, 1)
    assert hn.tolist() == [6] and np.array_equal(hand[0], fsig[0])
    assert m.events == [("filtered", ("mh",), M.rule(("alnum",)), 16, 14)]
    # charspans and the caller's own rule do not see the ctx's filter; a stop rule without a stop set is refused
    assert len(m.charspans(b, "plain", True, "rune")[0]) == 16
    assert m.filter_batch(b, "plain", True, M.rule((), 2))[3].tolist() == [16, 0, 0, 8, 0]
    m.set_filter(M.rule(stop=True))
    m.last_tokens = None
    with pytest.raises(M.ModelError):
        m.join(b, "plain", True, b" ", b"\n")
    assert m.last_tokens == 16  # (the filter step refuses after the cut)
    m.last_tokens = None
    with pytest.raises(M.ModelError):
        m.filter_batch(b, "plain", True, M.rule(stop=True))
    assert m.last_tokens is None  # (jb_cut_batch_filter refuses before it)
    m.set_stop(["上海".encode(), "我".encode()])
    assert m.join(b, "plain", True, b" ", b"\n")[0].decode() == "今天 天氣 很 好 abc 去\n今天 天氣 很 好 xyz 去\n"
    m.set_stop(["去".encode()])
    assert m.join(b, "plain", True, b" ", b"\n")[0].decode() == "今天 天氣 很 好 abc 我 上海\n今天 天氣 很 好 xyz 我 上海\n"
    m.set_filter(None)
    assert np.array_equal(m.minhash(b, "plain", True, 2, 16, 1)[0], sig)


def test_hand_worked_index_and_search(mini):
    """Three documents, five keys, three queries: the lists, the ranks and the scores of the one-term queries by
    the formula in plain floats."""
    d, e = mini
    m = M.Model(d.encode(), e)
    docs = M.from_texts(("ix",), ["上海 上海 今天", "今天天氣很好", "我去上海"])
    m.set_vocab([k.encode() for k in ("上海", "今天", "天氣", "好", "去")])
    q = M.from_texts(("q",), ["上海", "很好", "大學", ""])
    with pytest.raises(M.ModelError):
        m.search(q, True, 2)
    po, pd, pt, dl = m.postings(docs, True, 0)
    assert po.tolist() == [0, 2, 4, 5, 6, 7] and pd.tolist() == [0, 2, 0, 1, 1, 1, 2] and pt.tolist() == [2, 1, 1, 1, 1, 1, 1]
    assert dl.tolist() == [3, 4, 3]  # (the spaces are no tokens)
    ix = m.build_index([M.Batch(("ix0",), docs.buf, docs.off[:3]), M.Batch(("ix1",), docs.buf, docs.off[2:])], True)
    assert ix.post_off.tolist() == po.tolist() and ix.post_doc.tolist() == pd.tolist() and ix.post_tf.tolist() == pt.tolist()
    m.set_index(ix)
    rd, rs, rn = m.search(q, True, 2)
    assert rn.tolist() == [2, 1, 0, 0] and rd.tolist() == [[0, 2], [1, M.UNK], [M.UNK, M.UNK], [M.UNK, M.UNK]]
    avg, k1, b = 10 / 3, 1.2, 0.75
    idf = math.log(1 + (3 - 2 + 0.5) / (2 + 0.5))
    for r, (tf, n) in enumerate(((2, 3), (1, 3))):
        x = float(np.float32(idf)) * (tf * (k1 + 1) / (tf + float(np.float32(k1 * (1 - b + b * n / avg)))))
        assert int(rs[0, r]) == int(x * 2 ** 24)
    assert m.last_tokens == 4  # (the queries' cut: 上海, 很, 好, 大學)
    # AddWord of a query's word: the index stays, the query's tokens move
    m.add_word("很好", 10 ** 6)
    assert m.search(q, True, 2)[2].tolist() == [2, 0, 0, 0]
    m.set_vocab([b"x"])
    with pytest.raises(M.ModelError):  # (five ids against one key)
        m.search(q, True, 2)
    m.set_index(None)
    with pytest.raises(M.ModelError):
        m.search(q, True, 2)


def test_hand_worked_collocations(mini):
    d, e = mini
    m = M.Model(d.encode(), e)
    with pytest.raises(M.ModelError):
        m.colloc_init()
    m.set_vocab([k.encode() for k in ("今天", "天氣", "很", "好")])
    m.colloc_init()
    m.colloc_batch(M.from_texts(("c1",), ["今天天氣很好", "今天天氣"]), True)
    m.colloc_batch(M.from_texts(("c2",), ["天氣很好abc今天"]), True)
    assert m.cl["table"] == {(0, 1): 2, (1, 2): 2, (2, 3): 2} and m.cl["uni"] == [3, 3, 2, 2]
    rows, totals = m.colloc_result("count", 1, float("-inf"))
    assert [r[:3] for r in rows] == [(0, 1, 2), (1, 2, 2), (2, 3, 2)] and totals == (11, 10, 6, 0, 3)
    m.set_filter(M.rule(("alnum",)))  # (with abc gone 好 and 今天 are neighbours)
    m.colloc_batch(M.from_texts(("c2",), ["天氣很好abc今天"]), True)
    assert m.cl["table"] == {(0, 1): 2, (1, 2): 3, (2, 3): 3, (3, 0): 1} and m.cl["uni"] == [4, 4, 3, 3]
    m.colloc_batch(M.from_texts(("c2",), ["天氣很好abc今天"]), True, contig=True)  # (but they do not touch)
    assert m.cl["table"] == {(0, 1): 2, (1, 2): 4, (2, 3): 4, (3, 0): 1}
    m.colloc_batch(M.from_texts(("c1",), ["今天天氣很好", "今天天氣"]), True, keep=np.array([1, 1, 0, 0], np.uint8))
    assert m.cl["table"] == {(0, 1): 4, (1, 2): 4, (2, 3): 4, (3, 0): 1} and m.cl["uni"] == [7, 7, 5, 5]


def test_hand_worked_duplicates(syn):
    """A dups batch: every planted exact copy is a pair with all K slots equal, every pair joins two documents of
    one family (a new document, its copies and its near-copies), and near-copies are found too."""
    d, e, s, source = syn
    m = M.Model(d, e, source=source)
    b = M.make_batch(s, ("dups", 900, 24))
    plan = M.dup_plan(900, 24)
    assert [p[0] for p in plan[:8]] == ["new", "new", "new", "near", "new", "copy", "new", "near"] and b.ndocs == 24
    o = [int(x) for x in b.off]
    doc = [bytes(b.buf[o[k]:o[k + 1]]) for k in range(24)]
    family = [k if p[0] == "new" else p[1] for k, p in enumerate(plan)]
    for k, (kind, src, _) in enumerate(plan):
        assert (doc[k] == doc[src]) == (kind == "copy") if kind != "new" else doc.index(doc[k]) == k
    sig, dn = m.minhash(b, "plain", True, 5, 128, 1)
    po, pd, pa, stat = m.neardup(sig, dn, 32, 4, 64, 64)
    pairs = {(int(pd[k]), j): int(pa[k]) for j in range(24) for k in range(int(po[j]), int(po[j + 1]))}
    assert len(pairs) >= 3 and int(stat[2]) == 0 and all(family[i] == family[j] and i < j for i, j in pairs)
    copies = {(src, j) for j, (kind, src, _) in enumerate(plan) if kind == "copy"}
    assert copies and all(pairs.get(p) == 128 for p in copies)
    near = [(src, j) for j, (kind, src, _) in enumerate(plan) if kind == "near"]
    assert sum(1 for p in near if 64 <= pairs.get(p, 0) < 128) >= len(near) // 2


# ---- the conditions the inputs of the GPU tests must meet, from the references alone -------------------------------
# The batches that cannot meet a condition below, by their exact specification: a rule cannot both keep and drop
# a token of a document of one token or of none, and the arena script searches with the four batches the other
# kinds use, not with queries; the one-query step of the shrinking calls has one answer only.
ONE_TOKEN = {("one",)}
NOT_QUERIES = {("large", 1700, T.LARGE3), ("tail",), ("one",), ("empty", 0, 5), ("oneq",)}


def inputs_hold(dr, sizes=(M.WC_NSLOTS, M.WC_POOL), wc=True, refusals=()):
    m = dr.m
    if wc:
        fits(m, sizes)
    if m.cl is not None:
        assert len(m.cl["table"]) <= M.COLLOC_NSLOTS // 4
    for _, spec, r, ntok, kept in m.events:  # every rule keeps a token and drops one
        assert 0 < kept < ntok or spec in ONE_TOKEN or (spec[0] == "empty" and ntok == 0), (spec, r, ntok, kept)
    assert any(ntok > 100 for _, _, _, ntok, _ in m.events)
    for entry in dr.log:
        if entry[0] == "neardup":
            assert entry[3] == 0, entry  # (no bucket over the window)
            assert not entry[1] or entry[2] >= 3, entry
        elif entry[0] == "search":  # (a query with documents, a query without)
            assert (entry[2] > 0 and entry[3] > 0) or entry[1] in NOT_QUERIES, entry
    assert sorted(e[1] for e in dr.log if e[0] == "refused") == sorted(refusals)


@pytest.mark.parametrize("seed", M.SEEDS3)
def test_the_third_sequences_inputs(syn, seed):
    """The sequence through the model alone: its tables are never what limits it, every rule keeps and drops, every
    answered search has a query with a hit and one without, a join on a dups batch finds pairs, and the searches
    the model refuses are the ones coverage3 counts on."""
    dr = T.dry_20k(syn)
    dr.set_vocab(dr.m.vocab_keys(0))
    ops = M.gen_ops3(seed, M.NSTEPS3)
    answered, other_count = [], 0
    for op in ops:
        n = len(dr.log)
        dr.run(op)
        if any(e[0] == "refused" for e in dr.log[n:]):
            # (refused for an index of another id count, which coverage3 takes every set_vocab to bring about)
            other_count += dr.m.index is not None and dr.m.index.nids != len(dr.m.keys)
        else:
            answered.append(op)
    refused = [e[1] for e in dr.log if e[0] == "refused"]
    assert set(refused) == {"search_batch"} and len(refused) == len(ops) - len(answered) and other_count >= 1
    # a refused search returns before it touches an arena: without them the sequence still covers everything but
    # the condition that asks for a refused search
    c = M.coverage3(answered)
    assert all(v >= 1 for v in c["kinds"].values())
    assert [k for k, v in c.items() if k != "kinds" and not v] == ["vocab_replaced_under_an_index"]
    inputs_hold(dr, refusals=refused)
    assert any(e[0] == "neardup" and e[1] and e[2] >= 3 for e in dr.log) and any(e[0] == "neardup" and not e[1] for e in dr.log)
    top, seen = 0, {}
    for op in ops:  # the size classes hold for the real batches
        if op[0] != "cut" and op[0] not in M.ALL_BATCH_OPS3:
            continue
        sp = M.spec_at3(op)
        b = dr.batches[sp]
        assert (b.nbytes > M.SMALL_MAX) == M.large3(sp) or sp[0] == "manydocs", sp
        if op[0] in M.NEWEST_BATCH_OPS:
            assert (24 << 10 <= b.nbytes <= 48 << 10 or not M.large3(sp)) and b.ndocs <= M.SMALL_MAX, (sp, b.nbytes)
        if sp[0] == "dups":
            assert b.ndocs <= 64
        if sp[0] == "queries":
            assert b.ndocs == sp[2] + 2 or sp[2] <= 8
        if sp[0] == "grow" and sp not in seen:
            assert b.nbytes > top
        seen[sp] = b
        top = max(top, b.nbytes)


def test_the_newest_scripts_inputs(syn, mini):
    d, e = mini
    for script, dr, wc, refusals in (
            (T.script_arenas3, T.dry_20k(syn), True, ()),
            (T.script_same_shape3, T.dry_20k(syn), False, ()),
            (T.script_errors, T.dry_20k(syn), True, ["minhash_batch", "colloc_batch"] * 2),
            (T.script_filter_life, T.dry_text(T.regrow_dict(d), e), True, ()),
            (T.script_index_life, T.dry_20k(syn), False, ["search_batch"] * 4),
            (T.script_colloc_dedup, T.dry_20k(syn), False, ())):
        script(dr)
        inputs_hold(dr, wc=wc, refusals=refusals)
