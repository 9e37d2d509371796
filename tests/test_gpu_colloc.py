"""GPU: collocations (jb_colloc_init_device, jb_colloc_add_device, jb_colloc_score_device, jb_colloc_read,
jb_colloc_batch; jb_colloc.hip) against jb_colloc_count and jb_colloc_score, the host form of the rule (which
tests/test_colloc_host.py pins to colloc_ref.py), on the inputs of colloc_cases.py, exactly, in both forms of the
count pass (JB_COLLOC_COMBINE, read at jb_open: one tokenizer per form).  The table, d_uni, the work buffer and the
candidate arrays sit between canaries that must not change, and the input arrays start off a 16-byte boundary."""
import os
import struct
import subprocess

import numpy as np
import pytest

import colloc_cases as CC
import colloc_ref as CR
import jiebahip as J
import oracle as O
import search_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [0, 1]  # JB_COLLOC_COMBINE
NG = 64  # canary bytes on each side of every guarded buffer
FILL = 0x33
CASES = list(CC.all_cases())
SCORES = list(CC.score_cases())
SCORERS = (J.JB_COLLOC_NPMI, J.JB_COLLOC_RATIO, J.JB_COLLOC_COUNT)
NINF = float("-inf")
_WANT = {}


@pytest.fixture(scope="module")
def forms(mini_paths):
    """{form: a tokenizer opened with JB_COLLOC_COMBINE=form} (the knob is read at jb_open)."""
    old = os.environ.get("JB_COLLOC_COMBINE")
    tks = {}
    try:
        for f in FORMS:
            os.environ["JB_COLLOC_COMBINE"] = str(f)
            tks[f] = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    finally:
        if old is None:
            os.environ.pop("JB_COLLOC_COMBINE", None)
        else:
            os.environ["JB_COLLOC_COMBINE"] = old
    yield tks
    for tk in tks.values():
        tk.close()


def want_of(c):
    """The host rule over a case's batches without a slot limit, computed once: (pairs dict, uni list, totals)."""
    if c["label"] not in _WANT:
        uni = np.zeros(c["nuni"], np.uint64)
        table, tot = {}, [0, 0, 0]
        for b in c["batches"]:
            r = J.colloc_count(b["ids"], b["doc_tok"], uni, c["keep"], c["flags"], b["starts"], b["ends"], b["ntok"],
                               b["ids_cap"])
            for a, bb, n in zip(r.a.tolist(), r.b.tolist(), r.count.tolist()):
                table[(a, bb)] = table.get((a, bb), 0) + n
            tot = [x + y for x, y in zip(tot, (r.tokens, r.known, r.pairs))]
        _WANT[c["label"]] = (table, uni.tolist(), tot)
    return _WANT[c["label"]]


def guarded(nbytes, fill=FILL):
    """A device buffer of nbytes between canaries: (tensor, pointer to the payload, 64-byte aligned)."""
    import torch
    pad = (-nbytes) % 8
    t = torch.full((nbytes + pad + 2 * NG,), fill, dtype=torch.uint8, device="cuda")
    t[:NG] = 0x7A
    t[NG + nbytes:] = 0x7A
    assert (t.data_ptr() + NG) % 64 == 0
    return t, t.data_ptr() + NG


def payload(t, nbytes, what):
    b = t.cpu().numpy()
    assert (b[:NG] == 0x7A).all() and (b[NG + nbytes:] == 0x7A).all(), "written outside " + what
    return b[NG:NG + nbytes]


def _up(a, shift):
    """An allocation of exactly the array's entries behind `shift` entries of its type: the array starts `shift`
    entries after a 16-byte boundary."""
    import torch
    flat = np.ascontiguousarray(a).reshape(-1)
    held = np.concatenate([np.full(shift, 3, flat.dtype), flat])
    t = torch.from_numpy((held if len(held) else np.zeros(1, flat.dtype)).view(np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift * flat.itemsize


class Table:
    """A pair table and d_uni on the device between canaries."""

    def __init__(self, tk, nslots, nuni, init=True):
        self.tk, self.nslots, self.nuni = tk, nslots, nuni
        self.ntable = J.colloc_table_bytes(nslots)
        self.t, self.p = guarded(self.ntable)
        self.u, self.pu = guarded(nuni * 8)
        if init:
            tk.colloc_init_device(self.p, self.ntable, nslots, self.pu, nuni)

    def add(self, c, b, shift=1, work=None, expect_error=None):
        import torch
        cap = b["ids_cap"]
        held = []

        def up(a, s=shift):
            if a is None:
                return 0
            t, p = _up(a, s)
            held.append(t)
            return p

        p_ids = up(b["ids"][:cap]) if cap else 0
        p_dt, p_nt = up(b["doc_tok"]), up(np.array([b["ntok"]], np.uint64))
        p_keep = up(c["keep"]) if c["keep"] is not None else 0
        p_s = up(None if b["starts"] is None else b["starts"][:cap])
        p_e = up(None if b["ends"] is None else b["ends"][:cap])
        need = J.colloc_work_bytes(cap, len(b["doc_tok"]) - 1)
        wk, p_wk = guarded(need, 0x5B)
        wmiss, wmis = work or (0, 0)
        args = (self.p, self.ntable, self.pu, self.nuni, p_ids, cap, p_dt, p_nt, len(b["doc_tok"]) - 1, p_keep,
                0 if c["keep"] is None else len(c["keep"]), c["flags"], p_s, p_e, p_wk + wmis, need - wmiss,
                torch.cuda.current_stream().cuda_stream)
        if expect_error is not None:
            before = self.raw()
            with pytest.raises(J.JbError) as ei:
                self.tk.colloc_add_device(*args)
            assert ei.value.code == expect_error
            torch.cuda.synchronize()  # nothing was queued
            assert (payload(wk, need, "the work buffer") == 0x5B).all() and self.raw() == before
            return
        self.tk.colloc_add_device(*args)
        torch.cuda.synchronize()
        payload(wk, need, "the work buffer")
        del held

    def raw(self):
        return payload(self.t, self.ntable, "the table").tobytes(), payload(self.u, self.nuni * 8, "d_uni").tobytes()

    def uni(self):
        return payload(self.u, self.nuni * 8, "d_uni").copy().view(np.uint64).tolist()

    def read(self, scorer=J.JB_COLLOC_COUNT, m=1, thr=NINF, topn=0, nuni=None):
        r = self.tk.colloc_read(self.p, self.ntable, self.pu, self.nuni if nuni is None else nuni, scorer, m, thr, topn)
        self.raw()  # (the canaries)
        return r

    def dump(self):
        """The table's contents: (pairs dict, totals), from the sorted read under COUNT."""
        r = self.read()
        keys = list(zip(r.a.tolist(), r.b.tolist()))
        order = sorted(range(len(keys)), key=lambda i: (-int(r.count[i]), keys[i]))
        assert order == list(range(len(keys))) and len(set(keys)) == len(keys), "the rule's order, each key once"
        assert r.score.tolist() == [float(np.float32(x)) for x in r.count.tolist()]
        return dict(zip(keys, r.count.tolist())), r.totals()


def run_case(tk, c, shift=1):
    tb = Table(tk, c["nslots"], c["nuni"])
    for b in c["batches"]:
        tb.add(c, b, shift)
    return tb


def check_case(tb, c, label):
    wt, wu, (wtok, wknown, wpairs) = want_of(c)
    got, (tokens, known, pairs, dropped, distinct) = tb.dump()
    assert (tokens, known, pairs) == (wtok, wknown, wpairs), f"{label}: totals {(tokens, known, pairs)}"
    assert tb.uni() == wu, f"{label}: uni differs"
    assert sum(got.values()) + dropped == pairs and sum(wu) == known, f"{label}: the identity"
    assert distinct == len(got)
    if c["drops"]:
        # which keys survive is not determined: every key present has its exact count, and the table filled
        assert dropped > 0 and distinct >= c["nslots"] // 2
        assert all(wt[k] == n for k, n in got.items()), f"{label}: a key in the table has another count"
        assert dropped == sum(n for k, n in wt.items() if k not in got)
    else:
        assert dropped == 0 and got == wt, f"{label}: pairs differ"
    return got, known


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_cases(forms, c, form):
    tb = run_case(forms[form], c)
    got, known = check_case(tb, c, c["label"])
    # the candidates of the three scorers: the device's score pass against the host rule over the same table
    a = np.array([k[0] for k in got], np.uint32)
    b = np.array([k[1] for k in got], np.uint32)
    n = np.array(list(got.values()), np.uint64)
    uni = np.array(tb.uni(), np.uint64)
    for scorer, m, thr in ((J.JB_COLLOC_NPMI, 1, NINF), (J.JB_COLLOC_NPMI, 2, 0.25), (J.JB_COLLOC_RATIO, 2, 1.0),
                           (J.JB_COLLOC_COUNT, 3, 4.0)):
        want = J.colloc_score(a, b, n, uni, known, scorer, m, thr)
        r = tb.read(scorer, m, thr)
        for x, y, name in ((r.a, want.a, "a"), (r.b, want.b, "b"), (r.count, want.count, "count"), (r.score, want.score, "score")):
            assert x.tobytes() == y.tobytes(), f"{c['label']}: scorer {scorer}: {name} differs"
        top = tb.read(scorer, m, thr, topn=3)
        assert top.a.tolist() == want.a[:3].tolist() and top.score.tobytes() == want.score[:3].tobytes()


def test_forms_and_runs_are_identical(forms):
    by = {c["label"]: c for c in CASES}
    for label in ("zipf", "eviction", "two batches"):
        dumps = []
        for form in FORMS:
            for _ in range(2):
                tb = run_case(forms[form], by[label])
                dumps.append((tb.dump(), tb.uni()))
        assert all(d == dumps[0] for d in dumps[1:]), label


def test_alignment(forms):
    by = {c["label"]: c for c in CASES}
    for label in ("contiguous over gaps and overlaps", "nkeep below nuni"):
        for shift in (0, 2, 3):
            check_case(run_case(forms[1], by[label], shift), by[label], f"{label} shift={shift}")


def test_refused_calls_and_no_table(forms):
    import torch
    by = {c["label"]: c for c in CASES}
    c = by["zipf"]
    b = c["batches"][0]
    tk = forms[1]
    tb = Table(tk, c["nslots"], c["nuni"])
    tb.add(c, b, work=(1, 0), expect_error=J.JB_EINVAL)
    tb.add(c, b, work=(0, 2), expect_error=J.JB_EINVAL)
    tb.add(dict(c, flags=2), b, expect_error=J.JB_EINVAL)
    tb.add(dict(c, flags=J.JB_COLLOC_CONTIG), b, expect_error=J.JB_EINVAL)  # the flag without spans
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(J.JbError) as ei:  # (the limit is checked before anything is read)
        tk.colloc_add_device(tb.p, tb.ntable, tb.pu, tb.nuni, tb.pu, (1 << 32) - J.JB_COLLOC_TILE, tb.pu, tb.pu, 0, 0, 0, 0,
                             0, 0, tb.pu, 1 << 40, st)
    assert ei.value.code == J.JB_ELIMIT
    for args in ((tb.p + 8, tb.ntable, tb.pu, tb.nuni), (tb.p, 100, tb.pu, tb.nuni), (tb.p, tb.ntable, tb.pu + 4, tb.nuni),
                 (0, tb.ntable, tb.pu, tb.nuni), (tb.p, tb.ntable, 0, tb.nuni)):
        with pytest.raises(J.JbError) as ei:
            tk.colloc_add_device(*args, tb.pu, 0, tb.pu, tb.pu, 0, 0, 0, 0, 0, 0, 0, 0, st)
        assert ei.value.code == J.JB_EINVAL
    for nslots, code in ((12, J.JB_EINVAL), (4, J.JB_EINVAL), (1 << 31, J.JB_ELIMIT), (c["nslots"] * 2, J.JB_EINVAL)):
        with pytest.raises(J.JbError) as ei:
            tk.colloc_init_device(tb.p, tb.ntable, nslots, tb.pu, tb.nuni)
        assert ei.value.code == code
    for kw in (dict(scorer=3), dict(m=0)):
        with pytest.raises(J.JbError) as ei:
            tb.read(**kw)
        assert ei.value.code == J.JB_EINVAL
    # a buffer that holds no table: the add leaves it, d_uni and the work buffer untouched, and the read says so
    for form in FORMS:
        no = Table(forms[form], c["nslots"], c["nuni"], init=False)
        before = no.raw()
        cap = b["ids_cap"]
        held = [_up(b["ids"], 1), _up(b["doc_tok"], 1), _up(np.array([cap], np.uint64), 0)]
        need = J.colloc_work_bytes(cap, len(b["doc_tok"]) - 1)
        wk, p_wk = guarded(need, 0x5B)
        forms[form].colloc_add_device(no.p, no.ntable, no.pu, no.nuni, held[0][1], cap, held[1][1], held[2][1],
                                      len(b["doc_tok"]) - 1, 0, 0, 0, 0, 0, p_wk, need, st)
        torch.cuda.synchronize()
        assert no.raw() == before and (payload(wk, need, "the work buffer") == 0x5B).all()
        with pytest.raises(J.JbError) as ei:
            no.read()
        assert ei.value.code == J.JB_EINVAL
        dn, p_dn = guarded(8)
        forms[form].colloc_score_device(no.p, no.ntable, no.pu, no.nuni, "count", 1, NINF, 0, 0, 0, 0, 0, p_dn, st)
        torch.cuda.synchronize()
        assert payload(dn, 8, "ncand").tobytes() == bytes(8) and no.raw() == before
    tb.add(c, b)  # the refused calls left the table usable
    check_case(tb, c, "after the refusals")


def test_candidate_capacity(forms):
    import torch
    c = {x["label"]: x for x in CASES}["zipf"]
    tk = forms[1]
    tb = run_case(tk, c)
    full = tb.read(J.JB_COLLOC_NPMI, 1, NINF)
    members = set(zip(full.a.tolist(), full.b.tolist(), full.count.tolist(), full.score.tolist()))
    n = len(full)
    assert n > 40
    st = torch.cuda.current_stream().cuda_stream
    for ccap in (0, 1, 7, n - 1, n, n + 9):
        before = tb.raw()
        ca, p_a = guarded(ccap * 4)
        cb, p_b = guarded(ccap * 4)
        cc, p_c = guarded(ccap * 8)
        cs, p_s = guarded(ccap * 4)
        dn, p_n = guarded(8)
        tk.colloc_score_device(tb.p, tb.ntable, tb.pu, tb.nuni, "npmi", 1, NINF, p_a, p_b, p_c, p_s, ccap, p_n, st)
        torch.cuda.synchronize()
        assert tb.raw() == before
        assert struct.unpack("<Q", payload(dn, 8, "ncand").tobytes())[0] == n, "ncand counts the complete set"
        w = min(n, ccap)
        a = payload(ca, ccap * 4, "cand_a")
        b = payload(cb, ccap * 4, "cand_b")
        k = payload(cc, ccap * 8, "cand_cnt")
        s = payload(cs, ccap * 4, "cand_score")
        for arr, size in ((a, 4), (b, 4), (k, 8), (s, 4)):
            assert (arr[w * size:] == FILL).all(), "an entry at or past the count or ccap was written"
        got = list(zip(a[:w * 4].copy().view(np.uint32).tolist(), b[:w * 4].copy().view(np.uint32).tolist(),
                       k[:w * 8].copy().view(np.uint64).tolist(), s[:w * 4].copy().view(np.float32).tolist()))
        assert len(set(got)) == w and set(got) <= members, f"ccap={ccap}: distinct members of the candidate set"


# ---- hand-made tables ------------------------------------------------------------------------------------------------
def _home(key, mask):
    """jb_cl_home (jb_colloc.h): splitmix64's finalizer."""
    m64 = (1 << 64) - 1
    x = (key + 0x9E3779B97F4A7C15) & m64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m64
    return (x ^ (x >> 31)) & mask


def table_image(rows, nslots, known):
    """A table's bytes as jb_colloc.h lays them out, holding rows of (a, b, count) with N = known."""
    keys = np.full(nslots, (1 << 64) - 1, np.uint64)
    cnt = np.zeros(nslots, np.uint64)
    for a, b, n in rows:
        key = (int(a) << 32) | int(b)
        s = _home(key, nslots - 1)
        while int(keys[s]) != (1 << 64) - 1:
            s = (s + 1) & (nslots - 1)
        keys[s], cnt[s] = key, n
    hdr = struct.pack("<7Q", 0x31544C43424A, nslots, 0, known, 0, 0, len(rows)).ljust(256, b"\0")
    return hdr + keys.tobytes() + cnt.tobytes()


@pytest.mark.parametrize("c", SCORES, ids=[c["label"] for c in SCORES])
def test_score_cases(forms, c):
    import torch
    tk = forms[0]
    rows = list(zip(c["a"].tolist(), c["b"].tolist(), c["count"].tolist()))
    tb = Table(tk, 64, len(c["uni"]), init=False)
    img = np.frombuffer(table_image(rows, 64, c["N"]), np.uint8)
    tb.t[NG:NG + len(img)] = torch.from_numpy(img.copy()).cuda()
    tb.u[NG:NG + len(c["uni"]) * 8] = torch.from_numpy(c["uni"].view(np.uint8).copy()).cuda()
    for scorer in SCORERS:
        full = J.colloc_score(c["a"], c["b"], c["count"], c["uni"], c["N"], scorer, c["m"], NINF, nuni=c["nuni"])
        thresholds = [float("nan"), float("inf"), 0.0, NINF]
        for s in full.score:  # at a pair's f32 score and one ulp above it
            thresholds += [float(s), float(np.nextafter(s, np.float32(np.inf)))]
        for thr in thresholds:
            want = J.colloc_score(c["a"], c["b"], c["count"], c["uni"], c["N"], scorer, c["m"], thr, nuni=c["nuni"])
            r = tb.read(scorer, c["m"], thr, nuni=c["nuni"])
            assert (r.a.tobytes(), r.b.tobytes(), r.count.tobytes(), r.score.tobytes()) == (
                want.a.tobytes(), want.b.tobytes(), want.count.tobytes(), want.score.tobytes()), (scorer, thr)
            assert r.known == c["N"] and r.distinct == len(rows)


# ---- the mini dictionary, end to end ---------------------------------------------------------------------------------
TEXTS = ["我昨天去上海交通大學", "今天天氣很好，我去上海", "这一刹那的上海 abc abc", "", "我去上海，我去上海，我昨天去上海",
         "今天很好 今天很好 abc 2024", "上海交通大學與老師討論量子力學"]


def _ids_of(tk, keys, texts, hmm):
    """Cut's tokens as ids under `keys`, with their byte spans: (ids, doc_tok, starts, ends)."""
    index = {k: i for i, k in enumerate(keys)}
    ids, starts, ends, dt = [], [], [], [0]
    base = 0
    for t in texts:
        bt = t.encode("utf-8")
        s, e = tk.cut_spans(t, hmm)
        for x, y in zip(s.tolist(), e.tolist()):
            ids.append(index.get(bt[x:y], J.JB_ID_UNK))
            starts.append(base + x)
            ends.append(base + y)
        base += len(bt)
        dt.append(len(ids))
    return np.array(ids, np.uint32), np.array(dt, np.uint64), np.array(starts, np.uint32), np.array(ends, np.uint32)


def test_collocations_on_texts(forms):
    for form in FORMS:
        tk = forms[form]
        keys, _ = tk.fit_vocab([TEXTS], hmm=True, nslots=1 << 12, pool_bytes=1 << 12)
        ids, dt, st, en = _ids_of(tk, keys, TEXTS, True)
        for contiguous in (False, True):
            table, uni, tot = CR.count(ids, dt, len(keys), None, int(contiguous), st, en)
            for scorer, m, thr in (("npmi", 2, 0.1), ("ratio", 1, 0.0), ("count", 1, 1.0)):
                want = CR.score([(a, b, n) for (a, b), n in table.items()], uni, len(keys), tot["known"],
                                J._SCORERS[scorer], m, thr)
                got = tk.collocations([TEXTS[:3], [], TEXTS[3:]], scorer, m, thr, contiguous=contiguous, nslots=1 << 10)
                assert got == [(keys[a], keys[b], n, float(s)) for a, b, n, s in want], (form, contiguous, scorer)
                assert got, "the texts have collocations"
        assert tk.collocations([TEXTS], "count", 1, 1.0, topn=2, contiguous=True, nslots=1 << 10) == got[:2]
        with pytest.raises(J.JbError) as ei:  # a table too small drops pairs: the convenience call refuses
            tk.collocations([TEXTS], "count", 1, 1.0, nslots=8)
        assert ei.value.code == J.JB_ELIMIT
        tk.set_vocab(None)
        with pytest.raises(J.JbError) as ei:
            tk.collocations([TEXTS])
        assert ei.value.code == J.JB_EINVAL


def test_find_new_words(mini_paths):
    o = O.Oracle.from_files(mini_paths[0], mini_paths[1], 0)
    tk = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    try:
        runes = "海力學師通氣"
        word = next(x + y for x in runes for y in runes
                    if x != y and not tk.dict_get(x + y) and o.cut(x + y, False) == [x, y])
        filler = ["abc ", "我去上海，", "今天很好 ", "2024 ", "我 ", "去 ", "上海 "]
        text = "".join(word + filler[i % len(filler)] for i in range(20))
        batches = [[text, "我昨天去上海"], [text[:0], "这一刹那"]]
        assert word not in tk.Cut(text, False)
        tk.fit_vocab(batches, hmm=False, nslots=1 << 12, pool_bytes=1 << 12)
        found = tk.find_new_words(batches, "npmi", 5, 0.5, nslots=1 << 10)
        assert found and found[0] == word, found
        assert tk.find_new_words(batches, "npmi", 5, 0.5, topn=1, nslots=1 << 10) == [word]
        tk.AddWord(word, 0)
        assert tk.Cut(text, False).count(word) == 20
        tk.fit_vocab(batches, hmm=False, nslots=1 << 12, pool_bytes=1 << 12)
        assert word not in tk.find_new_words(batches, "npmi", 5, 0.5, nslots=1 << 10)
    finally:
        tk.close()


def test_colloc_batch_with_a_batch_filter(forms):
    tk = forms[1]
    keys, _ = tk.fit_vocab([TEXTS], hmm=True, nslots=1 << 12, pool_bytes=1 << 12)
    ids, dt, st, en = _ids_of(tk, keys, TEXTS, True)
    buf, off = R.batch_of(TEXTS)
    tk.set_batch_filter(drop=("other", "invalid", "alnum", "num"))
    try:
        # the filtered list: the tokens whose every rune is Han, with their spans
        han = np.array([J.is_han_key(keys[i]) if i != J.JB_ID_UNK else False for i in ids.tolist()])
        fdt = np.array([int(han[:int(x)].sum()) for x in dt], np.uint64)
        for flags in (0, J.JB_COLLOC_CONTIG):
            uni = np.zeros(len(keys), np.uint64)
            want = J.colloc_count(ids[han], fdt, uni, None, flags, st[han], en[han])
            tb = Table(tk, 1 << 10, len(keys))
            tk.colloc_batch(buf, off, True, tb.p, tb.ntable, tb.pu, tb.nuni, None, flags)
            got, totals = tb.dump()
            assert got == dict(zip(zip(want.a.tolist(), want.b.tolist()), want.count.tolist())) and tb.uni() == uni.tolist()
            assert totals == want.totals()
        a = J.colloc_count(ids[han], fdt, np.zeros(len(keys), np.uint64), None, 0, st[han], en[han]).pairs
        assert want.pairs < a, "a pair across a filtered-out token does not count under JB_COLLOC_CONTIG"
    finally:
        tk.clear_batch_filter()
    with pytest.raises(J.JbError) as ei:
        tk.colloc_batch(buf, np.array([0, 5, 3], np.uint64), True, tb.p, tb.ntable, tb.pu, tb.nuni)
    assert ei.value.code == J.JB_EINVAL
    tk.set_vocab(None)
    with pytest.raises(J.JbError) as ei:
        tk.colloc_batch(buf, off, True, tb.p, tb.ntable, tb.pu, tb.nuni)
    assert ei.value.code == J.JB_EINVAL


def test_profile_lists_the_kernels(forms):
    by = {c["label"]: c for c in CASES}
    tk = forms[1]
    tk.profile(True)
    try:
        for label in ("documents of 1 and 2 tokens", "zipf"):  # the launches do not depend on the data
            tk.profile_reset()
            tb = run_case(tk, by[label])
            tb.read()
            prof = tk.profile_read()
            for k in ("k_cl_zero", "k_cl_bounds", "k_cl_claim", "k_cl_count", "k_cl_score"):
                assert prof[k][1] == 1, k
    finally:
        tk.profile(False)


def test_c_and_cpp_consumers(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "c_abi_colloc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_colloc.c"), "-L", lib,
                           "-ljiebahip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "colloc ok" in r.stdout, r.stdout + r.stderr
    exe = str(tmp_path / "cpp_colloc_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_colloc_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "colloc ok" in r.stdout, r.stdout + r.stderr
