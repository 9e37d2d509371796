"""GPU: word counts (jb_wc_init_device, jb_wc_add_device, jb_wc_read, jb_wc_batch; jb_wc.hip) against
jb_wc_count, the host form of the rule, and against wc_ref.py: keys, counts, order and the five totals,
exactly.  Most tests hand the kernels spans they built themselves, so the table is checked independently of
segmentation, in both forms of the count pass (JB_WC_COMBINE, read at jb_open: one tokenizer per form).  The
table, the span arrays' neighbours and the work buffer lie between canaries that must not change."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import full_ref as F
import jiebahip as J
import oracle as O
import search_ref as R
import synth
import wc_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [0, 1]  # JB_WC_COMBINE
T = 256  # tokens per workgroup and trip of the three passes (kWcTile)
NG = 64  # canary bytes on each side of the table and of the work buffer
MODES = [("cut", False), ("cut", True), ("search", False), ("search", True), ("full", False)]
MIXED = "english번역『하다』今天天氣很好，ステーションabc1231+1=2我昨天去上海*important*去"  # (test_gpu_ids.MIXED)
INVALID = b"\xff\xfe" + "中文".encode() + b"\x80abc\xe4\xb8"
TEXTS = [MIXED, INVALID, "这一刹那", MIXED, "今天天氣很好", "", "这一刹那的上海"]


def _open_forms(dp, ep, bits=None):
    old = {k: os.environ.get(k) for k in ("JB_WC_COMBINE", "JB_WC_HASHBITS")}
    tks = {}
    try:
        if bits is not None:
            os.environ["JB_WC_HASHBITS"] = str(bits)
        for f in FORMS:
            os.environ["JB_WC_COMBINE"] = str(f)
            tks[f] = J.Tokenizer(J.make_config(dict_path=dp, emit_path=ep))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return tks


@pytest.fixture(scope="module")
def forms(mini_paths):
    """{form: a tokenizer opened with JB_WC_COMBINE=form} (the knob is read at jb_open)."""
    tks = _open_forms(*mini_paths)
    yield tks
    for tk in tks.values():
        tk.close()


@pytest.fixture(scope="module")
def forms4(mini_paths):
    """The same with JB_WC_HASHBITS=4: 15 fingerprints, so keys collide at will."""
    tks = _open_forms(*mini_paths, bits=4)
    yield tks
    for tk in tks.values():
        tk.close()


@pytest.fixture(scope="module")
def syn_forms(syn_small):
    tks = _open_forms(syn_small[0], syn_small[1])
    yield tks
    for tk in tks.values():
        tk.close()


class Table:
    """A word-count table in device memory between canaries, and what the tests do to it."""

    def __init__(self, tk, nslots=1024, pool_bytes=4096, init=True):
        import torch
        self.tk, self.n = tk, J.wc_table_bytes(nslots, pool_bytes)
        self.buf = torch.full((self.n + 2 * NG,), 0x11, dtype=torch.uint8, device="cuda")
        self.buf[:NG] = 0x7A
        self.buf[NG + self.n:] = 0x7A
        self.ptr = self.buf.data_ptr() + NG
        assert self.ptr % 32 == 0
        self.st = torch.cuda.current_stream().cuda_stream
        if init:
            tk.wc_init_device(self.ptr, self.n, nslots, pool_bytes, self.st)

    def add(self, text, starts, ends, ntok=None, cap=None, nbytes=None, work=None, table=None, expect_error=None):
        """jb_wc_add_device on host arrays: the span arrays are allocations of exactly cap entries, the work
        buffer lies between canaries.  work = (missing bytes, misalignment) and table = (missing bytes,
        misalignment) ask for bad buffers."""
        import torch
        text = bytes(text)
        cap = len(starts) if cap is None else cap
        ntok = len(starts) if ntok is None else ntok
        nbytes = len(text) if nbytes is None else nbytes
        d_text = torch.from_numpy(np.frombuffer(text + b"\0" * 64, np.uint8).copy()).cuda()
        d_s = torch.from_numpy(np.ascontiguousarray(starts, np.uint32)[:cap].view(np.int32).copy()).cuda() if cap else \
            torch.zeros(1, dtype=torch.int32, device="cuda")
        d_e = torch.from_numpy(np.ascontiguousarray(ends, np.uint32)[:cap].view(np.int32).copy()).cuda() if cap else \
            torch.zeros(1, dtype=torch.int32, device="cuda")
        d_n = torch.tensor([ntok], dtype=torch.int64, device="cuda")
        need = J.wc_work_bytes(cap)
        wk = torch.full((need + 2 * NG + 8,), 0x5B, dtype=torch.uint8, device="cuda")
        wk[:NG] = 0x7A
        wk[NG + need:] = 0x7A
        wmiss, wmis = work or (0, 0)
        tmiss, tmis = table or (0, 0)
        args = (self.ptr + tmis, self.n - tmiss, d_text.data_ptr(), nbytes, d_s.data_ptr(), d_e.data_ptr(), d_n.data_ptr(),
                cap, wk.data_ptr() + NG + wmis, need - wmiss, self.st)
        if expect_error is not None:
            with pytest.raises(J.JbError) as ei:
                self.tk.wc_add_device(*args)
            assert ei.value.code == expect_error
        else:
            self.tk.wc_add_device(*args)
        torch.cuda.synchronize()
        wb = wk.cpu().numpy()
        assert (wb[:NG] == 0x7A).all() and (wb[NG + need:] == 0x7A).all(), "written outside the work buffer"
        self.canaries()
        return wb[NG:NG + need]

    def canaries(self):
        b = self.buf.cpu().numpy()
        assert (b[:NG] == 0x7A).all() and (b[NG + self.n:] == 0x7A).all(), "written outside the table"
        return b[NG:NG + self.n]

    def read(self, min_count=1, max_keys=0):
        r = self.tk.wc_read(self.ptr, self.n, min_count, max_keys, self.st)
        self.canaries()
        return r


def check(tk, text, starts, ends, ntok=None, cap=None, label="", nslots=1024, pool_bytes=1 << 16):
    """device == wc_ref == jb_wc_count, exactly, and the accounting; returns the device's result."""
    ref = W.wc_ref(text, starts, ends, ntok, cap)
    t = Table(tk, nslots, pool_bytes)
    t.add(text, starts, ends, ntok, cap)
    got = t.read()
    assert W.same(got, ref) is None, (label, W.same(got, ref))
    host = J.wc_count(text, starts, ends, ntok=ntok, cap=cap)
    assert W.same(host, ref) is None, (label, "jb_wc_count", W.same(host, ref))
    assert int(got.counts.sum()) + got.bad + got.long + got.dropped + got.collided == got.tokens == ref.tokens
    return got


def words(n, seed, nkeys=40, maxlen=6, invalid=0.05):
    """n tokens drawn (skewed) from nkeys random keys of 1 to maxlen letters, some of them one invalid byte."""
    rng = np.random.default_rng(seed)
    keys = [bytes(rng.integers(0x61, 0x7B, int(l)).astype(np.uint8)) for l in rng.integers(1, maxlen + 1, nkeys)]
    pick = np.minimum((rng.random(n) ** 2 * nkeys).astype(int), nkeys - 1)
    toks = [bytes([0x80 + int(rng.integers(0, 128))]) if rng.random() < invalid else keys[i] for i in pick]
    return W.from_keys(toks)


# ---- 1. hand spans: token counts around the wave and the tile, cap on every side of ntok ------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ntok", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
def test_token_counts(forms, form, ntok):
    text, s, e = words(ntok, 100 + ntok)
    check(forms[form], text, s, e, label=f"form={form} ntok={ntok}")
    for cap_ntok, cap in ((ntok, max(ntok - 7, 0)), (ntok, ntok // 2), (ntok + 9, ntok), (max(ntok - 3, 0), ntok)):
        check(forms[form], text, s, e, ntok=cap_ntok, cap=cap, label=f"form={form} ntok={cap_ntok} cap={cap}")


@pytest.mark.parametrize("form", FORMS)
def test_key_lengths(forms, form):
    rng = np.random.default_rng(5)
    keys = []
    for ln in (1, 3, 8, 9, 16, 17, 24, 25, 26, 255, 256):
        k = bytes(rng.integers(0x30, 0x3A, ln).astype(np.uint8))
        keys += [k] * (1 + ln % 3)
        keys.append(k[:-1] + b"x")  # the same length, the last byte different
    keys += [keys[0], keys[9], keys[-2]] * 2
    text, s, e = W.from_keys(keys, gap=b"-")
    got = check(forms[form], text, s, e, label=f"form={form}", pool_bytes=1 << 12)
    assert got.long == sum(len(k) > 255 for k in keys) >= 3 and max(len(k) for k in got.keys) == 255 and got.dropped == 0


@pytest.mark.parametrize("form", FORMS)
def test_invalid_bytes(forms, form):
    """Runs of invalid bytes, each a token of its own keyed as U+FFFD, beside a real U+FFFD and its prefixes."""
    rng = np.random.default_rng(7)
    text = rng.integers(0x80, 0x100, 3000).astype(np.uint8)
    text[rng.random(3000) < 0.2] = 0x2E
    text[100:103] = list(W.REPL)
    s = np.arange(3000, dtype=np.uint32)
    e = s + 1
    s, e = np.append(s, [100, 100]).astype(np.uint32), np.append(e, [103, 102]).astype(np.uint32)
    got = check(forms[form], text.tobytes(), s, e, label=f"form={form}")
    assert got.keys[0] == W.REPL and int(got.counts[0]) == int((text >= 0x80).sum()) + 1


@pytest.mark.parametrize("form", FORMS)
def test_malformed_spans(forms, form):
    """Reversed and empty spans, spans past the end, starts near 2^32, keys of up to 300 bytes, clamps."""
    for seed in range(16):
        text, s, e, ntok, cap = W.random_case(seed)
        check(forms[form], text, s, e, ntok, cap, label=f"form={form} seed={seed}")
    text, s, e, ntok, cap = W.random_case(99, ntokens=3 * T + 77, nbytes=5000, clamp=False)
    got = check(forms[form], text, s, e, ntok, cap, label=f"form={form} seed=99")
    assert got.bad > 0 and got.long > 0


@pytest.mark.parametrize("form", FORMS)
def test_overlapping_spans(forms, form):
    """Full mode's shape: every span of 1 to 4 bytes at every position of a text over a small alphabet."""
    rng = np.random.default_rng(8)
    text = rng.integers(0x61, 0x64, 700).astype(np.uint8).tobytes()
    s = np.repeat(np.arange(700), 4)
    e = np.minimum(s + np.tile(np.arange(1, 5), 700), 700)
    check(forms[form], text, s.astype(np.uint32), e.astype(np.uint32), label=f"form={form}")


@pytest.mark.parametrize("form", FORMS)
def test_contention(forms, form):
    """20,000 copies of one key among 50 others."""
    rng = np.random.default_rng(9)
    others = [b"w%02d" % i for i in range(50)]
    toks = [b"the"] * 20_000 + [others[i] for i in rng.integers(0, 50, 1500)]
    toks = [toks[i] for i in rng.permutation(len(toks))]
    text, s, e = W.from_keys(toks)
    got = check(forms[form], text, s, e, label=f"form={form}")
    assert got.keys[0] == b"the" and int(got.counts[0]) == 20_000 and len(got.keys) == 51


@pytest.mark.parametrize("form", FORMS)
def test_all_distinct(forms, form):
    """3,000 keys, each once: every token claims a slot, and the order is the bytes' alone."""
    rng = np.random.default_rng(10)
    toks = [b"%d" % i for i in rng.permutation(3000)] + [b"k" * n for n in range(25, 60)]
    text, s, e = W.from_keys(toks, gap=b" ")
    got = check(forms[form], text, s, e, label=f"form={form}", nslots=8192, pool_bytes=4096)
    assert got.keys == sorted(toks) and (got.counts == 1).all()
    t = Table(forms[form], 8192, 4096)
    t.add(text, s, e)
    top = t.read(min_count=1, max_keys=10)
    assert top.keys == sorted(toks)[:10] and t.read(min_count=2).keys == []


# ---- 2. accumulation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_three_batches(forms, form):
    t = Table(forms[form], 1024, 1 << 16)
    total = Counter()
    bad = long = tokens = 0
    before = None
    for b, seed in enumerate((21, 22, 23)):
        text, s, e, ntok, cap = W.random_case(seed, ntokens=T + 50 * b, nbytes=900)
        ref = W.wc_ref(text, s, e, ntok, cap)
        total.update(ref.all)
        bad, long, tokens = bad + ref.bad, long + ref.long, tokens + ref.tokens
        t.add(text, s, e, ntok, cap)
        items = W.order(total)
        want = W.Ref([k for k, _ in items], [v for _, v in items], bad, long, tokens, dict(total))
        snap = t.canaries().copy()
        got = t.read()
        assert W.same(got, want) is None, (form, b, W.same(got, want))
        assert (t.canaries() == snap).all(), "jb_wc_read changed the table"
        assert W.same(t.read(), want) is None
        before = got
    assert before.tokens == tokens and tokens > 0


# ---- 3. real cuts -------------------------------------------------------------------------------------------------
def _oracle_spans(o, buf, off, mode, hmm):
    if mode == "cut":
        return o.cut_batch(buf, off, hmm)
    if mode == "search":
        return R.expected(o, buf, off, hmm)
    return F.expected(o, buf[:int(off[-1])], off)


@pytest.fixture(scope="module")
def real_refs(mini_paths, syn_small):
    """{(dict, mode, hmm): wc_ref over the oracle's tokens}, and the two batches, computed once."""
    mini = R.batch_of(TEXTS)
    buf, off, _ = syn_small[2].corpus(synth.KIND_DOCS, 3, target_bytes=96 << 10)
    syn = (np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(off, np.uint64))
    out = {"mini": mini, "syn": syn}
    for name, (b, f), paths in (("mini", mini, mini_paths), ("syn", syn, syn_small[:2])):
        o = O.Oracle.from_files(paths[0], paths[1], 0)
        for mode, hmm in MODES:
            s, e, _ = _oracle_spans(o, b, f, mode, hmm)
            out[name, mode, hmm] = W.wc_ref(bytes(b[:int(f[-1])]), s, e)
    return out


@pytest.mark.parametrize("mode,hmm", MODES)
@pytest.mark.parametrize("name", ["mini", "syn"])
def test_real_cuts(forms, syn_forms, real_refs, name, mode, hmm):
    """jb_wc_batch over a host batch in every mode, both forms: the oracle's tokens, counted."""
    ref = real_refs[name, mode, hmm]
    buf, off = real_refs[name]
    assert ref.bad == 0 and ref.long == 0 and ref.tokens > (20 if name == "mini" else 20_000)
    for f in FORMS:
        tk = (forms if name == "mini" else syn_forms)[f]
        t = Table(tk, 1 << 16, 1 << 16)
        tk.wc_batch(buf, off, hmm, t.ptr, t.n, mode)
        got = t.read()
        assert W.same(got, ref) is None, (name, mode, hmm, f, W.same(got, ref))
        tk.wc_batch(buf, off, hmm, t.ptr, t.n, mode)  # once more into the same table: every count doubles
        twice = t.read()
        assert twice.keys == ref.keys and twice.counts.tolist() == [2 * c for c in ref.counts]


def test_device_chain(syn_forms, real_refs):
    """cut_device, then wc_add_device on its device arrays, queued on one stream without a wait between."""
    import torch
    buf, off = real_refs["syn"]
    nb, nd = int(off[-1]), len(off) - 1
    d_text = torch.from_numpy(np.concatenate([buf[:nb], np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for f in FORMS:
        tk = syn_forms[f]
        t = Table(tk, 1 << 16, 1 << 16)
        ps, pe, _, pn = tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, st)
        need = J.wc_work_bytes(nb)
        wk = torch.empty(need, dtype=torch.uint8, device="cuda")
        tk.wc_add_device(t.ptr, t.n, d_text.data_ptr(), nb, ps, pe, pn, nb, wk.data_ptr(), need, st)
        assert W.same(t.read(), real_refs["syn", "cut", True]) is None


# ---- 4. overflow --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_table_overflow(forms, form):
    """nslots = 8 and 20 distinct keys of 2 bytes: new keys are accepted while fewer than 4 slots are taken, so
    tokens are dropped, and only for lack of a slot (the host rule shows no bad span, no long key and no key
    that needs the pool).  Every reported count is at most the true one, and the accounting holds."""
    rng = np.random.default_rng(12)
    keys = [b"%c%c" % (0x41 + i, 0x61 + i) for i in range(20)]
    toks = [keys[i] for i in rng.integers(0, 20, 600)]
    text, s, e = W.from_keys(toks)
    ref = J.wc_count(text, s, e)
    assert len(ref.keys) == 20 and ref.bad == 0 and ref.long == 0 and max(map(len, ref.keys)) <= 24
    true = dict(zip(ref.keys, ref.counts.tolist()))
    t = Table(forms[form], 8, 0)
    t.add(text, s, e)
    got = t.read()
    assert got.dropped > 0 and got.collided == 0 and got.bad == 0 and got.long == 0
    assert 4 <= len(got.keys) <= 8
    for k, c in zip(got.keys, got.counts.tolist()):
        assert c <= true[k], (k, c, true[k])
    assert int(got.counts.sum()) + got.dropped == got.tokens == 600


@pytest.mark.parametrize("form", FORMS)
def test_pool_overflow(forms, form):
    """A pool one byte too small for the one key of 25 bytes: its 7 tokens are dropped, in this batch and in
    the next, and nothing else is (every other key is short, and the table has room; the host rule says so)."""
    long25 = b"p" * 25
    toks = [b"ab", b"cd", long25, b"ab", b"x" * 24] + [long25] * 6 + [b"cd", b"ab"]
    text, s, e = W.from_keys(toks, gap=b" ")
    ref = J.wc_count(text, s, e)
    assert ref.bad == 0 and ref.long == 0 and sorted(map(len, ref.keys)) == [2, 2, 24, 25]
    t = Table(forms[form], 64, 24)
    t.add(text, s, e)
    got = t.read()
    assert got.dropped == 7 and got.collided == 0
    assert dict(zip(got.keys, got.counts.tolist())) == {b"ab": 3, b"cd": 2, b"x" * 24: 1}
    assert int(got.counts.sum()) + got.dropped == got.tokens == len(toks)
    t.add(text, s, e)
    got = t.read()
    assert got.dropped == 14 and dict(zip(got.keys, got.counts.tolist())) == {b"ab": 6, b"cd": 4, b"x" * 24: 2}
    roomy = Table(forms[form], 64, 25)  # one byte more: the key fits
    roomy.add(text, s, e)
    assert W.same(roomy.read(), W.wc_ref(text, s, e)) is None


# ---- 5. collisions ------------------------------------------------------------------------------------------------
def test_collisions(forms4):
    """JB_WC_HASHBITS=4 and 40 distinct keys: a fingerprint keeps the key whose first token comes earliest, in
    the first batch that brings one; every token of another key with that fingerprint is a collision."""
    rng = np.random.default_rng(13)
    keys = [b"key%02d" % i for i in range(40)]
    batches = [[keys[i] for i in rng.integers(0, 25, 900)], [keys[i] for i in rng.integers(10, 40, 700)]]
    fp = {k: J.wc_fp(k, 4) for k in keys}
    assert len(set(fp.values())) < 16 and all(1 <= v < 16 for v in fp.values())
    owner, kept, collided, tokens = {}, Counter(), 0, 0
    for toks in batches:
        for k in toks:  # (the earliest token of a batch first, the earlier batch first)
            owner.setdefault(fp[k], k)
        for k in toks:
            tokens += 1
            if owner[fp[k]] == k:
                kept[k] += 1
            else:
                collided += 1
    assert collided > 0 and len(kept) == len(set(fp.values()))
    items = W.order(kept)
    want = W.Ref([k for k, _ in items], [v for _, v in items], 0, 0, tokens, dict(kept))
    results = []
    for f in (0, 1, 1, 0):
        t = Table(forms4[f], 64, 0)
        for toks in batches:
            t.add(*W.from_keys(toks))
        got = t.read()
        assert W.same(got, want, collided=collided) is None, (f, W.same(got, want, collided=collided))
        assert int(got.counts.sum()) + got.collided == got.tokens
        results.append((got.keys, got.counts.tolist(), got.collided))
    assert all(r == results[0] for r in results)


# ---- 6. bad buffers, errors, the profile ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_bad_buffers(forms, form):
    text, s, e = words(300, 15)
    t = Table(forms[form])
    snap = t.canaries().copy()
    for kw in (dict(work=(4, 0)), dict(work=(0, 1)), dict(work=(0, 2)), dict(table=(0, 8)), dict(table=(0, 16)),
               dict(table=(t.n - 600, 0))):
        wb = t.add(text, s, e, expect_error=J.JB_EINVAL, **kw)
        assert (wb == 0x5B).all() and (t.canaries() == snap).all(), kw  # (nothing was queued)
    tk = forms[form]
    with pytest.raises(J.JbError) as ei:
        tk.wc_init_device(t.ptr, t.n, 1000, 0, t.st)  # not a power of two
    assert ei.value.code == J.JB_EINVAL
    with pytest.raises(J.JbError) as ei:
        tk.wc_init_device(t.ptr, t.n, 4096, 0, t.st)  # larger than the buffer
    assert ei.value.code == J.JB_EINVAL
    with pytest.raises(J.JbError) as ei:
        tk.wc_init_device(t.ptr + 8, t.n - 8, 8, 0, t.st)
    assert ei.value.code == J.JB_EINVAL
    assert (t.canaries() == snap).all()
    # a buffer that was never initialised is left alone, and jb_wc_read says that it holds no table
    raw = Table(tk, init=False)
    snap = raw.canaries().copy()
    raw.add(text, s, e)
    assert (raw.canaries() == snap).all()
    with pytest.raises(J.JbError) as ei:
        raw.read()
    assert ei.value.code == J.JB_EINVAL
    t.add(text, s, e)  # (and the good table still works)
    assert W.same(t.read(), W.wc_ref(text, s, e)) is None


def test_batch_errors(forms):
    tk = forms[1]
    t = Table(tk)
    buf = np.frombuffer(b"abc def" + b"\0" * 16, np.uint8)
    with pytest.raises(J.JbError) as ei:
        tk.wc_batch(buf, [0, 7], True, t.ptr, t.n, 3)
    assert ei.value.code == J.JB_EINVAL
    with pytest.raises(ValueError):
        tk.wc_batch(buf, [0, 7], True, t.ptr, t.n, "nope")
    with pytest.raises(J.JbError) as ei:
        tk.wc_batch(buf, [0, 7, 3], True, t.ptr, t.n)
    assert ei.value.code == J.JB_EINVAL
    tk.wc_batch(buf, [0], True, t.ptr, t.n)  # no documents
    assert t.read().tokens == 0
    tk.wc_batch(buf, [0, 7], True, t.ptr, t.n)
    got = t.read()
    assert got.keys == [b"abc", b"def"] and got.tokens == 2


def test_profile_lists_the_kernels(forms):
    tk = forms[1]
    text, s, e = words(3 * T, 17)
    t = Table(tk)
    tk.profile(True)
    try:
        tk.profile_reset()
        t.add(text, s, e)
        prof = tk.profile_read()
    finally:
        tk.profile(False)
    for k in ("k_wc_claim", "k_wc_store", "k_wc_count"):
        assert prof[k][1] == 1, prof


# ---- 7. end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cut", "search", "full"])
def test_fit_vocab_leaves_no_unknown(forms, mode):
    tk = forms[1]
    spans = {"cut": lambda t: tk.cut_spans(t, True), "search": lambda t: tk.cut_search_spans(t, True),
             "full": lambda t: tk.cut_full_spans(t)}[mode]
    try:
        keys, counts = tk.fit_vocab([TEXTS[:3], TEXTS[3:]], mode=mode, nslots=4096, pool_bytes=4096)
        assert tk.vocab_size == len(keys) > 10 and int(counts[0]) >= int(counts[-1]) >= 1
        total = 0
        for text in TEXTS:
            s, e = spans(text)
            ids = tk.spans_ids(text, s, e)
            assert (ids != J.JB_ID_UNK).all(), (text, ids)
            b = J._b(text)
            for i, a, z in zip(ids.tolist(), s.tolist(), e.tolist()):
                assert keys[i] == (W.REPL if z - a == 1 and b[a] >= 0x80 else b[a:z])
            total += len(ids)
        assert total == int(counts.sum())
        k2, c2 = tk.word_counts([TEXTS], mode=mode, min_count=2, max_keys=3, nslots=4096, pool_bytes=4096)
        assert k2 == keys[:len(k2)] and len(k2) <= 3 and (c2 >= 2).all()
        with pytest.raises(J.JbError):
            tk.word_counts([TEXTS], mode=mode, nslots=8, pool_bytes=0)  # dropped tokens, strict
        k3, c3 = tk.word_counts([TEXTS], mode=mode, nslots=8, pool_bytes=0, strict=False)
        assert 0 < len(k3) <= 8
    finally:
        tk.set_vocab(None)


def test_c_and_cpp_consumers(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "c_abi_wc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_wc.c"), "-L", lib,
                           "-ljiebahip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "wc ok" in r.stdout, r.stdout + r.stderr
    exe = str(tmp_path / "cpp_wc_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_wc_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "wc ok" in r.stdout, r.stdout + r.stderr
