"""GPU: near-duplicate pairs (jb_neardup_device, jb_neardup_sig, Tokenizer.dedup; jb_neardup.hip) against the
host rule jb_neardup (which tests/test_neardup_host.py pins to neardup_ref.py) on the inputs of neardup_cases.py,
byte for byte.  Every output and the work buffer sit between canaries that must not change, and the input arrays
start off a 16-byte boundary."""
import os
import subprocess

import numpy as np
import pytest

import jiebahip as J
import neardup_cases as NC
import search_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T = J.JB_ND_TILE
NG = 64  # canary bytes on each side of every output and of the work buffer
FILL = 0x33
CASES = list(NC.all_cases())
assert T == NC.TILE
_WANT = {}


@pytest.fixture(scope="module")
def tk(mini_paths):
    t = J.Tokenizer(J.make_config(dict_path=mini_paths[0], emit_path=mini_paths[1]))
    yield t
    t.close()


def want_of(c):
    """jb_neardup's result for a case, computed once: (pair_doc, pair_agree, pair_off, npairs, stat)."""
    if c["label"] not in _WANT:
        _WANT[c["label"]] = J.neardup(c["key"], c["sig"], c["W"], c["min_agree"])
    return _WANT[c["label"]]


def guarded(nbytes, fill):
    """A device buffer of nbytes between canaries: (tensor, pointer to the payload)."""
    import torch
    pad = (-nbytes) % 8
    t = torch.full((nbytes + pad + 2 * NG,), fill, dtype=torch.uint8, device="cuda")
    t[:NG] = 0x7A
    t[NG + nbytes:] = 0x7A
    assert (t.data_ptr() + NG) % 8 == 0
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


def device(tk, c, pcap=None, shift=1, work=None, alias=None, expect_error=None, **over):
    """jb_neardup_device on a case -> (pair_doc, pair_agree, pair_off, npairs, stat): the first two hold the
    min(npairs, pcap) entries the call writes; what lies behind them must still hold the fill.  work = (missing
    bytes, misalignment) asks for a bad buffer; alias names an output to pass another array's pointer for."""
    import torch
    (nd, B), K = c["key"].shape, c["sig"].shape[1]
    B, K = over.get("B", B), over.get("K", K)
    W, m = over.get("W", c["W"]), over.get("min_agree", c["min_agree"])
    pcap = want_of(c)[3] if pcap is None else pcap
    tkey, p_key = _up(c["key"], shift)
    tsig, p_sig = _up(c["sig"], shift)
    assert (p_key % 16 != 0) == (shift % 2 != 0) and (p_sig % 16 != 0) == (shift % 4 != 0)
    need = J.neardup_work_bytes(nd, c["key"].shape[1])
    wk, p_wk = guarded(need, 0x5B)
    pd, p_pd = guarded(pcap * 4, FILL)
    pa, p_pa = guarded(pcap * 4, FILL)
    po, p_po = guarded((nd + 1) * 8, FILL)
    pn, p_pn = guarded(8, FILL)
    ps, p_ps = guarded(J.JB_ND_NSTAT * 8, FILL)
    st = torch.cuda.current_stream().cuda_stream
    wmiss, wmis = work or (0, 0)
    if alias == "pair_doc":
        p_pd = p_sig
    if alias == "pair_agree":
        p_pa = p_pd
    if alias == "pair_off":
        p_po = p_key
    if alias == "npairs":
        p_pn = p_po
    if alias == "stat":
        p_ps = p_wk
    args = (p_key, p_sig, nd, B, K, W, m, p_pd, p_pa, pcap, p_po, p_pn, p_ps, p_wk + wmis, need - wmiss, st)
    if expect_error is not None:
        with pytest.raises(J.JbError) as ei:
            tk.neardup_device(*args)
        assert ei.value.code == expect_error
        torch.cuda.synchronize()  # nothing was queued: every buffer holds its fill
        assert (payload(wk, need, "the work buffer") == 0x5B).all()
        for t, nb in ((pd, pcap * 4), (pa, pcap * 4), (po, (nd + 1) * 8), (pn, 8), (ps, J.JB_ND_NSTAT * 8)):
            assert (payload(t, nb, "an output") == FILL).all()
        return None
    tk.neardup_device(*args)
    torch.cuda.synchronize()
    payload(wk, need, "the work buffer")
    n = int(payload(pn, 8, "npairs").copy().view(np.uint64)[0])
    off = payload(po, (nd + 1) * 8, "pair_off").copy().view(np.uint64)
    stat = payload(ps, J.JB_ND_NSTAT * 8, "stat").copy().view(np.uint64)
    w = min(n, pcap)
    outs = []
    for t, what in ((pd, "pair_doc"), (pa, "pair_agree")):
        b = payload(t, pcap * 4, what)
        assert (b[w * 4:] == FILL).all(), what + ": an entry at or past the count or pcap was written"
        outs.append(b[:w * 4].copy().view(np.uint32))
    del tkey, tsig
    return outs[0], outs[1], off, n, stat


def same(got, want, label, pcap=None):
    wd, wa, wo, n, ws = want
    w = n if pcap is None else min(n, pcap)
    assert got[3] == n, f"{label}: npairs {got[3]}, want {n}"
    assert got[4].tolist() == ws.tolist(), f"{label}: stat {got[4].tolist()}, want {ws.tolist()}"
    assert got[2].tobytes() == wo.tobytes(), f"{label}: pair_off differs"
    for g, x, name in ((got[0], wd, "pair_doc"), (got[1], wa, "pair_agree")):
        if g.tobytes() != x[:w].tobytes():
            bad = np.flatnonzero(g != x[:w])
            raise AssertionError(f"{label}: {name} differs at {len(bad)} positions; first {bad[0]}: got "
                                 f"{g[bad[:6]].tolist()} want {x[bad[:6]].tolist()}")


@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_cases(tk, c):
    same(device(tk, c), want_of(c), c["label"])


def test_capacity_and_alignment(tk):
    by = {c["label"]: c for c in CASES}
    for label in ("crowded", "several common bands"):
        c = by[label]
        want = want_of(c)
        n = want[3]
        assert n > 1
        for pcap in (0, n - 1, n, n + 5):
            same(device(tk, c, pcap=pcap), want, f"{label} pcap={pcap}", pcap)
        for shift in (0, 2, 3):
            same(device(tk, c, shift=shift), want, f"{label} shift={shift}")


def test_run_to_run(tk):
    c = [x for x in CASES if x["label"] == "mixed"][0]
    a, b = device(tk, c), device(tk, c)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3] and a[4].tolist() == b[4].tolist()


def test_refused_calls_queue_nothing(tk):
    c = [x for x in CASES if x["label"] == "B=5 K=70"][0]
    device(tk, c, work=(1, 0), expect_error=J.JB_EINVAL)
    device(tk, c, work=(0, 4), expect_error=J.JB_EINVAL)
    for name in ("pair_doc", "pair_agree", "pair_off", "npairs", "stat"):
        device(tk, c, alias=name, expect_error=J.JB_EINVAL)
    for kw in (dict(B=0), dict(K=0), dict(W=0), dict(min_agree=0)):
        device(tk, c, expect_error=J.JB_EINVAL, **kw)
    for kw in (dict(B=257), dict(K=257), dict(W=65), dict(min_agree=71)):
        device(tk, c, expect_error=J.JB_ELIMIT, **kw)
    with pytest.raises(J.JbError) as ei:
        tk.neardup_device(0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0)
    assert ei.value.code == J.JB_EINVAL
    with pytest.raises(J.JbError) as ei:
        tk.neardup_device(8, 8, (1 << 32) - T, 1, 1, 1, 1, 8, 8, 0, 8, 8, 8, 8, 1 << 40)
    assert ei.value.code == J.JB_ELIMIT


def test_profile_lists_the_kernels(tk):
    by = {c["label"]: c for c in CASES}
    tk.profile(True)
    try:
        for label in ("ndocs=1", "runs across tiles"):  # the launches do not depend on the data
            tk.profile_reset()
            same(device(tk, by[label]), want_of(by[label]), "profiled " + label)
            prof = tk.profile_read()
            assert prof["k_nd_hist"][1] == 9 and prof["k_nd_scan"][1] == 9 and prof["k_nd_scatter"][1] == 9
            for k in ("k_nd_mask", "k_nd_tsum", "k_nd_base", "k_nd_off", "k_nd_write"):
                assert prof[k][1] == 1, k
    finally:
        tk.profile(False)


# ---- host signatures and texts in ------------------------------------------------------------------------------------
def planted_docs(seed=277, ndocs=48):
    """Short documents over the mini dictionary's words and ASCII words; some are exact copies of earlier ones and
    some copies with one word edited."""
    rng = np.random.default_rng(seed)
    parts = ["今天", "天氣", "很好", "我", "昨天", "去", "上海", "交通", "大學", "這", "的", "一刹那", "，", "。", "abc", "2024"]
    docs = []
    for _ in range(ndocs):
        n = int(rng.integers(30, 80))
        docs.append([parts[int(rng.integers(0, len(parts)))] if rng.random() < 0.4 else "w%d " % int(rng.integers(0, 3000))
                     for _ in range(n)])
    docs[4] = []
    exact, edited = [(10, 1), (22, 1), (33, 12), (47, 0)], [(15, 6), (29, 20), (40, 8)]
    for c, o in exact:
        docs[c] = list(docs[o])
    for c, o in edited:
        docs[c] = list(docs[o])
        docs[c][len(docs[c]) // 2] = "edited "
    return ["".join(d).encode() for d in docs], exact


def host_chain(tk, docs, n, K, B, rows, W, m):
    """The GPU's plain cut, then the host rules: jb_minhash -> jb_minhash_bands -> jb_neardup -> jb_neardup_labels."""
    buf, off = R.batch_of(docs)
    s, e, dt = tk.cut_batch(buf, off, True)
    sig, doc_n = J.minhash(buf[:int(off[-1])], s, e, dt, n, K, 1)
    keys = J.minhash_bands(sig, doc_n, B, rows)
    pd, pa, po, npairs, st = J.neardup(keys, sig, W, m)
    return sig, doc_n, (pd, pa, po, st), J.neardup_labels(po, pd)


def test_neardup_sig_and_dedup(tk):
    docs, exact = planted_docs()
    buf, off = R.batch_of(docs)
    cut0 = tk.cut_batch(buf, off, True)
    for (n, K, B, Rr, W, m) in ((5, 128, 32, 4, 64, None), (3, 64, 16, 4, 1, 40), (2, 33, 33, 1, 64, 33)):
        mm = J._default_agree(K) if m is None else m
        sig, doc_n, (pd, pa, po, st), label = host_chain(tk, docs, n, K, B, Rr, W, mm)
        gsig, gdn = tk.minhash_batch(buf, off, True, n, K, 1)
        assert np.array_equal(gsig, sig) and np.array_equal(gdn, doc_n)
        go, gd, ga, gs = tk.near_duplicates(gsig, gdn, B, Rr, W, m)
        assert go.tobytes() == po.tobytes() and gd.tobytes() == pd.tobytes() and ga.tobytes() == pa.tobytes()
        assert gs.tolist() == st.tolist()
        lab, keep = tk.dedup(docs, n, K, B, Rr, W, m)
        assert np.array_equal(lab, label) and np.array_equal(keep, label == np.arange(len(docs)))
        for c, o in exact:
            assert lab[c] == lab[o] and not keep[c]
        assert keep[4] and int(keep.sum()) <= len(docs) - len(exact)
        # the cap protocol: a short pcap reports the full count
        npairs = len(pd)
        assert npairs >= len(exact)
        with pytest.raises(J.JbError) as ei:
            tk.near_duplicates(gsig, gdn, B, Rr, W, m, pcap=npairs - 1)
        assert ei.value.code == J.JB_ELIMIT
        assert tk.near_duplicates(gsig, gdn, B, Rr, W, m, pcap=npairs)[1].tobytes() == pd.tobytes()
    # no document
    go, gd, ga, gs = tk.near_duplicates(np.zeros((0, 8), np.uint32), np.zeros(0, np.uint32), 2, 4)
    assert go.tolist() == [0] and len(gd) == 0 and gs.tolist() == [0, 0, 0]
    # a cut and a minhash batch on the same ctx give what they gave before
    cut1 = tk.cut_batch(buf, off, True)
    assert all(np.array_equal(x, y) for x, y in zip(cut0, cut1))
    gsig2, gdn2 = tk.minhash_batch(buf, off, True, 2, 33, 1)
    assert np.array_equal(gsig2, gsig) and np.array_equal(gdn2, gdn)


def test_cpp_consumer(mini_paths, tmp_path):
    lib = os.path.join(ROOT, "jieba-go_amd", "lib")
    exe = str(tmp_path / "cpp_neardup_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "jieba-go_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp_neardup_smoke.cpp"), "-L", lib, "-ljbtok", "-ljiebahip",
                           "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, mini_paths[0], mini_paths[1]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "neardup ok" in r.stdout, r.stderr + r.stdout
