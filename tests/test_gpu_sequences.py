"""GPU: one tokenizer kept open over a sequence of calls, every call checked against the shadow model of
tests/ctx_model.py (the references of the other GPU files, and nothing of the library): spans, doc_tok,
ids, counters, keyword records with their f32 score bits, kw_n and jb_last_stats' token count, all exact.
What the sequences cross is the state a jb_ctx keeps between calls: the grow-only workspace and the buffers
that follow it, the three captured graphs, the image AddWord swaps in (with full mode's look-back reach),
the vocabulary, the four arenas of the *_batch calls, and the flags behind jb_last_stats (DESIGN.md,
"One context over many calls").  The second half does the same for joined text, character offsets and word
counts: their batch calls carve the same arenas in another layout (and four more), move the span arrays into
the ids/terms arena when a full-mode list outgrows its batch, overwrite span arrays in place, hand out a
pinned block that one process-wide cache recycles, and add to a table the caller keeps; join_ref,
charspans_ref and wc_ref over the model's spans answer them, byte for byte.  The last part follows the calls
that came after those (MinHash, the caller's filter, postings, BM25 search, near-duplicate pairs, collocations)
through the same arenas and their own six, which only grow and are never cleared, with the stop set, the batch
filter and the index changing under them and JB_ELIMIT / JB_EINVAL returned half-way through a call."""
import ctypes as C
import gc

import numpy as np
import pytest

import bm25_ref as BR
import charspans_ref as CR
import ctx_model as M
import full_ref as F
import jiebahip as J
import join_ref as JR
import search_ref as R
import synth
import wc_ref as W

pytestmark = pytest.mark.gpu

GUARD = 0x7A7A7A7A
NG = 64  # canary words on each side of a caller-owned device output
JUNK = 0x33333333  # what every output holds before a call
X4 = "\U00020000"  # a 4-byte Han rune
TILE = 4096  # kTileBytes
COMBOS = (("plain", True), ("plain", False), ("search", True), ("full", False))


# ---- comparing ----------------------------------------------------------------------------------------------
def same_spans(got, want, label):
    gs, ge, gd = (np.asarray(x, np.uint64) for x in got)
    ws, we, wd = (np.asarray(x, np.uint64) for x in want)
    if not (np.array_equal(gs, ws) and np.array_equal(ge, we)):
        n = min(len(gs), len(ws))
        ne = (gs[:n] != ws[:n]) | (ge[:n] != we[:n])
        bad = int(np.argmax(ne)) if ne.any() else n
        raise AssertionError(f"{label}: {len(gs)} vs {len(ws)} spans; first diff #{bad}: "
                             f"gpu={list(zip(gs[bad:bad + 6].tolist(), ge[bad:bad + 6].tolist()))} "
                             f"want={list(zip(ws[bad:bad + 6].tolist(), we[bad:bad + 6].tolist()))}")
    assert np.array_equal(gd, wd), f"{label}: doc_tok"


def same_bits(got, want, label):
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"{label}: output {k}"


def guarded(n, dtype):
    import torch
    t = torch.full((n + 2 * NG,), JUNK, dtype=dtype, device="cuda")
    t[:NG] = GUARD
    t[NG + n:] = GUARD
    return t


def inner(t, n, dtype):
    a = t.cpu().numpy()
    assert (a[:NG] == GUARD).all() and (a[NG + n:] == GUARD).all(), "written outside a caller-owned output"
    return a[NG:NG + n].view(dtype)


def guarded_bytes(n):
    import torch
    t = torch.full((n + 2 * NG,), JUNK & 0xFF, dtype=torch.uint8, device="cuda")
    t[:NG] = GUARD & 0xFF
    t[NG + n:] = GUARD & 0xFF
    return t


def inner_bytes(t, n):
    a = t.cpu().numpy()
    assert (a[:NG] == GUARD & 0xFF).all() and (a[NG + n:] == GUARD & 0xFF).all(), "written outside a caller-owned output"
    return a[NG:NG + n]


# ---- the driver: makes the library's call and the model's, and compares ------------------------------------
class Dev:
    """A batch on the device, kept for the whole sequence: a repeat finds the same pointers."""

    def __init__(self, batch):
        import torch
        text, off = batch.rel()
        self.nb, self.nd = batch.nbytes, batch.ndocs
        self.text = torch.from_numpy(np.ascontiguousarray(text[:self.nb + 64])).cuda()
        self.off = torch.from_numpy(off.astype(np.int64)).cuda()
        self.base = int(batch.off[0])
        self.outs = {}

    def args(self):
        return self.text.data_ptr(), self.nb, self.off.data_ptr(), self.nd


class Driver:
    def __init__(self, tk, model, s=None, wc_sizes=(M.WC_NSLOTS, M.WC_POOL)):
        self.tk, self.m, self.s = tk, model, s
        self.batches, self.devs = {}, {}
        self.last = None  # the last cut: (batch, its expected spans)
        self.stream = None
        # the last device cut while no other call has cut since (ctx_model.dev_state): where its spans lie
        self.lastdev = None
        self.wc_sizes, self.table = wc_sizes, None  # one word-count table for the driver's life
        self.cs_out, self.cs_cap = None, None  # the arrays of the last charspans_batch, and their size
        self.calls = []  # (kind, bytes of the batch) of every *_batch call
        self.too_small = self.restored = 0  # charspans_batch retries; cuts repeated after an in-place charspans
        self.sig = None  # the last minhash_batch: the model's (sig, doc_n, whether the batch has duplicates)
        self.ctable = None  # one collocation table and d_uni per vocabulary
        self.log = []  # ("refused", kind), ("search", spec, hits, misses), ("neardup", dups, pairs, over the window)

    def st(self):
        """A stream of the driver's own, for every device call: the library captures a graph only for a
        pipeline queued on a caller's stream, never on the null stream (which is torch's current one)."""
        import torch
        if self.stream is None:
            self.stream = torch.cuda.Stream()
        torch.cuda.synchronize()  # (the uploads and fills before the call ran on torch's stream)
        return self.stream.cuda_stream

    def batch(self, b):
        if isinstance(b, M.Batch):
            return self.batches.setdefault(b.spec, b)
        if b not in self.batches:
            self.batches[b] = M.make_batch(self.s, b)
        return self.batches[b]

    def dev(self, b):
        if b.spec not in self.devs:
            self.devs[b.spec] = Dev(b)
        return self.devs[b.spec]

    # -- cuts
    def cut(self, mode, hmm, route, b, reps=None, label=""):
        """One cut; a device cut is made three times (direct, captured, replayed) unless reps says otherwise."""
        b = self.batch(b)
        want = self.m.cut(b, mode, hmm)
        label = f"{label} {mode} hmm={hmm} {route} {b.spec}"
        if route == "host":
            tk = self.tk
            self.lastdev = None
            got = tk.cut_batch_full(b.buf, b.off) if mode == "full" else (
                tk.cut_batch_search if mode == "search" else tk.cut_batch)(b.buf, b.off, hmm)
            same_spans(got, want, label)
        else:
            for rep in range(3 if reps is None else reps):
                self._device(mode, hmm, b, want, route == "device_into", f"{label} call {rep}")
        self.last = (b, want)
        return want

    def _device(self, mode, hmm, b, want, into, label):
        import torch
        tk, dv = self.tk, self.dev(b)
        base = np.uint64(dv.base)
        want = (want[0] - base, want[1] - base, want[2])
        nw = len(want[0])
        if into:
            cap = max(nw, dv.nb, 1)
            key = (mode, cap)
            if key not in dv.outs:  # (kept, so that a repeat's graph key matches)
                dv.outs[key] = (guarded(cap, torch.int32), guarded(cap, torch.int32), guarded(dv.nd + 1, torch.int64),
                                guarded(1, torch.int64))
            o = dv.outs[key]
            for t in o:
                t[NG:-NG] = JUNK
            p = [t.data_ptr() + NG * t.element_size() for t in o]
            st = self.st()
            if mode == "full":
                tk.cut_device_full_into(*dv.args(), p[0], p[1], cap, p[2], p[3], st)
            else:
                (tk.cut_device_search_into if mode == "search" else tk.cut_device_into)(
                    *dv.args(), hmm, p[0], p[1], cap, p[2], p[3], st)
            torch.cuda.synchronize()
            tk.device_status(st)
            n = int(inner(o[3], 1, np.uint64)[0])
            assert n == nw, f"{label}: {n} spans, want {nw}"
            got = (inner(o[0], cap, np.uint32)[:n], inner(o[1], cap, np.uint32)[:n], inner(o[2], dv.nd + 1, np.uint64))
            same_spans(got, want, label)
            self.lastdev = dict(b=b, mode=mode, hmm=hmm, into=True, ptrs=tuple(p), cap=cap, outs=o)
            return
        st = self.st()
        if mode == "full":
            ps, pe, pd, pn = tk.cut_device_full(*dv.args(), st)
        else:
            ps, pe, pd, pn = (tk.cut_device_search if mode == "search" else tk.cut_device)(*dv.args(), hmm, st)
        torch.cuda.synchronize()
        code = J.JB_OK
        try:
            tk.device_status(st)
        except J.JbError as e:
            code = e.code
        # (the ctx-owned arrays hold nbytes spans: a longer full-mode list is counted and reported)
        assert code == (J.JB_ELIMIT if nw > dv.nb else J.JB_OK), f"{label}: status {code}"
        n = int(J.dev_to_host(pn, 8, np.uint64)[0])
        assert n == nw, f"{label}: {n} spans, want {nw}"
        k = min(n, dv.nb)
        got = (J.dev_to_host(ps, 4 * k, np.uint32), J.dev_to_host(pe, 4 * k, np.uint32),
               J.dev_to_host(pd, 8 * (dv.nd + 1), np.uint64))
        same_spans(got, (want[0][:k], want[1][:k], want[2]), label)
        self.lastdev = dict(b=b, mode=mode, hmm=hmm, into=False, ptrs=(ps, pe, pd, pn), cap=dv.nb, outs=None)

    # -- ids of the last cut's spans
    def ids(self, route, label=""):
        import torch
        b, (ws, we, _) = self.last
        label = f"{label} ids {route} {b.spec}"
        if route == "host":
            if len(ws):
                got = self.tk.spans_ids(b.buf, ws, we)
                assert np.array_equal(got, self.m.ids(b.buf, ws, we, int(b.off[-1]))), label
            return
        dv = self.dev(b)
        base = np.uint64(dv.base)
        # the spans, and three the kernel must not trust: empty, reversed, past the text
        s = np.concatenate([ws - base, np.array([3, 9, dv.nb], np.uint64)]).astype(np.uint32)
        e = np.concatenate([we - base, np.array([3, 6, dv.nb + 3], np.uint64)]).astype(np.uint32)
        n = len(s)
        d_s, d_e = torch.from_numpy(s.view(np.int32)).cuda(), torch.from_numpy(e.view(np.int32)).cuda()
        d_n = torch.tensor([n], dtype=torch.int64, device="cuda")
        o = guarded(n, torch.int32)
        self.tk.ids_device(dv.text.data_ptr(), dv.nb, d_s.data_ptr(), d_e.data_ptr(), d_n.data_ptr(), n,
                           o.data_ptr() + 4 * NG, self.st())
        torch.cuda.synchronize()
        text = b.rel()[0]
        assert np.array_equal(inner(o, n, np.uint32), self.m.ids(text, s, e, dv.nb)), label

    # -- the *_batch calls, into outputs that start as garbage
    def keywords(self, hmm, b, topk, label=""):
        b = self.batch(b)
        self.lastdev = None
        self.calls.append(("keywords_batch", b.nbytes))
        w = self.m.weights
        nd = b.ndocs
        ki, ks, kc = (np.full(nd * topk, JUNK, np.uint32) for _ in range(3))
        kn = np.full(nd, JUNK, np.uint32)
        J._check(J.lib().jb_keywords_batch(self.tk.h, b.buf.ctypes.data, b.off.ctypes.data, nd, int(hmm),
                                           w.ctypes.data if len(w) else None, len(w), topk, ki.ctypes.data,
                                           ks.ctypes.data, kc.ctypes.data, kn.ctypes.data))
        got = (ki.reshape(nd, topk), ks.view(np.float32).reshape(nd, topk), kc.reshape(nd, topk), kn)
        same_bits(got, self.m.keywords(b, hmm, topk), f"{label} keywords_batch hmm={hmm} {b.spec} topk={topk}")
        return got

    def df(self, hmm, b, label=""):
        b = self.batch(b)
        self.lastdev = None
        self.calls.append(("df_batch", b.nbytes))
        ndf = len(self.m.keys)
        before = (np.arange(ndf, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(8)  # (the counters are added to)
        got = self.tk.df_batch(b.buf, b.off, hmm, before.copy())
        assert np.array_equal(got, before + self.m.df(b, hmm, ndf)), f"{label} df_batch hmm={hmm} {b.spec}"
        return got - before

    def textrank(self, hmm, b, span=5, iters=10, topk=20, label=""):
        b = self.batch(b)
        self.lastdev = None
        self.calls.append(("textrank_batch", b.nbytes))
        k = self.m.keep
        nd = b.ndocs
        ki, ks = np.full(nd * topk, JUNK, np.uint32), np.full(nd * topk, JUNK, np.uint32)
        kn = np.full(nd, JUNK, np.uint32)
        J._check(J.lib().jb_textrank_batch(self.tk.h, b.buf.ctypes.data, b.off.ctypes.data, nd, int(hmm),
                                           k.ctypes.data if len(k) else None, len(k), span, iters, topk,
                                           ki.ctypes.data, ks.ctypes.data, kn.ctypes.data))
        got = (ki.reshape(nd, topk), ks.view(np.float32).reshape(nd, topk), kn)
        same_bits(got, self.m.textrank(b, hmm, span, iters, topk),
                  f"{label} textrank_batch hmm={hmm} {b.spec} span={span} iters={iters} topk={topk}")
        return got

    # -- joined text, character offsets and word counts of a host batch
    def join_batch(self, mode, hmm, b, sep, term, label="", buf=None):
        """jb_cut_batch_join; buf: the batch's bytes at another host address.  Returns the library's array."""
        b = self.batch(b)
        self.lastdev = None
        self.calls.append(("join_batch", b.nbytes))
        label = f"{label} join_batch {mode} hmm={hmm} {b.spec} sep={sep!r} term={term!r}"
        try:
            want, woff = self.m.join(b, mode, hmm, sep, term)
        except M.ModelError:  # (a batch filter that asks for a stop set that is gone)
            return self.refused(lambda: self.tk.cut_batch_join(b.buf, b.off, hmm, M.LIB_MODE[mode], sep, term), label)
        if self.tk is None:
            return None
        got, off = self.tk.cut_batch_join(b.buf if buf is None else buf, b.off, hmm, M.LIB_MODE[mode], sep, term)
        assert off.tolist() == woff, f"{label}: out_doc_off"
        assert got.tobytes() == want, f"{label}: {len(got)} bytes, want {len(want)}"
        return got

    def charspans_batch(self, mode, hmm, b, unit, reuse, label="", buf=None):
        """jb_cut_batch_charspans through Tokenizer.cut_batch_charspans; reuse: into the span arrays of the call
        before, which the binding replaces after JB_ELIMIT when they are too small."""
        b = self.batch(b)
        self.lastdev = None
        self.calls.append(("charspans_batch", b.nbytes))
        wcs, wce, wd, wun = self.m.charspans(b, mode, hmm, unit)
        # the binding's rule: new arrays of max(1024, bytes / 2) entries unless it is handed some, and after
        # JB_ELIMIT arrays of exactly the count
        cap = self.cs_cap if reuse and self.cs_cap is not None else max(1024, b.nbytes // 2)
        if reuse and self.cs_cap is not None and len(wcs) > cap:
            self.too_small += 1
        self.cs_cap = max(cap, len(wcs))
        if self.tk is None:
            return
        label = f"{label} charspans_batch {mode} hmm={hmm} {b.spec} {unit} reuse={reuse}"
        nd, n, out = b.ndocs, len(wcs), None
        if reuse and self.cs_out is not None:
            out = (self.cs_out[0], self.cs_out[1], np.full(nd + 1, JUNK, np.uint64), np.full(max(nd, 1), JUNK, np.uint32))
            out[0][:] = JUNK
            out[1][:] = JUNK
        cs, ce, tok, un, kept = self.tk.cut_batch_charspans(b.buf if buf is None else buf, b.off, hmm, M.LIB_MODE[mode],
                                                            unit, out)
        if out is not None:
            assert (kept[0] is out[0]) == (n <= len(out[0])), f"{label}: {n} tokens, arrays of {len(out[0])}"
            if n > len(out[0]):
                assert len(kept[0]) == len(kept[1]) == n, label
            else:  # (nothing past the count is written)
                assert (out[0][n:] == JUNK).all() and (out[1][n:] == JUNK).all(), f"{label}: written past the count"
        assert np.array_equal(tok, wd), f"{label}: doc_tok"
        assert np.array_equal(cs, wcs) and np.array_equal(ce, wce), f"{label}: offsets"
        assert np.array_equal(un, wun), f"{label}: doc_units"
        assert len(kept[0]) == self.cs_cap, f"{label}: arrays of {len(kept[0])}, want {self.cs_cap}"
        self.cs_out = kept

    def wc_table(self):
        """The driver's table between canaries: (pointer, bytes)."""
        import torch
        if self.table is None:
            nslots, pool = self.wc_sizes
            n = J.wc_table_bytes(nslots, pool)
            t = guarded_bytes(n)
            assert (t.data_ptr() + NG) % 32 == 0
            self.tk.wc_init_device(t.data_ptr() + NG, n, nslots, pool, self.st())
            torch.cuda.synchronize()
            self.table = (t, n)
        return self.table[0].data_ptr() + NG, self.table[1]

    def wc_batch(self, mode, hmm, b, label="", buf=None):
        b = self.batch(b)
        self.lastdev = None
        self.calls.append(("wc_batch", b.nbytes))
        try:
            self.m.wc_batch(b, mode, hmm)
        except M.ModelError:  # (raised before the model's table is touched; the library's must stay as it is too)
            if self.tk is not None:
                ptr, n = self.wc_table()
                self.refused(lambda: self.tk.wc_batch(b.buf, b.off, hmm, ptr, n, M.LIB_MODE[mode]), f"{label} wc_batch")
            return
        if self.tk is None:
            return
        ptr, n = self.wc_table()
        self.tk.wc_batch(b.buf if buf is None else buf, b.off, hmm, ptr, n, M.LIB_MODE[mode])

    def wc_read(self, label=""):
        """jb_wc_read against the model's Counter: keys, counts, order and the five totals; nothing dropped."""
        import torch
        if self.tk is None:
            return None
        ptr, n = self.wc_table()
        got = self.tk.wc_read(ptr, n, 1, 0, self.st())
        torch.cuda.synchronize()
        t = self.table[0]
        assert (t[:NG].cpu().numpy() == GUARD & 0xFF).all() and (t[NG + n:].cpu().numpy() == GUARD & 0xFF).all(), \
            "written outside the table"
        assert got.dropped == 0 and got.collided == 0, f"{label} wc_read: {got!r}"
        diff = W.same(got, self.m.wc_result())
        assert diff is None, f"{label} wc_read: {diff}"
        return got

    # -- jb_join_device, jb_charspans_device and jb_wc_add_device on the last cut's spans
    def spans_host(self):
        """(batch, starts, ends, doc_tok, ntok, cap) of the span list those calls are given, relative to the
        batch's first byte: the last device cut's arrays while they hold (lastdev), else the last cut's spans
        with three the kernels must not trust behind them, as Driver.ids uploads them."""
        if self.lastdev is not None:
            b, cap = self.lastdev["b"], self.lastdev["cap"]
            ws, we, wd = self.m.cut(b, self.lastdev["mode"], self.lastdev["hmm"], count=False)
            base = np.uint64(int(b.off[0]))
            return b, (ws - base)[:cap].astype(np.uint32), (we - base)[:cap].astype(np.uint32), wd, len(ws), cap
        if self.last is None:
            return None
        b, (ws, we, wd) = self.last
        base = np.uint64(int(b.off[0]))
        s = np.concatenate([ws - base, np.array([3, 9, b.nbytes], np.uint64)]).astype(np.uint32)
        e = np.concatenate([we - base, np.array([3, 6, b.nbytes + 3], np.uint64)]).astype(np.uint32)
        return b, s, e, wd, len(s), len(s)

    def spans_dev(self, s, e, wd, ntok):
        """Device pointers (start, end, doc_tok, ntok) of spans_host's list, and what keeps them alive."""
        import torch
        if self.lastdev is not None:
            return self.lastdev["ptrs"], self.lastdev["outs"]
        n = len(s)
        keep = (guarded(n, torch.int32), guarded(n, torch.int32), torch.from_numpy(wd.astype(np.int64)).cuda(),
                torch.tensor([ntok], dtype=torch.int64, device="cuda"))
        keep[0][NG:NG + n] = torch.from_numpy(s.view(np.int32).copy()).cuda()
        keep[1][NG:NG + n] = torch.from_numpy(e.view(np.int32).copy()).cuda()
        return (keep[0].data_ptr() + 4 * NG, keep[1].data_ptr() + 4 * NG, keep[2].data_ptr(), keep[3].data_ptr()), keep

    def join(self, sep, term, label=""):
        import torch
        src = self.spans_host()
        if src is None or self.tk is None:
            return
        b, s, e, wd, ntok, cap = src
        dv = self.dev(b)
        label = f"{label} join {b.spec} sep={sep!r} term={term!r}"
        want, woff = JR.join_ref(b.rel()[0][:dv.nb], s, e, wd, sep, term, ntok, cap, dv.nb)
        ptrs, keep = self.spans_dev(s, e, wd, ntok)
        nwork = J.join_work_bytes(cap, dv.nd)
        out, ooff, nout, work = (guarded_bytes(len(want)), guarded(dv.nd + 1, torch.int64), guarded(1, torch.int64),
                                 guarded_bytes(nwork))
        self.tk.join_device(dv.text.data_ptr(), dv.nb, ptrs[0], ptrs[1], ptrs[2], ptrs[3], cap, dv.nd, sep, term,
                            out.data_ptr() + NG, len(want), ooff.data_ptr() + 8 * NG, nout.data_ptr() + 8 * NG,
                            work.data_ptr() + NG, nwork, self.st())
        torch.cuda.synchronize()
        inner_bytes(work, nwork)
        assert int(inner(nout, 1, np.uint64)[0]) == len(want), f"{label}: nout"
        assert inner(ooff, dv.nd + 1, np.uint64).tolist() == woff, f"{label}: out_doc_off"
        assert inner_bytes(out, len(want)).tobytes() == want, f"{label}: bytes"

    def charspans(self, unit, inplace, label=""):
        """jb_charspans_device; in place it overwrites the span arrays, and when those were a device cut's the
        same cut is made again afterwards: byte spans must be back."""
        import torch
        src = self.spans_host()
        if src is None or self.tk is None:
            self.restored += self.tk is None and inplace and self.lastdev is not None
            return
        b, s, e, wd, ntok, cap = src
        dv = self.dev(b)
        label = f"{label} charspans {b.spec} {unit} inplace={inplace}"
        n = min(ntok, cap)
        wcs, wce, wun = CR.charspans_ref(b.rel()[0][:dv.nb], b.rel()[1], s, e, wd, M.UNITS[unit], ntok, cap)
        ptrs, keep = self.spans_dev(s, e, wd, ntok)
        nwork = J.charspans_work_bytes(dv.nb, dv.nd)
        units, work = guarded(dv.nd, torch.int32), guarded_bytes(nwork)
        if inplace:
            pcs, pce = ptrs[0], ptrs[1]
        else:
            ocs, oce = guarded(cap, torch.int32), guarded(cap, torch.int32)
            pcs, pce = ocs.data_ptr() + 4 * NG, oce.data_ptr() + 4 * NG
        self.tk.charspans_device(dv.text.data_ptr(), dv.nb, dv.off.data_ptr(), dv.nd, ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                                 cap, unit, pcs, pce, units.data_ptr() + 4 * NG, work.data_ptr() + NG, nwork, self.st())
        torch.cuda.synchronize()
        inner_bytes(work, nwork)
        assert inner(units, dv.nd, np.uint32).tolist() == wun, f"{label}: doc_units"
        if not inplace:
            gcs, gce = inner(ocs, cap, np.uint32), inner(oce, cap, np.uint32)
            assert (gcs[n:] == JUNK).all() and (gce[n:] == JUNK).all(), f"{label}: written past the count"
        elif keep is None:  # (the ctx-owned arrays)
            gcs, gce = J.dev_to_host(ptrs[0], 4 * n, np.uint32), J.dev_to_host(ptrs[1], 4 * n, np.uint32)
        else:
            gcs, gce = inner(keep[0], len(keep[0]) - 2 * NG, np.uint32), inner(keep[1], len(keep[1]) - 2 * NG, np.uint32)
        assert gcs[:n].tolist() == wcs and gce[:n].tolist() == wce, f"{label}: offsets"
        if inplace and self.lastdev is not None:
            ld = self.lastdev
            self._device(ld["mode"], ld["hmm"], b, self.m.cut(b, ld["mode"], ld["hmm"], count=False), ld["into"],
                         f"{label}: the cut again")
            self.restored += 1

    def wc_add(self, label=""):
        """jb_wc_add_device on the last cut's spans, into the driver's table."""
        import torch
        src = self.spans_host()
        if src is None:
            return
        b, s, e, wd, ntok, cap = src
        self.m.wc_add(b.rel()[0][:b.nbytes], s, e, ntok, cap, b.nbytes)
        if self.tk is None:
            return
        dv = self.dev(b)
        ptrs, keep = self.spans_dev(s, e, wd, ntok)
        ptr, nt = self.wc_table()
        nwork = J.wc_work_bytes(cap)
        work = guarded_bytes(nwork)
        self.tk.wc_add_device(ptr, nt, dv.text.data_ptr(), dv.nb, ptrs[0], ptrs[1], ptrs[3], cap, work.data_ptr() + NG,
                              nwork, self.st())
        torch.cuda.synchronize()
        inner_bytes(work, nwork)

    # -- MinHash, the caller's filter, postings, search, near-duplicates and collocations; the stop set, the batch
    # filter and the index.  Without a library (DryDriver) each makes the model's call alone.
    def _both(self, kind, b, want_fn, lib_fn, label):
        """One *_batch call of `kind` on batch b: (the model's answer, the library's).  Where the model refuses the
        call (ModelError) the library must return JB_EINVAL: (None, None)."""
        self.lastdev = None
        self.calls.append((kind, b.nbytes))
        try:
            want = want_fn()
        except M.ModelError:
            want = None
            self.log.append(("refused", kind))
        if self.tk is None:
            return want, None
        if want is None:
            self.refused(lib_fn, label)
            return None, None
        return want, lib_fn()

    def refused(self, lib_fn, label):
        """A call the model refuses: the library's JB_EINVAL."""
        if self.tk is not None:
            with pytest.raises(J.JbError) as ei:
                lib_fn()
            assert ei.value.code == J.JB_EINVAL, f"{label}: {ei.value}"

    def minhash_batch(self, mode, hmm, b, n=5, K=128, seed=1, label="", dups=False):
        """jb_minhash_batch; the model's signatures are kept for neardup (sig, doc_n, whether b has duplicates)."""
        b = self.batch(b)
        label = f"{label} minhash_batch {mode} hmm={hmm} {b.spec} n={n} K={K} seed={seed}"
        want, got = self._both("minhash_batch", b, lambda: self.m.minhash(b, mode, hmm, n, K, seed),
                               lambda: self.tk.minhash_batch(b.buf, b.off, hmm, n, K, seed, M.LIB_MODE[mode]), label)
        if want is not None:
            self.sig = (want[0], want[1], dups)
        if got is not None:
            assert np.array_equal(got[1], want[1]), f"{label}: doc_n"
            assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), f"{label}: signatures"
        return want

    def filter_batch(self, mode, hmm, b, rule, short=0, label=""):
        """jb_cut_batch_filter with a caller's rule into arrays of the exact count less `short`: too small, it is
        JB_ELIMIT with the count and the statistics right and nothing else written."""
        b = self.batch(b)
        label = f"{label} filter_batch {mode} hmm={hmm} {b.spec} {rule} short={short}"
        nd = b.ndocs

        def call():
            n = len(self.m.filter_batch(b, mode, hmm, rule)[0])
            cap = max(n - short, 0)
            s, e = np.full(max(cap, 1), JUNK, np.uint32), np.full(max(cap, 1), JUNK, np.uint32)
            tok, cnt, stats = np.full(nd + 1, JUNK, np.uint64), C.c_uint64(JUNK), np.full(5, JUNK, np.uint64)
            r = J.jb_filter_rule(J.JB_FILTER_STOP if rule.stop else 0, rule.drop, rule.min_runes, rule.max_runes)
            rc = J.lib().jb_cut_batch_filter(self.tk.h, b.buf.ctypes.data, b.off.ctypes.data, nd, int(hmm),
                                             J._MODES[M.LIB_MODE[mode]], C.byref(r), s.ctypes.data, e.ctypes.data, cap,
                                             tok.ctypes.data, C.byref(cnt), stats.ctypes.data)
            if rc == J.JB_EINVAL:
                J._check(rc)
            return rc, s, e, tok, cnt.value, stats, cap

        want, got = self._both("filter_batch", b, lambda: self.m.filter_batch(b, mode, hmm, rule), call, label)
        if got is not None:
            rc, s, e, tok, cnt, stats, cap = got
            ws, we, wd, wst = want
            assert cnt == len(ws) and np.array_equal(stats, wst), f"{label}: count {cnt}, statistics {stats.tolist()}"
            if len(ws) > cap:
                assert rc == J.JB_ELIMIT, f"{label}: {rc}"
                assert (s == JUNK).all() and (e == JUNK).all() and (tok == JUNK).all(), f"{label}: written after JB_ELIMIT"
            else:
                assert rc == J.JB_OK, f"{label}: {rc}"
                assert np.array_equal(s[:cnt], ws) and np.array_equal(e[:cnt], we), f"{label}: spans"
                assert (s[cnt:] == JUNK).all() and (e[cnt:] == JUNK).all(), f"{label}: written past the count"
                assert np.array_equal(tok, wd), f"{label}: doc_tok"
        return want

    def postings_batch(self, hmm, b, doc_base=0, short=0, label=""):
        """jb_postings_batch into arrays of the exact count less `short`: too small, it is JB_ELIMIT with the count
        and post_off right and no list written."""
        b = self.batch(b)
        label = f"{label} postings_batch hmm={hmm} {b.spec} doc_base={doc_base} short={short}"
        nd = b.ndocs

        def call():
            nids = len(self.m.keys)
            pcap = max(len(self.m.postings(b, hmm, doc_base)[1]) - short, 0)
            po, dl = np.full(nids + 1, JUNK, np.uint64), np.full(max(nd, 1), JUNK, np.uint32)
            pd, pt = np.full(max(pcap, 1), JUNK, np.uint32), np.full(max(pcap, 1), JUNK, np.uint32)
            n = C.c_uint64(JUNK)
            rc = J.lib().jb_postings_batch(self.tk.h, b.buf.ctypes.data, b.off.ctypes.data, nd, int(hmm), doc_base, pcap,
                                           po.ctypes.data, nids, pd.ctypes.data, pt.ctypes.data, C.byref(n), dl.ctypes.data)
            if rc == J.JB_EINVAL:
                J._check(rc)
            return rc, po, pd, pt, n.value, dl[:nd], pcap

        want, got = self._both("postings_batch", b, lambda: self.m.postings(b, hmm, doc_base), call, label)
        if got is not None:
            rc, po, pd, pt, n, dl, pcap = got
            wo, wd, wt, wl = want
            assert n == len(wd) and np.array_equal(po, wo), f"{label}: count {n} (want {len(wd)}) or post_off"
            if len(wd) > pcap:
                assert rc == J.JB_ELIMIT, f"{label}: {rc}"
                assert (pd == JUNK).all() and (pt == JUNK).all(), f"{label}: lists written after JB_ELIMIT"
            else:
                assert rc == J.JB_OK, f"{label}: {rc}"
                assert np.array_equal(pd[:n], wd) and np.array_equal(pt[:n], wt), f"{label}: the lists"
                assert (pd[n:] == JUNK).all() and (pt[n:] == JUNK).all(), f"{label}: written past the count"
                assert np.array_equal(dl, wl), f"{label}: doc_len"
        return want

    def search_batch(self, hmm, b, topk, label=""):
        """jb_search_batch: the records of every query, every slot; JB_EINVAL where the model has no answer."""
        b = self.batch(b)
        label = f"{label} search_batch hmm={hmm} {b.spec} topk={topk}"

        def call():
            rows = max(b.ndocs, 1) * topk
            rd, rs, rn = np.full(rows, JUNK, np.uint32), np.full(rows, JUNK, np.uint64), np.full(max(b.ndocs, 1), JUNK, np.uint32)
            J._check(J.lib().jb_search_batch(self.tk.h, b.buf.ctypes.data, b.off.ctypes.data, b.ndocs, int(hmm), topk,
                                             rd.ctypes.data, rs.ctypes.data, rn.ctypes.data))
            return rd.reshape(-1, topk)[:b.ndocs], rs.reshape(-1, topk)[:b.ndocs], rn[:b.ndocs]

        want, got = self._both("search_batch", b, lambda: self.m.search(b, hmm, topk), call, label)
        if want is not None:
            self.log.append(("search", b.spec, int((want[2] > 0).sum()), int((want[2] == 0).sum())))
        if got is not None:
            for g, w, name in zip(got, want, ("res_doc", "res_score", "res_n")):
                assert g.shape == w.shape and np.array_equal(g, w), f"{label}: {name}"
        return want

    def neardup(self, B, R, W=64, min_agree=None, short=None, label=""):
        """jb_neardup_sig on the signatures of the last minhash_batch, into arrays of the exact count less `short`
        (None: arrays of no entry at all, which gives the counts only)."""
        if self.sig is None:
            return None
        sig, doc_n, _ = self.sig
        nd, K = sig.shape
        min_agree = J._default_agree(K) if min_agree is None else min_agree
        label = f"{label} neardup B={B} R={R} W={W} min_agree={min_agree} short={short}"
        wo, wd, wa, wst = want = self.m.neardup(sig, doc_n, B, R, W, min_agree)
        self.log.append(("neardup", self.sig[2], len(wd), int(wst[2])))
        if self.tk is None:
            return want
        pcap = 0 if short is None else max(len(wd) - short, 0)
        po, st, n = np.full(nd + 1, JUNK, np.uint64), np.full(J.JB_ND_NSTAT, JUNK, np.uint64), C.c_uint64(JUNK)
        pd, pa = np.full(max(pcap, 1), JUNK, np.uint32), np.full(max(pcap, 1), JUNK, np.uint32)
        rc = J.lib().jb_neardup_sig(self.tk.h, sig.ctypes.data, doc_n.ctypes.data, nd, K, B, R, W, min_agree,
                                    pd.ctypes.data if pcap else None, pa.ctypes.data if pcap else None, pcap,
                                    po.ctypes.data, C.byref(n), st.ctypes.data)
        assert n.value == len(wd) and np.array_equal(po, wo) and np.array_equal(st, wst), \
            f"{label}: count {n.value} (want {len(wd)}), pair_off or the counters {st.tolist()} (want {wst.tolist()})"
        if len(wd) > pcap:
            assert rc == J.JB_ELIMIT, f"{label}: {rc}"
            assert (pd == JUNK).all() and (pa == JUNK).all(), f"{label}: pairs written after JB_ELIMIT"
        else:
            assert rc == J.JB_OK, f"{label}: {rc}"
            k = n.value
            if pcap:
                assert np.array_equal(pd[:k], wd) and np.array_equal(pa[:k], wa), f"{label}: the pairs"
                assert (pd[k:] == JUNK).all() and (pa[k:] == JUNK).all(), f"{label}: written past the count"
        return want

    def colloc_table(self):
        """The driver's collocation table and d_uni between canaries, for the vocabulary as it is: (table pointer,
        bytes, d_uni pointer, nuni).  set_vocab drops both; the next call makes and initialises new ones."""
        import torch
        if self.m.cl is None:
            self.m.colloc_init()
        if self.tk is None:
            return None
        if self.ctable is None:
            nuni = len(self.m.keys)
            n = J.colloc_table_bytes(M.COLLOC_NSLOTS)
            t, u = guarded_bytes(n), guarded(nuni, torch.int64)
            assert (t.data_ptr() + NG) % 32 == 0
            self.tk.colloc_init_device(t.data_ptr() + NG, n, M.COLLOC_NSLOTS, u.data_ptr() + 8 * NG, nuni, self.st())
            torch.cuda.synchronize()
            self.ctable = (t, n, u, nuni)
        t, n, u, nuni = self.ctable
        return t.data_ptr() + NG, n, u.data_ptr() + 8 * NG, nuni

    def colloc_raw(self):
        """The table's and d_uni's bytes, the canaries checked."""
        t, n, u, nuni = self.ctable
        return inner_bytes(t, n).tobytes(), inner(u, nuni, np.uint64).tobytes()

    def colloc_batch(self, hmm, b, keep=None, contig=False, label=""):
        """jb_colloc_batch into the driver's table; keep: None, or a u8 mask over the vocabulary's ids."""
        b = self.batch(b)
        label = f"{label} colloc_batch hmm={hmm} {b.spec} contig={contig}"
        p = self.colloc_table() if self.m.vocab is not None else (0, 0, 0, 0)

        def call():
            self.tk.colloc_batch(b.buf, b.off, hmm, p[0], p[1], p[2], p[3], keep, J.JB_COLLOC_CONTIG if contig else 0)
            return True

        # (a refused call adds nothing: the model raises before it counts)
        self._both("colloc_batch", b, lambda: self.m.colloc_batch(b, hmm, keep, contig) or True, call, label)

    def colloc_read(self, scorer="count", min_count=1, threshold=float("-inf"), topn=0, label=""):
        """jb_colloc_read against the model's table: the candidates in the rule's order with their f32 score bits,
        and the five totals; nothing dropped."""
        import torch
        if self.m.cl is None:
            return None
        rows, totals = self.m.colloc_result(scorer, min_count, threshold, topn)
        if self.tk is None:
            return rows
        p = self.colloc_table()
        label = f"{label} colloc_read {scorer} min_count={min_count} threshold={threshold} topn={topn}"
        r = self.tk.colloc_read(p[0], p[1], p[2], p[3], scorer, min_count, threshold, topn, self.st())
        torch.cuda.synchronize()
        self.colloc_raw()
        assert r.totals() == totals, f"{label}: totals {r.totals()}, want {totals}"
        assert (r.a.tolist(), r.b.tolist(), r.count.tolist()) == (
            [x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows]), f"{label}: the candidates"
        want = np.array([x[3] for x in rows], np.float32)
        assert np.array_equal(r.score.view(np.uint32), want.view(np.uint32)), f"{label}: the scores' bits"
        return rows

    def set_stop(self, keys):
        self.m.set_stop(keys)
        if self.tk is not None:
            self.tk.set_stop_words(keys)
            assert self.tk.stop_words_size == (-1 if keys is None else len(set(keys)))

    def set_filter(self, rule):
        """jb_batch_filter_set; None clears."""
        self.m.set_filter(rule)
        if self.tk is None:
            return
        if rule is None:
            self.tk.clear_batch_filter()
        else:
            self.tk.set_batch_filter(rule.drop, rule.min_runes, rule.max_runes, rule.stop)

    def build_index(self, batches, hmm=True, k1=1.2, b=0.75, label=""):
        """postings_batch of each batch with doc_base advancing (each checked), the model's merge of them, and
        jb_index_set of that: jb_index_info must describe it."""
        batches = [self.batch(x) for x in batches]
        base = 0
        for x in batches:
            self.postings_batch(hmm, x, base, label=f"{label} build_index")
            base += x.ndocs
        ix = self.m.build_index(batches, hmm)
        self.m.set_index(ix, k1, b)
        if self.tk is not None:
            self.tk.set_index(ix.post_off, ix.post_doc, ix.post_tf, ix.doc_len, k1=k1, b=b)
            assert self.tk.index_info() == (len(ix.doc_len), ix.nids, len(ix.post_doc), BR.avgdl(ix.doc_len)), label
        return ix

    def clear_index(self):
        self.m.set_index(None)
        if self.tk is not None:
            self.tk.clear_index()

    # -- the rest
    def add_word(self, word, freq):
        assert self.m.reachable(word), word  # (every word these tests add becomes an edge of buildDag)
        self.lastdev = None
        self.tk.AddWord(word, freq)
        f = self.m.add_word(word, freq)
        assert self.m.is_edge(word), word
        assert self.tk.dict_get(word) == f and self.tk.size == self.m.o.size, (word, freq)

    def set_vocab(self, keys):
        self.tk.set_vocab(keys)
        self.m.set_vocab(keys)
        assert self.tk.vocab_size == len(keys)
        self.ctable = self.m.cl = None  # (the table's ids were the old vocabulary's: colloc_table starts anew)

    def stats(self, label=""):
        """jb_last_stats describes the ctx's last cut, whichever call made it."""
        if self.m.last_tokens is not None:
            assert self.tk.last_stats()["tokens"] == self.m.last_tokens, f"{label} last_stats"

    def run(self, op):
        k = op[0]
        if k == "cut":
            self.cut(op[1], op[2], op[3], op[4])
        elif k == "add_word":
            self.add_word(self.m.pick_word(op[1]), op[2])
        elif k == "set_vocab":
            self.set_vocab(self.m.vocab_keys(op[1]))
        elif k == "ids":
            if self.last is not None:
                self.ids(op[1])
        elif k == "keywords_batch":
            self.keywords(op[1], op[2], op[3])
        elif k == "df_batch":
            self.df(op[1], op[2])
        elif k == "textrank_batch":
            self.textrank(op[1], op[2], *op[3:])
        elif k == "last_stats":
            self.stats()
        elif k == "join_batch":
            self.join_batch(*op[1:])
        elif k == "join":
            self.join(op[1], op[2])
        elif k == "charspans_batch":
            self.charspans_batch(*op[1:])
        elif k == "charspans":
            self.charspans(op[1], op[2])
        elif k == "wc_batch":
            self.wc_batch(op[1], op[2], op[3])
        elif k == "wc_read":
            self.wc_read()
        elif k == "minhash_batch":
            self.minhash_batch(op[1], op[2], op[3], op[4], op[5], dups=op[3][0] == "dups")
        elif k == "filter_batch":
            self.filter_batch(op[1], op[2], op[3], M.RULES[op[4]])
        elif k == "postings_batch":
            self.postings_batch(op[1], op[2])
        elif k == "search_batch":
            self.search_batch(op[1], op[2], op[3])
        elif k == "colloc_batch":
            self.colloc_batch(op[1], op[2], self.m.keep if op[3] else None, op[4])
        elif k == "colloc_read":
            self.colloc_read(op[1], 2 if op[1] != "count" else 1, 0.1 if op[1] != "count" else float("-inf"))
        elif k == "neardup":
            self.neardup(op[1], op[2], 64, op[3], short=0)
        elif k == "set_stop":
            self.set_stop(self.m.stop_keys(op[1]))
        elif k == "set_filter":
            self.set_filter(M.RULES[op[1]])
        elif k == "clear_filter":
            self.set_filter(None)
        elif k == "build_index":
            self.build_index([x for x in op[1:3] if x is not None], True, op[3], op[4])
        elif k == "clear_index":
            self.clear_index()
        else:
            raise ValueError(op)


class DryDriver(Driver):
    """A Driver without a library: the model's side of every call and nothing else.  test_ctx_model.py runs the
    scripts below through it on the CPU, to see what their word-count tables have to hold."""

    def __init__(self, model, s=None):
        super().__init__(None, model, s)

    def cut(self, mode, hmm, route, b, reps=None, label=""):
        b = self.batch(b)
        want = self.m.cut(b, mode, hmm)
        self.last = (b, want)
        into = route == "device_into"
        self.lastdev = None if route == "host" else dict(
            b=b, mode=mode, hmm=hmm, into=into, ptrs=None, outs=None,
            cap=max(len(want[0]), b.nbytes, 1) if into else b.nbytes)
        return want

    def _batch_call(self, kind, b):
        self.lastdev = None
        self.calls.append((kind, self.batch(b).nbytes))

    def ids(self, route, label=""):
        pass

    def keywords(self, hmm, b, topk, label=""):
        self._batch_call("keywords_batch", b)

    def df(self, hmm, b, label=""):
        self._batch_call("df_batch", b)

    def textrank(self, hmm, b, span=5, iters=10, topk=20, label=""):
        self._batch_call("textrank_batch", b)

    def add_word(self, word, freq):
        self.lastdev = None
        self.m.add_word(word, freq)

    def set_vocab(self, keys):
        self.m.set_vocab(keys)
        self.m.cl = None

    def stats(self, label=""):
        pass


# ---- fixtures -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def syn(syn_small):
    dp, ep, s = syn_small
    with open(dp, "rb") as f:
        d = f.read()
    with open(ep, "rb") as f:
        e = f.read()
    return d, e, s, M.make_batch(s, M.VOCAB_SOURCE)


@pytest.fixture(scope="module")
def mini(mini_paths):
    with open(mini_paths[0], encoding="utf-8") as f:
        d = f.read()
    with open(mini_paths[1], "rb") as f:
        e = f.read()
    return d if d.endswith("\n") else d + "\n", e


def open_20k(syn, wc_sizes=(M.WC_NSLOTS, M.WC_POOL)):
    d, e, s, source = syn
    tk = J.Tokenizer(J.make_config(dict_bytes=d, emit_bytes=e))
    return Driver(tk, M.Model(d, e, source=source), s, wc_sizes)


def open_text(dict_text, emit, wc_sizes=(M.WC_NSLOTS, M.WC_POOL)):
    tk = J.Tokenizer(J.make_config(dict_bytes=dict_text.encode(), emit_bytes=emit))
    return Driver(tk, M.Model(dict_text.encode(), emit), None, wc_sizes)


def dry_20k(syn):
    d, e, s, source = syn
    return DryDriver(M.Model(d, e, source=source), s)


def dry_text(dict_text, emit):
    return DryDriver(M.Model(dict_text.encode(), emit))


def at_edge(d, run, before="a", after="b"):
    """A document of two text tiles: `before` bytes, then `run`, whose byte d lies on the edge between them."""
    rb = run.encode()
    pre = TILE - d
    assert 0 < pre and pre + len(rb) < 2 * TILE
    return before.encode() * pre + rb + b" " + after.encode() * (2 * TILE - pre - len(rb) - 1)


def every_route(dr, b, combos=COMBOS, label=""):
    for mode, hmm in combos:
        for route in M.ROUTES:
            dr.cut(mode, hmm, route, b, reps=1 if route == "device_into" else None, label=label)


# ---- scripted sequences ---------------------------------------------------------------------------------------
def test_add_word_reaches_every_mode(syn):
    """A 64 KiB device batch in each mode three times (direct, captured, replayed), AddWord, the same twelve
    calls, then the ids of the new spans: no mode may replay a graph that holds the old image."""
    dr = open_20k(syn)
    try:
        m, b = dr.m, dr.batch(("small", 31, 64 << 10))
        assert 32 << 10 < b.nbytes <= 64 << 10
        dr.set_vocab(m.vocab_keys(0))
        for mode, hmm in COMBOS:
            dr.cut(mode, hmm, "device", b, label="before")
        before = m.cut(b, "plain", True, count=False)
        word = m.pick_word(0, b)
        dr.add_word(word, 10_000_000)
        after = m.cut(b, "plain", True, count=False)
        assert len(after[0]) != len(before[0]) or not np.array_equal(after[0], before[0])  # (the reference's lists)
        for mode, hmm in COMBOS:
            dr.cut(mode, hmm, "device", b, label="after")
            dr.ids("device", "after")
            dr.ids("host", "after")
        fs, fe, _ = m.cut(b, "full", False, count=False)
        wb = word.encode()
        assert any(bytes(b.buf[int(x):int(y)]) == wb for x, y in zip(fs[fe - fs == len(wb)], fe[fe - fs == len(wb)]))
    finally:
        dr.tk.close()


G12 = "鼠牛虎兔龍蛇馬羊猴雞狗豬"  # (none of them in the mini dictionary)
# Words of n distinct runes, one per n, that start at different runes and are not inside one another
FAM = {9: G12[:9], 10: G12[1:11], 12: G12[::-1]}
FAM2 = 10 ** 12  # the frequency of a word's first two runes (see reach_dict)


def reach_dict(mini_text, chain):
    """The chain of 甲 (chain: its lines) with 甲 x 11 as a key of frequency 0, the mini dictionary, and the
    makings of three look-backs: the runes of G12 frequent, so that Cut takes them one by one, and of each
    word of FAM its prefixes of 3 .. n - 1 runes as keys of frequency 0.  Its two-rune prefix is missing, so
    nothing of a family can be reached and the longest reachable key has 8 runes.  AddWord of the two-rune
    prefix opens the family; its frequency FAM2 lies where the reference's maxIndexProba (tokenizer.go:565-578,
    which compares each item with the one before it) still takes the single rune: over the whole word's
    weight plus n - 2 singles, under two singles."""
    return (chain + mini_text + f"{'甲' * 11} 0\n" + "".join(f"{r} {10 ** 14}\n" for r in G12) +
            "".join(f"{w[:k]} 0\n" for n, w in FAM.items() for k in range(3, n)))


@pytest.mark.parametrize("chain", ["as the issue states it", "with a plain record first"])
def test_add_word_moves_maxlen_and_the_record_limits(mini, chain):
    """AddWord of 甲 x 9, x 10 and x 12 to a dictionary whose longest key has 8 runes: the first edge longer
    than 8 runes, then a longest key past full_back's `maxlen > 9` branch.  After each add, search and full
    mode through the host and both device calls, on 甲 x 200 between ASCII and a 4-byte rune around a
    text-tile edge.

    Two corrections to the issue's recipe, both asserted from Oracle.build_dag below.  With F.chain_dict(8)
    the first 甲 of a run has 8 edges before any add, so its record is zero from the start (more than four
    edges); the second parametrisation keeps 甲 x 2 .. x 7 as keys of frequency 0, so that 甲 has the two
    edges {1, 8} and the add of 甲 x 9 is what turns the record zero.  And 甲 x 12 is reachable only with
    甲 x 11 a key (AddWord adds no prefixes): the dictionary holds it with frequency 0, out of reach until
    甲 x 9 and x 10 are keys.
    A text of 甲 alone never looks back further than one rune, whatever maxlen is (every 甲 but the last has
    a word), so the reach itself is checked with a second family: after 甲 x n, a word of n distinct runes
    is added (FAM), whose last rune, a plain token of its own, finds the word n - 1 runes back, which takes
    maxlen >= n."""
    mini_text, emit = mini
    lines = F.chain_dict(8) if chain == "as the issue states it" else (
        "甲 100\n" + "".join(f"{'甲' * k} 0\n" for k in range(2, 8)) + f"{'甲' * 8} 108\n")
    dr = open_text(reach_dict(mini_text, lines), emit)
    try:
        m = dr.m
        run = "甲" * 200
        fam = "".join(w + w[0] + X4 + "c" for w in FAM.values())
        docs = [("a" * 5 + fam + "b " + run).encode()]  # (the head of a batch: bytes under 32)
        docs += [at_edge(d, run + X4 + "c" + fam) for d in (1, 2, 3, 299, 300, 598, 599, 600, 601, 604, 605)]
        docs += [at_edge(d, fam + run) for d in range(0, len(fam.encode()), 5)]
        b = M.from_texts(("reach",), docs)
        edges0 = m.o.build_dag(run)[0]
        assert edges0 == (list(range(1, 9)) if chain == "as the issue states it" else [1, 8])
        every_route(dr, b, COMBOS[2:], "before")
        for n, w in FAM.items():
            dr.add_word("甲" * n, 100 + n)
            edges = m.o.build_dag(run)[0]
            # (an edge of more than 8 runes: a zero record)
            assert edges == edges0 + [k for k in FAM if k <= n] and max(edges) == n
            every_route(dr, b, COMBOS[2:], f"甲 x {n}")
            assert not m.reachable(w)
            dr.add_word(w[:2], FAM2)
            dr.add_word(w, 1)
            assert m.o.build_dag(w + w[0])[0] == [1, 2, n] and m.o.cut(w + w[0], False) == list(w + w[0])
            # (from the reference: the word's last rune is covered from n - 1 runes back, the rune behind is not)
            assert F.expected_text(m.o, w + w[0], m.blocks) == [w[:2], w, w[0]]
            every_route(dr, b, COMBOS[2:], f"{n} distinct runes")
            dr.stats()
    finally:
        dr.tk.close()


def test_a_fifth_edge(mini):
    """甲 has exactly four edges in chain_dict(4); 甲 x 5 gives it a fifth, so its record turns zero and the
    mode passes walk the trie for it (srch_edges, full_walk)."""
    mini_text, emit = mini
    dr = open_text(F.chain_dict(4) + mini_text, emit)
    try:
        m = dr.m
        run = "甲" * 40
        assert m.o.build_dag(run)[0] == [1, 2, 3, 4]
        docs = [run, "今天天氣很好" + run + "，一刹那" + "甲" * 5, "甲" * 4 + "a" + "甲" * 5 + X4 + "甲" * 6]
        docs += [at_edge(d, run + X4 + "一刹那") for d in (2, 3, 30, 60, 119, 120)]
        b = M.from_texts(("fifth",), docs)
        every_route(dr, b, label="four edges")
        dr.add_word("甲" * 5, 105)
        assert m.o.build_dag(run)[0] == [1, 2, 3, 4, 5]
        every_route(dr, b, label="five edges")
        dr.stats()
    finally:
        dr.tk.close()


def test_a_word_with_a_four_byte_rune(mini):
    """A word whose runes include 4-byte ones, added to a dictionary that holds its proper prefixes, cut in
    the three modes around a text-tile edge before and after."""
    _, emit = mini
    word = "𠀀𠀁中𪜀"
    lines = "𠀀 10\n𠀀𠀁 20\n𠀀𠀁中 30\n𠀁 3\n𠀁中 9\n中 50\n中𪜀 8\n𪜀 4\n"
    dr = open_text(lines, emit)
    try:
        m = dr.m
        run = "a" + word + "𠀀𠀁中" + word
        n = len(run.encode())
        b = M.from_texts(("x4",), [run] + [at_edge(d, run) for d in range(0, n + 1)])
        assert m.o.get(word) is None and 4 not in m.o.build_dag(word)[0]
        every_route(dr, b, label="before")
        dr.add_word(word, 40)
        assert 4 in m.o.build_dag(word)[0]
        # (now the dictionary of the hand-worked example)
        assert R.expected_text(m.o, "a𠀀𠀁中𪜀𠀀𠀁中", True) == R.EXAMPLES[2][1][0][1]
        every_route(dr, b, label="after")
    finally:
        dr.tk.close()


def test_frequency_change_and_suggested_frequency(syn):
    """An existing word added again with another frequency: the dictionary's size, and with it every weight,
    moves.  Then AddWord(w, 0), whose frequency the library suggests from its own cut of the word."""
    dr = open_20k(syn)
    try:
        m, b = dr.m, dr.batch(("small", 310, 40 << 10))
        for mode, hmm in (("plain", True), ("search", True)):
            dr.cut(mode, hmm, "host", b, label="before")
            dr.cut(mode, hmm, "device", b, label="before")
        s, e, _ = m.cut(b, "plain", True, count=False)
        two = [bytes(b.buf[int(x):int(y)]).decode("utf-8", "replace") for x, y in zip(s[e - s == 6], e[e - s == 6])]
        word = next(w for w in two if len(w) == 2 and (m.o.get(w) or 0) > 0 and m.reachable(w))
        size0, f0 = m.o.size, m.o.get(word)
        dr.add_word(word, 50 * f0 + 12_345)
        assert dr.tk.size == size0 + 50 * f0 + 12_345 == m.o.size  # (addTerm adds to the size, tokenizer.go:580-585)
        for mode, hmm in (("plain", True), ("search", True)):
            dr.cut(mode, hmm, "host", b, label="another frequency")
            dr.cut(mode, hmm, "device", b, label="another frequency")
        w2 = m.pick_word(0)
        want, pieces = m.suggest(w2)
        assert dr.tk.suggest_freq(w2) == want
        dr.add_word(w2, 0)
        assert dr.tk.dict_get(w2) == want and m.last_tokens == len(pieces)
        dr.stats("the cut AddWord made")
        for mode, hmm in (("plain", True), ("search", True)):
            dr.cut(mode, hmm, "host", b, label="suggested frequency")
            dr.cut(mode, hmm, "device", b, label="suggested frequency")
    finally:
        dr.tk.close()


def test_saved_image_in_every_mode(syn, tmp_path):
    """save after two AddWords, FromImage: the new tokenizer cuts, looks ids up and ranks as the same model."""
    dr = open_20k(syn)
    tk2 = None
    try:
        m, b = dr.m, dr.batch(("small", 520, 48 << 10))
        dr.cut("plain", True, "device", b)
        dr.add_word(m.pick_word(0), 10_000_000)
        dr.cut("full", False, "device", b)
        dr.add_word(m.pick_word(1), 0)
        path = str(tmp_path / "two_adds.jbimg")
        dr.tk.save(path)
        tk2 = J.Tokenizer.FromImage(path)
        assert tk2.size == m.o.size
        m.last_tokens = None  # (a new ctx has cut nothing)
        d2 = Driver(tk2, m, dr.s)
        d2.set_vocab(m.vocab_keys(2))
        every_route(d2, b, label="from the image")
        d2.ids("device")
        d2.ids("host")
        d2.textrank(True, dr.batch(("small", 530, 36 << 10)))
        d2.stats()
    finally:
        dr.tk.close()
        if tk2 is not None:
            tk2.close()


def test_workspace_growth_between_captured_graphs(syn):
    """A (8 KiB), B (300 KiB), A again on the same device buffers, C (1,500 documents of one or two runes:
    growth by the document count alone), A again: each three times in each mode, so that every mode has a
    captured graph when the workspace is replaced under it.
    The issue words the first condition as "A is under the 4,096-byte minimum"; with A at 8 KiB that cannot
    hold, and what the sequence needs is asserted instead: A is over the minimum, so the first call
    allocates A's own size and no more, and B, over every earlier size, has to grow it."""
    dr = open_20k(syn)
    try:
        buf, off, _ = dr.s.corpus(synth.KIND_SENTENCES, 40, target_bytes=8 << 10)
        a = M.Batch(("A",), buf, off)
        b, c = dr.batch(("grow", 50, 300 << 10)), dr.batch(("manydocs", 60, 1500))
        assert M.WORK_MIN_BYTES < a.nbytes <= 9 << 10 and a.ndocs <= M.WORK_MIN_DOCS
        assert b.nbytes > 250 << 10 and b.nbytes > a.nbytes and b.ndocs <= M.WORK_MIN_DOCS
        assert c.nbytes < b.nbytes and c.ndocs == 1500 > M.WORK_MIN_DOCS
        assert 1 <= np.diff(c.off.astype(np.int64)).min() and np.diff(c.off.astype(np.int64)).max() <= 8
        for x in (a, b, a, c, a):
            for mode, hmm in COMBOS:
                dr.cut(mode, hmm, "device", x)
            dr.stats()
        for x in (b, a):  # (and into caller-owned arrays)
            for mode, hmm in COMBOS:
                dr.cut(mode, hmm, "device_into", x, reps=3)
    finally:
        dr.tk.close()


def test_small_batches_follow_the_image(syn):
    """Plain host batches of at most 4,096 bytes (k_small) between a 64 KiB host batch (the piece pipeline)
    and a device call, with batches of empty documents among them, before and after AddWord; after every call
    jb_last_stats reports that call's tokens."""
    dr = open_20k(syn)
    try:
        m = dr.m
        t1, t2 = dr.batch(("tiny", 900, 8)), dr.batch(("tiny", 910, 3))
        h, d = dr.batch(("small", 920, 64 << 10)), dr.batch(("small", 930, 40 << 10))
        none = dr.batch(("empty", 0, 4))
        assert t1.nbytes <= M.SMALL_MAX and t2.nbytes <= M.SMALL_MAX and h.nbytes > 32 << 10
        word = m.pick_word(0, t1)

        def lap(label):
            for hmm in (True, False):
                for x, mode, route in ((t1, "plain", "host"), (h, "plain", "host"), (t2, "plain", "host"),
                                       (d, "plain", "device"), (t1, "plain", "host"), (d, "search", "device"),
                                       (t2, "plain", "host"), (h, "full", "host"), (t1, "search", "host"),
                                       (t2, "plain", "host"), (d, "plain", "device_into"), (t1, "plain", "host"),
                                       (none, "plain", "host"), (t2, "plain", "host"), (none, "search", "host"),
                                       (d, "plain", "device"), (none, "plain", "device"), (h, "plain", "host"),
                                       (none, "full", "device_into"), (t1, "plain", "host")):
                    dr.cut(mode, hmm, route, x, reps=1, label=label)
                    dr.stats(f"{label} after {mode} {route} {x.spec} hmm={hmm}")

        lap("before")
        before = [m.cut(x, "plain", hmm, count=False) for x in (t1, t2) for hmm in (True, False)]
        dr.add_word(word, 10_000_000)
        dr.stats("after AddWord")
        after = [m.cut(x, "plain", hmm, count=False) for x in (t1, t2) for hmm in (True, False)]
        assert any(len(x[0]) != len(y[0]) for x, y in zip(before, after))  # (the small batches' answers move)
        lap("after")
    finally:
        dr.tk.close()


def test_batch_calls_share_their_buffers(syn):
    """keywords_batch, textrank_batch and df_batch on one ctx, in a changing order: a 200 KiB batch, one
    3-byte document, five empty documents, the large buffer from its document 3 on (doc_off[0] != 0), a
    smaller vocabulary with a longer longest key, AddWord, and the large batch again."""
    dr = open_20k(syn)
    try:
        m = dr.m
        big = dr.batch(("large", 1700, 200 << 10))
        one, none = M.from_texts(("one",), ["中"]), dr.batch(("empty", 0, 5))
        tail = M.Batch(("tail",), big.buf, big.off[3:])
        assert big.nbytes > 150 << 10 and one.nbytes == 3 and none.nbytes == 0 and none.ndocs == 5 and int(tail.off[0]) > 0
        v1, v2 = m.vocab_keys(0), m.vocab_keys(1)
        assert len(v2) < len(v1) and max(map(len, v2)) > max(map(len, v1)) == 6
        assert sum(1 for k in v2[:-1] if len(k) > 6) > 20  # (tokens of the text that only the new maxlen admits)

        def calls(b, order, label):
            out = {}
            for k in order:
                if k == "k":
                    out[k] = dr.keywords(True, b, 20, label)
                elif k == "t":
                    out[k] = dr.textrank(True, b, label=label)
                else:
                    out[k] = dr.df(True, b, label)
                dr.stats(label)
            return out

        dr.set_vocab(v1)
        got = calls(big, "ktd", "1")
        assert got["k"][3].max() == 20 and got["t"][2].max() == 20 and int(got["d"].sum()) > 10 * big.ndocs
        calls(one, "tdk", "2")
        got = calls(none, "dkt", "3")
        assert not got["d"].any()  # the counters unchanged
        assert not got["k"][3].any() and (got["k"][0] == J.JB_ID_UNK).all() and not got["k"][1].any()
        assert not got["t"][2].any() and (got["t"][0] == J.JB_ID_UNK).all() and not got["t"][1].any()
        calls(tail, "tkd", "4")
        dr.set_vocab(v2)
        calls(big, "dtk", "5")
        calls(one, "kdt", "5")
        dr.add_word(m.pick_word(0, big), 10_000_000)
        calls(big, "kdt", "6")
        calls(none, "tkd", "6")
        calls(big, "tdk", "7")
    finally:
        dr.tk.close()


# ---- random sequences -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", M.SEEDS)
def test_random_sequences(syn, seed):
    """gen_ops(seed, NSTEPS) on one tokenizer, every step against the model.  A failure names the seed, the
    step and the ops up to it: `Driver.run` over that list replays it."""
    ops = M.gen_ops(seed, M.NSTEPS)
    dr = open_20k(syn)
    try:
        dr.set_vocab(dr.m.vocab_keys(0))
        for i, op in enumerate(ops):
            try:
                dr.run(op)
            except (AssertionError, J.JbError) as e:
                raise AssertionError(f"seed {seed}, step {i}: {op!r}\nops = {ops[:i + 1]!r}\n{e}") from e
    finally:
        dr.tk.close()


# ---- joined text, character offsets and word counts among the older calls --------------------------------------
# Each script takes a Driver and makes the calls; the test opens a tokenizer for it.  test_ctx_model.py runs the
# scripts that fill a word-count table through a DryDriver first: the table must never be what limits a test.
def arena_order(first, second):
    """Kinds alternately of `first` and of `second`: every pair of one of `first` directly followed by one of
    `second`, and every pair the other way round, is a neighbouring pair (2 * len(first) * len(second) + 1 kinds:
    19 for three kinds each)."""
    seq = []
    for shift in range(len(second)):
        for i in range(len(first)):
            seq += [first[i], second[(i + shift) % len(second)]]
    return seq + [first[0]]


def arena_pairs(calls):
    """{(kind, next kind, tiny_then_large)} of the neighbouring *_batch calls that cross 4,096 bytes."""
    return {(k0, k1, n1 > M.SMALL_MAX) for (k0, n0), (k1, n1) in zip(calls, calls[1:])
            if (n0 > M.SMALL_MAX) != (n1 > M.SMALL_MAX)}


def script_arenas(dr):
    m = dr.m
    big = dr.batch(("large", 1700, 200 << 10))
    one, none = M.from_texts(("one",), ["中"]), dr.batch(("empty", 0, 5))
    tail = M.Batch(("tail",), big.buf, big.off[3:])
    assert big.nbytes > 150 << 10 and one.nbytes == 3 and none.nbytes == 0 and none.ndocs == 5 and int(tail.off[0]) > 0
    v1, v2 = m.vocab_keys(0), m.vocab_keys(1)
    assert len(v2) < len(v1)
    # (a large batch keeps one mode per kind, so that the references are few; the tiny ones take them in turn)
    modes = {("join_batch", big.spec): "plain", ("join_batch", tail.spec): "search",
             ("charspans_batch", big.spec): "search", ("charspans_batch", tail.spec): "full",
             ("wc_batch", big.spec): "full", ("wc_batch", tail.spec): "plain"}
    step = [0]

    def call(kind, b):
        i = step[0]
        step[0] += 1
        label = f"call {i}"
        mode = modes.get((kind, b.spec), M.MODES[i % 3])
        hmm = mode != "full" and (b.nbytes > M.SMALL_MAX or i % 2 == 0)
        if kind == "keywords_batch":
            dr.keywords(True, b, 20, label)
        elif kind == "df_batch":
            dr.df(True, b, label)
        elif kind == "textrank_batch":
            dr.textrank(True, b, label=label)
        elif kind == "join_batch":
            dr.join_batch(mode, hmm, b, JR.SEPS[i % 4], JR.SEPS[(i + 1) % 4], label)
        elif kind == "charspans_batch":
            # (new arrays for a tiny batch, 1,024 entries; a large one is handed the arrays of the call before)
            dr.charspans_batch(mode, hmm, b, ("rune", "utf16")[i % 2], b.nbytes > M.SMALL_MAX, label)
        else:
            dr.wc_batch(mode, hmm, b, label)
        dr.stats(label)

    dr.set_vocab(v1)
    # the five batches of test_batch_calls_share_their_buffers in their order, a kind of each set in turn
    for kind, b in zip(("keywords_batch", "join_batch", "df_batch", "charspans_batch", "textrank_batch", "wc_batch"),
                       (big, one, none, tail, big, big)):
        call(kind, b)
    # then the sizes alternate: an older kind on each large batch and a new kind on each tiny one, ...
    for k, kind in enumerate(arena_order(M.BATCH_OPS, M.NEW_BATCH_OPS)):
        call(kind, ((big, tail)[(k // 2) % 2], (one, none)[(k // 2) % 2])[k % 2])
    dr.wc_read("half way")
    dr.set_vocab(v2)
    # ... and the other way round
    for k, kind in enumerate(arena_order(M.NEW_BATCH_OPS, M.BATCH_OPS)):
        if k == 14:
            dr.add_word(m.pick_word(0, big), 10_000_000)
            dr.stats("after AddWord")
        call(kind, ((big, tail)[(k // 2) % 2], (one, none)[(k // 2) % 2])[k % 2])
    dr.wc_read("at the end")
    want = {(a, b, up) for a in M.BATCH_OPS for b in M.NEW_BATCH_OPS for up in (False, True)}
    want |= {(b, a, up) for a, b, up in want}
    assert len(want) == 36 and want <= arena_pairs(dr.calls), sorted(want - arena_pairs(dr.calls))
    assert dr.too_small >= 1  # (the span arrays of a tiny batch were handed to a large one)


def test_new_batch_calls_share_the_arenas(syn):
    """The six *_batch kinds on one ctx with a vocabulary, over a 200 KiB batch, one 3-byte document, five empty
    documents and the large buffer from its document 3 on, a smaller vocabulary and an AddWord in between,
    jb_last_stats after every call: every ordered pair of an older kind and a new one, both ways round, lies on
    a large-then-tiny and on a tiny-then-large transition (asserted from the driver's call list)."""
    dr = open_20k(syn)
    try:
        script_arenas(dr)
    finally:
        dr.tk.close()


REGROW_K, REGROW_N = 5, 11  # the smallest chain and run whose full-mode list is longer than the text (test_ctx_model.py)


def regrow_dict(mini_text):
    return F.chain_dict(REGROW_K) + mini_text


def script_regrow(dr):
    m = dr.m
    full = M.from_texts(("regrow",), ["甲" * REGROW_N])
    tiny = M.from_texts(("mini",), ["今天天氣很好", "", "一刹那，量子力學"])
    smaller = M.from_texts(("smaller",), ["甲" * 3 + "很好"])
    fs, fe, _ = m.cut(full, "full", False, count=False)
    assert len(fs) > full.nbytes and smaller.nbytes < full.nbytes  # (from full_ref.expected: the call cuts twice)
    keys = set()
    for b in (full, tiny, smaller):
        s, e, _ = m.cut(b, "plain", True, count=False)
        keys |= {bytes(b.buf[int(x):int(y)]) for x, y in zip(s, e)}
    dr.set_vocab(sorted(keys))
    for k, (what, args) in enumerate((
            ("join", ("full", False, full, b" ", b"\n")), ("keywords", (True, tiny, 5)),
            ("charspans", ("full", False, full, "rune", False)), ("charspans", ("full", False, full, "utf16", True)),
            ("textrank", (True, full)), ("wc", ("full", False, full)), ("df", (True, full)),
            ("join", ("full", False, full, b"<-sep8->", b"")), ("join", ("plain", True, smaller, b"\xe3\x80\x80", b"\n")))):
        f = {"join": dr.join_batch, "keywords": dr.keywords, "charspans": dr.charspans_batch, "textrank": dr.textrank,
             "wc": dr.wc_batch, "df": dr.df}[what]
        f(*args, label=f"call {k}")
        dr.stats(f"after call {k} ({what})")
    dr.wc_read()


def test_full_mode_regrow_then_everything_else(mini):
    """A full-mode list longer than its batch has bytes makes the three new calls move the span arrays into the
    ids/terms arena and cut again; here each is followed by the calls that own that arena, and by itself."""
    mini_text, emit = mini
    dr = open_text(regrow_dict(mini_text), emit)
    try:
        script_regrow(dr)
    finally:
        dr.tk.close()


HAN = ("一", "龥")  # (three bytes each)


def twin(b):
    """A batch of b's shape (doc_off, bytes, documents) and other content: every Han rune replaced by the next
    Han rune of the text."""
    a, end = int(b.off[0]), int(b.off[-1])
    text = bytes(b.buf[a:end]).decode("utf-8")
    han = [c for c in text if HAN[0] <= c <= HAN[1]]
    nxt = iter(han[1:] + han[:1])
    out = "".join(next(nxt) if HAN[0] <= c <= HAN[1] else c for c in text).encode()
    assert len(out) == end - a and out != bytes(b.buf[a:end])
    buf = b.buf.copy()
    buf[a:end] = np.frombuffer(out, np.uint8)
    return M.Batch(("twin",) + tuple(b.spec), buf, b.off)


SAME_SHAPE_TABLE = (1 << 16, 1 << 18)  # (read after every call: a small one)


def script_same_shape(dr):
    m = dr.m
    b = dr.batch(("small", 777, 36 << 10))
    t = dr.batch(twin(b))
    assert np.array_equal(b.off, t.off) and b.nbytes == t.nbytes and b.ndocs == t.ndocs and len(b.buf) == len(t.buf)
    ps, pt = m.cut(b, "plain", True, count=False), m.cut(t, "plain", True, count=False)
    assert len(ps[0]) != len(pt[0]) or not np.array_equal(ps[0], pt[0])  # (the model's spans differ)
    dr.set_vocab(m.vocab_keys(0))
    shared = np.zeros_like(b.buf)
    for own in (False, True):  # from one host address, then from each batch's own
        for kind in M.NEW_BATCH_OPS:
            for mode in M.MODES:
                for k, x in enumerate((b, b, t, t, b)):
                    label = f"{'own' if own else 'shared'} buffer, call {k}"
                    shared[:] = x.buf
                    buf = None if own else shared
                    if kind == "join_batch":
                        dr.join_batch(mode, mode != "full", x, b" ", b"\n", label, buf=buf)
                    elif kind == "charspans_batch":
                        dr.charspans_batch(mode, mode != "full", x, "utf16", True, label, buf=buf)
                    else:
                        dr.wc_batch(mode, mode != "full", x, label, buf=buf)
                        dr.wc_read(label)
                    dr.stats(label)
    for x in (b, t, t, b):
        dr.keywords(True, x, 5, "same shape")


def test_same_shape_other_text(syn):
    """Two batches of one shape and different content, B B B' B' B, through each new *_batch call in each mode:
    the cut's graph key holds no text, so the second and later calls replay; each must answer for its own text."""
    dr = open_20k(syn, SAME_SHAPE_TABLE)
    try:
        script_same_shape(dr)
    finally:
        dr.tk.close()


def test_charspans_in_place_on_the_ctx_arrays(syn):
    """jb_charspans_device in place on the arrays jb_cut_device returned (the ctx's own), then the same cut
    again, a replay, which must put byte spans back; ids and the joined text of the result."""
    dr = open_20k(syn)
    try:
        b = dr.batch(("small", 410, 40 << 10))
        dr.set_vocab(dr.m.vocab_keys(0))
        for mode in ("plain", "search"):
            for unit in ("rune", "utf16"):
                dr.cut(mode, True, "device", b)  # (direct, captured, replayed)
                assert dr.lastdev is not None and not dr.lastdev["into"]
                n = dr.restored
                dr.charspans(unit, True, f"{mode}")
                assert dr.restored == n + 1 and dr.lastdev is not None
                dr.ids("device", mode)
                dr.join(b" ", b"\n", mode)
                dr.charspans(unit, False, f"{mode}")
                dr.stats(mode)
    finally:
        dr.tk.close()


def test_joined_results_outlive_calls_and_contexts(syn):
    """The arrays Tokenizer.cut_batch_join hands out are the library's pinned blocks, of which jb_joined_free
    keeps one per process: a held result stays what it was over later joins, a second ctx and its owner's close."""
    d, e, s, source = syn
    m = M.Model(d, e, source=source)
    big, mid, small = (M.make_batch(s, sp) for sp in (("large", 1700, 120 << 10), ("small", 1710, 40 << 10), ("tiny", 1720, 6)))

    def join(tk, b, sep=b" ", term=b"\n"):
        out, off = tk.cut_batch_join(b.buf, b.off, True, "cut", sep, term)
        want, woff = m.join(b, "plain", True, sep, term)
        assert out.tobytes() == want and off.tolist() == woff, (b.spec, sep)
        return out, want

    tk1 = J.Tokenizer(J.make_config(dict_bytes=d, emit_bytes=e))
    tk2 = tk3 = None
    try:
        # A: a held result over two smaller joins, their release, and a larger one
        held, want = join(tk1, big)
        s1, s2 = join(tk1, mid), join(tk1, small)
        del s1, s2
        gc.collect()
        larger, wl = join(tk1, big, b"<-sep8->", b"<-sep8->")
        assert len(larger) > len(held) and held.tobytes() == want and larger.tobytes() == wl
        # B: a second ctx, joins on both in turn, the first closed under a held result
        tk2 = J.Tokenizer(J.make_config(dict_bytes=d, emit_bytes=e))
        a1, w1 = join(tk1, mid)
        a2, w2 = join(tk2, mid, b"")
        b1, x1 = join(tk1, small)
        b2, x2 = join(tk2, big)
        assert [x.tobytes() for x in (held, larger, a1, a2, b1, b2)] == [want, wl, w1, w2, x1, x2]
        del larger, b1, b2
        gc.collect()
        tk1.close()  # (drops the cached block, not the blocks that are out)
        tk1 = None
        assert held.tobytes() == want and a1.tobytes() == w1 and a2.tobytes() == w2
        n1 = len(a1)
        del a1, w1
        gc.collect()  # (a block freed after its ctx was closed: the cache takes it)
        c2, y2 = join(tk2, mid, b"")
        assert len(c2) <= n1 and c2.tobytes() == y2 and a2.tobytes() == w2 and held.tobytes() == want
        del held, a2, c2
        gc.collect()
        # C: everything closed, a new ctx
        tk2.close()
        tk2 = None
        tk3 = J.Tokenizer(J.make_config(dict_bytes=d, emit_bytes=e))
        for b in (small, big, mid):
            out, w = join(tk3, b, b"\xe3\x80\x80")
            assert out.tobytes() == w
            del out
            gc.collect()
    finally:
        for tk in (tk1, tk2, tk3):
            if tk is not None:
                tk.close()


def script_wc_life(dr):
    m = dr.m
    b1, b2, b3 = dr.batch(m.source), dr.batch(("offset", 620, 20 << 10)), dr.batch(("tiny", 630, 6))
    grow = dr.batch(("grow", 640, 150 << 10))
    assert grow.nbytes > 2 * b1.nbytes
    # The word to add: pick_word(0)'s one occurrence in the source batch is never cut as a token, whatever its
    # frequency, and a count of 0 would show nothing.  So: the most frequent pair of neighbouring one-rune
    # tokens of b1 (one document, both Han) that is reachable and not a key.
    s, e, d = m.cut(b1, "plain", False, count=False)
    firsts, pairs = set(d.tolist()), {}
    for k in range(len(s) - 1):
        if e[k] - s[k] == 3 and e[k + 1] - s[k + 1] == 3 and e[k] == s[k + 1] and k + 1 not in firsts:
            w = bytes(b1.buf[int(s[k]):int(e[k + 1])]).decode("utf-8", "replace")
            if all(HAN[0] <= c <= HAN[1] for c in w) and m.o.get(w) is None and m.reachable(w):
                pairs[w] = pairs.get(w, 0) + 1
    word = min(pairs, key=lambda w: (-pairs[w], w))
    key = word.encode()

    def occurs(b, mode):
        s, e, _ = m.cut(b, mode, False, count=False)
        return sum(1 for x, y in zip(s.tolist(), e.tolist()) if bytes(b.buf[x:y]) == key)

    dr.wc_batch("plain", False, b1)
    dr.cut("plain", False, "device", grow)  # (replaces the workspace)
    dr.wc_batch("search", False, b2)
    assert m.wc[key] == 0
    dr.add_word(word, 10_000_000)
    dr.wc_batch("plain", False, b1)
    assert m.wc[key] == occurs(b1, "plain") > 0
    r1 = dr.wc_read("first")
    dr.wc_batch("full", False, b2)
    dr.cut("plain", False, "device", b3, reps=1)
    dr.wc_add()
    # (from the model, before the library's answer: only the batches after the add count the word)
    assert m.wc[key] == occurs(b1, "plain") + occurs(b2, "full") + occurs(b3, "plain")
    r2 = dr.wc_read("second")
    r3 = dr.wc_read("third")
    if r2 is not None:
        assert r1.tokens < r2.tokens and r2.keys == r3.keys and np.array_equal(r2.counts, r3.counts)
        assert (r2.bad, r2.long, r2.dropped, r2.collided, r2.tokens) == (r3.bad, r3.long, r3.dropped, r3.collided, r3.tokens)
        assert int(r2.counts[r2.keys.index(key)]) == m.wc[key]


def test_word_counts_over_a_contexts_life(syn):
    """One caller-owned table over plain, search and full mode, a workspace replaced in between, an AddWord (the
    word counts only from then on), jb_wc_add_device on a device cut's spans, and two reads that agree."""
    dr = open_20k(syn)
    try:
        script_wc_life(dr)
    finally:
        dr.tk.close()


@pytest.mark.parametrize("seed", M.SEEDS2)
def test_random_sequences2(syn, seed):
    """gen_ops2(seed, NSTEPS2): test_random_sequences with the six new kinds of call in the deck."""
    ops = M.gen_ops2(seed, M.NSTEPS2)
    dr = open_20k(syn)
    try:
        dr.set_vocab(dr.m.vocab_keys(0))
        for i, op in enumerate(ops):
            try:
                dr.run(op)
            except (AssertionError, J.JbError) as e:
                raise AssertionError(f"seed {seed}, step {i}: {op!r}\nops = {ops[:i + 1]!r}\n{e}") from e
        dr.wc_read("at the end")
        assert dr.too_small >= 1 and dr.restored >= 1  # (what covered2 promises did happen)
    finally:
        dr.tk.close()


# ---- MinHash, the caller's filter, postings, search, near-duplicates and collocations on a long-lived context ----
# These calls came after the ones above and share their front (batch_front / batch_chain, jb_batch.cpp): kArText and
# kArTokens with every older call, and a grow-only buffer each that is never cleared.  The scripts take a Driver (or a
# DryDriver: test_ctx_model.py checks their inputs on the CPU).
NEWEST_BATCH_OPS = M.NEWEST_BATCH_OPS
LARGE3 = 48 << 10  # the large batch of these scripts: the thresholds are 4,096 bytes / documents and 256-byte pieces


def newest_call(dr, kind, b, i, label, modes=None):
    """Call number i of a script: one *_batch call of `kind` on b, its parameters turned by i."""
    mode = (modes or {}).get((kind, b.spec), M.MODES[i % 3])
    hmm = mode != "full" and (b.nbytes > M.SMALL_MAX or i % 2 == 0)
    if kind == "keywords_batch":
        dr.keywords(True, b, 20, label)
    elif kind == "df_batch":
        dr.df(True, b, label)
    elif kind == "textrank_batch":
        dr.textrank(True, b, label=label)
    elif kind == "join_batch":
        dr.join_batch(mode, hmm, b, JR.SEPS[i % 4], JR.SEPS[(i + 1) % 4], label)
    elif kind == "charspans_batch":
        dr.charspans_batch(mode, hmm, b, ("rune", "utf16")[i % 2], b.nbytes > M.SMALL_MAX, label)
    elif kind == "wc_batch":
        dr.wc_batch(mode, hmm, b, label)
    elif kind == "minhash_batch":
        dr.minhash_batch(mode, hmm, b, (1, 3, 5)[i % 3], (16, 128, 64)[i % 3], 1 + i % 2, label)
    elif kind == "filter_batch":
        dr.filter_batch(mode, hmm, b, M.RULES[i % 2], label=label)
    elif kind == "postings_batch":
        dr.postings_batch(i % 2 == 0, b, (0, 7)[i % 2], label=label)
    elif kind == "search_batch":
        dr.search_batch(i % 2 == 0, b, (1, 10, 64)[i % 3], label)
    elif kind == "colloc_batch":
        dr.colloc_batch(i % 2 == 0, b, (None, dr.m.keep)[(i // 2) % 2], i % 3 == 0, label)
    else:
        raise ValueError(kind)
    dr.stats(label)


def script_arenas3(dr):
    m = dr.m
    big = dr.batch(("large", 1700, LARGE3))
    one, none = M.from_texts(("one",), ["中"]), dr.batch(("empty", 0, 5))
    tail = M.Batch(("tail",), big.buf, big.off[1:])  # (48 KiB are few documents: from document 1 on)
    assert 32 << 10 < big.nbytes <= LARGE3 and one.nbytes == 3 and none.nbytes == 0 and none.ndocs == 5
    assert int(tail.off[0]) > 0 and tail.nbytes > M.SMALL_MAX
    v1, v2 = m.vocab_keys(0), m.vocab_keys(1)
    assert len(v2) < len(v1)
    modes = {("join_batch", big.spec): "plain", ("join_batch", tail.spec): "search",
             ("charspans_batch", big.spec): "search", ("charspans_batch", tail.spec): "full",
             ("wc_batch", big.spec): "full", ("wc_batch", tail.spec): "plain",
             ("minhash_batch", big.spec): "full", ("minhash_batch", tail.spec): "plain",
             ("filter_batch", big.spec): "search", ("filter_batch", tail.spec): "full"}
    step = [0]

    def call(kind, b):
        i = step[0]
        step[0] += 1
        newest_call(dr, kind, b, i, f"call {i}", modes)

    dr.set_vocab(v1)
    dr.build_index([m.source])
    # an older kind on each large batch and one of the newest on each tiny one, ...
    for k, kind in enumerate(arena_order(M.ALL_BATCH_OPS, NEWEST_BATCH_OPS)):
        call(kind, ((big, tail)[(k // 2) % 2], (one, none)[(k // 2) % 2])[k % 2])
    dr.colloc_read("npmi", 2, 0.1, label="half way")
    dr.wc_read("half way")
    dr.set_vocab(v2)
    dr.build_index([m.source], k1=1.6, b=0.5)
    # ... and the other way round
    for k, kind in enumerate(arena_order(NEWEST_BATCH_OPS, M.ALL_BATCH_OPS)):
        if k == 30:
            dr.add_word(m.pick_word(0, big), 10_000_000)
            dr.stats("after AddWord")
        call(kind, ((big, tail)[(k // 2) % 2], (one, none)[(k // 2) % 2])[k % 2])
    dr.colloc_read("count", label="at the end")
    dr.wc_read("at the end")
    want = {(a, b, up) for a in M.ALL_BATCH_OPS for b in NEWEST_BATCH_OPS for up in (False, True)}
    want |= {(b, a, up) for a, b, up in want}
    assert len(want) == 120 and want <= arena_pairs(dr.calls), sorted(want - arena_pairs(dr.calls))


def test_newest_batch_calls_share_the_arenas(syn):
    """The five newest *_batch kinds and the six older ones on one ctx with a vocabulary and an index, over a 48 KiB
    batch, one 3-byte document, five empty documents and the large buffer from its document 1 on, a smaller
    vocabulary and an AddWord in between, jb_last_stats after every call: every ordered pair of a newest kind and
    an older one, both ways round, lies on a large-then-tiny and on a tiny-then-large transition (asserted from the
    driver's call list)."""
    dr = open_20k(syn)
    try:
        script_arenas3(dr)
    finally:
        dr.tk.close()


def script_same_shape3(dr):
    m = dr.m
    a = dr.batch(("offset", 787, 30 << 10))  # (sentences: many documents)
    t = dr.batch(twin(a))

    def other(x, y):
        """Whether two of the model's answers differ in some array."""
        return any(np.shape(i) != np.shape(j) or not np.array_equal(i, j) for i, j in zip(x, y))

    qa = dr.batch(("queries", 797, 6))
    qt = dr.batch(twin(qa))
    d = dr.batch(("dups", 807, 64))
    few = M.Batch(("few",), d.buf, d.off[:4])
    assert np.array_equal(a.off, t.off) and np.array_equal(qa.off, qt.off) and qa.ndocs == 8 and few.ndocs == 3
    v0, v1 = m.vocab_keys(0), m.vocab_keys(1)
    dr.set_vocab(v0)
    dr.build_index([m.source])
    for mode, hmm in COMBOS[1:]:
        got = [dr.minhash_batch(mode, hmm, x, 5, 64, label=f"same shape {k}") for k, x in enumerate((a, t, a))]
        assert got[0] is got[2] and other(got[0], got[1])  # (the model's answers differ)
        got = [dr.filter_batch(mode, hmm, x, M.RULES[0], label=f"same shape {k}") for k, x in enumerate((a, t, a))]
        assert other(got[0], got[1])
        dr.stats(mode)
    for hmm in (True, False):
        got = [dr.postings_batch(hmm, x, label=f"same shape {k}") for k, x in enumerate((a, t, a))]
        assert other(got[0], got[1])
        got = [dr.search_batch(hmm, x, 10, label=f"same shape {k}") for k, x in enumerate((qa, qt, qa))]
        assert other(got[0], got[1])
        for k, x in enumerate((a, t, a)):
            dr.colloc_batch(hmm, x, label=f"same shape {k}")
            dr.colloc_read("count", label=f"same shape {k}")
        dr.stats(f"hmm={hmm}")
    # shrinking calls: the larger call's tail lies right behind the live data of the smaller one
    dr.minhash_batch("plain", True, d, 5, 128, label="K 128, 64 documents", dups=True)
    big = dr.neardup(32, 4, 64, 64, short=0, label="B 32")
    dr.minhash_batch("plain", True, few, 5, 16, label="K 16, 3 documents")
    dr.neardup(4, 4, 64, 8, short=0, label="3 documents")
    dr.minhash_batch("plain", True, d, 5, 128, label="K 128 again", dups=True)
    small = dr.neardup(4, 2, 64, 120, short=0, label="B 4, fewer pairs")
    assert 0 < len(small[1]) < len(big[1])  # (pcap shrinks with the count)
    dr.neardup(4, 2, 64, 120, short=None, label="B 4, no arrays")
    many = dr.postings_batch(True, a, label="many keys")
    wide = dr.search_batch(True, qa, 64, label="topk 64, 8 queries")
    one = M.Batch(("oneq",), qa.buf, qa.off[:2])
    dr.search_batch(True, one, 1, label="topk 1, 1 query")
    assert int(wide[2].max()) > 1
    dr.colloc_batch(True, a, np.ones(len(v0), np.uint8), label="keep: every id")
    dr.colloc_batch(True, a, None, label="keep: none")
    dr.colloc_read("npmi", 2, 0.1, label="after the keep masks")
    dr.set_vocab(v1)
    fewer = dr.postings_batch(True, a, label="few keys")
    assert len(fewer[0]) < len(many[0]) and len(fewer[1]) < len(many[1])
    dr.colloc_batch(True, a, label="few keys")
    dr.colloc_read("count", label="few keys")
    dr.stats("at the end")


def test_newest_calls_same_shape_other_text(syn):
    """Per newest kind: a batch, its twin of identical document lengths and other runes, the batch again, each answer
    its own; then per kind a large call followed by a small one (K 128 then 16 and 64 documents then 3; many keys
    then few; topk 64 then 1 and 8 queries then 1; B and pcap shrinking; a keep mask of every id, then none)."""
    dr = open_20k(syn)
    try:
        script_same_shape3(dr)
    finally:
        dr.tk.close()


def every_newest(dr, big, tiny, q, label, skip=(), filtered=True):
    """One call of every newest kind (but `skip`; the filtered ones only with `filtered`) and of one older kind."""
    if "minhash_batch" not in skip and filtered:
        dr.minhash_batch("search", True, tiny, 3, 32, label=label)
        dr.neardup(8, 4, 64, 16, short=0, label=label)
    if "filter_batch" not in skip:
        dr.filter_batch("plain", True, tiny, M.RULES[1], label=label)
    if "postings_batch" not in skip:
        dr.postings_batch(True, tiny, 3, label=label)
    if "search_batch" not in skip:
        dr.search_batch(True, q, 5, label)
    if "colloc_batch" not in skip and filtered:
        dr.colloc_batch(True, tiny, label=label)
        dr.colloc_read("count", label=label)
    dr.keywords(True, big, 5, label)
    dr.stats(label)


def script_errors(dr):
    m = dr.m
    big, tiny = dr.batch(("small", 2100, 30 << 10)), dr.batch(("tiny", 2110, 5))
    q, d = dr.batch(("queries", 2120, 6)), dr.batch(("dups", 2130, 24))
    dr.set_vocab(m.vocab_keys(0))
    dr.build_index([big])
    dr.set_stop(m.stop_keys(0))
    # jb_postings_batch: one entry short, then with room
    dr.postings_batch(True, big, short=1, label="one short")
    dr.stats("postings one short")
    every_newest(dr, big, tiny, q, "after postings' JB_ELIMIT", skip=("postings_batch",))
    dr.postings_batch(True, big, label="with room")
    # jb_cut_batch_filter
    dr.filter_batch("search", True, big, M.RULES[2], short=1, label="one short")
    dr.stats("filter one short")
    every_newest(dr, big, tiny, q, "after the filter's JB_ELIMIT", skip=("filter_batch",))
    dr.filter_batch("search", True, big, M.RULES[2], label="with room")
    # jb_neardup_sig: counts only, one short, an exact fit
    dr.minhash_batch("plain", True, d, 5, 128, label="dups", dups=True)
    want = dr.neardup(32, 4, 64, 64, short=None, label="counts only")
    assert len(want[1]) >= 3
    dr.neardup(32, 4, 64, 64, short=1, label="one short")
    every_newest(dr, big, tiny, q, "after neardup's JB_ELIMIT", skip=("minhash_batch",))
    dr.minhash_batch("plain", True, d, 5, 128, label="dups", dups=True)
    dr.neardup(32, 4, 64, 64, short=0, label="an exact fit")
    # a batch filter that asks for a stop set that is gone: JB_EINVAL after the cut, both tables untouched
    dr.wc_batch("plain", True, tiny, "before")
    dr.colloc_batch(True, big, label="before")
    dr.set_stop(None)
    dr.set_filter(M.RULES[2])
    before = None
    if dr.tk is not None:
        import torch
        torch.cuda.synchronize()
        before = (inner_bytes(dr.table[0], dr.table[1]).tobytes(), dr.colloc_raw())
    for k, x in enumerate((big, tiny)):
        dr.join_batch("search", True, x, b" ", b"\n", f"no stop set {k}")
        dr.stats("after join's JB_EINVAL")  # (the cut ran: its count)
        dr.wc_batch("full", False, x, f"no stop set {k}")
        dr.minhash_batch("plain", False, x, label=f"no stop set {k}")
        dr.colloc_batch(True, x, label=f"no stop set {k}")
        dr.stats("after colloc's JB_EINVAL")
    if dr.tk is not None:
        torch.cuda.synchronize()
        assert before == (inner_bytes(dr.table[0], dr.table[1]).tobytes(), dr.colloc_raw()), "a refused call changed a table"
    every_newest(dr, big, tiny, q, "the unfiltered kinds under the broken filter", filtered=False)
    dr.wc_read("after the refusals")
    dr.colloc_read("npmi", 2, 0.1, label="after the refusals")
    dr.set_filter(None)
    every_newest(dr, big, tiny, q, "after the filter's JB_EINVAL")
    dr.set_stop(m.stop_keys(1))
    dr.set_filter(M.RULES[2])
    every_newest(dr, big, tiny, q, "a stop set again")
    dr.wc_batch("plain", True, tiny, "a stop set again")
    dr.wc_read("at the end")


def test_error_returns_leave_the_context_whole(syn):
    """JB_ELIMIT from jb_postings_batch, jb_cut_batch_filter and jb_neardup_sig (arrays one entry short; none at all)
    with the counts, post_off / pair_off and the statistics right and nothing else written, and JB_EINVAL from join,
    wc, MinHash and colloc under a batch filter whose stop set is gone, with the word-count and collocation tables
    bit-identical before and after: after each, a call of every other newest kind and of an older one equals the
    model, and so does the refused call once it has room."""
    dr = open_20k(syn)
    try:
        script_errors(dr)
    finally:
        dr.tk.close()


MINI_PARTS = ("今天", "天氣", "很好", "我", "昨天", "去", "上海", "交通", "大學", "這", "的", "一刹那", "量子力學", "，", "。", " ",
              "abc ", "2024 ", "甲甲甲", "\x80")


def mini_docs(seed, ndocs, most):
    rng = np.random.default_rng(seed)
    return ["".join(MINI_PARTS[int(rng.integers(0, len(MINI_PARTS)))] for _ in range(int(rng.integers(0, most))))
            .encode("utf-8", "surrogateescape").replace(b"\xc2\x80", b"\x80") for _ in range(ndocs)]


def script_filter_life(dr):
    m = dr.m
    b = dr.batch(M.from_texts(("mini", 41), mini_docs(41, 300, 40)))
    t = dr.batch(M.from_texts(("mini", 43), mini_docs(43, 6, 12)))
    q = dr.batch(M.from_texts(("miniq",), ["今天天氣很好", "上海交通大學", "", "zzz 未知", "昨天去上海 abc"]))
    regrow = dr.batch(M.from_texts(("regrow12",), ["甲" * 12, X4 + "甲" * 12]))
    assert 24 << 10 <= b.nbytes <= LARGE3 and t.nbytes <= M.SMALL_MAX
    assert len(m.cut(regrow, "full", False, count=False)[0]) > regrow.nbytes  # (the front cuts twice)
    keys = set()
    for x in (b, t, q, regrow):
        s, e, _ = m.cut(x, "plain", True, count=False)
        keys |= {bytes(x.buf[int(i):int(j)]) for i, j in zip(s, e) if j - i > 1 or x.buf[int(i)] < 0x80}
    dr.set_vocab(sorted(keys))
    dr.build_index([b, t])
    stop1 = ["今天".encode(), "的".encode(), b"abc", ("甲" * 3).encode()]
    stop2 = ["上海".encode(), ("甲" * 2).encode(), ("甲" * 4).encode(), b"2024", "。".encode()]
    dr.set_stop(stop1)
    own = M.RULES[1]

    def lap(label, x=b, unfiltered=True):
        out = []
        for mode, hmm in (("plain", True), ("search", True), ("full", False)):
            dr.join_batch(mode, hmm, x, b" ", b"\n", label)
            out.append(m.join(x, mode, hmm, b" ", b"\n"))
            dr.wc_batch(mode, hmm, x, label)
            out.append(dr.minhash_batch(mode, hmm, x, 2, 32, label=label))
            if unfiltered:
                dr.charspans_batch(mode, hmm, x, "rune", False, label)
                dr.filter_batch(mode, hmm, x, own, label=label)
            dr.stats(f"{label} {mode}")
        dr.colloc_batch(True, x, label=label)
        out.append({k: v for k, v in m.cl["table"].items()})
        if unfiltered:
            dr.keywords(True, x, 5, label)
            dr.df(True, x, label)
            dr.textrank(True, x, label=label)
            dr.postings_batch(True, x, label=label)
            dr.search_batch(True, q, 10, label)
            dr.stats(label)
        dr.colloc_read("count", label=label)
        dr.wc_read(label)
        return out

    def differ(x, y):
        """Whether every filtered answer of two laps differs (joined bytes, signatures); the tables only grow."""
        return all(not np.array_equal(np.asarray(i[0]), np.asarray(j[0])) for i, j in zip(x[:-1], y[:-1]))

    before = lap("before")
    before_t = lap("before, tiny", t)
    dr.set_filter(M.RULES[0])
    first = lap("the first rule")
    assert differ(before, first)
    lap("the first rule, tiny", t)
    dr.set_filter(M.RULES[1])  # (replaces the first)
    second = lap("the second rule")
    assert differ(first, second) and differ(before, second)
    dr.set_filter(M.RULES[2])
    s1 = lap("a stop-using rule", unfiltered=False)
    dr.set_stop(stop2)
    s2 = lap("the stop set replaced", unfiltered=False)
    assert differ(s1, s2) and differ(before, s2)
    # (a word of b that t does not hold: t's answers stay, as the model confirms at the end)
    ttext = bytes(t.buf[:int(t.off[-1])]).decode("utf-8", "replace")
    word = next(w for w in (m.pick_word(k, b) for k in range(8)) if w not in ttext)
    dr.add_word(word, 10_000_000)
    s3 = lap("after AddWord")
    assert differ(s2, s3)  # (the filtered results follow the new dictionary)
    # full mode's regrow with the filter on, then the calls that cut kArTokens up as ids, terms and work
    for k, (hand, after) in enumerate((("join", "postings"), ("wc", "search"), ("minhash", "colloc"), ("join", "colloc"),
                                       ("minhash", "postings"), ("wc", "search"))):
        label = f"regrow {k}"
        if hand == "join":
            dr.join_batch("full", False, regrow, b" ", b"\n", label)
        elif hand == "wc":
            dr.wc_batch("full", False, regrow, label)
        else:
            dr.minhash_batch("full", False, regrow, 2, 16, label=label)
        dr.stats(label)
        if after == "postings":
            dr.postings_batch(True, (b, regrow)[k % 2], label=label)
        elif after == "search":
            dr.search_batch(True, q, 10, label)
        else:
            dr.colloc_batch(True, (b, regrow)[k % 2], label=label)
            dr.colloc_read("count", label=label)
        dr.stats(label)
    dr.set_filter(None)
    # cleared: every kind answers as with no filter.  For b that is the unfiltered answer under the dictionary with
    # the added word; for t, which does not hold the word, it is what it was before the first set, to the byte
    after = lap("cleared")
    assert differ(s3, after) and m.bfilter is None
    after_t = lap("cleared, tiny", t)
    for x, y in zip(before_t[:-1], after_t[:-1]):
        assert np.array_equal(np.asarray(x[0]), np.asarray(y[0])) and np.array_equal(np.asarray(x[1]), np.asarray(y[1]))


def test_batch_filter_over_a_contexts_life(mini):
    """One ctx (the mini dictionary with the regrow chain): every filtered and every unfiltered kind in plain, search
    and full mode with no filter, a rule, a rule that replaces it, a stop-using rule under two stop sets, after
    AddWord, around a full-mode regrow batch (followed by postings, search and colloc, which cut kArTokens up
    differently), and cleared; the model says where the answers must differ."""
    mini_text, emit = mini
    dr = open_text(regrow_dict(mini_text), emit)
    try:
        script_filter_life(dr)
    finally:
        dr.tk.close()


def rune_pairs(m, b, hmm, keys):
    """{word: count} of the pairs of neighbouring one-rune Han tokens of b's plain cut (inside one document) whose
    runes are both among `keys` and whose concatenation is reachable and no dictionary key: a word AddWord can make
    one token of."""
    s, e, d = m.cut(b, "plain", hmm, count=False)
    firsts, pairs, keys = set(d.tolist()), {}, set(keys)
    for k in range(len(s) - 1):
        if e[k] - s[k] == 3 and e[k + 1] - s[k + 1] == 3 and e[k] == s[k + 1] and k + 1 not in firsts:
            w = bytes(b.buf[int(s[k]):int(e[k + 1])]).decode("utf-8", "replace")
            if all(HAN[0] <= c <= HAN[1] for c in w) and m.o.get(w) is None and m.reachable(w) and \
                    w[0] != w[1] and w[0].encode() in keys and w[1].encode() in keys:
                pairs[w] = pairs.get(w, 0) + 1
    return pairs


def script_index_life(dr):
    m = dr.m
    b1, b2 = dr.batch(("offset", 2300, 28 << 10)), dr.batch(("small", 2310, 24 << 10))
    large, q = dr.batch(("large", 2320, LARGE3)), dr.batch(("queries", 2330, 6))
    tiny = dr.batch(("tiny", 2340, 4))
    v0, v1 = m.vocab_keys(0), m.vocab_keys(1)
    assert len(v0) != len(v1) and b1.ndocs + b2.ndocs > 10 * tiny.ndocs

    def hits(r):
        return int((r[2] > 0).sum()), int((r[2] == 0).sum())

    dr.set_vocab(v0)
    dr.search_batch(True, q, 10, "no index yet")  # JB_EINVAL
    dr.build_index([b1, b2])
    first = [dr.search_batch(True, q, k, "the first index") for k in (10, 1, 64)]
    dr.stats("the first index")
    assert min(hits(first[0])) > 0  # (queries with documents and queries without)
    dr.postings_batch(True, large, label="between two searches")
    dr.minhash_batch("full", False, large, 5, 128, label="between two searches")
    again = [dr.search_batch(True, q, k, "again") for k in (10, 1, 64)]
    assert all(x is y for x, y in zip(first, again))
    # a word of a query: the index stays, the query's cut moves
    pairs = rune_pairs(m, q, True, v0)
    word = min(pairs, key=lambda w: (-pairs[w], w))
    dr.add_word(word, 10_000_000)
    moved = dr.search_batch(True, q, 10, "after AddWord")
    assert m.index.vversion == m.vversion and not all(np.array_equal(x, y) for x, y in zip(first[0], moved))
    dr.stats("after AddWord")
    # a vocabulary of another key count: search is refused, every other kind answers
    dr.set_vocab(v1)
    stats = m.last_tokens
    dr.search_batch(True, q, 10, "the vocabulary replaced")
    assert m.last_tokens == stats  # (refused before the cut)
    dr.stats("after the refusal")
    dr.minhash_batch("plain", True, tiny, label="the vocabulary replaced")
    dr.filter_batch("search", True, b2, M.RULES[0], label="the vocabulary replaced")
    dr.postings_batch(True, b2, label="the vocabulary replaced")
    dr.colloc_batch(True, b2, label="the vocabulary replaced")
    dr.colloc_read("npmi", 2, 0.1, label="the vocabulary replaced")
    dr.keywords(True, tiny, 5, "the vocabulary replaced")
    dr.join_batch("plain", True, tiny, b" ", b"\n", "the vocabulary replaced")
    dr.search_batch(True, q, 10, "still refused")
    dr.build_index([b1, b2])
    rebuilt = dr.search_batch(True, q, 64, "rebuilt")
    assert min(hits(rebuilt)) > 0
    # an index over far fewer documents, other parameters: kArSearch keeps the larger size
    dr.build_index([tiny], k1=2.0, b=0.0)
    small = dr.search_batch(True, q, 64, "few documents")
    assert int(small[2].max()) <= tiny.ndocs < int(rebuilt[2].max())
    dr.search_batch(False, q, 1, "few documents")
    dr.stats("few documents")
    dr.clear_index()
    dr.search_batch(True, q, 10, "no index")
    dr.postings_batch(True, tiny, label="no index")
    dr.stats("at the end")


def test_index_over_a_contexts_life(syn):
    """An index built from two batches, attached and searched; a large postings_batch and a full-mode minhash_batch
    between two searches that agree; AddWord of a word of a query (the old index, the new cut: other answers, from
    the model); a vocabulary of another key count (JB_EINVAL from search alone); rebuilt; replaced by a much
    smaller one with other k1 / b; cleared (JB_EINVAL).  The fixtures offer one setting of JB_BM25_FORM, the
    default; test_gpu_bm25.py compares the two forms."""
    dr = open_20k(syn)
    try:
        script_index_life(dr)
    finally:
        dr.tk.close()


def noisy_copies(d):
    """The documents of a batch, each followed by a copy with ASCII words behind some of its punctuation: tokens a
    filter of alnum, num and other removes, and with them every difference."""
    o = [int(x) for x in d.off]
    docs = []
    for k in range(d.ndocs):
        text = bytes(d.buf[o[k]:o[k + 1]]).decode("utf-8")
        out, n = [], 0
        for c in text:
            out.append(c)
            if c in "，。！？；：、" :
                n += 1
                if n % 3 == 0:
                    out.append(f" memo{n} 20{n:02d} ")
        docs += [text, "".join(out)]
    return M.from_texts(("noisy",) + tuple(d.spec), docs)


def script_colloc_dedup(dr):
    m = dr.m
    b1, b2, b3 = dr.batch(m.source), dr.batch(("offset", 2420, 28 << 10)), dr.batch(("tiny", 2430, 6))
    none, large, b6 = dr.batch(("empty", 0, 3)), dr.batch(("large", 2440, LARGE3)), dr.batch(("tiny", 2450, 2))
    # The word to add: as script_wc_life picks it, the most frequent pair of neighbouring one-rune tokens of b1 that
    # is reachable and no key, here with both runes keys of the vocabulary (so the table counts the pair); the
    # vocabulary holds the word itself too, so that it has a unigram counter once the dictionary cuts it.
    v0 = m.vocab_keys(0)
    pairs = rune_pairs(m, b1, False, v0)
    word = min(pairs, key=lambda w: (-pairs[w], w))
    keys = v0 + [word.encode()]
    dr.set_vocab(keys)
    pair, wid = (keys.index(word[0].encode()), keys.index(word[1].encode())), len(keys) - 1

    def read(label):
        dr.colloc_read("npmi", 2, 0.1, label=label)
        dr.colloc_read("count", label=label)
        dr.stats(label)

    for k, (x, hmm, keep, contig) in enumerate(((b1, False, None, False), (b3, True, None, True), (b2, True, m.keep, False),
                                                (none, True, None, False), (large, False, None, True),
                                                (b6, False, m.keep, True))):
        dr.colloc_batch(hmm, x, keep, contig, label=f"batch {k}")
        read(f"batch {k}")
    counted, uni = m.cl["table"][pair], m.cl["uni"][wid]
    assert counted >= pairs[word] > 1 and uni == 0
    dr.add_word(word, 10_000_000)
    dr.colloc_batch(False, b1, label="after AddWord")
    read("after AddWord")
    assert m.cl["table"][pair] == counted and m.cl["uni"][wid] > 0  # (the pair is one token now)
    distinct = len(m.cl["table"])
    dr.set_vocab(m.vocab_keys(1))
    assert m.cl is None
    dr.colloc_batch(True, b2, label="a new table")
    read("a new table")
    assert 0 < len(m.cl["table"]) < distinct
    # near-duplicates: a dups batch, then copies that differ in tokens a batch filter removes
    dd = dr.batch(("dups", 2460, 32))
    dr.minhash_batch("plain", True, dd, 5, 128, label="dups", dups=True)
    po, pd, pa, _ = dr.neardup(32, 4, 64, 64, short=0, label="dups")
    plan = M.dup_plan(2460, 32)
    got = {(int(pd[k]), j) for j in range(dd.ndocs) for k in range(int(po[j]), int(po[j + 1]))}
    assert {(src, j) for j, (kind, src, _) in enumerate(plan) if kind == "copy"} <= got and len(pd) >= 3
    assert all(int(pa[k]) == 128 for j, (kind, _, _) in enumerate(plan) if kind == "copy" for k in range(int(po[j]), int(po[j + 1]))
               if plan[int(pd[k])][0] == "new")
    noisy = dr.batch(noisy_copies(M.Batch(("dd16",), dd.buf, dd.off[:17])))
    sig, _ = dr.minhash_batch("plain", True, noisy, 5, 128, label="noisy copies")
    po, pd, pa, _ = dr.neardup(32, 4, 64, 64, short=0, label="noisy copies")
    assert all(not np.array_equal(sig[2 * k], sig[2 * k + 1]) for k in range(16))
    dr.set_filter(M.rule(("alnum", "num", "other")))
    sig, _ = dr.minhash_batch("plain", True, noisy, 5, 128, label="noisy copies, filtered")
    assert all(np.array_equal(sig[2 * k], sig[2 * k + 1]) for k in range(16))  # (exact duplicates now)
    po, pd, pa, _ = dr.neardup(32, 4, 64, 64, short=0, label="noisy copies, filtered")
    for k in range(16):
        row = {int(pd[i]): int(pa[i]) for i in range(int(po[2 * k + 1]), int(po[2 * k + 2]))}
        assert row.get(2 * k) == 128, (k, row)
    dr.set_filter(None)
    dr.stats("at the end")


def test_collocations_and_dedup_over_a_contexts_life(syn):
    """One caller-owned collocation table and d_uni (between canaries) over six colloc_batch calls of different sizes,
    keep masks and flags, read with two scorers after each; AddWord of an adjacent pair the table counts (the pair
    stops growing, the new word's unigram starts); a new vocabulary, a new table.  Then MinHash and the pairs of a
    batch with planted copies, and of copies that differ only in tokens a batch filter removes: exact duplicates
    once it is set."""
    dr = open_20k(syn)
    try:
        script_colloc_dedup(dr)
    finally:
        dr.tk.close()


@pytest.fixture(scope="module", params=M.SEEDS3)
def seq3(request, syn):
    """(seed, ops, the references of gen_ops3(seed, NSTEPS3)): the sequence through the model alone, once, so that
    the test below spends its time on the library.  The references are the model's cache, whose keys hold the
    batch, the call's parameters and the versions of the dictionary, the vocabulary, the filter, the stop set and
    the index, which the same ops reach in the same order."""
    seed = request.param
    ops = M.gen_ops3(seed, M.NSTEPS3)
    dry = dry_20k(syn)
    dry.set_vocab(dry.m.vocab_keys(0))
    for op in ops:
        dry.run(op)
    return seed, ops, dry.m._cache, dry.batches


def test_random_sequences3(syn, seq3):
    """gen_ops3(seed, NSTEPS3): test_random_sequences2 with the newest kinds of call, the stop set, the batch filter
    and the index in the sequence, jb_last_stats after every step."""
    seed, ops, refs, batches = seq3
    dr = open_20k(syn)
    dr.m._cache, dr.batches = refs, dict(batches)
    try:
        dr.set_vocab(dr.m.vocab_keys(0))
        for i, op in enumerate(ops):
            try:
                dr.run(op)
                dr.stats()
            except (AssertionError, J.JbError) as e:
                raise AssertionError(f"seed {seed}, step {i}: {op!r}\nops = {ops[:i + 1]!r}\n{e}") from e
        dr.wc_read("at the end")
        dr.colloc_read("count", label="at the end")
    finally:
        dr.tk.close()
