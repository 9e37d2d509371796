#!/usr/bin/env python3
"""The cost of jb_terms_device and jb_keywords_device on the benchmark's corpus.

Corpus, dictionary and vocabulary as tools/ids_bench.py (bench.py's config 4: C_syn against the
350k-word D_syn dictionary, JB_DICT_PREFIX, size 60,101,967; the vocabulary is the dictionary's words
with freq > 0), at 1 GiB, at 128 MiB and for the 10,000-sentence batch, and one 1,000,000-rune
document whose terms go through the merge passes.  Per batch: the plain jb_cut_device step,
jb_ids_device, jb_terms_device and jb_keywords_device (topk 20), each timed with device events on the
launch stream (--steps after --warmup), the term kernels once more through jb_profile_read, and
jb_keywords_batch from host memory beside jb_cut_batch_into32 for the largest corpus.  The weights
are a fixed-seed IDF-like table, 0 for one-rune keys.
Then, on the CSR the terms step left on the device, the document-frequency steps with the same event
method in the same process: the hipMemsetAsync of df, jb_df_device in both forms (JB_DF_COMBINE 0 and 1,
the order alternated from step to step) and jb_idf_device, each beside the terms step of the same run;
and jb_df_batch from host memory beside jb_keywords_batch.
Then, on the ids and the CSR of the first corpus (1 GiB), jb_textrank_device with jieba's arguments (span 5,
10 rounds, top 20; the keep mask drops one-rune keys) in both forms of its push kernel (JB_TR_WINDOW 0 and
1, the order alternated from step to step), beside the cut and terms steps of the same run, its kernels
once more through jb_profile_read, and the two forms' records compared byte for byte.
Writes three JSON documents (--out, --df-out for the document-frequency rows, --tr-out for the TextRank
rows) and prints them.  --textrank-only measures the TextRank rows alone and leaves the other two files.

    python tools/terms_bench.py --out profiles/terms_bench.json --df-out profiles/df_bench.json \
        --tr-out profiles/textrank_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("gen", os.path.join("jieba-go_amd", "python")):
    sys.path.insert(0, os.path.join(ROOT, sub))

TOPK = 20


def timed(torch, fn, steps, warmup):
    """Median and spread (ms) of fn() over `steps` calls, device events around each call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4)}


def timed_ab(torch, fns, steps, warmup):
    """timed() for two forms of one step, in one loop: each step runs both, in alternating order."""
    names = list(fns)
    for _ in range(warmup):
        for n in names:
            fns[n]()
    torch.cuda.synchronize()
    ev = {n: [] for n in names}
    for k in range(steps):
        for n in (names if k % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fns[n]()
            b.record()
            ev[n].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for n in names:
        ms = np.array([a.elapsed_time(b) for a, b in ev[n]])
        out[n] = {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
                  "max_ms": round(float(ms.max()), 4)}
    return out


def measure_df(torch, J, forms, hip, t_id, t_n, nterms, cap, nw, nd, t_terms, steps, warmup):
    """The document-frequency steps on the CSR the terms step of this run left on the device: the
    hipMemsetAsync of df, jb_df_device in both forms (forms: {name: a tokenizer opened with that
    JB_DF_COMBINE}), jb_idf_device; the forms' counters are compared with each other and with numpy."""
    stream = torch.cuda.current_stream().cuda_stream
    d_df = torch.zeros(nw, dtype=torch.int32, device="cuda")
    d_wt = torch.empty(nw, dtype=torch.float32, device="cuda")
    any_tk = next(iter(forms.values()))
    zero = lambda: hip.hipMemsetAsync(C.c_void_p(d_df.data_ptr()), 0, C.c_size_t(4 * nw), C.c_void_p(stream))  # noqa: E731
    df_fn = {n: (lambda t=t: t.df_device(t_id.data_ptr(), t_n.data_ptr(), cap, d_df.data_ptr(), nw, stream))
             for n, t in forms.items()}
    idf = lambda: any_tk.idf_device(d_df.data_ptr(), nw, nd, d_wt.data_ptr(), stream_ptr=stream)  # noqa: E731
    t_zero = timed(torch, zero, steps, warmup)
    t_df = timed_ab(torch, df_fn, steps, warmup)
    counts = {}
    for n in forms:
        zero()
        df_fn[n]()
        torch.cuda.synchronize()
        counts[n] = d_df.cpu().numpy().view(np.uint32).copy()
    t_idf = timed(torch, idf, steps, warmup)  # (on real counters: the last form's)
    ref = np.bincount(t_id[:nterms].cpu().numpy().view(np.uint32).astype(np.int64), minlength=nw)[:nw].astype(np.uint32)
    names = list(forms)
    best = min(names, key=lambda n: t_df[n]["median_ms"])
    res = {"ndf": nw, "nterms": nterms, "memset_df": t_zero, "idf_device": t_idf,
           "counters_equal_numpy": bool(all(np.array_equal(counts[n], ref) for n in names)),
           "max_df": int(ref.max()), "ids_with_df_over_half_the_docs": int((ref > nd // 2).sum()),
           "faster_form": best, "terms_device_median_ms": t_terms["median_ms"]}
    for n in names:
        res["df_device_" + n] = t_df[n]
        res["df_" + n + "_over_terms"] = round(t_df[n]["median_ms"] / t_terms["median_ms"], 4)
        res["df_" + n + "_entries_per_us"] = round(nterms / (t_df[n]["median_ms"] * 1e3), 1)
    res["idf_over_terms"] = round(t_idf["median_ms"] / t_terms["median_ms"], 4)
    return res


TR_SPAN, TR_ITERS = 5, 10


def measure_textrank(torch, J, forms, d_ids, pd, pn, ntok, nd, t_id, t_off, nterms, d_keep, nkeep, t_cut, t_terms, steps,
                     warmup):
    """jb_textrank_device on the ids and the CSR this run left on the device, in both forms of the push
    kernel (forms: {name: a tokenizer opened with that JB_TR_WINDOW}).  The capacities are the token count,
    as a chain that reads nothing on the host has them."""
    stream = torch.cuda.current_stream().cuda_stream
    need = J.textrank_work_bytes(ntok, ntok, nd)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    outs = {n: (torch.empty(nd * TOPK, dtype=torch.int32, device="cuda"), torch.empty(nd * TOPK, dtype=torch.int32, device="cuda"),
                torch.empty(nd, dtype=torch.int32, device="cuda")) for n in forms}
    fn = {n: (lambda t=t, o=outs[n]: t.textrank_device(d_ids.data_ptr(), ntok, pd, pn, nd, t_id.data_ptr(), t_off.data_ptr(),
                                                        ntok, d_keep.data_ptr(), nkeep, o[0].data_ptr(), o[1].data_ptr(),
                                                        o[2].data_ptr(), work.data_ptr(), need, TR_SPAN, TR_ITERS, TOPK, stream))
          for n, t in forms.items()}
    t_tr = timed_ab(torch, fn, steps, warmup)
    names = list(forms)
    same = all(torch.equal(a, b) for a, b in zip(outs[names[0]], outs[names[1]]))
    prof = {}
    for n, t in forms.items():
        t.profile(True)
        t.profile_reset()
        for _ in range(steps):
            fn[n]()
        torch.cuda.synchronize()
        prof[n] = {k: round(v[0] / steps, 4) for k, v in t.profile_read().items() if k.startswith("k_tr_")}
        t.profile(False)
    best = min(names, key=lambda n: t_tr[n]["median_ms"])
    res = {"span": TR_SPAN, "iters": TR_ITERS, "topk": TOPK, "tokens": ntok, "nterms": nterms, "docs": nd,
           "work_bytes": int(need), "rows_filled": int(outs[names[0]][2].sum().item()),
           "forms_give_identical_bytes": bool(same), "faster_form": best,
           "cut_device_hmm1_median_ms": t_cut["median_ms"], "terms_device_median_ms": t_terms["median_ms"],
           "kernels_profile_ms_per_call": prof}
    for n in names:
        res["textrank_device_" + n] = t_tr[n]
        res["textrank_" + n + "_over_cut"] = round(t_tr[n]["median_ms"] / t_cut["median_ms"], 4)
        res["textrank_" + n + "_over_terms"] = round(t_tr[n]["median_ms"] / t_terms["median_ms"], 4)
    del work
    return res


def measure(torch, J, tk, d_w, nw, label, buf, off, steps, warmup, forms=None, hip=None, tr_forms=None, d_keep=None):
    stream = torch.cuda.current_stream().cuda_stream
    nb, nd = int(off[-1]), len(off) - 1
    d_text = torch.from_numpy(np.ascontiguousarray(buf[:nb])).cuda()
    d_text = torch.cat([d_text, torch.zeros(64, dtype=torch.uint8, device="cuda")])
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    cut = lambda: tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)  # noqa: E731
    ps, pe, pd, pn = cut()
    torch.cuda.synchronize()
    tk.device_status(stream)
    ntok = int(J.dev_to_host(pn, 8, np.uint64)[0])
    doc_tok = J.dev_to_host(pd, 8 * (nd + 1), np.uint64).astype(np.int64)
    T = J.JB_TERMS_TILE
    multi = (doc_tok[1:] > doc_tok[:-1]) & ((doc_tok[1:] - 1) // T != doc_tok[:-1] // T)
    d_ids = torch.empty(ntok, dtype=torch.int32, device="cuda")
    t_id = torch.empty(ntok, dtype=torch.int32, device="cuda")
    t_cnt = torch.empty(ntok, dtype=torch.int32, device="cuda")
    t_off = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
    t_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    k_id = torch.empty(nd * TOPK, dtype=torch.int32, device="cuda")
    k_sc = torch.empty(nd * TOPK, dtype=torch.float32, device="cuda")
    k_cnt = torch.empty(nd * TOPK, dtype=torch.int32, device="cuda")
    k_n = torch.empty(nd, dtype=torch.int32, device="cuda")
    need = J.terms_work_bytes(ntok, nd)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = lambda: tk.ids_device(d_text.data_ptr(), nb, ps, pe, pn, ntok, d_ids.data_ptr(), stream)  # noqa: E731
    terms = lambda: tk.terms_device(d_ids.data_ptr(), ntok, pd, pn, nd, t_id.data_ptr(), t_cnt.data_ptr(), ntok,  # noqa: E731
                                    t_off.data_ptr(), t_n.data_ptr(), work.data_ptr(), need, stream)
    kw = lambda: tk.keywords_device(t_id.data_ptr(), t_cnt.data_ptr(), t_off.data_ptr(), nd, ntok, d_w.data_ptr(), nw,  # noqa: E731
                                    TOPK, k_id.data_ptr(), k_sc.data_ptr(), k_cnt.data_ptr(), k_n.data_ptr(), stream)
    t_cut = timed(torch, cut, steps, warmup)
    t_ids = timed(torch, ids, steps, warmup)
    t_terms = timed(torch, terms, steps, warmup)
    t_kw = timed(torch, kw, steps, warmup)
    nterms = int(t_n.cpu()[0])
    known = int((d_ids != -1).sum().item())
    tk.profile(True)
    tk.profile_reset()
    for _ in range(steps):
        terms()
        kw()
    torch.cuda.synchronize()
    prof = {k: round(v[0] / max(v[1], 1) * (v[1] / steps), 4) for k, v in tk.profile_read().items()
            if k.startswith("k_terms") or k == "k_keywords"}
    tk.profile(False)
    base = t_cut["median_ms"]
    # the call's own traffic: the ids in, the sorted runs out and in twice more (count, write), the CSR out
    moved = 4 * ntok + 8 * T * ((ntok + T - 1) // T) + 8 * known + 2 * 8 * ntok + 8 * nterms
    res = {
        "batch": label, "bytes": nb, "docs": nd, "tokens": ntok, "known_tokens": known, "nterms": nterms,
        "kw_rows_filled": int(k_n.sum().item()),
        "multi_tile_docs": int(multi.sum()),
        "tokens_in_multi_tile_docs_share": round(float((doc_tok[1:] - doc_tok[:-1])[multi].sum()) / max(ntok, 1), 4),
        "work_bytes": int(need),
        "cut_device_hmm1": t_cut, "ids_device": t_ids, "terms_device": t_terms, "keywords_device_top20": t_kw,
        "ids_over_cut": round(t_ids["median_ms"] / base, 4), "terms_over_cut": round(t_terms["median_ms"] / base, 4),
        "keywords_over_cut": round(t_kw["median_ms"] / base, 4),
        "kernels_profile_ms_per_call": prof,
        "terms_bytes_moved_per_token": round(moved / max(ntok, 1), 2),
        "terms_algorithmic_min_bytes_per_token": round((4 * ntok + 8 * nterms) / max(ntok, 1), 2),
        "terms_moved_gb_per_s": round(moved / (t_terms["median_ms"] * 1e-3) / 1e9, 1),
    }
    if forms:
        res["df"] = measure_df(torch, J, forms, hip, t_id, t_n, nterms, ntok, nw, nd, t_terms, steps, warmup)
    if tr_forms:
        del work
        res["textrank"] = measure_textrank(torch, J, tr_forms, d_ids, pd, pn, ntok, nd, t_id, t_off, nterms, d_keep, nw,
                                           t_cut, t_terms, steps, warmup)
        work = None
    print(f"terms_bench.py: {label} measured", file=sys.stderr, flush=True)
    del d_text, d_off, d_ids, t_id, t_cnt, work
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", type=float, nargs="+", default=[1024.0, 128.0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nwords", type=int, default=350_000)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terms_bench.json"))
    ap.add_argument("--df-out", default=os.path.join(ROOT, "profiles", "df_bench.json"))
    ap.add_argument("--tr-out", default=os.path.join(ROOT, "profiles", "textrank_bench.json"))
    ap.add_argument("--textrank-only", action="store_true",
                    help="measure the first corpus and its TextRank rows alone; write --tr-out only")
    args = ap.parse_args()

    import torch

    import jiebahip as J
    import synth

    if not torch.cuda.is_available():
        print("terms_bench.py: no GPU (this measurement does not fall back)", file=sys.stderr)
        return 2
    s = synth.Synth(nwords=args.nwords)
    tmp = tempfile.mkdtemp(prefix="jb_terms_bench_")
    dpath, epath = s.write_files(tmp)
    tk = J.Tokenizer(J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX,
                                   size_override=J.JIEBA_SIZE, device=0))
    with open(dpath, encoding="utf-8") as f:
        keys = [p[0].encode() for p in (ln.split(" ") for ln in f if ln.strip()) if int(p[1]) > 0]
    keys = list(dict.fromkeys(keys))
    tk.set_vocab(keys)
    rng = np.random.default_rng(7)
    w = (1.0 + 10.0 * rng.random(len(keys))).astype(np.float32)
    w[np.array([len(k.decode("utf-8", "replace")) < 2 for k in keys])] = 0.0
    d_w = torch.from_numpy(w).cuda()
    # jb_df_device's two forms: the knob is read at jb_open, so one more tokenizer per form (the call
    # needs no vocabulary); hipMemsetAsync from the runtime the library is bound to
    forms = {}
    old = os.environ.get("JB_DF_COMBINE")
    for name, val in (("atomic", "0"), ("combine", "1")):
        os.environ["JB_DF_COMBINE"] = val
        forms[name] = J.Tokenizer(J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX,
                                                size_override=J.JIEBA_SIZE, device=0))
    if old is None:
        del os.environ["JB_DF_COMBINE"]
    else:
        os.environ["JB_DF_COMBINE"] = old
    # jb_textrank_device's two forms, likewise
    tr_forms = {}
    old = os.environ.get("JB_TR_WINDOW")
    for name, val in (("plain", "0"), ("window", "1")):
        os.environ["JB_TR_WINDOW"] = val
        tr_forms[name] = J.Tokenizer(J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX,
                                                   size_override=J.JIEBA_SIZE, device=0))
    if old is None:
        del os.environ["JB_TR_WINDOW"]
    else:
        os.environ["JB_TR_WINDOW"] = old
    d_keep = torch.from_numpy((w != 0).astype(np.uint8)).cuda()
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "topk": TOPK,
           "tile_tokens": J.JB_TERMS_TILE, "vocabulary_keys": len(keys), "zero_weights": int((w == 0).sum()),
           "batches": []}
    threads = max(1, min(16, os.cpu_count() or 1))
    big = None
    tr_doc = {k: out[k] for k in ("device", "steps", "warmup", "vocabulary_keys")}
    tr_doc["kept_keys"] = int((w != 0).sum())
    tr_doc["forms"] = {"plain": "JB_TR_WINDOW=0: k_tr_push, a gather from memory and one global atomic per kept token",
                       "window": "JB_TR_WINDOW=1: k_tr_push_win, an LDS tile with a halo and a table that combines a "
                                 "workgroup's adds"}

    def write(path, doc):
        text = json.dumps(doc, indent=1)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
        print(text)

    for mib in args.sizes_mib:
        buf, off, _ = s.corpus_parallel(synth.KIND_DOCS, 0, target_bytes=int(mib * (1 << 20)), threads=threads)
        first = big is None
        if first:
            big = (buf, off, mib)
        out["batches"].append(measure(torch, J, tk, d_w, len(w), f"C_syn {mib:g} MiB", buf, off, args.steps, args.warmup,
                                      None if args.textrank_only else forms, hip, tr_forms if first else None, d_keep))
        if first:
            b = out["batches"][-1]
            tr_doc["batches"] = [dict(batch=b["batch"], bytes=b["bytes"], **b.pop("textrank"))]
            if args.textrank_only:
                break
    for t in tr_forms.values():
        t.close()
    write(args.tr_out, tr_doc)
    if args.textrank_only:
        tk.close()
        for t in forms.values():
            t.close()
        return 0
    buf, off, _ = s.corpus(synth.KIND_SENTENCES, 0, max_docs=10_000, target_bytes=64 << 20)
    out["batches"].append(measure(torch, J, tk, d_w, len(w), "S10k: 10,000 sentences", buf, off, args.steps, args.warmup,
                                  forms, hip))
    buf, off, _ = s.corpus(synth.KIND_LONG_PUNCT, 0, target_runes=1_000_000)
    out["batches"].append(measure(torch, J, tk, d_w, len(w), "L1M: one 1,000,000-rune document", buf, off, args.steps,
                                  args.warmup, forms, hip))
    # host memory in, records out, beside the span-returning host call, same machine and run
    buf, off, mib = big
    nb = int(off[-1])
    host = {"batch": f"C_syn {mib:g} MiB from pageable host memory", "bytes": nb}
    o32 = None
    hdf = np.zeros(len(keys), np.uint32)
    for name, fn in (("cut_batch_into32_hmm1", lambda: tk.cut_batch_into32(buf, off, True, o32)),
                     ("keywords_batch_hmm1_top20", lambda: tk.keywords_batch(buf, off, True, w, TOPK)),
                     ("df_batch_hmm1", lambda: tk.df_batch(buf, off, True, hdf))):
        ts = []
        for k in range(args.host_steps + 1):
            t0 = time.perf_counter()
            r = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
            if name.startswith("cut"):
                o32 = r[3]
        ts = ts[1:]  # (the first call grows buffers)
        host[name] = {"median_ms": round(float(np.median(ts)), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
    host["keywords_over_into32"] = round(host["keywords_batch_hmm1_top20"]["median_ms"] /
                                         host["cut_batch_into32_hmm1"]["median_ms"], 4)
    host["df_batch_over_keywords_batch"] = round(host["df_batch_hmm1"]["median_ms"] /
                                                 host["keywords_batch_hmm1_top20"]["median_ms"], 4)
    out["host"] = host
    tk.close()
    for t in forms.values():
        t.close()
    # the document-frequency rows as a document of their own, beside the terms step of the same run
    df_doc = {k: out[k] for k in ("device", "steps", "warmup", "vocabulary_keys")}
    df_doc["forms"] = {"atomic": "JB_DF_COMBINE=0: k_df, one global atomic per entry",
                       "combine": "JB_DF_COMBINE=1: k_df_combine, a table in LDS per workgroup"}
    df_doc["batches"] = [dict(batch=b["batch"], docs=b["docs"], tokens=b["tokens"], **b.pop("df")) for b in out["batches"]]
    df_doc["host"] = {k: host[k] for k in ("batch", "bytes", "keywords_batch_hmm1_top20", "df_batch_hmm1",
                                           "df_batch_over_keywords_batch")}
    write(args.out, out)
    write(args.df_out, df_doc)
    return 0


if __name__ == "__main__":
    sys.exit(main())
