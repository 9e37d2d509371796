#!/usr/bin/env python3
"""The cost of jb_bm25_search_device and jb_search_batch on the benchmark's corpus.

Corpus, dictionary and vocabulary as tools/postings_bench.py (bench.py's config 4: C_syn against the 350k-word
D_syn dictionary, JB_DICT_PREFIX, size 60,101,967; the vocabulary is the dictionary's words with freq > 0), at
1 GiB.  The index is built on the device (cut -> ids -> terms -> postings) and stays there.  The queries are
--queries seeded lists of 1 to 8 ids drawn by corpus frequency (an id's share of all term occurrences), at
--topk.  With device events on the launch stream (--steps after --warmup), all in one process:
  - the plain jb_cut_device step and jb_postings_device: the steps that build what is searched;
  - jb_bm25_norms_device and jb_bm25_idf_device;
  - jb_bm25_search_device in both forms (JB_BM25_FORM 0 and 1, read at jb_open: one tokenizer per form, the order
    alternated from step to step), the kernels once more through jb_profile_read (form 0's memset of the dense
    rows is inside the call's time and outside the kernels');
  - both forms' rows compared with each other byte for byte and with jb_bm25_search, the host rule, on every
    query;
  - the path it replaces: the postings copied to the host and scored there by the numpy reference
    (tests/bm25_ref.py), timed on the first --host-queries queries;
and, from host query text (the ids' keys joined by spaces), jb_search_batch after jb_index_set.
Writes one JSON document (--out) and prints it.

    python tools/bm25_bench.py --out profiles/bm25_bench.json
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("gen", os.path.join("jieba-go_amd", "python"), "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))

from terms_bench import timed, timed_ab  # noqa: E402

FORMS = (("dense", "0"), ("tiles", "1"))


def note(msg):
    print("bm25_bench.py: " + msg, file=sys.stderr, flush=True)


def draw_queries(rng, cf, nq):
    """nq queries of 1 to 8 ids, each id drawn with its share of the corpus's term occurrences."""
    p = cf.astype(np.float64) / float(cf.sum())
    lens = rng.integers(1, 9, nq)
    ids = rng.choice(len(cf), size=int(lens.sum()), p=p).astype(np.uint32)
    return ids, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mib", type=float, default=1024.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nwords", type=int, default=350_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--host-queries", type=int, default=32)
    ap.add_argument("--host-steps", type=int, default=5)
    ap.add_argument("--k1", type=float, default=1.2)
    ap.add_argument("--b", type=float, default=0.75)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bm25_bench.json"))
    args = ap.parse_args()

    import torch

    import bm25_ref as BR
    import jiebahip as J
    import synth

    if not torch.cuda.is_available():
        print("bm25_bench.py: no GPU (this measurement does not fall back)", file=sys.stderr)
        return 2
    s = synth.Synth(nwords=args.nwords)
    tmp = tempfile.mkdtemp(prefix="jb_bm25_bench_")
    dpath, epath = s.write_files(tmp)
    cfg = lambda: J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX, size_override=J.JIEBA_SIZE,  # noqa: E731
                                device=0)
    tk = J.Tokenizer(cfg())
    with open(dpath, encoding="utf-8") as f:
        keys = [p[0].encode() for p in (ln.split(" ") for ln in f if ln.strip()) if int(p[1]) > 0]
    keys = list(dict.fromkeys(keys))
    tk.set_vocab(keys)
    nids = len(keys)
    forms = {}
    old = os.environ.get("JB_BM25_FORM")
    for name, val in FORMS:
        os.environ["JB_BM25_FORM"] = val
        forms[name] = J.Tokenizer(cfg())
    if old is None:
        del os.environ["JB_BM25_FORM"]
    else:
        os.environ["JB_BM25_FORM"] = old
    steps, warmup, nq, topk, k1, b = args.steps, args.warmup, args.queries, args.topk, args.k1, args.b
    note(f"generating {args.size_mib:g} MiB")
    threads = max(1, min(16, os.cpu_count() or 1))
    buf, off, _ = s.corpus_parallel(synth.KIND_DOCS, 0, target_bytes=int(args.size_mib * (1 << 20)), threads=threads)

    # ---- the index, on the device ---------------------------------------------------------------------------------
    stream = torch.cuda.current_stream().cuda_stream
    nb, nd = int(off[-1]), len(off) - 1
    d_text = torch.from_numpy(np.ascontiguousarray(buf[:nb])).cuda()
    d_text = torch.cat([d_text, torch.zeros(64, dtype=torch.uint8, device="cuda")])
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    cut = lambda: tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)  # noqa: E731
    ps, pe, pdt, pn = cut()
    torch.cuda.synchronize()
    tk.device_status(stream)
    ntok = int(J.dev_to_host(pn, 8, np.uint64)[0])
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")  # noqa: E731
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device="cuda")  # noqa: E731
    d_ids, t_id, t_cnt = i32(ntok), i32(ntok), i32(ntok)
    t_off, t_n = i64(nd + 1), torch.zeros(1, dtype=torch.int64, device="cuda")
    need = J.terms_work_bytes(ntok, nd)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    tk.ids_device(d_text.data_ptr(), nb, ps, pe, pn, ntok, d_ids.data_ptr(), stream)
    tk.terms_device(d_ids.data_ptr(), ntok, pdt, pn, nd, t_id.data_ptr(), t_cnt.data_ptr(), ntok, t_off.data_ptr(),
                    t_n.data_ptr(), work.data_ptr(), need, stream)
    torch.cuda.synchronize()
    doc_len = np.diff(J.dev_to_host(pdt, (nd + 1) * 8, np.uint64).astype(np.int64)).astype(np.uint32)
    t_cut = timed(torch, cut, steps, warmup)
    nterms = int(t_n.cpu()[0])
    del work, d_ids
    pneed = J.postings_work_bytes(nterms, nids, nd)
    pwork = torch.empty(pneed, dtype=torch.uint8, device="cuda")
    p_doc, p_tf, p_off, p_n = i32(nterms), i32(nterms), i64(nids + 1), torch.zeros(1, dtype=torch.int64, device="cuda")
    post = lambda: tk.postings_device(t_id.data_ptr(), t_cnt.data_ptr(), t_off.data_ptr(), t_n.data_ptr(), nterms, nd, nids,  # noqa: E731
                                      0, p_doc.data_ptr(), p_tf.data_ptr(), nterms, p_off.data_ptr(), p_n.data_ptr(),
                                      pwork.data_ptr(), pneed, stream)
    t_post = timed(torch, post, steps, warmup)
    npost = int(p_n.cpu()[0])
    del pwork, t_id, t_cnt, d_text
    torch.cuda.empty_cache()
    note("index built")

    # ---- norms and weights ----------------------------------------------------------------------------------------
    avgdl = J.bm25_avgdl(doc_len)
    d_len = torch.from_numpy(doc_len.view(np.int32).copy()).cuda()
    d_norm = torch.empty(nd, dtype=torch.float32, device="cuda")
    d_wt = torch.empty(nids, dtype=torch.float32, device="cuda")
    norms = lambda: tk.bm25_norms_device(d_len.data_ptr(), nd, k1, b, avgdl, d_norm.data_ptr(), stream)  # noqa: E731
    idf = lambda: tk.bm25_idf_device(p_off.data_ptr(), nids, nd, d_wt.data_ptr(), stream)  # noqa: E731
    t_norms, t_idf = timed(torch, norms, steps, warmup), timed(torch, idf, steps, warmup)

    # ---- the postings on the host (what the replaced path copies), the queries ------------------------------------
    t0 = time.perf_counter()
    h_doc = p_doc[:npost].cpu().numpy().view(np.uint32)
    h_tf = p_tf[:npost].cpu().numpy().view(np.uint32)
    h_off = p_off.cpu().numpy().view(np.uint64)
    copy_ms = (time.perf_counter() - t0) * 1e3
    h_norm, h_wt = d_norm.cpu().numpy(), d_wt.cpu().numpy()
    norms_ok = bool(h_norm.tobytes() == J.bm25_norms(doc_len, k1, b, avgdl).tobytes())
    idf_ok = bool(h_wt.tobytes() == J.bm25_idf(h_off, nd).tobytes())
    csum = np.concatenate([[0], np.cumsum(h_tf, dtype=np.uint64)])
    cf = (csum[h_off[1:].astype(np.int64)] - csum[h_off[:-1].astype(np.int64)]).astype(np.uint64)
    q_id, q_off = draw_queries(np.random.default_rng(args.seed), cf, nq)
    q_post = int(np.diff(h_off.astype(np.int64))[q_id].sum())
    d_qid = torch.from_numpy(q_id.view(np.int32).copy()).cuda()
    d_qoff = torch.from_numpy(q_off.view(np.int64).copy()).cuda()

    # ---- the search, both forms -----------------------------------------------------------------------------------
    wneed = J.bm25_work_bytes(nq, nd, topk)
    wbuf = torch.empty(wneed, dtype=torch.uint8, device="cuda")
    outs = {n: (i32(nq * topk), i64(nq * topk), i32(nq)) for n in forms}
    fn = {n: (lambda t=t, o=outs[n]: t.bm25_search_device(p_doc.data_ptr(), p_tf.data_ptr(), p_off.data_ptr(), npost, nids,
                                                          d_norm.data_ptr(), nd, d_wt.data_ptr(), nids, k1, d_qid.data_ptr(),
                                                          len(q_id), d_qoff.data_ptr(), nq, topk, o[0].data_ptr(),
                                                          o[1].data_ptr(), o[2].data_ptr(), wbuf.data_ptr(), wneed, stream))
          for n, t in forms.items()}
    t_search = timed_ab(torch, fn, steps, warmup)
    names = list(forms)
    oa, ob = outs[names[0]], outs[names[1]]
    same = bool(all(torch.equal(x, y) for x, y in zip(oa, ob)))
    prof = {}
    for n, t in forms.items():
        t.profile(True)
        t.profile_reset()
        for _ in range(steps):
            fn[n]()
        torch.cuda.synchronize()
        prof[n] = {k: round(v[0] / steps, 4) for k, v in t.profile_read().items() if k.startswith("k_bm25_") and v[1]}
        t.profile(False)
    best = min(names, key=lambda n: t_search[n]["median_ms"])
    note("device search measured")
    t0 = time.perf_counter()
    w_doc, w_score, w_n = J.bm25_search(h_doc, h_tf, h_off, h_norm, h_wt, k1, q_id, q_off, topk)
    host_rule_ms = (time.perf_counter() - t0) * 1e3
    agree = {}
    for n in names:
        o = outs[n]
        agree[n] = bool(np.array_equal(o[0].cpu().numpy().view(np.uint32).reshape(nq, topk), w_doc) and
                        np.array_equal(o[1].cpu().numpy().view(np.uint64).reshape(nq, topk), w_score) and
                        np.array_equal(o[2].cpu().numpy().view(np.uint32), w_n))
    # the path this replaces: the copy above, then numpy on the host, on a subset
    hq = min(args.host_queries, nq)
    sub_off = q_off[:hq + 1]
    t0 = time.perf_counter()
    r_doc, r_score, r_n = BR.search(h_doc, h_tf, h_off, npost, nids, h_norm, nd, h_wt, nids, k1, q_id, int(sub_off[-1]),
                                    sub_off, topk)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    numpy_ok = bool(np.array_equal(r_doc, w_doc[:hq]) and np.array_equal(r_score, w_score[:hq]) and np.array_equal(r_n, w_n[:hq]))
    note("host paths measured")

    # ---- host text in ---------------------------------------------------------------------------------------------
    qs = [b" ".join(keys[int(t)] for t in q_id[int(q_off[q]):int(q_off[q + 1])]) for q in range(nq)]
    t_off_q = np.zeros(nq + 1, np.uint64)
    t_off_q[1:] = np.cumsum([len(q) for q in qs], dtype=np.uint64)
    qbuf = np.frombuffer(b"".join(qs) + b"\0" * 16, np.uint8)
    t0 = time.perf_counter()
    tk.set_index(h_off, h_doc, h_tf, doc_len, k1=k1, b=b)
    set_ms = (time.perf_counter() - t0) * 1e3
    ts = []
    for _ in range(args.host_steps + 1):
        t0 = time.perf_counter()
        s_doc, s_score, s_n = tk.search_batch(qbuf, t_off_q, True, topk)
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[1:]  # (the first call grows buffers)
    # the same rows when the cut gives back the keys: compare where it does
    cut_ids, cut_off = [], [0]
    s_, e_, dt_ = tk.cut_batch(qbuf, t_off_q, True)
    all_ids = tk.spans_ids(qbuf, s_, e_)
    for q in range(nq):
        cut_ids.append(all_ids[int(dt_[q]):int(dt_[q + 1])])
        cut_off.append(cut_off[-1] + len(cut_ids[-1]))
    c_doc, c_score, c_n = J.bm25_search(h_doc, h_tf, h_off, h_norm, h_wt, k1, np.concatenate(cut_ids).astype(np.uint32),
                                        np.array(cut_off, np.uint64), topk)
    batch_ok = bool(np.array_equal(s_doc, c_doc) and np.array_equal(s_score, c_score) and np.array_equal(s_n, c_n))

    out = {"device": torch.cuda.get_device_name(0), "steps": steps, "warmup": warmup, "vocabulary_keys": nids,
           "tile_documents": J.JB_BM25_TILE,
           "forms": {"dense": "JB_BM25_FORM=0: a dense u64 row per query in the work buffer, one global atomicAdd per "
                              "posting, then the selection per tile and the merge",
                     "tiles": "JB_BM25_FORM=1: one workgroup per query and tile of 8192 documents, the scores in LDS, "
                              "then the merge"},
           "batch": f"C_syn {args.size_mib:g} MiB", "bytes": nb, "docs": nd, "tokens": ntok, "postings": npost, "avgdl": avgdl,
           "k1": k1, "b": b, "queries": nq, "topk": topk, "query_entries": int(len(q_id)),
           "postings_under_the_queries": q_post, "seed": args.seed, "work_bytes": int(wneed),
           "cut_device_hmm1": t_cut, "postings_device": t_post, "bm25_norms_device": t_norms, "bm25_idf_device": t_idf,
           "norms_are_the_host_rule's": norms_ok, "weights_are_the_host_rule's": idf_ok,
           "forms_give_identical_bytes": same, "faster_form": best, "kernels_profile_ms_per_call": prof,
           "rows_are_the_host_rule's": agree, "host_rule_ms": round(host_rule_ms, 1),
           "hits": int(w_n.sum())}
    for n in names:
        ms = t_search[n]["median_ms"]
        out["bm25_search_device_" + n] = t_search[n]
        out["bm25_search_" + n + "_postings_per_us"] = round(q_post / (ms * 1e3), 1)
        out["bm25_search_" + n + "_us_per_query"] = round(ms * 1e3 / nq, 3)
    out["host_path"] = {"copy_postings_ms": round(copy_ms, 1), "numpy_queries": hq, "numpy_ms": round(numpy_ms, 1),
                        "numpy_ms_per_query": round(numpy_ms / max(hq, 1), 2),
                        "numpy_ms_for_all_queries_extrapolated": round(numpy_ms / max(hq, 1) * nq, 1),
                        "numpy_rows_are_the_host_rule's": numpy_ok,
                        "note": "the numpy reference was timed on the first numpy_queries queries only"}
    out["host_text"] = {"query_bytes": int(t_off_q[-1]), "index_set_ms": round(set_ms, 1),
                        "search_batch_hmm1": {"median_ms": round(float(np.median(ts)), 2), "min_ms": round(min(ts), 2),
                                              "max_ms": round(max(ts), 2)},
                        "shipped_form": "JB_BM25_FORM unset", "rows_are_the_host_rule's_over_the_cut's_ids": batch_ok}
    for t in forms.values():
        t.close()
    tk.close()
    text = json.dumps(out, indent=1, ensure_ascii=False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
