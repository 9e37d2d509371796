#!/usr/bin/env python3
"""The cost of jb_postings_device and jb_postings_batch on the benchmark's corpus.

Corpus, dictionary and vocabulary as tools/terms_bench.py (bench.py's config 4: C_syn against the 350k-word D_syn
dictionary, JB_DICT_PREFIX, size 60,101,967; the vocabulary is the dictionary's words with freq > 0), at 1 GiB.
Per batch, with device events on the launch stream (--steps after --warmup), all in one process:
  - the plain jb_cut_device step, jb_terms_device and jb_df_device: the steps before it and its sibling;
  - jb_postings_device in both forms of its scatter kernel (JB_POSTINGS_FORM 0 and 1, read at jb_open: one
    tokenizer per form, the order alternated from step to step), the kernels once more through jb_profile_read;
  - both forms' outputs compared with each other byte for byte and with jb_postings, the host rule, over the
    whole CSR copied back;
  - the path it replaces: the CSR copied to the host and np.argsort(kind="stable") with np.searchsorted there;
and, from pageable host memory, jb_postings_batch beside jb_df_batch.
Writes one JSON document (--out) and prints it.

    python tools/postings_bench.py --out profiles/postings_bench.json
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("gen", os.path.join("jieba-go_amd", "python"), "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub))

from terms_bench import timed, timed_ab  # noqa: E402

FORMS = (("lanes", "0"), ("runs", "1"))


def note(msg):
    print("postings_bench.py: " + msg, file=sys.stderr, flush=True)


def measure(torch, J, tk, forms, nids, label, buf, off, steps, warmup, host_check):
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
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")  # noqa: E731
    d_ids, t_id, t_cnt = i32(ntok), i32(ntok), i32(ntok)
    t_off = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
    t_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    need = J.terms_work_bytes(ntok, nd)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    tk.ids_device(d_text.data_ptr(), nb, ps, pe, pn, ntok, d_ids.data_ptr(), stream)
    terms = lambda: tk.terms_device(d_ids.data_ptr(), ntok, pd, pn, nd, t_id.data_ptr(), t_cnt.data_ptr(), ntok,  # noqa: E731
                                    t_off.data_ptr(), t_n.data_ptr(), work.data_ptr(), need, stream)
    d_df = torch.zeros(nids, dtype=torch.int32, device="cuda")
    df = lambda: tk.df_device(t_id.data_ptr(), t_n.data_ptr(), ntok, d_df.data_ptr(), nids, stream)  # noqa: E731
    t_cut = timed(torch, cut, steps, warmup)
    t_terms = timed(torch, terms, steps, warmup)
    t_df = timed(torch, df, steps, warmup)
    nterms = int(t_n.cpu()[0])
    del work
    # the capacity is the token count, as a chain that reads nothing on the host has it
    cap = ntok
    pneed = J.postings_work_bytes(cap, nids, nd)
    pwork = torch.empty(pneed, dtype=torch.uint8, device="cuda")
    outs = {n: (i32(cap), i32(cap), torch.empty(nids + 1, dtype=torch.int64, device="cuda"),
                torch.zeros(1, dtype=torch.int64, device="cuda")) for n in forms}
    fn = {n: (lambda t=t, o=outs[n]: t.postings_device(t_id.data_ptr(), t_cnt.data_ptr(), t_off.data_ptr(), t_n.data_ptr(),
                                                       cap, nd, nids, 0, o[0].data_ptr(), o[1].data_ptr(), cap,
                                                       o[2].data_ptr(), o[3].data_ptr(), pwork.data_ptr(), pneed, stream))
          for n, t in forms.items()}
    t_post = timed_ab(torch, fn, steps, warmup)
    names = list(forms)
    nposts = int(outs[names[0]][3].cpu()[0])
    oa, ob = outs[names[0]], outs[names[1]]
    same = bool(torch.equal(oa[0][:nposts], ob[0][:nposts]) and torch.equal(oa[1][:nposts], ob[1][:nposts]) and
                torch.equal(oa[2], ob[2]) and torch.equal(oa[3], ob[3]))
    prof = {}
    for n, t in forms.items():
        t.profile(True)
        t.profile_reset()
        for _ in range(steps):
            fn[n]()
        torch.cuda.synchronize()
        prof[n] = {k: round(v[0] / steps, 4) for k, v in t.profile_read().items() if k.startswith("k_post_")}
        t.profile(False)
    best = min(names, key=lambda n: t_post[n]["median_ms"])
    passes = max(1, (int(nids).bit_length() + 7) // 8)
    tile = J.JB_POSTINGS_TILE
    slots = (nterms + tile - 1) // tile * tile
    res = {"batch": label, "bytes": nb, "docs": nd, "tokens": ntok, "nterms": nterms, "nposts": nposts, "nids": nids,
           "capacity": cap, "passes": passes, "launches": 3 * passes + 1, "sorted_slots": slots, "work_bytes": int(pneed),
           "cut_device_hmm1": t_cut, "terms_device": t_terms, "df_device": t_df,
           "forms_give_identical_bytes": same, "faster_form": best, "kernels_profile_ms_per_call": prof,
           # per pass: keys read twice (histogram, scatter), payloads read once, both written once
           "bytes_moved_per_pass": 28 * slots}
    for n in names:
        ms = t_post[n]["median_ms"]
        res["postings_device_" + n] = t_post[n]
        res["postings_" + n + "_over_terms"] = round(ms / t_terms["median_ms"], 4)
        res["postings_" + n + "_over_cut"] = round(ms / t_cut["median_ms"], 4)
        res["postings_" + n + "_entries_per_us"] = round(nterms / (ms * 1e3), 1)
        res["postings_" + n + "_moved_gb_per_s"] = round(passes * 28 * slots / (ms * 1e-3) / 1e9, 1)
    note(f"{label}: device steps measured")
    # the path it replaces: the CSR to the host, a stable argsort there
    t0 = time.perf_counter()
    h_id = t_id[:nterms].cpu().numpy().view(np.uint32)
    h_cnt = t_cnt[:nterms].cpu().numpy().view(np.uint32)
    h_off = t_off.cpu().numpy().view(np.uint64)
    t1 = time.perf_counter()
    take = np.flatnonzero(h_id < nids)
    order = take[np.argsort(h_id[take], kind="stable")]
    a_doc = (np.searchsorted(h_off, order, side="right") - 1).astype(np.uint32)
    a_tf = h_cnt[order]
    a_off = np.searchsorted(h_id[order], np.arange(nids + 1, dtype=np.uint32), side="left").astype(np.uint64)
    t2 = time.perf_counter()
    res["host_path"] = {"copy_csr_ms": round((t1 - t0) * 1e3, 1), "argsort_stable_and_gather_ms": round((t2 - t1) * 1e3, 1),
                        "total_ms": round((t2 - t0) * 1e3, 1)}
    res["host_path_over_postings_" + best] = round((t2 - t0) * 1e3 / t_post[best]["median_ms"], 1)
    g = outs[best]
    g_doc, g_tf = g[0][:nposts].cpu().numpy().view(np.uint32), g[1][:nposts].cpu().numpy().view(np.uint32)
    g_off = g[2].cpu().numpy().view(np.uint64)
    res["device_outputs_are_numpy's"] = bool(nposts == len(order) and np.array_equal(g_doc, a_doc) and
                                             np.array_equal(g_tf, a_tf) and np.array_equal(g_off, a_off))
    del a_doc, a_tf, order, take
    if host_check:
        t0 = time.perf_counter()
        w_doc, w_tf, w_off, w_n = J.postings(h_id, h_cnt, h_off, nids)
        res["host_rule_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["device_outputs_are_the_host_rule's"] = bool(w_n == nposts and np.array_equal(g_doc, w_doc[:w_n]) and
                                                         np.array_equal(g_tf, w_tf[:w_n]) and np.array_equal(g_off, w_off))
    lens = np.diff(g_off.astype(np.int64))
    res["longest_list"] = int(lens.max()) if len(lens) else 0
    res["empty_lists"] = int((lens == 0).sum())
    res["list_lengths_are_df_device's"] = bool(np.array_equal(
        lens * (steps + warmup), d_df.cpu().numpy().view(np.uint32).astype(np.int64)))
    note(f"{label}: host paths measured")
    del d_text, d_off, d_ids, t_id, t_cnt, pwork, outs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", type=float, nargs="+", default=[1024.0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nwords", type=int, default=350_000)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--no-host-check", action="store_true", help="skip the comparison with jb_postings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postings_bench.json"))
    args = ap.parse_args()

    import torch

    import jiebahip as J
    import synth

    if not torch.cuda.is_available():
        print("postings_bench.py: no GPU (this measurement does not fall back)", file=sys.stderr)
        return 2
    s = synth.Synth(nwords=args.nwords)
    tmp = tempfile.mkdtemp(prefix="jb_postings_bench_")
    dpath, epath = s.write_files(tmp)
    cfg = lambda: J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX, size_override=J.JIEBA_SIZE,  # noqa: E731
                                device=0)
    tk = J.Tokenizer(cfg())
    with open(dpath, encoding="utf-8") as f:
        keys = [p[0].encode() for p in (ln.split(" ") for ln in f if ln.strip()) if int(p[1]) > 0]
    keys = list(dict.fromkeys(keys))
    tk.set_vocab(keys)
    nids = len(keys)
    # the scatter kernel's two forms: the knob is read at jb_open, so one more tokenizer per form (the call needs
    # no vocabulary)
    forms = {}
    old = os.environ.get("JB_POSTINGS_FORM")
    for name, val in FORMS:
        os.environ["JB_POSTINGS_FORM"] = val
        forms[name] = J.Tokenizer(cfg())
    if old is None:
        del os.environ["JB_POSTINGS_FORM"]
    else:
        os.environ["JB_POSTINGS_FORM"] = old
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "vocabulary_keys": nids,
           "tile_entries": J.JB_POSTINGS_TILE,
           "forms": {"lanes": "JB_POSTINGS_FORM=0: every entry written from its lane to its global position",
                     "runs": "JB_POSTINGS_FORM=1: the tile reordered by digit in LDS, then written in runs"},
           "batches": []}
    threads = max(1, min(16, os.cpu_count() or 1))
    big = None
    for mib in args.sizes_mib:
        note(f"generating {mib:g} MiB")
        buf, off, _ = s.corpus_parallel(synth.KIND_DOCS, 0, target_bytes=int(mib * (1 << 20)), threads=threads)
        if big is None:
            big = (buf, off, mib)
        out["batches"].append(measure(torch, J, tk, forms, nids, f"C_syn {mib:g} MiB", buf, off, args.steps, args.warmup,
                                      not args.no_host_check))
    for t in forms.values():
        t.close()
    # host memory in, the index out, beside the document frequencies of the same chain, same machine and run
    buf, off, mib = big
    host = {"batch": f"C_syn {mib:g} MiB from pageable host memory", "bytes": int(off[-1]), "docs": len(off) - 1,
            "shipped_form": "JB_POSTINGS_FORM unset"}
    hdf = np.zeros(nids, np.uint32)
    pcap = out["batches"][0]["nposts"]
    for name, fn in (("df_batch_hmm1", lambda: tk.df_batch(buf, off, True, hdf)),
                     ("postings_batch_hmm1", lambda: tk.postings_batch(buf, off, True, 0, nids, pcap))):
        ts = []
        for k in range(args.host_steps + 1):
            t0 = time.perf_counter()
            r = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        if name.startswith("postings"):
            host["postings_returned"] = int(len(r[1]))
        del r
        ts = ts[1:]  # (the first call grows buffers)
        host[name] = {"median_ms": round(float(np.median(ts)), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
        note(name + " measured")
    host["postings_batch_over_df_batch"] = round(host["postings_batch_hmm1"]["median_ms"] / host["df_batch_hmm1"]["median_ms"], 4)
    out["host"] = host
    tk.close()
    text = json.dumps(out, indent=1, ensure_ascii=False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
