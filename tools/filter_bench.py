#!/usr/bin/env python3
"""The cost of jb_filter_device and of the batch filter on the benchmark's corpus.

Corpus and dictionary as tools/minhash_bench.py (bench.py's config 4: C_syn against the 350k-word D_syn
dictionary, JB_DICT_PREFIX, size 60,101,967), at 1 GiB.  Per batch, with device events on the launch stream
(--steps after --warmup), all in one process:
  - the plain jb_cut_device step, jb_charspans_device and jb_join_device on the plain spans: the yardsticks,
    comparable one-lane-per-token passes over the same spans;
  - jb_filter_device on plain, search-mode and full-mode spans (copied out of the ctx's arrays first) with the
    rule drop = OTHER | INVALID, min_runes = 2, STOP against a stop set of the 1,000 most frequent keys of the
    corpus's first spans, and once with the class test alone; the outputs compared with jb_filter, the host rule,
    on the spans copied back (--host-check);
  - the kernels once more through jb_profile_read;
  - jb_join_device on the filtered list against the unfiltered one;
and, from pageable host memory, jb_cut_batch_join with the batch filter set against the same call without it.
Writes one JSON document (--out) and prints it.

    python tools/filter_bench.py --out profiles/filter_bench.json
"""
import argparse
import collections
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("gen", os.path.join("jieba-go_amd", "python"), "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub))

from terms_bench import timed  # noqa: E402

NSTOP = 1000


def note(msg):
    print("filter_bench.py: " + msg, file=sys.stderr, flush=True)


def measure(torch, J, tk, label, buf, off, steps, warmup, host_check):
    stream = torch.cuda.current_stream().cuda_stream
    nb, nd = int(off[-1]), len(off) - 1
    d_text = torch.from_numpy(np.ascontiguousarray(buf[:nb])).cuda()
    d_text = torch.cat([d_text, torch.zeros(64, dtype=torch.uint8, device="cuda")])
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    res = {"batch": label, "bytes": nb, "docs": nd}
    full_rule = J.filter_rule(("other", "invalid"), 2, 0, True)
    class_rule = J.filter_rule(("other", "invalid"))

    def spans_of(mode):
        """The mode's spans and doc_tok in arrays of this function's own (the ctx's are rewritten by the next cut)."""
        if mode == "cut":
            p = tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)
        elif mode == "search":
            p = tk.cut_device_search(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)
        else:
            p = tk.cut_device_full(d_text.data_ptr(), nb, d_off.data_ptr(), nd, stream)
        torch.cuda.synchronize()
        ntok = int(J.dev_to_host(p[3], 8, np.uint64)[0])
        n = min(ntok, nb)  # (the ctx's arrays hold nb entries)
        hs, he = J.dev_to_host(p[0], 4 * n, np.int32), J.dev_to_host(p[1], 4 * n, np.int32)
        ht = J.dev_to_host(p[2], 8 * (nd + 1), np.int64)
        s, e, t = torch.from_numpy(hs).cuda(), torch.from_numpy(he).cuda(), torch.from_numpy(ht).cuda()
        c = torch.tensor([ntok], dtype=torch.int64, device="cuda")
        return s, e, t, c, ntok, n, (hs.view(np.uint32), he.view(np.uint32), ht.view(np.uint64))

    cut = lambda: tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)  # noqa: E731
    t_cut = timed(torch, cut, steps, warmup)
    res["cut_device_hmm1"] = t_cut
    stop_keys = None
    for mode in ("cut", "search", "full"):
        s, e, t, c, ntok, cap, host_spans = spans_of(mode)
        if stop_keys is None:  # the most frequent keys of the first spans
            hs, he, _ = host_spans
            raw = bytes(buf[:int(he[min(len(he), 400_000) - 1])])
            cnt = collections.Counter(raw[a:b] for a, b in zip(hs[:400_000].tolist(), he[:400_000].tolist()) if b - a <= 255)
            stop_keys = [k for k, _ in cnt.most_common(NSTOP)]
            tk.set_stop_words(stop_keys)
            res["stop_keys"] = len(stop_keys)
        need = J.filter_work_bytes(cap, nd)
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        os_ = torch.empty(cap, dtype=torch.int32, device="cuda")
        oe = torch.empty(cap, dtype=torch.int32, device="cuda")
        odt = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
        on = torch.zeros(1, dtype=torch.int64, device="cuda")
        ost = torch.zeros(5, dtype=torch.int64, device="cuda")
        row = {"mode": mode, "hmm": mode != "full", "spans": ntok, "span_capacity": cap, "work_bytes": int(need)}

        def filt(rule):
            return lambda: tk.filter_device(d_text.data_ptr(), nb, s.data_ptr(), e.data_ptr(), t.data_ptr(), c.data_ptr(),
                                            cap, nd, rule, os_.data_ptr(), oe.data_ptr(), 0, cap, odt.data_ptr(),
                                            on.data_ptr(), ost.data_ptr(), work.data_ptr(), need, stream)

        if mode == "cut":  # the yardsticks on the same spans
            cneed = J.charspans_work_bytes(nb, nd)
            cwork = torch.empty(cneed, dtype=torch.uint8, device="cuda")
            cs = torch.empty(cap, dtype=torch.int32, device="cuda")
            ce = torch.empty(cap, dtype=torch.int32, device="cuda")
            cu = torch.empty(nd, dtype=torch.int32, device="cuda")
            chars = lambda: tk.charspans_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, s.data_ptr(), e.data_ptr(),  # noqa: E731
                                                t.data_ptr(), c.data_ptr(), cap, "rune", cs.data_ptr(), ce.data_ptr(),
                                                cu.data_ptr(), cwork.data_ptr(), cneed, stream)
            row["charspans_device_rune"] = timed(torch, chars, steps, warmup)
            del cwork, cs, ce, cu
        jneed = J.join_work_bytes(cap, nd)
        jwork = torch.empty(jneed, dtype=torch.uint8, device="cuda")
        jcap = nb + cap + nd + 256
        jout = torch.empty(jcap, dtype=torch.uint8, device="cuda")
        joff = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
        jn = torch.zeros(1, dtype=torch.int64, device="cuda")

        def join(ps, pe, pt, pc):
            return lambda: tk.join_device(d_text.data_ptr(), nb, ps, pe, pt, pc, cap, nd, b" ", b"\n", jout.data_ptr(), jcap,
                                          joff.data_ptr(), jn.data_ptr(), jwork.data_ptr(), jneed, stream)

        if mode != "full":  # (full mode's overlapping spans join to more than nb + cap bytes)
            row["join_device_unfiltered"] = timed(torch, join(s.data_ptr(), e.data_ptr(), t.data_ptr(), c.data_ptr()), steps, warmup)
            row["join_unfiltered_bytes"] = int(jn[0])
        for name, rule in (("class_length_stop", full_rule), ("class_only", class_rule)):
            tm = timed(torch, filt(rule), steps, warmup)
            st = ost.cpu().numpy().view(np.uint64)
            sub = {"filter_device": tm, "filter_over_cut": round(tm["median_ms"] / t_cut["median_ms"], 4),
                   "kept": int(on[0]), "stats": dict(zip(("ntokens", "nbad", "nclass", "nlength", "nstop"), st.tolist()))}
            tk.profile(True)
            tk.profile_reset()
            for _ in range(steps):
                filt(rule)()
            torch.cuda.synchronize()
            sub["kernels_profile_ms_per_call"] = {k: round(v[0] / steps, 4) for k, v in tk.profile_read().items()
                                                  if k.startswith("k_filt_")}
            tk.profile(False)
            if host_check and mode in host_check:
                hs, he, ht = host_spans
                t0 = time.perf_counter()
                want = J.filter_spans(np.ascontiguousarray(buf[:nb]), hs, he, ht, rule, J.Vocab(stop_keys), ntok=ntok, cap=cap,
                                      src=False)
                sub["host_rule_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                k = want[4]
                sub["device_outputs_are_the_host_rule's"] = bool(
                    k == int(on[0]) and np.array_equal(os_.cpu().numpy().view(np.uint32)[:k], want[0][:k]) and
                    np.array_equal(oe.cpu().numpy().view(np.uint32)[:k], want[1][:k]) and
                    np.array_equal(odt.cpu().numpy().view(np.uint64), want[3]) and np.array_equal(st, want[5]))
            if name == "class_length_stop" and mode != "full":
                filt(rule)()
                sub["join_device_filtered"] = timed(torch, join(os_.data_ptr(), oe.data_ptr(), odt.data_ptr(), on.data_ptr()),
                                                    steps, warmup)
                sub["join_filtered_bytes"] = int(jn[0])
            row[name] = sub
            note(f"{label} {mode} {name} measured")
        res.setdefault("modes", []).append(row)
        del s, e, t, work, os_, oe, jwork, jout
        torch.cuda.empty_cache()
    del d_text, d_off
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", type=float, nargs="+", default=[1024.0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nwords", type=int, default=350_000)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--host-check", nargs="*", default=["cut"], help="modes whose device outputs are compared with jb_filter")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_bench.json"))
    args = ap.parse_args()

    import torch

    import jiebahip as J
    import synth

    if not torch.cuda.is_available():
        print("filter_bench.py: no GPU (this measurement does not fall back)", file=sys.stderr)
        return 2
    s = synth.Synth(nwords=args.nwords)
    tmp = tempfile.mkdtemp(prefix="jb_filter_bench_")
    dpath, epath = s.write_files(tmp)
    tk = J.Tokenizer(J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX, size_override=J.JIEBA_SIZE,
                                   device=0))
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "rules": {"class_length_stop": "drop OTHER | INVALID, min_runes 2, JB_FILTER_STOP", "class_only": "drop OTHER | INVALID"},
           "batches": []}
    threads = max(1, min(16, os.cpu_count() or 1))
    big = None
    for mib in args.sizes_mib:
        note(f"generating {mib:g} MiB")
        buf, off, _ = s.corpus_parallel(synth.KIND_DOCS, 0, target_bytes=int(mib * (1 << 20)), threads=threads)
        if big is None:
            big = (buf, off, mib)
        out["batches"].append(measure(torch, J, tk, f"C_syn {mib:g} MiB", buf, off, args.steps, args.warmup, args.host_check))
    # host memory in: the joined text with and without the batch filter, same machine and run
    buf, off, mib = big
    host = {"batch": f"C_syn {mib:g} MiB from pageable host memory", "bytes": int(off[-1]), "docs": len(off) - 1}
    for name, on in (("cut_batch_join_hmm1", False), ("cut_batch_join_hmm1_batch_filter", True)):
        if on:
            tk.set_batch_filter(("other", "invalid"), 2, 0, True)
        ts, nout = [], 0
        for k in range(args.host_steps + 1):
            t0 = time.perf_counter()
            r = tk.cut_batch_join(buf, off, True, "cut", b" ", b"\n")
            ts.append((time.perf_counter() - t0) * 1e3)
            nout = int(len(r[0]))
            del r
        ts = ts[1:]  # (the first call grows buffers)
        host[name] = {"median_ms": round(float(np.median(ts)), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2),
                      "joined_bytes": nout}
        note(name + " measured")
    tk.clear_batch_filter()
    host["filtered_over_unfiltered"] = round(host["cut_batch_join_hmm1_batch_filter"]["median_ms"] /
                                             host["cut_batch_join_hmm1"]["median_ms"], 4)
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
