#!/usr/bin/env python3
"""The cost of jb_wc_add_device, jb_wc_read and jb_wc_batch on the benchmark's corpus.

Corpus and dictionary as tools/terms_bench.py (bench.py's config 4: C_syn against the 350k-word D_syn
dictionary, JB_DICT_PREFIX, size 60,101,967), at 1 GiB and at 128 MiB.  Per batch, with device events on the
launch stream (--steps after --warmup), all in one process:
  - the plain jb_cut_device step;
  - jb_wc_add_device on its spans in both forms of the count pass (JB_WC_COMBINE 0 and 1: one tokenizer and
    one table per form, the two alternating from step to step), into a table that already holds the batch's
    keys (the steady state of a corpus of many batches) and, with jb_wc_init_device in front, into an empty
    one (every key is claimed and stored); the two tables' results compared key for key;
  - the same A/B on search-mode and full-mode spans (copied out of the ctx's arrays first);
  - the three kernels once more through jb_profile_read;
  - jb_wc_read (the copy of the table, the sort), by the host's clock;
  - jb_ids_device on the plain spans with the vocabulary the counts give (jb_vocab_set with the keys read);
and, for the largest corpus from pageable host memory, jb_wc_batch beside jb_cut_batch_into32 and beside the
path it replaces: jb_cut_batch_into32 plus a count of its spans on the host, both with jb_wc_count (a C++
unordered_map over the span strings, once) and with Python's Counter over the spans of the first
--counter-mib MiB.  Writes one JSON document (--out) and prints it.

    python tools/wc_bench.py --out profiles/wc_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("gen", os.path.join("jieba-go_amd", "python"), "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub))

from terms_bench import timed, timed_ab  # noqa: E402

NAMES = ("atomic", "combine")


def read_ms(J, tk, ptr, n, reps=3):
    """jb_wc_read alone (no Python lists are built), by the host's clock: (median ms, keys)."""
    ts, nkeys = [], 0
    for _ in range(reps):
        r = J.jb_wc_result()
        t0 = time.perf_counter()
        J._check(J.lib().jb_wc_read(tk.h, C.c_void_p(ptr), n, None, 1, 0, C.byref(r)))
        ts.append((time.perf_counter() - t0) * 1e3)
        nkeys = int(r.nkeys)
        J.lib().jb_wc_result_free(C.byref(r))
    return round(float(np.median(ts)), 2), nkeys


def measure(torch, J, forms, label, buf, off, steps, warmup, nslots, pool):
    stream = torch.cuda.current_stream().cuda_stream
    tk = forms["combine"]
    nb, nd = int(off[-1]), len(off) - 1
    d_text = torch.from_numpy(np.ascontiguousarray(buf[:nb])).cuda()
    d_text = torch.cat([d_text, torch.zeros(64, dtype=torch.uint8, device="cuda")])
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    res = {"batch": label, "bytes": nb, "docs": nd}
    ntable = J.wc_table_bytes(nslots, pool)
    tables = {n: torch.empty(ntable, dtype=torch.uint8, device="cuda") for n in NAMES}

    def spans_of(mode):
        """The mode's spans in arrays of this function's own (the ctx's are rewritten by the next cut)."""
        if mode == "cut":
            p = tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)
        elif mode == "search":
            p = tk.cut_device_search(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)
        else:
            p = tk.cut_device_full(d_text.data_ptr(), nb, d_off.data_ptr(), nd, stream)
        torch.cuda.synchronize()
        ntok = int(J.dev_to_host(p[3], 8, np.uint64)[0])
        n = min(ntok, nb)  # (the ctx's arrays hold nb entries)
        s = torch.from_numpy(J.dev_to_host(p[0], 4 * n, np.int32)).cuda()
        e = torch.from_numpy(J.dev_to_host(p[1], 4 * n, np.int32)).cuda()
        c = torch.tensor([ntok], dtype=torch.int64, device="cuda")
        return s, e, c, ntok, n

    cut = lambda: tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)  # noqa: E731
    t_cut = timed(torch, cut, steps, warmup)
    res["cut_device_hmm1"] = t_cut
    init = {n: (lambda n=n: forms[n].wc_init_device(tables[n].data_ptr(), ntable, nslots, pool, stream)) for n in NAMES}
    res["wc_init_device"] = timed(torch, init["combine"], steps, warmup)
    for mode in ("cut", "search", "full"):
        s, e, c, ntok, cap = spans_of(mode)
        need = J.wc_work_bytes(cap)
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        add = {n: (lambda n=n: forms[n].wc_add_device(tables[n].data_ptr(), ntable, d_text.data_ptr(), nb, s.data_ptr(),
                                                      e.data_ptr(), c.data_ptr(), cap, work.data_ptr(), need, stream))
               for n in NAMES}

        def fresh(n):
            init[n]()
            add[n]()
        row = {"mode": mode, "hmm": mode != "full", "spans": ntok, "span_capacity": cap, "work_bytes": int(need)}
        t_first = timed_ab(torch, {n: (lambda n=n: fresh(n)) for n in NAMES}, max(3, steps // 2), 1)
        # one batch in each table, read and compared; then the steady state: the keys are all there
        for n in NAMES:
            fresh(n)
        got = {n: forms[n].wc_read(tables[n].data_ptr(), ntable, 1, 0, stream) for n in NAMES}
        a, b = got["atomic"], got["combine"]
        row["distinct_keys"] = len(b.keys)
        row["totals"] = {"tokens": b.tokens, "bad": b.bad, "long": b.long, "dropped": b.dropped, "collided": b.collided}
        row["counted_plus_totals_is_tokens"] = bool(int(b.counts.sum()) + b.bad + b.long + b.dropped + b.collided == b.tokens)
        row["forms_give_identical_results"] = bool(
            a.keys == b.keys and np.array_equal(a.counts, b.counts) and
            (a.tokens, a.bad, a.long, a.dropped, a.collided) == (b.tokens, b.bad, b.long, b.dropped, b.collided))
        row["top_keys"] = [[k.decode("utf-8", "replace"), int(v)] for k, v in zip(b.keys[:5], b.counts[:5].tolist())]
        t_warm = timed_ab(torch, add, steps, warmup)
        for n in NAMES:
            row["wc_add_device_" + n] = t_warm[n]
            row["wc_add_" + n + "_over_cut"] = round(t_warm[n]["median_ms"] / t_cut["median_ms"], 4)
            row["wc_init_and_first_add_" + n] = t_first[n]
        row["faster_form"] = min(NAMES, key=lambda n: t_warm[n]["median_ms"])
        row["faster_form_first_add"] = min(NAMES, key=lambda n: t_first[n]["median_ms"])
        prof = {}
        for n in NAMES:
            forms[n].profile(True)
            forms[n].profile_reset()
            for _ in range(steps):
                add[n]()
            torch.cuda.synchronize()
            prof[n] = {k: round(v[0] / steps, 4) for k, v in forms[n].profile_read().items() if k.startswith("k_wc_")}
            forms[n].profile(False)
        row["kernels_profile_ms_per_call"] = prof
        ms, nkeys = read_ms(J, tk, tables["combine"].data_ptr(), ntable)
        row["wc_read_ms"] = ms
        row["table_bytes"] = int(ntable)
        if mode == "cut":  # the vocabulary the counts give, and the id step with it
            tk.set_vocab(b.keys)
            ids = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda")
            idf = lambda: tk.ids_device(d_text.data_ptr(), nb, s.data_ptr(), e.data_ptr(), c.data_ptr(), cap,  # noqa: E731
                                        ids.data_ptr(), stream)
            row["ids_device_with_fitted_vocab"] = timed(torch, idf, steps, warmup)
            row["unknown_ids_after_fit"] = int((ids[:cap] == -1).sum().item())
            for n in NAMES:
                row["wc_add_" + n + "_over_ids"] = round(t_warm[n]["median_ms"] / row["ids_device_with_fitted_vocab"]["median_ms"], 4)
            tk.set_vocab(None)
            del ids
        res.setdefault("modes", []).append(row)
        del s, e, work
        torch.cuda.empty_cache()
        print(f"wc_bench.py: {label} {mode} measured", file=sys.stderr, flush=True)
    del d_text, d_off, tables
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", type=float, nargs="+", default=[1024.0, 128.0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nwords", type=int, default=350_000)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--counter-mib", type=float, default=16.0)
    ap.add_argument("--nslots", type=int, default=1 << 22)
    ap.add_argument("--pool-mib", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wc_bench.json"))
    args = ap.parse_args()

    import torch

    import jiebahip as J
    import synth

    if not torch.cuda.is_available():
        print("wc_bench.py: no GPU (this measurement does not fall back)", file=sys.stderr)
        return 2
    s = synth.Synth(nwords=args.nwords)
    tmp = tempfile.mkdtemp(prefix="jb_wc_bench_")
    dpath, epath = s.write_files(tmp)
    forms = {}
    old = os.environ.get("JB_WC_COMBINE")
    for name, val in (("atomic", "0"), ("combine", "1")):  # (the knob is read at jb_open)
        os.environ["JB_WC_COMBINE"] = val
        forms[name] = J.Tokenizer(J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX,
                                                size_override=J.JIEBA_SIZE, device=0))
    if old is None:
        del os.environ["JB_WC_COMBINE"]
    else:
        os.environ["JB_WC_COMBINE"] = old
    pool = args.pool_mib << 20
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "nslots": args.nslots,
           "pool_bytes": pool,
           "forms": {"atomic": "JB_WC_COMBINE=0: one global u64 atomic per token",
                     "combine": "JB_WC_COMBINE=1: a workgroup's adds to a slot combined in an LDS table first"},
           "batches": []}
    threads = max(1, min(16, os.cpu_count() or 1))
    big = None
    for mib in args.sizes_mib:
        print(f"wc_bench.py: generating {mib:g} MiB", file=sys.stderr, flush=True)
        buf, off, _ = s.corpus_parallel(synth.KIND_DOCS, 0, target_bytes=int(mib * (1 << 20)), threads=threads)
        if big is None:
            big = (buf, off, mib)
        out["batches"].append(measure(torch, J, forms, f"C_syn {mib:g} MiB", buf, off, args.steps, args.warmup,
                                      args.nslots, pool))
    # host memory in, beside the span-returning host call and the host count it feeds, same machine and run
    buf, off, mib = big
    nb = int(off[-1])
    host = {"batch": f"C_syn {mib:g} MiB from pageable host memory", "bytes": nb}
    tk = forms["combine"]
    ntable = J.wc_table_bytes(args.nslots, pool)
    table = torch.empty(ntable, dtype=torch.uint8, device="cuda")
    tk.wc_init_device(table.data_ptr(), ntable, args.nslots, pool)
    o32 = None
    spans = None
    for name, fn in (("cut_batch_into32_hmm1", lambda: tk.cut_batch_into32(buf, off, True, o32)),
                     ("wc_batch_hmm1", lambda: tk.wc_batch(buf, off, True, table.data_ptr(), ntable, "cut"))):
        ts = []
        for k in range(args.host_steps + 1):
            t0 = time.perf_counter()
            r = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
            if name.startswith("cut_batch_into32"):
                o32 = r[3]
                spans = (r[0], r[1])
        ts = ts[1:]  # (the first call grows buffers)
        host[name] = {"median_ms": round(float(np.median(ts)), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
    host["wc_batch_over_into32"] = round(host["wc_batch_hmm1"]["median_ms"] / host["cut_batch_into32_hmm1"]["median_ms"], 4)
    ms, nkeys = read_ms(J, tk, table.data_ptr(), ntable)
    host["wc_read_ms"], host["distinct_keys"] = ms, nkeys
    # the path this replaces: the spans on the host, sliced into strings and counted there
    text = np.ascontiguousarray(buf[:nb])
    t0 = time.perf_counter()
    ref = J.wc_count(text, spans[0], spans[1])
    host["host_count_cpp_unordered_map_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    got = tk.wc_read(table.data_ptr(), ntable)
    per = args.host_steps + 1  # (every call above added the batch once more)
    host["device_counts_are_the_host_counts"] = bool(
        got.keys == ref.keys and got.counts.tolist() == [per * v for v in ref.counts.tolist()] and got.dropped == 0 and
        got.collided == 0)
    host["replaced_path_ms"] = round(host["cut_batch_into32_hmm1"]["median_ms"] + host["host_count_cpp_unordered_map_ms"], 1)
    host["replaced_path_over_wc_batch"] = round(host["replaced_path_ms"] / host["wc_batch_hmm1"]["median_ms"], 2)
    share = int(args.counter_mib * (1 << 20))
    nd = int(np.searchsorted(off, share, side="right")) - 1
    k = int(np.searchsorted(spans[1], int(off[nd]), side="right"))
    raw = text[:int(off[nd])].tobytes()
    ss, ee = spans[0][:k].tolist(), spans[1][:k].tolist()
    t0 = time.perf_counter()
    cnt = Counter(raw[a:b] for a, b in zip(ss, ee))
    py_ms = (time.perf_counter() - t0) * 1e3
    host["python_counter"] = {"bytes": int(off[nd]), "spans": k, "distinct_keys": len(cnt), "ms": round(py_ms, 1),
                              "ms_per_mib": round(py_ms / (int(off[nd]) / (1 << 20)), 2)}
    out["host"] = host
    for t in forms.values():
        t.close()
    text = json.dumps(out, indent=1, ensure_ascii=False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
