#!/usr/bin/env python3
"""The cost of jb_minhash_device and jb_minhash_batch on the benchmark's corpus.

Corpus and dictionary as tools/wc_bench.py (bench.py's config 4: C_syn against the 350k-word D_syn dictionary,
JB_DICT_PREFIX, size 60,101,967), at 1 GiB and at 128 MiB.  Per batch, with device events on the launch stream
(--steps after --warmup), all in one process:
  - the plain jb_cut_device step and jb_wc_add_device on its spans, for comparison;
  - jb_minhash_device on plain, search-mode and full-mode spans (copied out of the ctx's arrays first), in both
    forms of the signature kernel (JB_MH_FORM 0 and 1: one tokenizer per form, the two alternating from step to
    step), at n = 5, K = 128 and at n = 1, K = 64; the two forms' outputs compared over the whole corpus, and
    compared with jb_minhash, the host rule, on the spans copied back;
  - the kernels once more through jb_profile_read;
  - jb_minhash_bands_device (16 bands of 8 rows);
and, for the largest corpus from pageable host memory, jb_minhash_batch beside jb_cut_batch_into32 and beside the
path it replaces: jb_cut_batch_into32 plus jb_minhash on the host, measured on the first --host-mib MiB and
reported per MiB.  Writes one JSON document (--out) and prints it.

    python tools/minhash_bench.py --out profiles/minhash_bench.json
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

NAMES = ("plain", "staged")
SHAPES = ((5, 128), (1, 64))  # (n, K)
SEED = 1


def note(msg):
    print("minhash_bench.py: " + msg, file=sys.stderr, flush=True)


def measure(torch, J, forms, label, buf, off, steps, warmup, host_check):
    stream = torch.cuda.current_stream().cuda_stream
    tk = forms["plain"]
    nb, nd = int(off[-1]), len(off) - 1
    d_text = torch.from_numpy(np.ascontiguousarray(buf[:nb])).cuda()
    d_text = torch.cat([d_text, torch.zeros(64, dtype=torch.uint8, device="cuda")])
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    res = {"batch": label, "bytes": nb, "docs": nd}

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
    for mode in ("cut", "search", "full"):
        s, e, t, c, ntok, cap, host_spans = spans_of(mode)
        need = J.minhash_work_bytes(cap, nd)
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        row = {"mode": mode, "hmm": mode != "full", "spans": ntok, "span_capacity": cap, "work_bytes": int(need)}
        if mode == "cut":  # the word-count step on the same spans, for comparison
            nslots, pool = 1 << 22, 64 << 20
            ntable = J.wc_table_bytes(nslots, pool)
            table = torch.empty(ntable, dtype=torch.uint8, device="cuda")
            wwork = torch.empty(J.wc_work_bytes(cap), dtype=torch.uint8, device="cuda")
            tk.wc_init_device(table.data_ptr(), ntable, nslots, pool, stream)
            wc = lambda: tk.wc_add_device(table.data_ptr(), ntable, d_text.data_ptr(), nb, s.data_ptr(), e.data_ptr(),  # noqa: E731
                                          c.data_ptr(), cap, wwork.data_ptr(), len(wwork), stream)
            row["wc_add_device"] = timed(torch, wc, steps, warmup)
            del table, wwork
        for n, K in SHAPES:
            sig = {f: torch.empty(nd * K, dtype=torch.int32, device="cuda") for f in NAMES}
            dn = {f: torch.empty(nd, dtype=torch.int32, device="cuda") for f in NAMES}
            run = {f: (lambda f=f: forms[f].minhash_device(d_text.data_ptr(), nb, s.data_ptr(), e.data_ptr(), t.data_ptr(),
                                                           c.data_ptr(), cap, nd, n, K, SEED, sig[f].data_ptr(),
                                                           dn[f].data_ptr(), work.data_ptr(), need, stream))
                   for f in NAMES}
            tm = timed_ab(torch, run, steps, warmup)
            sub = {"n": n, "K": K}
            for f in NAMES:
                sub["minhash_device_" + f] = tm[f]
                sub["minhash_" + f + "_over_cut"] = round(tm[f]["median_ms"] / t_cut["median_ms"], 4)
            sub["faster_form"] = min(NAMES, key=lambda f: tm[f]["median_ms"])
            sub["forms_give_identical_bits"] = bool(torch.equal(sig["plain"], sig["staged"]) and
                                                    torch.equal(dn["plain"], dn["staged"]))
            sub["shingles"] = int(dn["plain"].cpu().numpy().view(np.uint32).astype(np.uint64).sum())
            prof = {}
            for f in NAMES:
                forms[f].profile(True)
                forms[f].profile_reset()
                for _ in range(steps):
                    run[f]()
                torch.cuda.synchronize()
                prof[f] = {k: round(v[0] / steps, 4) for k, v in forms[f].profile_read().items() if k.startswith("k_mh_")}
                forms[f].profile(False)
            sub["kernels_profile_ms_per_call"] = prof
            if (n, K) == SHAPES[0]:
                B, R = 16, 8
                keys = torch.empty(nd * B, dtype=torch.int64, device="cuda")
                bands = lambda: tk.minhash_bands_device(sig["plain"].data_ptr(), dn["plain"].data_ptr(), nd, K, B, R,  # noqa: E731
                                                        keys.data_ptr(), stream)
                sub["minhash_bands_device_16x8"] = timed(torch, bands, steps, warmup)
            if host_check and mode in host_check:
                hs, he, ht = host_spans
                t0 = time.perf_counter()
                want = J.minhash(np.ascontiguousarray(buf[:nb]), hs, he, ht, n, K, SEED, ntok=ntok, cap=cap)
                sub["host_rule_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                sub["device_bits_are_the_host_rule's"] = bool(
                    np.array_equal(sig["plain"].cpu().numpy().view(np.uint32).reshape(nd, K), want[0]) and
                    np.array_equal(dn["plain"].cpu().numpy().view(np.uint32), want[1]))
            row.setdefault("shapes", []).append(sub)
            note(f"{label} {mode} n={n} K={K} measured")
        res.setdefault("modes", []).append(row)
        del s, e, t, work
        torch.cuda.empty_cache()
    del d_text, d_off
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", type=float, nargs="+", default=[1024.0, 128.0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nwords", type=int, default=350_000)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--host-mib", type=float, default=16.0)
    ap.add_argument("--host-check", nargs="*", default=["cut"], help="modes whose device bits are compared with jb_minhash")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minhash_bench.json"))
    args = ap.parse_args()

    import torch

    import jiebahip as J
    import synth

    if not torch.cuda.is_available():
        print("minhash_bench.py: no GPU (this measurement does not fall back)", file=sys.stderr)
        return 2
    s = synth.Synth(nwords=args.nwords)
    tmp = tempfile.mkdtemp(prefix="jb_mh_bench_")
    dpath, epath = s.write_files(tmp)
    forms = {}
    old = os.environ.get("JB_MH_FORM")
    for name, val in (("plain", "0"), ("staged", "1")):  # (the knob is read at jb_open)
        os.environ["JB_MH_FORM"] = val
        forms[name] = J.Tokenizer(J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX,
                                                size_override=J.JIEBA_SIZE, device=0))
    if old is None:
        del os.environ["JB_MH_FORM"]
    else:
        os.environ["JB_MH_FORM"] = old
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "seed": SEED,
           "forms": {"plain": "JB_MH_FORM=0: one lane per token walks the K functions, atomicMin where a load shows a larger slot",
                     "staged": "JB_MH_FORM=1: a tile's hashes and shingles in LDS, one lane per function, one atomicMin "
                               "per document run"},
           "batches": []}
    threads = max(1, min(16, os.cpu_count() or 1))
    big = None
    for mib in args.sizes_mib:
        note(f"generating {mib:g} MiB")
        buf, off, _ = s.corpus_parallel(synth.KIND_DOCS, 0, target_bytes=int(mib * (1 << 20)), threads=threads)
        if big is None:
            big = (buf, off, mib)
        out["batches"].append(measure(torch, J, forms, f"C_syn {mib:g} MiB", buf, off, args.steps, args.warmup,
                                      args.host_check))
    # host memory in, beside the span-returning host call and the host sketch it feeds, same machine and run
    buf, off, mib = big
    nb, nd = int(off[-1]), len(off) - 1
    host = {"batch": f"C_syn {mib:g} MiB from pageable host memory", "bytes": nb, "docs": nd}
    tk = forms["staged"]  # (the form that ships)
    n, K = SHAPES[0]
    o32, spans, got = None, None, None
    for name, fn in (("cut_batch_into32_hmm1", lambda: tk.cut_batch_into32(buf, off, True, o32)),
                     ("minhash_batch_hmm1", lambda: tk.minhash_batch(buf, off, True, n, K, SEED, "cut"))):
        ts = []
        for k in range(args.host_steps + 1):
            t0 = time.perf_counter()
            r = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
            if name.startswith("cut_batch_into32"):
                o32 = r[3]
                spans = (r[0], r[1], r[2])
            else:
                got = r
        ts = ts[1:]  # (the first call grows buffers)
        host[name] = {"median_ms": round(float(np.median(ts)), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
        note(name + " measured")
    host["n"], host["K"] = n, K
    host["bytes_copied_back"] = int(got[0].nbytes + got[1].nbytes)
    host["minhash_batch_over_into32"] = round(host["minhash_batch_hmm1"]["median_ms"] / host["cut_batch_into32_hmm1"]["median_ms"], 4)
    # the path this replaces: the spans on the host, hashed K times there; on a slice of whole documents
    share = int(args.host_mib * (1 << 20))
    d1 = max(1, int(np.searchsorted(off, share, side="right")) - 1)
    k1 = int(spans[2][d1])
    text = np.ascontiguousarray(buf[:int(off[d1])])
    t0 = time.perf_counter()
    want = J.minhash(text, spans[0][:k1], spans[1][:k1], spans[2][:d1 + 1], n, K, SEED)
    ms = (time.perf_counter() - t0) * 1e3
    host["host_rule_on_slice"] = {"bytes": int(off[d1]), "docs": d1, "spans": k1, "ms": round(ms, 1),
                                  "ms_per_mib": round(ms / (int(off[d1]) / (1 << 20)), 2)}
    host["batch_bits_are_the_host_rule's_on_slice"] = bool(np.array_equal(got[0][:d1], want[0]) and
                                                           np.array_equal(got[1][:d1], want[1]))
    host["replaced_path_ms_estimate"] = round(host["cut_batch_into32_hmm1"]["median_ms"] +
                                              host["host_rule_on_slice"]["ms_per_mib"] * nb / (1 << 20), 1)
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
