#!/usr/bin/env python3
"""The cost of jb_join_device and jb_cut_batch_join on the benchmark's corpus.

Corpus and dictionary as tools/terms_bench.py (bench.py's config 4: C_syn against the 350k-word D_syn
dictionary, JB_DICT_PREFIX, size 60,101,967), at 1 GiB and at 128 MiB, sep " " and term "\\n".  Per batch,
with device events on the launch stream (--steps after --warmup), all in one process:
  - the plain jb_cut_device step, and jb_join_device on its spans in both forms of the write kernel
    (JB_JOIN_STAGE 0 and 1: one tokenizer per form, the two alternating from step to step), their outputs
    compared byte for byte;
  - the same A/B on search-mode and full-mode spans (copied out of the ctx's arrays first);
  - the join kernels once more through jb_profile_read;
  - the pass's counted bytes (spans read by the count and by the write pass, key bytes read, output
    written) and the share of the HBM peak that is;
and, for the largest corpus from pageable host memory, jb_cut_batch_join beside jb_cut_batch_into32.
Writes one JSON document (--out) and prints it.

    python tools/join_bench.py --out profiles/join_bench.json
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

HBM_PEAK = 8.0e12  # bytes per second (the figure DESIGN.md's shares use)
SEP, TERM = b" ", b"\n"


def joiner(torch, J, tk, d_text, nb, ps, pe, pd, pn, cap, nd, out, ooff, nout, work, need):
    stream = torch.cuda.current_stream().cuda_stream
    return lambda: tk.join_device(d_text.data_ptr(), nb, ps, pe, pd, pn, cap, nd, SEP, TERM, out.data_ptr(), out.numel(),
                                  ooff.data_ptr(), nout.data_ptr(), work.data_ptr(), need, stream)


def counted(ntok, key_bytes, nout, ms):
    """The pass's own traffic: the spans twice (count, write), the key bytes, the output."""
    moved = 16 * ntok + key_bytes + nout
    return {"spans_read_bytes": 16 * ntok, "key_bytes_read": key_bytes, "output_bytes": nout, "moved_bytes": moved,
            "moved_gb_per_s": round(moved / (ms * 1e-3) / 1e9, 1),
            "share_of_hbm_peak": round(moved / (ms * 1e-3) / HBM_PEAK, 4)}


def measure(torch, J, forms, label, buf, off, steps, warmup):
    stream = torch.cuda.current_stream().cuda_stream
    tk = forms["staged"]
    nb, nd = int(off[-1]), len(off) - 1
    d_text = torch.from_numpy(np.ascontiguousarray(buf[:nb])).cuda()
    d_text = torch.cat([d_text, torch.zeros(64, dtype=torch.uint8, device="cuda")])
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    res = {"batch": label, "bytes": nb, "docs": nd}

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
        d = torch.from_numpy(J.dev_to_host(p[2], 8 * (nd + 1), np.int64)).cuda()
        c = torch.tensor([ntok], dtype=torch.int64, device="cuda")
        return s, e, d, c, ntok, n

    cut = lambda: tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)  # noqa: E731
    t_cut = timed(torch, cut, steps, warmup)
    res["cut_device_hmm1"] = t_cut
    for mode in ("cut", "search", "full"):
        s, e, d, c, ntok, cap = spans_of(mode)
        need = J.join_work_bytes(cap, nd)
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        ooff = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
        nout = torch.zeros(1, dtype=torch.int64, device="cuda")
        ocap = (4 if mode == "full" else 2) * nb + nd + 4096
        names = ("plain", "staged")
        outs = {n: torch.empty(ocap, dtype=torch.uint8, device="cuda") for n in names}
        fn = {n: joiner(torch, J, forms[n], d_text, nb, s.data_ptr(), e.data_ptr(), d.data_ptr(), c.data_ptr(), cap, nd,
                        outs[n], ooff, nout, work, need) for n in names}
        row = {"mode": mode, "hmm": mode != "full", "spans": ntok, "span_capacity": cap, "work_bytes": int(need)}
        if len(names) == 2:
            t = timed_ab(torch, fn, steps, warmup)
        else:
            t = {"staged": timed(torch, fn["staged"], steps, warmup)}
        n_out = int(nout.cpu()[0])
        assert n_out <= ocap, (mode, n_out, ocap)
        s64, e64 = s.to(torch.int64), e.to(torch.int64)
        key_bytes = int((e64 - s64).clamp(min=0).sum().item())
        row["output_bytes"] = n_out
        for n in names:
            row["join_device_" + n] = t[n]
            row["join_" + n + "_over_cut"] = round(t[n]["median_ms"] / t_cut["median_ms"], 4)
            row["counted_" + n] = counted(cap, key_bytes, n_out, t[n]["median_ms"])
        if len(names) == 2:
            row["forms_give_identical_bytes"] = bool(torch.equal(outs["plain"][:n_out], outs["staged"][:n_out]))
            row["faster_form"] = min(names, key=lambda n: t[n]["median_ms"])
        prof = {}
        for n in names:
            forms[n].profile(True)
            forms[n].profile_reset()
            for _ in range(steps):
                fn[n]()
            torch.cuda.synchronize()
            prof[n] = {k: round(v[0] / steps, 4) for k, v in forms[n].profile_read().items() if k.startswith("k_join_")}
            forms[n].profile(False)
        row["kernels_profile_ms_per_call"] = prof
        res.setdefault("modes", []).append(row)
        del s, e, d, work, outs, s64, e64
        torch.cuda.empty_cache()
        print(f"join_bench.py: {label} {mode} measured", file=sys.stderr, flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join_bench.json"))
    args = ap.parse_args()

    import torch

    import jiebahip as J
    import synth

    if not torch.cuda.is_available():
        print("join_bench.py: no GPU (this measurement does not fall back)", file=sys.stderr)
        return 2
    s = synth.Synth(nwords=args.nwords)
    tmp = tempfile.mkdtemp(prefix="jb_join_bench_")
    dpath, epath = s.write_files(tmp)
    forms = {}
    old = os.environ.get("JB_JOIN_STAGE")
    for name, val in (("plain", "0"), ("staged", "1")):  # (the knob is read at jb_open)
        os.environ["JB_JOIN_STAGE"] = val
        forms[name] = J.Tokenizer(J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX,
                                                size_override=J.JIEBA_SIZE, device=0))
    if old is None:
        del os.environ["JB_JOIN_STAGE"]
    else:
        os.environ["JB_JOIN_STAGE"] = old
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "sep": SEP.decode(), "term": TERM.decode(), "tile_tokens": J.JB_JOIN_TILE, "long_key_bytes": J.JB_JOIN_LONG,
           "hbm_peak_bytes_per_s": HBM_PEAK,
           "forms": {"plain": "JB_JOIN_STAGE=0: one lane per token, byte by byte",
                     "staged": "JB_JOIN_STAGE=1: a tile's output assembled in LDS, 16-byte stores"},
           "batches": []}
    threads = max(1, min(16, os.cpu_count() or 1))
    big = None
    for mib in args.sizes_mib:
        buf, off, _ = s.corpus_parallel(synth.KIND_DOCS, 0, target_bytes=int(mib * (1 << 20)), threads=threads)
        if big is None:
            big = (buf, off, mib)
        out["batches"].append(measure(torch, J, forms, f"C_syn {mib:g} MiB", buf, off, args.steps, args.warmup))
    # host memory in, joined text out, beside the span-returning host call, same machine and run
    buf, off, mib = big
    host = {"batch": f"C_syn {mib:g} MiB from pageable host memory", "bytes": int(off[-1])}
    tk = forms["staged"]
    o32 = None
    for name, fn in (("cut_batch_into32_hmm1", lambda: tk.cut_batch_into32(buf, off, True, o32)),
                     ("cut_batch_join_hmm1", lambda: tk.cut_batch_join(buf, off, True, "cut", SEP, TERM))):
        ts = []
        r = None
        for k in range(args.host_steps + 1):
            r = None  # (a result is released before the next call, which then reuses its page-locked block)
            t0 = time.perf_counter()
            r = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
            if name.startswith("cut_batch_into32"):
                o32 = r[3]
            else:
                host["joined_bytes"] = int(len(r[0]))
        ts = ts[1:]  # (the first call grows buffers)
        host[name] = {"median_ms": round(float(np.median(ts)), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
    host["join_over_into32"] = round(host["cut_batch_join_hmm1"]["median_ms"] / host["cut_batch_into32_hmm1"]["median_ms"], 4)
    out["host"] = host
    for t in forms.values():
        t.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
