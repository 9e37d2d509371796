#!/usr/bin/env python3
"""The cost of jb_charspans_device and jb_cut_batch_charspans on the benchmark's corpus.

Corpus and dictionary as tools/join_bench.py (bench.py's config 4: C_syn against the 350k-word D_syn
dictionary, JB_DICT_PREFIX, size 60,101,967), at 1 GiB and at 128 MiB.  Per batch, with device events on the
launch stream (--steps after --warmup), all in one process:
  - the plain jb_cut_device step and jb_join_device (sep " ", term "\\n") on its spans;
  - jb_charspans_device on the spans of each mode (copied out of the ctx's arrays first) in both units, into
    arrays of its own;
  - the pass's kernels once more through jb_profile_read;
  - the pass's counted bytes (the text read once, the bitmaps and prefixes written and read back, the spans
    read and the character spans written) and the share of the HBM peak that is;
and, for the largest corpus from pageable host memory, jb_cut_batch_charspans beside jb_cut_batch_into32 of
the same batch plus the numpy conversion of its spans on the host (a cumulative sum over the rune-start mask
and two gathers: the path the call replaces), whose offsets are compared with the call's.
Writes one JSON document (--out) and prints it.

    python tools/charspans_bench.py --out profiles/charspans_bench.json
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

from terms_bench import timed  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second (the figure DESIGN.md's shares use)
UNITS = ("rune", "utf16")


def counted(nb, ntok, utf16, ms):
    """The pass's own traffic: the text, the bitmaps (one u64 word per 64 bytes, two in UTF-16) and the u32
    prefixes written by the classification and read by the lookup, 8 bytes per token in and 8 out."""
    maps = (nb // 64 + 1) * ((16 if utf16 else 8) + 4)
    moved = nb + 2 * maps + 16 * ntok
    return {"text_bytes_read": nb, "bitmap_and_prefix_bytes": maps, "span_bytes_read_and_written": 16 * ntok,
            "moved_bytes": moved, "moved_gb_per_s": round(moved / (ms * 1e-3) / 1e9, 1),
            "share_of_hbm_peak": round(moved / (ms * 1e-3) / HBM_PEAK, 4)}


def measure(torch, J, tk, label, buf, off, steps, warmup):
    stream = torch.cuda.current_stream().cuda_stream
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
    need = J.charspans_work_bytes(nb, nd)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    units = torch.empty(max(nd, 1), dtype=torch.int32, device="cuda")
    res["work_bytes"] = int(need)
    for mode in ("cut", "search", "full"):
        s, e, d, c, ntok, cap = spans_of(mode)
        row = {"mode": mode, "hmm": mode != "full", "spans": ntok, "span_capacity": cap}
        if mode == "cut":  # the join of the same run, on the same spans
            jneed = J.join_work_bytes(cap, nd)
            jwork = torch.empty(jneed, dtype=torch.uint8, device="cuda")
            jout = torch.empty(2 * nb + nd + 4096, dtype=torch.uint8, device="cuda")
            joff = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
            jn = torch.zeros(1, dtype=torch.int64, device="cuda")
            join = lambda: tk.join_device(d_text.data_ptr(), nb, s.data_ptr(), e.data_ptr(), d.data_ptr(),  # noqa: E731
                                          c.data_ptr(), cap, nd, b" ", b"\n", jout.data_ptr(), jout.numel(),
                                          joff.data_ptr(), jn.data_ptr(), jwork.data_ptr(), jneed, stream)
            res["join_device"] = timed(torch, join, steps, warmup)
            del jwork, jout, joff, jn
            torch.cuda.empty_cache()
        cs = torch.empty(cap, dtype=torch.int32, device="cuda")
        ce = torch.empty(cap, dtype=torch.int32, device="cuda")
        for unit in UNITS:
            fn = lambda: tk.charspans_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, s.data_ptr(),  # noqa: E731
                                             e.data_ptr(), d.data_ptr(), c.data_ptr(), cap, unit, cs.data_ptr(),
                                             ce.data_ptr(), units.data_ptr(), work.data_ptr(), need, stream)
            t = timed(torch, fn, steps, warmup)
            row["charspans_device_" + unit] = t
            row["charspans_" + unit + "_over_cut"] = round(t["median_ms"] / t_cut["median_ms"], 4)
            row["counted_" + unit] = counted(nb, min(ntok, cap), unit == "utf16", t["median_ms"])
            row["units_total_" + unit] = int(units[:nd].to(torch.int64).sum().item())
            tk.profile(True)
            tk.profile_reset()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            row["kernels_profile_ms_per_call_" + unit] = {k: round(v[0] / steps, 4) for k, v in tk.profile_read().items()
                                                          if k.startswith("k_cs_")}
            tk.profile(False)
        res.setdefault("modes", []).append(row)
        del s, e, d, cs, ce
        torch.cuda.empty_cache()
        print(f"charspans_bench.py: {label} {mode} measured", file=sys.stderr, flush=True)
    del d_text, d_off, work
    torch.cuda.empty_cache()
    return res


def numpy_charspans(buf, off, s, e, doc_tok):
    """Rune offsets per document of u32 byte spans over valid UTF-8, on the host: what a caller of
    jb_cut_batch_into32 does today."""
    nb = int(off[-1] - off[0])
    text = buf[int(off[0]):int(off[0]) + nb]
    before = np.zeros(nb + 1, np.uint32)
    np.cumsum((text & 0xC0) != 0x80, dtype=np.uint32, out=before[1:])  # (runes that start before each byte)
    base = np.repeat(before[(off[:-1] - off[0]).astype(np.int64)], np.diff(doc_tok.astype(np.int64)))
    return before[s] - base, before[e] - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", type=float, nargs="+", default=[1024.0, 128.0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nwords", type=int, default=350_000)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "charspans_bench.json"))
    args = ap.parse_args()

    import torch

    import jiebahip as J
    import synth

    if not torch.cuda.is_available():
        print("charspans_bench.py: no GPU (this measurement does not fall back)", file=sys.stderr)
        return 2
    sy = synth.Synth(nwords=args.nwords)
    tmp = tempfile.mkdtemp(prefix="jb_charspans_bench_")
    dpath, epath = sy.write_files(tmp)
    tk = J.Tokenizer(J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX, size_override=J.JIEBA_SIZE,
                                   device=0))
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "tile_bytes": J.JB_CHARSPANS_TILE, "hbm_peak_bytes_per_s": HBM_PEAK, "batches": []}
    threads = max(1, min(16, os.cpu_count() or 1))
    big = None
    for mib in args.sizes_mib:
        buf, off, _ = sy.corpus_parallel(synth.KIND_DOCS, 0, target_bytes=int(mib * (1 << 20)), threads=threads)
        if big is None:
            big = (buf, off, mib)
        out["batches"].append(measure(torch, J, tk, f"C_syn {mib:g} MiB", buf, off, args.steps, args.warmup))
    # host memory in, character spans out, beside the byte-span host call plus the conversion on the host
    buf, off, mib = big
    buf, off = np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(off, np.uint64)
    host = {"batch": f"C_syn {mib:g} MiB from pageable host memory", "bytes": int(off[-1]), "unit": "rune"}
    keep = {"o32": None, "ocs": None}

    def into32():
        r = tk.cut_batch_into32(buf, off, True, keep["o32"])
        keep["o32"] = r[3]
        return r

    def into32_numpy():
        s, e, d, _ = into32()
        return numpy_charspans(buf, off, s, e, d)

    def charspans():
        r = tk.cut_batch_charspans(buf, off, True, "cut", "rune", keep["ocs"])
        keep["ocs"] = r[4]
        return r

    last = {}
    for name, fn in (("cut_batch_into32_hmm1", into32), ("cut_batch_into32_hmm1_plus_numpy_conversion", into32_numpy),
                     ("cut_batch_charspans_hmm1", charspans)):
        ts = []
        for _ in range(args.host_steps + 1):
            t0 = time.perf_counter()
            last[name] = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[1:]  # (the first call grows buffers)
        host[name] = {"median_ms": round(float(np.median(ts)), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
    ncs, nce = last["cut_batch_into32_hmm1_plus_numpy_conversion"]
    cs, ce = last["cut_batch_charspans_hmm1"][:2]
    host["spans"] = int(len(cs))
    host["call_equals_numpy_conversion"] = bool(np.array_equal(cs, ncs) and np.array_equal(ce, nce))
    host["charspans_over_into32"] = round(host["cut_batch_charspans_hmm1"]["median_ms"] /
                                          host["cut_batch_into32_hmm1"]["median_ms"], 4)
    host["charspans_over_into32_plus_numpy"] = round(host["cut_batch_charspans_hmm1"]["median_ms"] /
                                                     host["cut_batch_into32_hmm1_plus_numpy_conversion"]["median_ms"], 4)
    out["host"] = host
    tk.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
