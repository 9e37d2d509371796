#!/usr/bin/env python3
"""The cost of k_ids (jb_ids_device) on the benchmark's corpus.

bench.py's config 4 (the fixed C_syn corpus against the 350k-word D_syn dictionary, JB_DICT_PREFIX,
size 60,101,967) at 1 GiB and at 128 MiB; the vocabulary is the dictionary's words with freq > 0.
Per size: the plain jb_cut_device step and jb_ids_device over its spans, each timed with device
events on the launch stream (--steps after --warmup), then k_ids once more through jb_profile_read.
Writes one JSON document (--out) and prints it.

    python tools/ids_bench.py --out profiles/ids_bench.json
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("gen", os.path.join("jieba-go_amd", "python")):
    sys.path.insert(0, os.path.join(ROOT, sub))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", type=float, nargs="+", default=[1024.0, 128.0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nwords", type=int, default=350_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ids_bench.json"))
    args = ap.parse_args()

    import torch

    import jiebahip as J
    import synth

    if not torch.cuda.is_available():
        print("ids_bench.py: no GPU (this measurement does not fall back)", file=sys.stderr)
        return 2
    s = synth.Synth(nwords=args.nwords)
    tmp = tempfile.mkdtemp(prefix="jb_ids_bench_")
    dpath, epath = s.write_files(tmp)
    tk = J.Tokenizer(J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX,
                                   size_override=J.JIEBA_SIZE, device=0))
    with open(dpath, encoding="utf-8") as f:
        keys = [p[0].encode() for p in (ln.split(" ") for ln in f if ln.strip()) if int(p[1]) > 0]
    keys = list(dict.fromkeys(keys))
    v = J.Vocab(keys)
    info = v.info()
    v.close()
    tk.set_vocab(keys)
    klen = np.array([len(k) for k in keys])
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "vocabulary": {"keys": len(keys), "slots": info["nslots"], "table_bytes": info["nslots"] * 32,
                          "maxlen": info["maxlen"], "mean_key_bytes": round(float(klen.mean()), 2),
                          "keys_over_24_bytes": int((klen > 24).sum())},
           "sizes": []}
    stream = torch.cuda.current_stream().cuda_stream
    for mib in args.sizes_mib:
        buf, off, _ = s.corpus_parallel(synth.KIND_DOCS, 0, target_bytes=int(mib * (1 << 20)),
                                        threads=max(1, min(16, os.cpu_count() or 1)))
        nb, nd = int(off[-1]), len(off) - 1
        d_text = torch.from_numpy(np.asarray(buf[:nb + 64])).cuda()
        d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
        cut = lambda: tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)  # noqa: E731
        ps, pe, pd, pn = cut()
        torch.cuda.synchronize()
        tk.device_status(stream)
        ntok = int(J.dev_to_host(pn, 8, np.uint64)[0])
        d_ids = torch.empty(ntok, dtype=torch.int32, device="cuda")
        ids = lambda: tk.ids_device(d_text.data_ptr(), nb, ps, pe, pn, ntok, d_ids.data_ptr(), stream)  # noqa: E731
        t_cut = timed(torch, cut, args.steps, args.warmup)
        t_ids = timed(torch, ids, args.steps, args.warmup)
        found = float((d_ids != -1).float().mean().item())
        tk.profile(True)
        tk.profile_reset()
        for _ in range(args.steps):
            ids()
        torch.cuda.synchronize()
        pms, pn_ = tk.profile_read()["k_ids"]
        tk.profile(False)
        alg = nb + 12 * ntok  # text once, start + end + id per token (the table's gathers are extra)
        out["sizes"].append({
            "corpus_mib": mib, "bytes": nb, "docs": nd, "tokens": ntok, "mean_token_bytes": round(nb / ntok, 3),
            "found_share": round(found, 4), "cut_device_hmm1": t_cut, "ids_device": t_ids,
            "k_ids_profile_ms": round(pms / max(pn_, 1), 4), "k_ids_profile_launches": int(pn_),
            "ids_over_cut": round(t_ids["median_ms"] / t_cut["median_ms"], 4),
            "ids_tokens_per_s": round(ntok / (t_ids["median_ms"] * 1e-3), 1),
            "ids_chars_equiv_bytes_per_s": round(nb / (t_ids["median_ms"] * 1e-3), 1),
            "streamed_bytes": alg, "streamed_gb_per_s": round(alg / (t_ids["median_ms"] * 1e-3) / 1e9, 1),
            "slot_gathers_at_64B_bytes": 64 * ntok,
        })
        del d_text, d_off, d_ids
        torch.cuda.empty_cache()
    tk.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
