#!/usr/bin/env python3
"""The cost of jb_neardup_device and jb_neardup_sig: near-duplicate pairs from band keys and signatures.

Corpus run.  The corpus and dictionary of tools/minhash_bench.py (bench.py's config 4: C_syn against the 350k-word
D_syn dictionary), at 1 GiB, with a seeded tenth of the documents replaced, at the text level and before the cut,
by copies of other documents in which a seeded 0 to 5 % of the tokens are overwritten by other tokens of the same
document.  n = 5, K = 128, B = 32, R = 4, W = 64, min_agree = the integer nearest 0.8 K.  With device events on the
launch stream (--steps after --warmup), all in one process: the plain jb_cut_device step, jb_minhash_device,
jb_minhash_bands_device and jb_neardup_device, the last one's kernels once more through jb_profile_read; npairs, the
counters and the number of labels kept; the outputs compared byte for byte with jb_neardup, the host rule, over the
whole input; the path it replaces: keys and signatures copied to the host, then numpy's grouping (a stable argsort
and the run boundaries per band) and, as the fair host form of the whole join, jb_neardup (C++); and from pageable
host memory jb_neardup_sig beside jb_minhash_batch.
Synthetic run.  A seeded signature matrix of --synthetic-docs rows generated on the device (a tenth of the rows
are copies of other rows with each slot redrawn with a seeded probability of 0 to 10 %), the same K, B, R: the
size at which the sort dominates.  The same device times; the host rule on the first --synthetic-host-docs rows,
compared with the device's result on those rows.
Writes one JSON document (--out) and prints it.

    python tools/neardup_bench.py --out profiles/neardup_bench.json
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

N_SHINGLE, K, B, R, W = 5, 128, 32, 4, 64


def note(msg):
    print("neardup_bench.py: " + msg, file=sys.stderr, flush=True)


def plant_copies(tk, buf, off, seed):
    """A tenth of the documents become edited copies of other documents.  Returns (buf, off, number planted)."""
    rng = np.random.default_rng(seed)
    nd = len(off) - 1
    s, e, dt = tk.cut_batch(buf, off, True)
    s, e, dt = np.asarray(s, np.int64), np.asarray(e, np.int64), np.asarray(dt, np.int64)
    victims = rng.choice(nd, nd // 10, replace=False)
    is_victim = np.zeros(nd, bool)
    is_victim[victims] = True
    sources = rng.choice(np.flatnonzero(~is_victim), len(victims))
    new = {}
    for v, o in zip(victims.tolist(), sources.tolist()):
        t0, t1 = int(dt[o]), int(dt[o + 1])
        doc = bytearray(buf[int(off[o]):int(off[o + 1])].tobytes())
        nedit = int(rng.random() * 0.05 * (t1 - t0))
        base = int(off[o])
        pieces, at = [], 0
        for k in np.sort(rng.choice(t1 - t0, nedit, replace=False)).tolist() if nedit else []:
            a, b = int(s[t0 + k]) - base, int(e[t0 + k]) - base
            r = t0 + int(rng.integers(0, t1 - t0))
            pieces.append(bytes(doc[at:a]))
            pieces.append(bytes(doc[int(s[r]) - base:int(e[r]) - base]))
            at = b
        pieces.append(bytes(doc[at:]))
        new[v] = np.frombuffer(b"".join(pieces), np.uint8)
    parts, lens = [], np.zeros(nd, np.int64)
    for d in range(nd):
        p = new[d] if d in new else buf[int(off[d]):int(off[d + 1])]
        parts.append(p)
        lens[d] = len(p)
    out_off = np.zeros(nd + 1, np.uint64)
    out_off[1:] = np.cumsum(lens)
    parts.append(np.zeros(64, np.uint8))
    return np.concatenate(parts), out_off, len(victims)


def run_neardup(torch, J, tk, d_key, d_sig, nd, m, steps, warmup):
    """jb_neardup_device on device arrays: (timing, kernel profile, outputs on the device, npairs, stat)."""
    stream = torch.cuda.current_stream().cuda_stream
    need = J.neardup_work_bytes(nd, B)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    p_off = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
    p_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    p_st = torch.zeros(J.JB_ND_NSTAT, dtype=torch.int64, device="cuda")
    pcap = max(1024, nd)
    for _ in range(2):  # (the second time with the count the first reports, when that is larger)
        p_doc = torch.empty(pcap, dtype=torch.int32, device="cuda")
        p_agree = torch.empty(pcap, dtype=torch.int32, device="cuda")
        fn = lambda: tk.neardup_device(d_key.data_ptr(), d_sig.data_ptr(), nd, B, K, W, m, p_doc.data_ptr(),  # noqa: E731
                                       p_agree.data_ptr(), pcap, p_off.data_ptr(), p_n.data_ptr(), p_st.data_ptr(),
                                       work.data_ptr(), need, stream)
        fn()
        torch.cuda.synchronize()
        npairs = int(p_n.cpu()[0])
        if npairs <= pcap:
            break
        pcap = npairs
    t = timed(torch, fn, steps, warmup)
    tk.profile(True)
    tk.profile_reset()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    prof = {k: round(v[0] / steps, 4) for k, v in tk.profile_read().items() if k.startswith("k_nd_")}
    tk.profile(False)
    stat = p_st.cpu().numpy().view(np.uint64)
    res = {"neardup_device": t, "kernels_profile_ms_per_call": prof, "entries": nd * B, "work_bytes": int(need),
           "launches": 32, "npairs": npairs, "nentries": int(stat[0]), "ncand": int(stat[1]), "ntrunc": int(stat[2]),
           "entries_per_us": round(nd * B / (t["median_ms"] * 1e3), 1)}
    return res, (p_doc, p_agree, p_off)


def to_host(p_doc, p_agree, p_off, npairs):
    return (p_doc[:npairs].cpu().numpy().view(np.uint32), p_agree[:npairs].cpu().numpy().view(np.uint32),
            p_off.cpu().numpy().view(np.uint64))


def corpus_run(torch, J, tk, buf, off, label, m, steps, warmup, host_steps):
    stream = torch.cuda.current_stream().cuda_stream
    nb, nd = int(off[-1]), len(off) - 1
    d_text = torch.from_numpy(np.ascontiguousarray(buf[:nb])).cuda()
    d_text = torch.cat([d_text, torch.zeros(64, dtype=torch.uint8, device="cuda")])
    d_off = torch.from_numpy(np.asarray(off, np.uint64).view(np.int64)).cuda()
    cut = lambda: tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)  # noqa: E731
    ps, pe, pd, pn = cut()
    torch.cuda.synchronize()
    tk.device_status(stream)
    ntok = int(J.dev_to_host(pn, 8, np.uint64)[0])
    d_sig = torch.empty(nd * K, dtype=torch.int32, device="cuda")
    d_dn = torch.empty(nd, dtype=torch.int32, device="cuda")
    d_key = torch.empty(nd * B, dtype=torch.int64, device="cuda")
    mneed = J.minhash_work_bytes(ntok, nd)
    mwork = torch.empty(mneed, dtype=torch.uint8, device="cuda")
    mh = lambda: tk.minhash_device(d_text.data_ptr(), nb, ps, pe, pd, pn, ntok, nd, N_SHINGLE, K, 1, d_sig.data_ptr(),  # noqa: E731
                                   d_dn.data_ptr(), mwork.data_ptr(), mneed, stream)
    bands = lambda: tk.minhash_bands_device(d_sig.data_ptr(), d_dn.data_ptr(), nd, K, B, R, d_key.data_ptr(), stream)  # noqa: E731
    res = {"batch": label, "bytes": nb, "docs": nd, "tokens": ntok, "n": N_SHINGLE, "K": K, "B": B, "R": R, "W": W,
           "min_agree": m}
    res["cut_device_hmm1"] = timed(torch, cut, steps, warmup)
    res["minhash_device"] = timed(torch, mh, steps, warmup)
    res["minhash_bands_device"] = timed(torch, bands, steps, warmup)
    del mwork
    r, outs = run_neardup(torch, J, tk, d_key, d_sig, nd, m, steps, warmup)
    res.update(r)
    res["neardup_over_cut"] = round(r["neardup_device"]["median_ms"] / res["cut_device_hmm1"]["median_ms"], 4)
    note(f"{label}: device steps measured")
    # the path it replaces: keys and signatures to the host, the join there
    t0 = time.perf_counter()
    h_key = d_key.cpu().numpy().view(np.uint64).reshape(nd, B)
    h_sig = d_sig.cpu().numpy().view(np.uint32).reshape(nd, K)
    t1 = time.perf_counter()
    nruns = 0
    for b in range(B):
        col = h_key[:, b]
        order = np.argsort(col, kind="stable")
        sk = col[order]
        nruns += int((sk[1:] == sk[:-1]).sum())
    t2 = time.perf_counter()
    w_doc, w_agree, w_off, w_n, w_st = J.neardup(h_key, h_sig, W, m)
    t3 = time.perf_counter()
    res["host_path"] = {"copy_keys_and_signatures_ms": round((t1 - t0) * 1e3, 1),
                        "numpy_grouping_only_ms": round((t2 - t1) * 1e3, 1), "numpy_adjacent_equal_keys": nruns,
                        "host_rule_jb_neardup_ms": round((t3 - t2) * 1e3, 1),
                        "copy_plus_host_rule_ms": round((t1 - t0 + t3 - t2) * 1e3, 1)}
    res["host_path_over_neardup_device"] = round((t1 - t0 + t3 - t2) * 1e3 / r["neardup_device"]["median_ms"], 1)
    g_doc, g_agree, g_off = to_host(*outs, r["npairs"])
    res["device_outputs_are_the_host_rule's"] = bool(
        w_n == r["npairs"] and g_doc.tobytes() == w_doc.tobytes() and g_agree.tobytes() == w_agree.tobytes() and
        g_off.tobytes() == w_off.tobytes() and [int(x) for x in w_st] == [r["nentries"], r["ncand"], r["ntrunc"]])
    label_ = J.neardup_labels(g_off, g_doc)
    res["labels_kept"] = int((label_ == np.arange(nd, dtype=np.uint32)).sum())
    res["documents_dropped"] = nd - res["labels_kept"]
    note(f"{label}: host paths measured")
    # from pageable host memory
    h_dn = d_dn.cpu().numpy().view(np.uint32)
    host = {}
    for name, fn in (("minhash_batch_hmm1", lambda: tk.minhash_batch(buf, off, True, N_SHINGLE, K, 1)),
                     ("neardup_sig", lambda: tk.near_duplicates(h_sig, h_dn, B, R, W, m, pcap=max(r["npairs"], 1)))):
        ts = []
        for _ in range(host_steps + 1):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        if name == "neardup_sig":
            host["neardup_sig_is_the_device_call's"] = bool(out[1].tobytes() == g_doc.tobytes() and
                                                            out[0].tobytes() == g_off.tobytes())
        del out
        ts = ts[1:]  # (the first call grows buffers)
        host[name] = {"median_ms": round(float(np.median(ts)), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
        note(name + " measured")
    res["host"] = host
    return res


def synthetic_run(torch, J, tk, nd, host_docs, m, steps, warmup, seed):
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    sig = (torch.randint(0, 1 << 32, (nd, K), dtype=torch.int64, device="cuda", generator=g) - (1 << 31)).to(torch.int32)
    ncopy = nd // 10
    dst = torch.randperm(nd, device="cuda", generator=g)[:ncopy]
    src = torch.randint(0, nd, (ncopy,), device="cuda", generator=g)
    p = torch.rand((ncopy, 1), device="cuda", generator=g) * 0.1
    keep = torch.rand((ncopy, K), device="cuda", generator=g) >= p
    sig[dst] = torch.where(keep, sig[src], sig[dst])  # (a chain of copies reads the rows as they were)
    del keep
    d_sig = sig.reshape(-1)
    d_dn = torch.ones(nd, dtype=torch.int32, device="cuda")
    d_key = torch.empty(nd * B, dtype=torch.int64, device="cuda")
    bands = lambda: tk.minhash_bands_device(d_sig.data_ptr(), d_dn.data_ptr(), nd, K, B, R, d_key.data_ptr(), stream)  # noqa: E731
    res = {"batch": f"synthetic signatures, {nd} rows", "docs": nd, "planted_copies": ncopy, "K": K, "B": B, "R": R, "W": W,
           "min_agree": m, "minhash_bands_device": timed(torch, bands, steps, warmup)}
    r, outs = run_neardup(torch, J, tk, d_key, d_sig, nd, m, steps, warmup)
    res.update(r)
    sort_ms = sum(v for k, v in r["kernels_profile_ms_per_call"].items() if k in ("k_nd_hist", "k_nd_scan", "k_nd_scatter"))
    res["sort_share_of_kernel_time"] = round(sort_ms / max(sum(r["kernels_profile_ms_per_call"].values()), 1e-9), 3)
    # 9 passes: keys and entries read twice (histogram, scatter) and written once
    res["sort_moved_gb_per_s"] = round(9 * 36 * nd * B / max(sort_ms * 1e-3, 1e-12) / 1e9, 1)
    note("synthetic: device steps measured")
    # the host rule on the first rows, against the device on the same rows
    hd = min(host_docs, nd)
    sub, sub_outs = run_neardup(torch, J, tk, d_key[:hd * B], d_sig[:hd * K], hd, m, 1, 0)
    t0 = time.perf_counter()
    h_key = d_key[:hd * B].cpu().numpy().view(np.uint64).reshape(hd, B)
    h_sig = d_sig[:hd * K].cpu().numpy().view(np.uint32).reshape(hd, K)
    t1 = time.perf_counter()
    w_doc, w_agree, w_off, w_n, w_st = J.neardup(h_key, h_sig, W, m)
    t2 = time.perf_counter()
    g_doc, g_agree, g_off = to_host(*sub_outs, sub["npairs"])
    res["host_fraction"] = {"docs": hd, "share_of_rows": round(hd / nd, 4), "copy_ms": round((t1 - t0) * 1e3, 1),
                            "host_rule_jb_neardup_ms": round((t2 - t1) * 1e3, 1), "npairs": int(w_n),
                            "neardup_device_ms_same_rows": sub["neardup_device"]["median_ms"],
                            "device_outputs_are_the_host_rule's": bool(
                                w_n == sub["npairs"] and g_doc.tobytes() == w_doc.tobytes() and
                                g_agree.tobytes() == w_agree.tobytes() and g_off.tobytes() == w_off.tobytes() and
                                [int(x) for x in w_st] == [sub["nentries"], sub["ncand"], sub["ntrunc"]])}
    note("synthetic: host fraction measured")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mib", type=float, default=1024.0)
    ap.add_argument("--synthetic-docs", type=int, default=4_000_000)
    ap.add_argument("--synthetic-host-docs", type=int, default=250_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nwords", type=int, default=350_000)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neardup_bench.json"))
    args = ap.parse_args()

    import torch

    import jiebahip as J
    import synth

    if not torch.cuda.is_available():
        print("neardup_bench.py: no GPU (this measurement does not fall back)", file=sys.stderr)
        return 2
    s = synth.Synth(nwords=args.nwords)
    tmp = tempfile.mkdtemp(prefix="jb_neardup_bench_")
    dpath, epath = s.write_files(tmp)
    tk = J.Tokenizer(J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX, size_override=J.JIEBA_SIZE,
                                   device=0))
    m = J._default_agree(K)
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "tile_entries": J.JB_ND_TILE, "form": "one form (no JB_ND_FORM)"}
    threads = max(1, min(16, os.cpu_count() or 1))
    note(f"generating {args.size_mib:g} MiB")
    buf, off, _ = s.corpus_parallel(synth.KIND_DOCS, 0, target_bytes=int(args.size_mib * (1 << 20)), threads=threads)
    buf, off, nplanted = plant_copies(tk, buf, off, 20261021)
    note(f"{nplanted} copies planted")
    out["corpus"] = corpus_run(torch, J, tk, buf, off, f"C_syn {args.size_mib:g} MiB, a tenth planted copies", m, args.steps,
                               args.warmup, args.host_steps)
    out["corpus"]["planted_copies"] = nplanted
    del buf, off
    torch.cuda.empty_cache()
    out["synthetic"] = synthetic_run(torch, J, tk, args.synthetic_docs, args.synthetic_host_docs, m, args.steps, args.warmup,
                                     20261021)
    tk.close()
    text = json.dumps(out, indent=1, ensure_ascii=False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
