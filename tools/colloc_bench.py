#!/usr/bin/env python3
"""The cost of jb_colloc_add_device and jb_colloc_score_device on the benchmark's corpus.

Corpus and dictionary as tools/wc_bench.py (bench.py's config 4: C_syn against the 350k-word D_syn dictionary,
JB_DICT_PREFIX, size 60,101,967), at 1 GiB, plain-mode ids under the vocabulary the word counts give (fit_vocab's
steps on the device).  With device events on the launch stream (--steps after --warmup), all in one process:
  - the plain jb_cut_device step, jb_wc_add_device and jb_ids_device, for scale;
  - jb_colloc_add_device in both forms of the count pass (JB_COLLOC_COMBINE 0 and 1: one tokenizer and one table per
    form, the two alternating from step to step), into a table that already holds the batch's pairs (the steady
    state of a corpus read more than once) and, with jb_colloc_init_device in front, into an empty one (every pair
    is claimed); with and without JB_COLLOC_CONTIG; the kernels once more through jb_profile_read;
  - the table's size: nslots grows by four until nothing is dropped, and the distinct pairs and the load are
    recorded;
  - jb_colloc_score_device (NPMI, min_count 5, threshold 0.5) and jb_colloc_read by the host's clock;
  - that the two forms' tables hold the same pairs, counts, unigrams and totals over the whole corpus, that the
    unigrams are numpy's bincount of the ids, and, over the first --check-mib MiB of documents, that both forms
    equal jb_colloc_count, the host rule;
  - the path this replaces: the ids copied to the host and np.unique over the u64 keys of adjacent ids, timed on
    the same first --check-mib MiB and compared with the host rule's pairs.
Writes one JSON document (--out) and prints it.

    python tools/colloc_bench.py --out profiles/colloc_bench.json
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

NAMES = ("atomic", "combine")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mib", type=float, default=1024.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nwords", type=int, default=350_000)
    ap.add_argument("--check-mib", type=float, default=64.0)
    ap.add_argument("--nslots", type=int, default=1 << 26)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colloc_bench.json"))
    args = ap.parse_args()

    import torch

    import jiebahip as J
    import synth

    if not torch.cuda.is_available():
        print("colloc_bench.py: no GPU (this measurement does not fall back)", file=sys.stderr)
        return 2
    s = synth.Synth(nwords=args.nwords)
    tmp = tempfile.mkdtemp(prefix="jb_colloc_bench_")
    dpath, epath = s.write_files(tmp)
    forms = {}
    old = os.environ.get("JB_COLLOC_COMBINE")
    for name, val in (("atomic", "0"), ("combine", "1")):  # (the knob is read at jb_open)
        os.environ["JB_COLLOC_COMBINE"] = val
        forms[name] = J.Tokenizer(J.make_config(dict_path=dpath, emit_path=epath, kind=J.JB_DICT_PREFIX,
                                                size_override=J.JIEBA_SIZE, device=0))
    if old is None:
        del os.environ["JB_COLLOC_COMBINE"]
    else:
        os.environ["JB_COLLOC_COMBINE"] = old
    tk = forms["combine"]
    steps, warmup = args.steps, args.warmup
    stream = torch.cuda.current_stream().cuda_stream
    print(f"colloc_bench.py: generating {args.size_mib:g} MiB", file=sys.stderr, flush=True)
    buf, off, _ = s.corpus_parallel(synth.KIND_DOCS, 0, target_bytes=int(args.size_mib * (1 << 20)),
                                    threads=max(1, min(16, os.cpu_count() or 1)))
    nb, nd = int(off[-1]), len(off) - 1
    out = {"device": torch.cuda.get_device_name(0), "steps": steps, "warmup": warmup,
           "batch": f"C_syn {args.size_mib:g} MiB", "bytes": nb, "docs": nd,
           "forms": {"atomic": "JB_COLLOC_COMBINE=0: one global u64 atomic per pair and per unigram",
                     "combine": "JB_COLLOC_COMBINE=1: a workgroup's adds combined in two LDS tables first"}}
    d_text = torch.from_numpy(np.ascontiguousarray(buf[:nb])).cuda()
    d_text = torch.cat([d_text, torch.zeros(64, dtype=torch.uint8, device="cuda")])
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    cut = lambda: tk.cut_device(d_text.data_ptr(), nb, d_off.data_ptr(), nd, True, stream)  # noqa: E731
    out["cut_device_hmm1"] = t_cut = timed(torch, cut, steps, warmup)
    p = cut()
    torch.cuda.synchronize()
    ntok = int(J.dev_to_host(p[3], 8, np.uint64)[0])
    d_s = torch.from_numpy(J.dev_to_host(p[0], 4 * ntok, np.int32)).cuda()
    d_e = torch.from_numpy(J.dev_to_host(p[1], 4 * ntok, np.int32)).cuda()
    doc_tok = J.dev_to_host(p[2], 8 * (nd + 1), np.uint64).copy()
    d_dt = torch.from_numpy(doc_tok.view(np.int64)).cuda()
    d_n = torch.tensor([ntok], dtype=torch.int64, device="cuda")
    out["tokens"] = ntok
    # the vocabulary: the word counts on the device, their keys by count (fit_vocab's steps)
    wslots, pool = 1 << 22, 64 << 20
    nwt = J.wc_table_bytes(wslots, pool)
    wt = torch.empty(nwt, dtype=torch.uint8, device="cuda")
    ww = torch.empty(J.wc_work_bytes(ntok), dtype=torch.uint8, device="cuda")
    tk.wc_init_device(wt.data_ptr(), nwt, wslots, pool, stream)
    wadd = lambda: tk.wc_add_device(wt.data_ptr(), nwt, d_text.data_ptr(), nb, d_s.data_ptr(), d_e.data_ptr(),  # noqa: E731
                                    d_n.data_ptr(), ntok, ww.data_ptr(), ww.numel(), stream)
    wadd()
    wc = tk.wc_read(wt.data_ptr(), nwt, 1, 0, stream)
    assert wc.dropped == 0 and wc.collided == 0
    out["wc_add_device"] = timed(torch, wadd, steps, warmup)
    nuni = len(wc.keys)
    out["vocabulary_keys"] = nuni
    for t in forms.values():
        t.set_vocab(wc.keys)
    del wt, ww
    d_ids = torch.empty(ntok, dtype=torch.int32, device="cuda")
    idf = lambda: tk.ids_device(d_text.data_ptr(), nb, d_s.data_ptr(), d_e.data_ptr(), d_n.data_ptr(), ntok,  # noqa: E731
                                d_ids.data_ptr(), stream)
    out["ids_device"] = timed(torch, idf, steps, warmup)
    need = J.colloc_work_bytes(ntok, nd)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    out["work_bytes"] = int(need)
    uni = {n: torch.empty(nuni, dtype=torch.int64, device="cuda") for n in NAMES}

    def adder(n, tab, ntable, flags, cap=ntok, ndocs=nd):
        return lambda: forms[n].colloc_add_device(tab.data_ptr(), ntable, uni[n].data_ptr(), nuni, d_ids.data_ptr(), cap,
                                                  d_dt.data_ptr(), d_n.data_ptr(), ndocs, 0, 0, flags, d_s.data_ptr(),
                                                  d_e.data_ptr(), work.data_ptr(), need, stream)

    # the table: four times larger until nothing is dropped
    nslots, tried = args.nslots, []
    while True:
        ntable = J.colloc_table_bytes(nslots)
        tables = {n: torch.empty(ntable, dtype=torch.uint8, device="cuda") for n in NAMES}
        init = {n: (lambda n=n: forms[n].colloc_init_device(tables[n].data_ptr(), ntable, nslots, uni[n].data_ptr(), nuni,
                                                            stream)) for n in NAMES}
        init["combine"]()
        adder("combine", tables["combine"], ntable, 0)()
        r = tk.colloc_read(tables["combine"].data_ptr(), ntable, uni["combine"].data_ptr(), nuni, "count", 1 << 40,
                           0.0, 0, stream)  # (no candidate: the totals alone)
        tried.append({"nslots": nslots, "table_bytes": int(ntable), "dropped": r.dropped, "distinct": r.distinct})
        if r.dropped == 0:
            break
        del tables
        torch.cuda.empty_cache()
        nslots *= 4
    out["table_sizes_tried"] = tried
    out["nslots"], out["table_bytes"] = nslots, int(ntable)
    out["totals"] = dict(zip(("tokens", "known", "pairs", "dropped", "distinct"), r.totals()))
    out["load"] = round(r.distinct / nslots, 4)
    out["colloc_init_device"] = timed(torch, init["combine"], steps, warmup)
    for flags, tag in ((0, "all_pairs"), (J.JB_COLLOC_CONTIG, "contiguous")):
        add = {n: adder(n, tables[n], ntable, flags) for n in NAMES}

        def fresh(n):
            init[n]()
            add[n]()
        row = {}
        t_first = timed_ab(torch, {n: (lambda n=n: fresh(n)) for n in NAMES}, max(3, steps // 2), 1)
        for n in NAMES:
            fresh(n)
        got = {n: forms[n].colloc_read(tables[n].data_ptr(), ntable, uni[n].data_ptr(), nuni, "count", 1,
                                       float("-inf"), 0, stream) for n in NAMES}
        a, b = got["atomic"], got["combine"]
        row["distinct_pairs"] = len(b)
        row["totals"] = dict(zip(("tokens", "known", "pairs", "dropped", "distinct"), b.totals()))
        row["counts_plus_dropped_is_pairs"] = bool(int(b.count.sum()) + b.dropped == b.pairs)
        row["forms_give_identical_results"] = bool(
            np.array_equal(a.a, b.a) and np.array_equal(a.b, b.b) and np.array_equal(a.count, b.count) and
            a.totals() == b.totals() and torch.equal(uni["atomic"], uni["combine"]))
        if flags == 0:
            ids_h = d_ids.cpu().numpy().view(np.uint32)
            row["uni_is_numpy_bincount_of_the_ids"] = bool(
                np.array_equal(uni["combine"].cpu().numpy(), np.bincount(ids_h[ids_h < nuni], minlength=nuni)))
            keys = tk._vocab_keys
            row["top_pairs"] = [[keys[int(x)].decode("utf-8", "replace"), keys[int(y)].decode("utf-8", "replace"), int(c)]
                                for x, y, c in zip(b.a[:5], b.b[:5], b.count[:5])]
        del got, a, b
        t_warm = timed_ab(torch, add, steps, warmup)
        for n in NAMES:
            row["colloc_add_device_" + n] = t_warm[n]
            row["colloc_add_" + n + "_over_cut"] = round(t_warm[n]["median_ms"] / t_cut["median_ms"], 4)
            row["colloc_init_and_first_add_" + n] = t_first[n]
        row["faster_form"] = min(NAMES, key=lambda n: t_warm[n]["median_ms"])
        row["faster_form_first_add"] = min(NAMES, key=lambda n: t_first[n]["median_ms"])
        prof = {}
        for n in NAMES:
            forms[n].profile(True)
            forms[n].profile_reset()
            for _ in range(steps):
                add[n]()
            torch.cuda.synchronize()
            prof[n] = {k: round(v[0] / steps, 4) for k, v in forms[n].profile_read().items() if k.startswith("k_cl_")}
            forms[n].profile(False)
        row["kernels_profile_ms_per_call"] = prof
        out[tag] = row
        print(f"colloc_bench.py: {tag} measured", file=sys.stderr, flush=True)
    # the score pass over the table of all pairs, and the read
    for n in NAMES:
        init[n]()
        adder(n, tables[n], ntable, 0)()
    ncand = torch.zeros(1, dtype=torch.int64, device="cuda")
    tk.colloc_score_device(tables["combine"].data_ptr(), ntable, uni["combine"].data_ptr(), nuni, "npmi", 5, 0.5, 0, 0, 0, 0,
                           0, ncand.data_ptr(), stream)
    torch.cuda.synchronize()
    nc = int(ncand.item())
    cand = torch.empty(max(nc, 1) * 20, dtype=torch.uint8, device="cuda")
    pc = cand.data_ptr()
    score = lambda: tk.colloc_score_device(tables["combine"].data_ptr(), ntable, uni["combine"].data_ptr(), nuni,  # noqa: E731
                                           "npmi", 5, 0.5, pc + 8 * nc, pc + 12 * nc, pc, pc + 16 * nc, nc,
                                           ncand.data_ptr(), stream)
    out["score"] = {"scorer": "npmi", "min_count": 5, "threshold": 0.5, "candidates": nc,
                    "colloc_score_device": timed(torch, score, steps, warmup)}
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = tk.colloc_read(tables["combine"].data_ptr(), ntable, uni["combine"].data_ptr(), nuni, "npmi", 5, 0.5, 0, stream)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["score"]["colloc_read_ms"] = round(float(np.median(ts)), 2)
    out["score"]["candidates_read"] = len(r)
    del cand, tables
    torch.cuda.empty_cache()
    # a part of the corpus against the host rule, and the path this replaces on the same part
    ndp = max(1, int(np.searchsorted(off, int(args.check_mib * (1 << 20)), side="right")) - 1)
    cap = int(doc_tok[ndp])
    part = {"docs": ndp, "bytes": int(off[ndp]), "tokens": cap}
    t0 = time.perf_counter()
    ids_h = d_ids.cpu().numpy().view(np.uint32)
    out["ids_copy_to_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    hu = np.zeros(nuni, np.uint64)
    t0 = time.perf_counter()
    want = J.colloc_count(ids_h[:cap], doc_tok[:ndp + 1], hu)
    part["host_rule_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    pslots = 1 << 26
    pt = J.colloc_table_bytes(pslots)
    tab = torch.empty(pt, dtype=torch.uint8, device="cuda")
    same = {}
    d_np = torch.tensor([cap], dtype=torch.int64, device="cuda")
    for n in NAMES:
        forms[n].colloc_init_device(tab.data_ptr(), pt, pslots, uni[n].data_ptr(), nuni, stream)
        forms[n].colloc_add_device(tab.data_ptr(), pt, uni[n].data_ptr(), nuni, d_ids.data_ptr(), cap, d_dt.data_ptr(),
                                   d_np.data_ptr(), ndp, 0, 0, 0, 0, 0, work.data_ptr(), need, stream)
        g = forms[n].colloc_read(tab.data_ptr(), pt, uni[n].data_ptr(), nuni, "count", 1, float("-inf"), 0, stream)
        order = np.lexsort((g.b, g.a))  # (the host rule's dump is sorted by key)
        same[n] = bool(np.array_equal(g.a[order], want.a) and np.array_equal(g.b[order], want.b) and
                       np.array_equal(g.count[order], want.count) and g.totals() == want.totals() and
                       np.array_equal(uni[n].cpu().numpy().view(np.uint64), hu))
    part["device_equals_host_rule"] = same
    part["distinct_pairs"] = len(want)
    # np.unique over the u64 keys of adjacent ids, document ends and unknown ids masked out
    t0 = time.perf_counter()
    a64 = ids_h[:cap - 1].astype(np.uint64)
    b64 = ids_h[1:cap].astype(np.uint64)
    ok = (a64 < nuni) & (b64 < nuni)
    ends = doc_tok[1:ndp + 1].astype(np.int64) - 1
    ok[ends[(ends >= 0) & (ends < cap - 1)]] = False
    ku, kc = np.unique((a64[ok] << np.uint64(32)) | b64[ok], return_counts=True)
    part["numpy_unique_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    part["numpy_unique_ms_per_million_tokens"] = round(part["numpy_unique_ms"] / (cap / 1e6), 2)
    part["numpy_equals_host_rule"] = bool(
        np.array_equal(ku, (want.a.astype(np.uint64) << np.uint64(32)) | want.b.astype(np.uint64)) and
        np.array_equal(kc.astype(np.uint64), want.count))
    out["first_part"] = part
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
