"""The near-duplicate rule of include/jiebahip.h once more, in plain Python: a dict from (band, key) to the bucket's
members, the window, the first common band, the agree count, the CSR by the later document, the three counters
and a union-find for the labels.  It shares no code with the C++.  A helper, not a test."""
import numpy as np

NOKEY = 0xFFFFFFFFFFFFFFFF


def neardup(key, sig, W, min_agree):
    """(pair_doc u32, pair_agree u32, pair_off u64[ndocs + 1], stat u64[3]) of keys uint64[ndocs, B] and signatures
    uint32[ndocs, K]."""
    key = np.asarray(key, np.uint64)
    sig = np.asarray(sig, np.uint32)
    nd, B = key.shape
    keys = key.tolist()
    buckets = {}
    for d in range(nd):  # documents ascending, so every member list is sorted
        for b in range(B):
            if keys[d][b] != NOKEY:
                buckets.setdefault((b, keys[d][b]), []).append(d)
    nentries = sum(len(m) for m in buckets.values())
    ncand = ntrunc = 0
    rows = [[] for _ in range(nd)]  # row j: (band, i, agree)
    for (b, _), members in buckets.items():
        for rank, j in enumerate(members):
            if rank > W:
                ntrunc += 1
            for i in members[max(0, rank - W):rank]:
                first = min(c for c in range(B) if keys[i][c] == keys[j][c] and keys[i][c] != NOKEY)
                if first != b:
                    continue
                ncand += 1
                agree = int((sig[i] == sig[j]).sum())
                if agree >= min_agree:
                    rows[j].append((b, i, agree))
    off, docs, agrees = [0], [], []
    for j in range(nd):
        for _, i, a in sorted(rows[j]):
            docs.append(i)
            agrees.append(a)
        off.append(len(docs))
    return (np.array(docs, np.uint32), np.array(agrees, np.uint32), np.array(off, np.uint64),
            np.array([nentries, ncand, ntrunc], np.uint64))


def labels(pair_off, pair_doc, ndocs, pcap=None):
    """label[d] = the least document of d's component; entries >= j of row j are skipped, offsets clamp to pcap."""
    pcap = len(pair_doc) if pcap is None else pcap
    parent = list(range(ndocs))

    def find(d):
        while parent[d] != d:
            d = parent[d]
        return d

    for j in range(ndocs):
        for k in range(min(int(pair_off[j]), pcap), min(int(pair_off[j + 1]), pcap)):
            i = int(pair_doc[k])
            if i >= j:
                continue
            a, c = find(i), find(j)
            if a != c:
                parent[max(a, c)] = min(a, c)
    return np.array([find(d) for d in range(ndocs)], np.uint32)
