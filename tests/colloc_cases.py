"""Seeded inputs for the collocation tests (tests/test_colloc_host.py on the CPU, tests/test_gpu_colloc.py on the
GPU), built from T = JB_COLLOC_TILE: the smallest shapes at which the kernels can go wrong.

An add case is a dict: label, batches (a list of batch dicts: ids, doc_tok, and optionally ntok, ids_cap, starts,
ends), nuni, keep (or None), flags, nslots (the device table's and, with `drops`, the host rule's).  A score case
is a dict: label, a, b, count, uni, nuni, N, m, and the thresholds to try."""
import numpy as np

TILE = 256
LDS = 2048
SHARE = 64
UNK = 0xFFFFFFFF
CONTIG = 1
T = TILE


def _pow2(n):
    p = 8
    while p < n:
        p *= 2
    return p


def _case(label, batches, nuni, keep=None, flags=0, nslots=None, drops=False):
    if isinstance(batches, dict):
        batches = [batches]
    for b in batches:
        b["ids"] = np.asarray(b["ids"], np.uint32)
        b["doc_tok"] = np.asarray(b["doc_tok"], np.uint64)
        b.setdefault("ids_cap", len(b["ids"]))
        b.setdefault("ntok", b["ids_cap"])
        for k in ("starts", "ends"):
            b[k] = None if b.get(k) is None else np.asarray(b[k], np.uint32)
    total = sum(len(b["ids"]) for b in batches)
    return dict(label=label, batches=batches, nuni=nuni, keep=None if keep is None else np.asarray(keep, np.uint8),
                flags=flags, nslots=nslots or _pow2(4 * max(total, 1)), drops=drops)


def _edges(ntok):
    """Document boundaries at T - 1, T and T + 1, each followed by a run of three empty documents."""
    dt = [0]
    for p in (T - 1, T, T + 1):
        dt += [min(p, ntok)] * 4
    return dt + [ntok]


def all_cases():
    rng = np.random.default_rng(20261021)
    for nd in (0, 1, 3):
        yield _case(f"ntok=0 ndocs={nd}", dict(ids=[], doc_tok=[0] * (nd + 1)), 5)
    yield _case("ntok=0 of a longer list", dict(ids=[1, 2, 1, 2], doc_tok=[0, 0, 0], ntok=0), 5)
    yield _case("documents of 1 and 2 tokens", dict(ids=[0, 1, 2, 0, 1, 2], doc_tok=[0, 1, 3, 4, 6]), 3)
    for ntok in (T, T + 1, 3 * T + 5):
        yield _case(f"edges ntok={ntok}", dict(ids=rng.integers(0, 6, ntok), doc_tok=_edges(ntok)), 6)
    yield _case("tokens of no document", dict(ids=rng.integers(0, 4, T + 40), doc_tok=[7, 30, 30, T + 3, T + 21]), 4)
    ids = rng.integers(0, 5, 2 * T + 9)
    yield _case("ntok above ids_cap", dict(ids=ids, doc_tok=[0, 100, T + 1, 2 * T + 200], ntok=2 * T + 109), 5)
    yield _case("ids_cap below the list", dict(ids=ids, doc_tok=[0, 100, T + 1, 2 * T + 9], ids_cap=T + 3, ntok=2 * T), 5)
    ids = rng.integers(0, 8, T + 77).astype(np.uint32)
    ids[rng.random(len(ids)) < 0.1] = UNK
    ids[rng.random(len(ids)) < 0.1] = 8
    ids[rng.random(len(ids)) < 0.05] = 0x80000001
    yield _case("unknown and out-of-range ids", dict(ids=ids, doc_tok=[0, 50, T, T + 77]), 8)
    yield _case("nuni=0", dict(ids=ids, doc_tok=[0, 50, T, T + 77]), 0)
    ids = rng.integers(0, 10, T + 50)
    yield _case("nkeep below nuni", dict(ids=ids, doc_tok=[0, T - 1, T + 50]), 10, keep=[1, 0, 1, 1, 0, 1, 1])
    # spans: token k is [s, e); a gap of dropped whitespace after some, an overlap (search mode) after others
    n = T + 30
    ids = rng.integers(0, 5, n)
    lens = rng.integers(1, 4, n)
    step = lens + (rng.random(n) < 0.25) * 1 - (rng.random(n) < 0.15) * 1
    starts = np.concatenate([[0], np.cumsum(np.maximum(step, 0))[:-1]])
    spans = dict(ids=ids, doc_tok=[0, T - 1, T, n], starts=starts, ends=starts + lens)
    yield _case("contiguous over gaps and overlaps", dict(spans), 5, flags=CONTIG)
    yield _case("the same spans without the flag", dict(spans), 5)
    yield _case("null spans without the flag", dict(ids=ids, doc_tok=[0, T - 1, T, n]), 5)
    yield _case("one hot pair", dict(ids=np.full(4 * T, 2), doc_tok=[0, 4 * T]), 3)
    # one workgroup's share (SHARE tiles) holds more distinct pairs and ids than four times the LDS tables' entries
    n = SHARE * T + T + 3
    ids = rng.integers(0, 20000, n)
    assert len(set(ids[:SHARE * T].tolist())) > 4 * LDS
    assert len(set(zip(ids[:SHARE * T - 1].tolist(), ids[1:SHARE * T].tolist()))) > 4 * LDS
    yield _case("eviction", dict(ids=ids, doc_tok=[0, 9, n]), 20000)
    ids = rng.integers(0, 7, 3 * T)
    assert len(set(zip(ids[:-1].tolist(), ids[1:].tolist()))) >= 40
    yield _case("nslots=8", dict(ids=ids, doc_tok=[0, 3 * T]), 7, nslots=8, drops=True)
    yield _case("two batches", [dict(ids=rng.integers(0, 6, T + 9), doc_tok=[0, 40, T + 9]),
                                dict(ids=rng.integers(0, 6, 2 * T + 1), doc_tok=[3, T, T, 2 * T])], 6)
    n = 3 * T + 5
    z = np.minimum(rng.zipf(1.3, n) - 1, 299)
    cuts = np.sort(rng.integers(0, n + 1, 49))
    yield _case("zipf", dict(ids=z, doc_tok=np.concatenate([[0], cuts, [n]])), 300)


def score_cases():
    m = 3
    uni = np.array([10, 20, 0, 7, 1 << 53, 40, 40, 5], np.uint64)
    # (a, b, count)
    rows = [(0, 1, m - 1), (0, 1, m), (1, 0, 9), (0, 2, 5), (2, 0, 5), (3, 7, 4), (7, 3, 4), (5, 6, 8), (6, 5, 8),
            (5, 5, 8), (0, 4, 5), (1, 3, 1 << 53), (0, 3, 1000), (3, 3, 6), (0, 0, 999)]
    a, b, c = (np.array(x) for x in zip(*rows))
    yield dict(label="hand-made", a=a.astype(np.uint32), b=b.astype(np.uint32), count=c.astype(np.uint64), uni=uni,
               nuni=8, N=1000, m=m)
    # an id at or past a smaller nuni than the table was built with
    yield dict(label="smaller nuni", a=a.astype(np.uint32), b=b.astype(np.uint32), count=c.astype(np.uint64), uni=uni,
               nuni=6, N=1000, m=m)
    # equal scores with different counts and keys: COUNT ties by key, RATIO ties by count
    uni2 = np.array([4, 4, 8, 8, 16, 16], np.uint64)
    rows = [(0, 1, 4), (1, 0, 4), (2, 3, 4), (3, 2, 4), (2, 2, 7), (4, 5, 13), (5, 4, 13), (0, 0, 2)]
    a, b, c = (np.array(x) for x in zip(*rows))
    yield dict(label="ties", a=a.astype(np.uint32), b=b.astype(np.uint32), count=c.astype(np.uint64), uni=uni2, nuni=6,
               N=100, m=1)
    yield dict(label="N at 2^53", a=a.astype(np.uint32), b=b.astype(np.uint32), count=c.astype(np.uint64), uni=uni2,
               nuni=6, N=1 << 53, m=1)
    yield dict(label="no pairs", a=np.zeros(0, np.uint32), b=np.zeros(0, np.uint32), count=np.zeros(0, np.uint64),
               uni=uni2, nuni=6, N=100, m=1)
