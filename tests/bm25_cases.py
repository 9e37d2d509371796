"""Seeded indexes and queries for the BM25 tests (tests/test_bm25_host.py on the host rule, tests/test_gpu_bm25.py
on the kernels): the smallest shapes at which the search can go wrong.  A case is a dict of the arguments of
jb_bm25_search: the index (post_doc, post_tf, post_off, npost, nids), doc_len, ndocs, k1, b, weight (None: the
rule's own weights), nweights, the queries (q_id, q_off, q_cap) and the topk values to run."""
import numpy as np

TILE = 8192
MAXQ = 1024
UNK = 0xFFFFFFFF
NIDS = 40  # id 0 is in every document, ids 1 .. 4 are rare (id 3 the rarest), the rest are drawn at 5 %


def index(ndocs, seed, nids=NIDS, equal=False):
    """Lists ascending by document.  equal: every tf is 1 and every document has 7 tokens, so documents tie."""
    rng = np.random.default_rng(seed)
    docs, tfs, off = [], [], [0]
    for t in range(nids):
        if t == 0:
            d = np.arange(ndocs)
        else:
            p = 0.003 if t == 3 else 0.01 if t <= 4 else 0.05
            d = np.flatnonzero(rng.random(ndocs) < p)
            if ndocs and t == 1:  # the first and the last document of every tile
                d = np.union1d(d, np.unique(np.clip(np.concatenate([np.arange(0, ndocs, TILE), np.arange(TILE - 1, ndocs, TILE),
                                                                   [ndocs - 1]]), 0, ndocs - 1)))
        docs.append(d.astype(np.uint32))
        tfs.append(np.ones(len(d), np.uint32) if equal else rng.integers(1, 9, len(d)).astype(np.uint32))
        off.append(off[-1] + len(d))
    doc_len = np.full(ndocs, 7, np.uint32) if equal else rng.integers(1, 200, ndocs).astype(np.uint32)
    return (np.concatenate(docs) if docs else np.zeros(0, np.uint32), np.concatenate(tfs) if tfs else np.zeros(0, np.uint32),
            np.array(off, np.uint64), doc_len)


def queries(nids, seed):
    """The query CSR: (q_id, q_off).  In order: the id of every document; empty; unknown ids only; a repeated
    id; more than MAXQ entries (the entries past MAXQ name an id the first MAXQ do not); two random queries."""
    rng = np.random.default_rng(seed)
    qs = [[0], [], [nids, nids + 5, UNK], [3, 3, 3], [1 + (k % 4) for k in range(MAXQ)] + [6] * 40,
          rng.integers(0, nids, 5).tolist(), rng.integers(0, nids + 3, 9).tolist()]
    off = np.cumsum([0] + [len(q) for q in qs]).astype(np.uint64)
    return np.array([t for q in qs for t in q], np.uint32), off


def case(label, ndocs, seed, k1=1.2, b=0.75, equal=False, topks=(1, 10, 64), **kw):
    pd, pt, po, dl = index(ndocs, seed, equal=equal)
    qi, qo = queries(NIDS, seed + 1)
    c = dict(label=label, post_doc=pd, post_tf=pt, post_off=po, npost=len(pd), nids=NIDS, doc_len=dl, ndocs=ndocs, k1=k1,
             b=b, weight=None, nweights=NIDS, q_id=qi, q_off=qo, q_cap=len(qi), topks=topks)
    c.update(kw)
    return c


def all_cases():
    for nd in (0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3):
        yield case(f"ndocs={nd}", nd, 100 + nd % 97)
    # equal tf and equal lengths: every document ties under id 0, across the tile boundaries; topk cuts the tie
    yield case("ties", 2 * TILE + 3, 7, equal=True, topks=(1, 10, 40, 64))
    yield case("ties-small", 50, 8, equal=True, topks=(1, 64))  # fewer candidates than topk = 64
    # the parameters' ends
    yield case("b=0", TILE + 1, 9, b=0.0, topks=(10,))
    yield case("b=1", TILE + 1, 10, b=1.0, topks=(10,))
    yield case("k1=0", TILE + 1, 11, k1=0.0, topks=(10,))
    yield case("k1=64", 300, 12, k1=64.0, b=1.0, topks=(10,))
    # weights that do not take part: 0, negative, NaN, +Inf, above WMAX; WMAX itself does
    c = case("weights", TILE + 1, 13, topks=(10,))
    w = np.linspace(0.5, 3.0, NIDS).astype(np.float32)
    w[0], w[1], w[2], w[3], w[5], w[6] = 0.0, -1.0, np.nan, np.inf, np.float32(2.0 ** 20) * np.float32(1.0000002), 2.0 ** 20
    c["weight"] = w
    yield c
    # fewer weights than ids: the ids past nweights do not take part
    c = case("nweights", 300, 14, topks=(10,))
    c["weight"], c["nweights"] = np.linspace(0.5, 3.0, 7).astype(np.float32), 7
    yield c
    # tf == 0 postings do not take part
    c = case("tf=0", TILE + 1, 15, topks=(10,))
    c["post_tf"] = c["post_tf"].copy()
    c["post_tf"][::3] = 0
    yield c
    # q_off past q_cap: the last queries are cut short or empty
    c = case("q_cap", 300, 16, topks=(10,))
    c["q_cap"] = int(c["q_off"][-2]) + 2
    yield c
    c = case("q_cap=0", 300, 17, topks=(10,))
    c["q_cap"] = 0
    yield c
    # npost below the offsets: the last lists are cut short or empty; documents at or past ndocs at the lists' ends
    c = case("npost", 300, 18, topks=(10,))
    c["npost"] = int(c["post_off"][30]) + 3
    yield c
    c = case("docs>=ndocs", 300, 19, topks=(10,))
    c["ndocs"], c["doc_len"] = 260, c["doc_len"][:260]
    yield c
    # one more id whose offsets decrease: an empty list
    c = case("offsets-decrease", 300, 20, topks=(10,))
    c["post_off"] = np.concatenate([c["post_off"], [5]]).astype(np.uint64)
    c["nids"] = c["nweights"] = NIDS + 1
    c["q_id"] = np.concatenate([c["q_id"], [NIDS, 2]]).astype(np.uint32)
    c["q_off"] = np.concatenate([c["q_off"], [len(c["q_id"])]]).astype(np.uint64)
    c["q_cap"] = len(c["q_id"])
    c["weight"] = np.full(NIDS + 1, 1.5, np.float32)  # (the rule's own weight of an empty list is 0)
    yield c
    # no query, no id
    c = case("nq=0", 300, 21, topks=(10,))
    c["q_id"], c["q_off"], c["q_cap"] = np.zeros(0, np.uint32), np.zeros(1, np.uint64), 0
    yield c
    c = case("nids=0", 300, 22, topks=(10,))
    c.update(post_doc=np.zeros(0, np.uint32), post_tf=np.zeros(0, np.uint32), post_off=np.zeros(1, np.uint64), npost=0,
             nids=0, nweights=0)
    yield c
