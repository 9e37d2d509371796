"""The CSRs the postings tests share (tests/test_postings_host.py on the host rule, tests/test_gpu_postings.py on
the kernels): every case is a dict with term_id, term_cnt, term_off, nterms, cap, nids, doc_base and a label.
A helper, not a test."""
import numpy as np

import postings_ref as PR

TILE = 4096  # JB_POSTINGS_TILE
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 70_001]
DIGIT_NIDS = [1, 2, 255, 256, 257, 65_535, 65_536, 65_537, (1 << 24) + 1]


def case(label, ti, tc, to, nids, doc_base=0, nterms=None, cap=None):
    ti, tc, to = np.asarray(ti, np.uint32), np.asarray(tc, np.uint32), np.asarray(to, np.uint64)
    return dict(label=label, term_id=ti, term_cnt=tc, term_off=to, nids=nids, doc_base=doc_base,
                nterms=len(ti) if nterms is None else nterms, cap=len(ti) if cap is None else cap)


def hand_checked():
    # three rows {1, 4, 9}, {4}, {0, 4, 9, 11} with distinct counts
    ti, tc, to = [1, 4, 9, 4, 0, 4, 9, 11], [3, 1, 2, 7, 5, 4, 6, 8], [0, 3, 4, 8]
    for nids in (10, 12, 1, 0):
        for base in (0, 1000):
            yield case(f"hand nids={nids} base={base}", ti, tc, to, nids, base)


def list_lengths():
    rng = np.random.default_rng(101)
    for n in LENGTHS:
        ti, tc, to = PR.random_csr(rng, n, max(1, min(n // 3, 500)), 300)
        if n:
            ti[n // 2] = 0xFFFFFFFF
        yield case(f"length {n}", ti, tc, to, 256)


def digit_edges(n=20_000):
    rng = np.random.default_rng(103)
    for nids in DIGIT_NIDS:
        top = max(nids.bit_length() - 1, 0) // 8 * 8  # the lowest bit of the top digit
        pool = np.unique(np.array([0, nids - 1, nids, nids + 1] + [(k << top) | 5 for k in range(1, 5)] +
                                  [(k << top) for k in range(1, 5)] + [(k << max(top - 8, 0)) | 3 for k in range(1, 5)] +
rng.integers(0, nids + 2, 40).tolist(), np.int64))
        ti, tc, to = PR.random_csr(rng, n, 700, 1)
        ti = pool[rng.integers(0, len(pool), n)].astype(np.uint32)
        ti[:3] = [nids - 1, 0, nids - 1]
        yield case(f"digits nids={nids}", ti, tc, to, nids)


def skew(n=70_001):
    rng = np.random.default_rng(107)
    _, tc, to = PR.random_csr(rng, n, 900, 1)
    yield case("one id", np.full(n, 77, np.uint32), tc, to, 300)
    yield case("low 8 bits shared", (rng.integers(0, 250, n).astype(np.uint32) << 8) | 0x5A, tc, to, 64_000)
    yield case("zipf", (rng.zipf(1.3, n) % 50_000).astype(np.uint32), tc, to, 40_000)


def stability():
    """A caller's CSR with ids repeated inside rows; term_cnt is the entry's own index."""
    rng = np.random.default_rng(109)
    n = 3 * TILE + 17
    _, _, to = PR.random_csr(rng, n, 40, 1)
    yield case("repeats", rng.integers(0, 23, n), np.arange(n), to, 20)
    yield case("repeats two digits", rng.integers(0, 23, n) * 256 + 1, np.arange(n), to, 22 * 256)


def counts_and_offsets():
    rng = np.random.default_rng(113)
    n = 10_000
    ti, tc, to = PR.random_csr(rng, n, 300, 500)
    for nterms, cap in ((777, n), (n, n), (n + 1000, n), (n + 1000, 4099), (5, 0), (0, n)):
        yield case(f"nterms={nterms} cap={cap}", ti, tc, to, 400, 7, nterms, cap)
    short = to.copy()
    short[-1] = 9000
    short = np.minimum(short, 9000)
    yield case("term_off[ndocs] below nterms", ti, tc, short, 400, 7)
    yield case("no rows", ti, tc, np.zeros(1, np.uint64), 400)


def all_cases():
    for gen in (hand_checked, list_lengths, digit_edges, skew, stability, counts_and_offsets):
        yield from gen()
