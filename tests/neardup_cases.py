"""The inputs the near-duplicate tests share (tests/test_neardup_host.py on the host rule, tests/test_gpu_neardup.py
on the kernels): every case is a dict with key (uint64[ndocs, B]), sig (uint32[ndocs, K]), W, min_agree and a
label.  Keys and slots are arbitrary bit patterns drawn from small pools, so that buckets form.  A helper, not a
test."""
import numpy as np

TILE = 4096  # JB_ND_TILE
NOKEY = 0xFFFFFFFFFFFFFFFF
TOPKEY = NOKEY - 1  # the greatest key that is in a bucket: its run ends the sorted list of its band


def case(label, key, sig, W, min_agree):
    key, sig = np.ascontiguousarray(key, np.uint64), np.ascontiguousarray(sig, np.uint32)
    assert key.ndim == 2 and sig.ndim == 2 and len(key) == len(sig)
    return dict(label=label, key=key, sig=sig, W=W, min_agree=min_agree)


def pooled(rng, nd, B, K, npool, nproto, noise, nokey=0.0):
    """Keys from a pool of npool arbitrary u64 values per band; signatures that are one of nproto prototype rows
    with a share `noise` of their slots redrawn; a share `nokey` of the keys is JB_MH_NOKEY."""
    pools = rng.integers(0, 1 << 63, (B, npool), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (B, npool)).astype(np.uint64)
    key = pools[np.arange(B)[None, :], rng.integers(0, npool, (nd, B))]
    if nokey:
        key[rng.random((nd, B)) < nokey] = NOKEY
    proto = rng.integers(0, 1 << 32, (nproto, K), dtype=np.uint64).astype(np.uint32)
    sig = proto[rng.integers(0, nproto, nd)].copy()
    redraw = rng.random((nd, K)) < noise
    sig[redraw] = rng.integers(0, 1 << 32, int(redraw.sum()), dtype=np.uint64).astype(np.uint32)
    return key, sig


def tiny():
    rng = np.random.default_rng(211)
    for nd in (0, 1, 2):
        key, sig = pooled(rng, nd, 4, 8, 1, 1, 0.0)
        yield case(f"ndocs={nd}", key.reshape(nd, 4), sig.reshape(nd, 8), 64, 8)


def shapes():
    rng = np.random.default_rng(223)
    for B, K, nd in ((1, 128, 300), (256, 256, 40), (7, 1, 90), (5, 70, 200), (3, 130, 200), (2, 64, 150), (9, 193, 120)):
        key, sig = pooled(rng, nd, B, K, 6, 5, 0.1, 0.05)
        yield case(f"B={B} K={K}", key, sig, 64, max(1, K // 2))


def one_bucket():
    """Every document in one bucket of band 0 (and alone in band 1): more members than W."""
    rng = np.random.default_rng(227)
    nd = 150
    key, sig = pooled(rng, nd, 2, 16, 40, 2, 0.05)
    key[:, 0] = 0x0123456789ABCDEF
    key[:, 1] = rng.permutation(nd).astype(np.uint64) << np.uint64(33)
    for W in (1, 2, 63, 64):
        yield case(f"one bucket W={W}", key, sig, W, 8)


def tile_edges():
    """ndocs * B on either side of a tile; in the last band several documents hold the greatest key, so the last
    run of the sorted list ends at position ndocs * B - 1."""
    rng = np.random.default_rng(229)
    for B, nd in ((3, 1365), (2, 2048), (17, 241)):
        assert B * nd in (TILE - 1, TILE, TILE + 1)
        key, sig = pooled(rng, nd, B, 8, nd // 3, 7, 0.1, 0.02)
        key[rng.integers(0, nd, 5), B - 1] = TOPKEY
        key[nd - 1, B - 1] = TOPKEY
        yield case(f"entries={B * nd}", key, sig, 4, 6)
    # 2 * TILE + 1 entries: band 0 is all distinct, band 1 (sorted positions 2731 .. 5461) one bucket that crosses
    # the first tile boundary, band 2 (5462 .. 8192) two buckets, the second crossing the next
    nd = 2731
    _, sig = pooled(rng, nd, 3, 8, 4, 3, 0.05)
    key = np.zeros((nd, 3), np.uint64)
    key[:, 0] = rng.permutation(nd).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    key[:, 1] = 0x00FF00FF00FF00FF
    key[:, 2] = np.where(np.arange(nd) % 5 == 0, np.uint64(7), np.uint64(TOPKEY))
    yield case("runs across tiles", key, sig, 3, 5)


def band_rules():
    rng = np.random.default_rng(233)
    K = 8
    same = np.tile(rng.integers(0, 1 << 32, K, dtype=np.uint64).astype(np.uint32), (6, 1))
    # documents 0, 1, 2 share band 0; 0 and 2 also share band 1, where they are neighbours: with W = 1 the pair
    # (0, 2) is beyond the window in its first common band and is not picked up by band 1
    key = np.array([[5, 9], [5, 1], [5, 9], [6, 2], [7, 3], [8, 4]], np.uint64)
    yield case("beyond the window in the first band", key, same, 1, K)
    yield case("inside the window in the first band", key, same, 2, K)
    # one key value in two different bands is no bucket; documents 2 and 3 do share band 1
    key = np.array([[77, 1], [2, 77], [3, 50], [4, 50], [NOKEY, NOKEY], [78, NOKEY]], np.uint64)
    yield case("one value in two bands", key, same, 64, K)
    # several common bands: reported once, at the first
    key = np.array([[1, 2, 3], [1, 2, 3], [9, 2, 3], [9, 8, 3], [NOKEY, 2, 3], [NOKEY, NOKEY, NOKEY]], np.uint64)
    yield case("several common bands", key, same[:, :K], 64, K)


def key_parts():
    """Keys that differ only in their high 32 bits, only in their low 32 bits, only in one byte: two documents of
    each, so a sort or a match on a part of the key merges buckets."""
    rng = np.random.default_rng(239)
    base = 0x8000000180000001
    vals = [base, base ^ (1 << 32), base ^ (1 << 63), base ^ 2, base ^ (1 << 31)] + [base ^ (0x5A << (8 * k)) for k in range(8)]
    nd, K = 2 * len(vals), 16
    key = np.array([[v, v ^ 1] for v in vals for _ in range(2)], np.uint64)[rng.permutation(nd)]
    sig = np.tile(rng.integers(0, 1 << 32, K, dtype=np.uint64).astype(np.uint32), (nd, 1))
    yield case("key parts", key, sig, 64, K)


def nokeys():
    rng = np.random.default_rng(241)
    key, sig = pooled(rng, 120, 4, 12, 5, 3, 0.05)
    key[::7] = NOKEY          # in all of a document's bands
    key[3::5, 1] = NOKEY      # in only some
    key[0] = NOKEY            # rows with no pairs at the start and the end of the CSR
    key[-2:] = NOKEY
    yield case("nokey", key, sig, 64, 6)
    yield case("all nokey", np.full((50, 3), NOKEY, np.uint64), sig[:50], 64, 1)


def thresholds():
    """Pairs whose agree is exactly min_agree - 1 and exactly min_agree, at min_agree 1 and K."""
    rng = np.random.default_rng(251)
    for K in (1, 64, 65, 100):
        a = rng.integers(0, 1 << 31, K, dtype=np.uint64).astype(np.uint32)
        other = a + np.uint32(1 << 31)  # differs from a in every slot
        one = other.copy()
        one[K - 1] = a[K - 1]           # agrees with a in exactly one slot
        but1 = a.copy()
        but1[0] = other[0]              # agrees with a in all but one
        sig = np.stack([a, other, one, a, but1])
        key = np.full((5, 1), 11, np.uint64)
        for m in sorted({1, K}):
            yield case(f"threshold K={K} min_agree={m}", key, sig, 64, m)


def mixed():
    rng = np.random.default_rng(257)
    key, sig = pooled(rng, 3000, 4, 32, 900, 60, 0.08, 0.03)
    yield case("mixed", key, sig, 64, 26)
    key, sig = pooled(rng, 1200, 6, 20, 12, 10, 0.1, 0.1)
    yield case("crowded", key, sig, 5, 15)


def all_cases():
    for gen in (tiny, shapes, one_bucket, tile_edges, band_rules, key_parts, nokeys, thresholds, mixed):
        yield from gen()
