"""Shared by the vocabulary tests (test_vocab_host.py, test_gpu_ids.py): seeded keys, near misses
and the reference of every lookup, a Python dict over the key bytes: vocab.get(key, UNK)."""
import functools

import numpy as np

UNK = 0xFFFFFFFF
FFFD = "�".encode()


@functools.lru_cache(maxsize=None)
def identity_keys(n=200_000, seed=20_241):
    """n distinct random keys of 1..40 bytes over all 256 byte values, then one more key of every length
    2..64 and one of 255 bytes (all 256 one-byte keys are among the random ones)."""
    rng = np.random.default_rng(seed)
    seen, out = set(), []

    def add(k):
        if k in seen:
            return False
        seen.add(k)
        out.append(k)
        return True

    while len(out) < n:
        lens = rng.integers(1, 41, size=n - len(out))
        # (half the 1-byte keys would collide: short keys are drawn again until they are new)
        raw = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8).tobytes()
        p = 0
        for ln in lens.tolist():
            add(raw[p:p + ln])
            p += ln
    for ln in list(range(2, 65)) + [255]:  # (every 1-byte key is in the list already)
        while not add(rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes()):
            pass
    assert {len(k) for k in out} >= set(range(1, 65)) | {255}
    return tuple(out)


def key_dict(keys):
    return {k: i for i, k in enumerate(keys)}


def near_misses(keys, n=200_000, seed=77):
    """n probes near the keys, a quarter each: the last byte changed, one byte dropped, one byte
    appended, a random string of 1..40 bytes.  (Some are keys: the dict says which.)"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(keys), size=n).tolist()
    r = rng.integers(0, 1 << 30, size=n).tolist()
    out = []
    for j in range(n):
        k = keys[pick[j]]
        kind = j & 3
        if kind == 0:
            out.append(k[:-1] + bytes([(k[-1] + 1 + r[j] % 255) & 255]))
        elif kind == 1:
            p = r[j] % len(k)
            out.append(k[:p] + k[p + 1:])  # (may be empty: found by nothing)
        elif kind == 2:
            out.append(k + bytes([r[j] & 255]))
        else:
            out.append(rng.integers(0, 256, size=1 + r[j] % 40, dtype=np.uint8).tobytes())
    return out


def span_key(text, s, e):
    """The key of the span [s, e) of `text` (bytes): its bytes, or EF BF BD for one invalid byte."""
    if e - s == 1 and text[s] >= 0x80:
        return FFFD
    return bytes(text[s:e])


def expect_ids(vocab, text, starts, ends, nbytes=None):
    """The dict applied to spans the kernel must not trust: empty, reversed or past the text -> UNK."""
    nbytes = len(text) if nbytes is None else nbytes
    out = np.empty(len(starts), np.uint32)
    for k, (s, e) in enumerate(zip(starts, ends)):
        out[k] = vocab.get(span_key(text, s, e), UNK) if s < e <= nbytes else UNK
    return out
