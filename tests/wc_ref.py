"""The word-count rule of include/jiebahip.h (jb_wc_count, the device table) restated in Python: the key of a
span, a Counter, the sort.  The tests pin the host function and the kernels to it."""
from collections import Counter

import numpy as np

REPL = b"\xef\xbf\xbd"
MAXKEY = 255


class Ref:
    """keys (bytes, in the rule's order, after the filters), counts, the totals, and `all`: every key's count
    before the filters."""

    def __init__(self, keys, counts, bad, long, tokens, all_counts):
        self.keys, self.counts, self.bad, self.long, self.tokens, self.all = keys, counts, bad, long, tokens, all_counts

    @property
    def counted(self):
        return sum(self.all.values())


def key_of(text, nbytes, s, e):
    """The key of span [s, e), "bad" or "long"."""
    if s >= e or e > nbytes:
        return "bad"
    if e - s > MAXKEY:
        return "long"
    if e - s == 1 and text[s] >= 0x80:
        return REPL
    return bytes(text[s:e])


def order(counts, min_count=1, max_keys=0):
    """[(key, count)] by count descending, then by bytes (Python's bytes order is memcmp's, a proper prefix
    first), without the keys below min_count, the first max_keys of them (0: all)."""
    items = sorted(counts.items(), key=lambda kv: (-kv[1], kv[0]))
    items = [kv for kv in items if kv[1] >= min_count]
    return items[:max_keys] if max_keys else items


def wc_ref(text, starts, ends, ntok=None, cap=None, nbytes=None, min_count=1, max_keys=0):
    text = bytes(text)
    s, e = np.asarray(starts).tolist(), np.asarray(ends).tolist()
    cap = len(s) if cap is None else cap
    ntok = len(s) if ntok is None else ntok
    nbytes = len(text) if nbytes is None else nbytes
    n = min(ntok, cap)
    c, bad, long = Counter(), 0, 0
    for k in range(n):
        key = key_of(text, nbytes, s[k], e[k])
        if key == "bad":
            bad += 1
        elif key == "long":
            long += 1
        else:
            c[key] += 1
    items = order(c, min_count, max_keys)
    return Ref([k for k, _ in items], [v for _, v in items], bad, long, n, dict(c))


def same(got, ref, dropped=0, collided=0):
    """Is a jiebahip.WcResult the reference, exactly?  Returns a description of the first difference, or None."""
    if got.keys != ref.keys:
        i = next((i for i, (a, b) in enumerate(zip(got.keys, ref.keys)) if a != b), min(len(got.keys), len(ref.keys)))
        return f"{len(got.keys)} keys, want {len(ref.keys)}; first difference at {i}: {got.keys[i:i + 2]} / {ref.keys[i:i + 2]}"
    if got.counts.tolist() != list(ref.counts):
        i = next(i for i, (a, b) in enumerate(zip(got.counts.tolist(), ref.counts)) if a != b)
        return f"count of {ref.keys[i]!r}: {got.counts[i]}, want {ref.counts[i]}"
    tot = (got.bad, got.long, got.dropped, got.collided, got.tokens)
    want = (ref.bad, ref.long, dropped, collided, ref.tokens)
    return None if tot == want else f"totals (bad, long, dropped, collided, tokens) {tot}, want {want}"


def from_keys(keys, gap=b""):
    """(text, starts, ends): the keys back to back (with `gap` between them), one span each."""
    parts, s, e, pos = [], [], [], 0
    for k in keys:
        s.append(pos)
        e.append(pos + len(k))
        parts.append(k + gap)
        pos += len(k) + len(gap)
    return b"".join(parts), np.array(s, np.uint32), np.array(e, np.uint32)


def random_case(seed, ntokens=None, nbytes=None, clamp=True):
    """A seeded span list over random text: ordered, overlapping and malformed spans (start >= end, end past the
    text, start near 2^32), invalid bytes, keys of up to 300 bytes, and (clamp) ntok / cap on either side of the
    arrays."""
    rng = np.random.default_rng(seed)
    nbytes = int(rng.integers(0, 600)) if nbytes is None else nbytes
    text = rng.integers(0x61, 0x67, nbytes).astype(np.uint8)
    text[rng.random(nbytes) < 0.15] = 0x80 + int(rng.integers(0, 128))
    n = int(rng.integers(0, 400)) if ntokens is None else ntokens
    s = rng.integers(0, nbytes + 1, n).astype(np.int64)
    ln = np.where(rng.random(n) < 0.4, 1, rng.integers(0, 7, n))
    ln = np.where(rng.random(n) < 0.02, rng.integers(200, 301, n), ln)
    e = np.minimum(s + ln, nbytes)
    kind = rng.integers(0, 25, n)
    e = np.where(kind == 0, s, e)
    s, e = np.where(kind == 1, e, s), np.where(kind == 1, s, e)
    e = np.where(kind == 2, nbytes + 1 + rng.integers(0, 1000, n), e)
    s = np.where(kind == 3, 0xFFFFFFF0, s)
    e = np.where(kind == 3, 0xFFFFFFFF, e)
    ntok, cap = n, n
    mode = int(rng.integers(0, 3)) if clamp else 0
    if mode == 1:
        ntok, cap = int(rng.integers(0, 2 * n + 2)), int(rng.integers(0, n + 1))
    elif mode == 2:
        ntok = int(rng.integers(0, n + 1))
    return text.tobytes(), s.astype(np.uint32)[:cap], e.astype(np.uint32)[:cap], ntok, cap


_M64 = (1 << 64) - 1


def vocab_hash(key):
    """jb_vocab_hash (jieba-go_amd/csrc/jb_vocab.h) of a key of 1 to 255 bytes: its 8-byte little-endian words,
    zero-padded, mixed in turn into a start value that depends on the length."""
    def mix(h, w):
        h = ((h ^ w) * 0x9E3779B97F4A7C15) & _M64
        return h ^ (h >> 32)
    h = 0x243F6A8885A308D3 ^ ((len(key) * 0xFF51AFD7ED558CCD) & _M64)
    for p in range(0, len(key), 8):
        h = mix(h, int.from_bytes(key[p:p + 8], "little"))
    h = (h * 0xD6E8FEB86659FD93) & _M64
    return h ^ (h >> 32)


def fp(key, bits=64):
    """jb_wc_fp: the hash's low `bits` bits, and 1 where they are 0."""
    h = vocab_hash(key) & ((1 << bits) - 1)
    return h or 1
