"""The MinHash rule of include/jiebahip.h (jb_minhash, jb_minhash_params, jb_minhash_bands) restated in Python
integers, from the constants of the header alone: the key of a span, its hash, the shingle fold, the splitmix64
hash family, the multiply-shift slot and the band key.  The tests pin the host functions and the kernels to it."""
import numpy as np

M64 = (1 << 64) - 1
REPL = b"\xef\xbf\xbd"
MAXKEY = 255
MAXN, MAXK, TILE = 8, 256, 1024
EMPTY = 0xFFFFFFFF
NOKEY = M64


def init(c):
    return 0x243F6A8885A308D3 ^ ((c * 0xFF51AFD7ED558CCD) & M64)


def mix(h, w):
    h = ((h ^ w) * 0x9E3779B97F4A7C15) & M64
    return h ^ (h >> 32)


def fin(h):
    h = (h * 0xD6E8FEB86659FD93) & M64
    return h ^ (h >> 32)


def key_hash(key):
    """The vocabulary's hash of a key of 0 to 255 bytes: 8-byte little-endian words, zero-padded, at least one."""
    h = init(len(key))
    for p in range(0, max(len(key), 1), 8):
        h = mix(h, int.from_bytes(key[p:p + 8], "little"))
    return fin(h)


def key_of(text, nbytes, s, e):
    if s >= e or e > nbytes:
        return b""
    if e - s == 1 and text[s] >= 0x80:
        return REPL
    return bytes(text[s:min(e, s + MAXKEY)])


def token_hashes(text, starts, ends, n, nbytes=None):
    text = bytes(text)
    nbytes = len(text) if nbytes is None else nbytes
    memo = {}
    out = []
    for s, e in zip(starts[:n], ends[:n]):
        k = key_of(text, nbytes, s, e)
        if k not in memo:
            memo[k] = key_hash(k)
        out.append(memo[k])
    return out


def params(seed, K):
    st, vals = seed & M64, []
    for _ in range(2 * K):
        st = (st + 0x9E3779B97F4A7C15) & M64
        z = st
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        vals.append(z ^ (z >> 31))
    return [v | 1 for v in vals[0::2]], vals[1::2]


def shingle_x(ts):
    g = init(len(ts))
    for t in ts:
        g = mix(g, t)
    return fin(g) & 0xFFFFFFFF


def doc_shingles(t, lo, hi, n):
    """x of every shingle of the document whose tokens are t[lo:hi]."""
    m = hi - lo
    if m <= 0:
        return []
    if m < n:
        return [shingle_x(t[lo:hi])]
    return [shingle_x(t[lo + i:lo + i + n]) for i in range(m - n + 1)]


def minhash_ref(text, starts, ends, doc_tok, n, K, seed, ntok=None, cap=None, nbytes=None):
    """(sig uint32[ndocs, K], doc_n uint32[ndocs]) by the rule."""
    s, e = np.asarray(starts).tolist(), np.asarray(ends).tolist()
    dt = np.asarray(doc_tok).tolist()
    cap = len(s) if cap is None else cap
    ntok = len(s) if ntok is None else ntok
    nt = min(ntok, cap)
    t = token_hashes(text, s, e, nt, nbytes)
    a, b = params(seed, K)
    av, bv = np.array(a, np.uint64), np.array(b, np.uint64)
    nd = len(dt) - 1
    sig = np.full((nd, K), EMPTY, np.uint32)
    doc_n = np.zeros(nd, np.uint32)
    for d in range(nd):
        xs = doc_shingles(t, min(dt[d], nt), min(dt[d + 1], nt), n)
        doc_n[d] = len(xs)
        if not xs:
            continue
        if len(xs) * K <= 64:  # plain integers
            for j in range(K):
                sig[d, j] = min(((a[j] * x + b[j]) & M64) >> 32 for x in xs)
        else:  # the same in uint64 arithmetic, which wraps modulo 2^64
            with np.errstate(over="ignore"):
                v = (av[None, :] * np.array(xs, np.uint64)[:, None] + bv[None, :]) >> np.uint64(32)
            sig[d] = v.min(axis=0).astype(np.uint32)
    return sig, doc_n


def bands_ref(sig, doc_n, B, R):
    sig = np.asarray(sig)
    nd = sig.shape[0]
    keys = np.full((nd, B), NOKEY, np.uint64)
    for d in range(nd):
        if int(doc_n[d]) == 0:
            continue
        row = sig[d].tolist()
        for band in range(B):
            g = mix(init(R), band)
            for r in range(R):
                g = mix(g, row[band * R + r])
            g = fin(g)
            keys[d, band] = NOKEY - 1 if g == NOKEY else g
    return keys


def from_keys(keys, gap=b""):
    """(text, starts, ends): the keys back to back (with `gap` between them), one span each."""
    parts, s, e, pos = [], [], [], 0
    for k in keys:
        s.append(pos)
        e.append(pos + len(k))
        parts.append(k + gap)
        pos += len(k) + len(gap)
    return b"".join(parts), np.array(s, np.uint32), np.array(e, np.uint32)
