"""The token filter's rule (include/jiebahip.h, "Token filtering") restated in plain Python: own byte loops, a
dict for the stop set, the Han ranges of Unicode 13 written out.  It calls nothing from the library."""

HAN, ALNUM, NUM, OTHER, INVALID = 1, 2, 4, 8, 16
STOP = 1
TILE = 2048
KEEP, BAD, CLASS, LENGTH, STOPPED = 0, 1, 2, 3, 4

# Unicode 13.0.0 Script=Han (Go 1.18's unicode.Han)
HAN_RANGES = [(0x2E80, 0x2E99), (0x2E9B, 0x2EF3), (0x2F00, 0x2FD5), (0x3005, 0x3005), (0x3007, 0x3007),
              (0x3021, 0x3029), (0x3038, 0x303B), (0x3400, 0x4DBF), (0x4E00, 0x9FFC), (0xF900, 0xFA6D),
              (0xFA70, 0xFAD9), (0x16FF0, 0x16FF1), (0x20000, 0x2A6DD), (0x2A700, 0x2B734), (0x2B740, 0x2B81D),
              (0x2B820, 0x2CEA1), (0x2CEB0, 0x2EBE0), (0x2F800, 0x2FA1D), (0x30000, 0x3134A)]


def is_han(r):
    return any(lo <= r <= hi for lo, hi in HAN_RANGES)


def decode_rune(b):
    """Go's utf8.DecodeRune over the bytes b (not empty): (rune, width); (0xFFFD, 1) for anything malformed or
    cut short."""
    b0 = b[0]
    if b0 < 0x80:
        return b0, 1
    if 0xC2 <= b0 <= 0xDF:
        need, lo, hi, cp = 2, 0x80, 0xBF, b0 & 0x1F
    elif 0xE0 <= b0 <= 0xEF:
        need, cp = 3, b0 & 0x0F
        lo = 0xA0 if b0 == 0xE0 else 0x80
        hi = 0x9F if b0 == 0xED else 0xBF
    elif 0xF0 <= b0 <= 0xF4:
        need, cp = 4, b0 & 0x07
        lo = 0x90 if b0 == 0xF0 else 0x80
        hi = 0x8F if b0 == 0xF4 else 0xBF
    else:
        return 0xFFFD, 1
    if len(b) < need or not lo <= b[1] <= hi:
        return 0xFFFD, 1
    cp = (cp << 6) | (b[1] & 0x3F)
    for i in range(2, need):
        if b[i] & 0xC0 != 0x80:
            return 0xFFFD, 1
        cp = (cp << 6) | (b[i] & 0x3F)
    return cp, need


def _alnum(b):
    return 0x30 <= b <= 0x39 or 0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A


def token_class(span):
    """The class of a good span's bytes."""
    if len(span) == 1 and span[0] >= 0x80:
        return INVALID
    if _alnum(span[0]):
        if len(span) <= 255 and all(0x30 <= b <= 0x39 for b in span):
            return NUM
        return ALNUM
    return HAN if is_han(decode_rune(span[:4])[0]) else OTHER


def runes(span, cls):
    if cls == INVALID:
        return 1
    if len(span) > 1024:
        return 256
    return min(256, sum(1 for b in span if b & 0xC0 != 0x80))


def reason(text, nbytes, s, e, flags, drop, min_runes, max_runes, stop):
    if s >= e or e > nbytes:
        return BAD
    span = bytes(text[s:e])
    cls = token_class(span)
    if drop & cls:
        return CLASS
    n = runes(span, cls)
    if n < min_runes or (max_runes and n > max_runes):
        return LENGTH
    if flags & STOP:
        key = b"\xef\xbf\xbd" if cls == INVALID else span
        if key in stop:
            return STOPPED
    return KEEP


def filter_ref(text, starts, ends, doc_tok, flags=0, drop=0, min_runes=0, max_runes=0, stop=None, ntok=None, cap=None,
               nbytes=None, out_cap=None):
    """-> (out_start, out_end, out_src, out_doc_tok, out_ntok, stats): Python lists; the first three hold the
    min(out_ntok, out_cap) entries the rule writes.  `stop` is a dict or set of bytes keys."""
    text = bytes(text)
    cap = len(starts) if cap is None else cap
    ntok = len(starts) if ntok is None else ntok
    nbytes = len(text) if nbytes is None else nbytes
    out_cap = cap if out_cap is None else out_cap
    stop = {} if stop is None else stop
    nt = min(ntok, cap)
    why = [reason(text, nbytes, int(starts[k]), int(ends[k]), flags, drop, min_runes, max_runes, stop) for k in range(nt)]
    R = [0]
    for w in why:
        R.append(R[-1] + (w == KEEP))
    kept = [k for k in range(nt) if why[k] == KEEP]
    w = kept[:out_cap]
    stats = [nt] + [sum(1 for x in why if x == q) for q in (BAD, CLASS, LENGTH, STOPPED)]
    return ([int(starts[k]) for k in w], [int(ends[k]) for k in w], w, [R[min(int(d), nt)] for d in doc_tok], len(kept),
            stats)
