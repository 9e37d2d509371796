"""Inputs the token filter's host and GPU tests share: one piece per class and length case of the rule
(include/jiebahip.h, "Token filtering"), and stop keys of every storage form of the table with near misses."""

HAN256 = "中".encode() * 256
# every class: a 255-byte and a 256-byte digit run, a 2,000-byte letter run, a lone continuation byte, a Han rune
# cut short, kana, hangul, an astral Han rune, U+3007 and U+3005 (Han) beside U+3006 (not), 256 Han runes, 1025 bytes
# of 4-byte runes
PIECES = ["中文".encode(), b"abc", b"123", b"9" * 255, b"9" * 256, b"x" * 2000, "，".encode(), b"\x80", b"\xe4\xb8",
          "カ".encode(), "한".encode(), b"a1", b"1a", b"0", "𠀀".encode(), "〇".encode(), b"\xbf\xbf", b"!", HAN256,
          "😀".encode() * 256 + b"\xf0", "的".encode(), b"Z9" * 130, b"\xff", "〆".encode(), "々".encode()]
LENGTH_PIECES = ["中".encode() * 255, "中".encode() * 254, b"ab", "中a".encode(), "😀".encode() * 256, b"\x80" * 1025,
                 b"\x80" * 1024, b"\xbf" * 5]
RUNE_BOUNDS = [(1, 0), (2, 0), (255, 0), (0, 1), (0, 2), (0, 255), (2, 2), (1, 255), (255, 255), (3, 1)]
# stop keys of 1, 8, 9, 24, 25 and 255 bytes (the table's 8-byte, inline and pool forms), EF BF BD, and others
STOP_KEYS = [b"a", b"abcdefgh", b"abcdefghi", b"x" * 24, b"y" * 25, b"z" * 255, b"\xef\xbf\xbd", "的".encode(), b"123"]
NEAR_KEYS = [b"b", b"abcdefgx", b"abcdefghj", b"x" * 23, b"x" * 25, b"y" * 24, b"y" * 26, b"z" * 254, b"z" * 256,
             b"\x80", b"\xff", "了".encode(), b"1234", b"12", b"ab"]


def spans_of(pieces, gap=b""):
    """Pieces (bytes) laid one after another with `gap` between: (text, starts, ends)."""
    s, e, parts, pos = [], [], [], 0
    for p in pieces:
        s.append(pos)
        pos += len(p)
        e.append(pos)
        parts.append(p + gap)
        pos += len(gap)
    return b"".join(parts), s, e
