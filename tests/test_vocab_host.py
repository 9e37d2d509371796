"""CPU: the vocabulary table of the token-id calls (jb_vocab_build / jb_vocab_lookup, the device
probe run on the host) against a Python dict over the key bytes.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest

import jiebahip as J
import vocab_ref as V

NEW = ["jb_vocab_build", "jb_vocab_free", "jb_vocab_lookup", "jb_vocab_info", "jb_vocab_set", "jb_vocab_size",
       "jb_ids_device", "jb_spans_ids"]


def _err():
    return J.lib().jb_last_error().decode()


def _build_raw(keys_bytes, off):
    """jb_vocab_build on raw arrays -> (rc, handle)."""
    buf = np.frombuffer(keys_bytes + b"\0", np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    h = C.c_void_p()
    rc = J.lib().jb_vocab_build(buf.ctypes.data, off.ctypes.data, len(off) - 1, C.byref(h))
    return rc, h


def test_exports_and_null_arguments():
    L = J.lib()
    for name in NEW:
        assert name in J.EXPORTS and hasattr(L, name), name
    assert J.JB_ID_UNK == V.UNK
    h, i = C.c_void_p(), C.c_uint32()
    n, ml, ns = C.c_uint32(), C.c_uint32(), C.c_uint64()
    sp = J.jb_spans()
    one = np.zeros(1, np.uint64)
    assert L.jb_vocab_build(None, None, 0, None) == J.JB_EINVAL
    assert L.jb_vocab_build(None, None, 3, C.byref(h)) == J.JB_EINVAL and not h.value
    assert L.jb_vocab_lookup(None, b"a", 1, C.byref(i)) == J.JB_EINVAL
    assert L.jb_vocab_info(None, C.byref(n), C.byref(ml), C.byref(ns)) == J.JB_EINVAL
    assert L.jb_vocab_set(None, b"a", one.ctypes.data, 0) == J.JB_EINVAL
    assert L.jb_vocab_size(None) == -1
    assert L.jb_ids_device(None, None, 0, None, None, one.ctypes.data, 0, None, None) == J.JB_EINVAL
    assert L.jb_spans_ids(None, b"a", C.byref(sp), None) == J.JB_EINVAL
    L.jb_vocab_free(None)  # (a no-op)


def test_build_rejects_an_empty_key():
    rc, h = _build_raw(b"abcd", [0, 2, 2, 4])
    assert rc == J.JB_EINVAL and not h.value and "key 1 is empty" in _err()


def test_build_rejects_offsets_that_do_not_start_at_zero():
    rc, h = _build_raw(b"abcd", [1, 2, 4])
    assert rc == J.JB_EINVAL and not h.value and "key_off[0]" in _err()


def test_build_rejects_decreasing_offsets():
    rc, h = _build_raw(b"abcd", [0, 3, 2, 4])
    assert rc == J.JB_EINVAL and not h.value and "decreases at key 1" in _err()


def test_build_rejects_a_key_over_255_bytes():
    rc, h = _build_raw(b"a" + b"x" * 256, [0, 1, 257])
    assert rc == J.JB_ELIMIT and not h.value and "key 1 has 256 bytes" in _err()
    rc, h = _build_raw(b"a" + b"x" * 255, [0, 1, 256])  # 255 bytes are fine
    assert rc == J.JB_OK
    J.lib().jb_vocab_free(h)


def test_build_rejects_a_duplicate_and_names_both():
    with pytest.raises(J.JbError) as ei:
        J.Vocab([b"a", b"bc", b"\xff\x00", b"bc"])
    assert ei.value.code == J.JB_EINVAL and "1" in str(ei.value) and "3" in str(ei.value)
    long = b"y" * 100  # the same for keys that live in the pool
    with pytest.raises(J.JbError) as ei:
        J.Vocab([long, b"a", b"b", b"c", b"d", long])
    assert ei.value.code == J.JB_EINVAL and "keys 0 and 5" in str(ei.value)
    J.Vocab([b"y" * 100, b"y" * 99 + b"z", b"y" * 99]).close()  # equal heads, different keys


def test_an_empty_vocabulary_finds_nothing():
    rc, h = _build_raw(b"", [0])
    assert rc == J.JB_OK
    J.lib().jb_vocab_free(h)
    h = C.c_void_p()
    assert J.lib().jb_vocab_build(None, None, 0, C.byref(h)) == J.JB_OK  # (no arrays at all)
    J.lib().jb_vocab_free(h)
    v = J.Vocab([])
    info = v.info()
    assert info["nkeys"] == 0 and info["maxlen"] == 0
    ns = info["nslots"]
    assert ns >= 1 and ns & (ns - 1) == 0
    for t in (b"a", b"", "中文", b"\xff", b"x" * 255, b"x" * 300):
        assert v.lookup(t) is None


def test_identity_and_near_misses():
    keys = V.identity_keys()
    d = V.key_dict(keys)
    assert len(d) == len(keys) == 200_064
    v = J.Vocab(keys)
    info = v.info()
    ns = info["nslots"]
    assert info["nkeys"] == len(keys) and info["maxlen"] == 255
    assert ns & (ns - 1) == 0 and ns >= 2 * len(keys)
    L, h, i = J.lib(), v.h, C.c_uint32()
    bad = [k for j, k in enumerate(keys)
           if L.jb_vocab_lookup(h, k, len(k), C.byref(i)) != 1 or i.value != j]
    assert not bad, (len(bad), bad[:3])
    miss = V.near_misses(keys)
    assert len(miss) == 200_000
    nfound = 0
    for t in miss:
        r = L.jb_vocab_lookup(h, t, len(t), C.byref(i))
        want = d.get(t, V.UNK)
        assert (i.value if r else V.UNK) == want and i.value == want, t
        nfound += r
    assert nfound < len(miss) // 20  # (near misses, not keys: a few one-byte ones are keys)
    v.close()


def test_maxlen_is_the_longest_key():
    for ks in ([b"a"], [b"ab", b"abcdefgh", b"xyz"], [b"x" * 24, b"y" * 25], [b"z" * 64, b"q"]):
        v = J.Vocab(ks)
        assert v.info()["maxlen"] == max(map(len, ks))
        for j, k in enumerate(ks):
            assert v.lookup(k) == j
            assert v.lookup(k + b"!") is None and v.lookup(k[:-1]) is None
