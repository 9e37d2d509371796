"""CPU: jb_idf, the host form of the IDF rule, against df_ref.idf bit for bit (as u32 views), and the
argument checks of the document-frequency calls.  No kernel is launched here."""
import itertools

import numpy as np
import pytest

import df_ref as DR
import jiebahip as J

NEW = ["jb_df_device", "jb_idf_device", "jb_idf", "jb_df_batch"]

# every value 0..65535 and the three large ones (df + 1 must not wrap, df = 2^32 - 1 is above every max_df but NOMAX)
DF = np.concatenate([np.arange(65536, dtype=np.uint32), np.array([2**31, 2**32 - 2, 2**32 - 1], np.uint32)])
NDOCS = [0, 1, 2, 73_443, 2**32 + 5, 2**53 - 2]
MIN_DF = [0, 1, 2, 1000]
MAX_DF = [J.JB_DF_NOMAX, 0, 5]
KEEP = {"null": None, "zero": np.zeros(len(DF), np.uint8), "alternating": (np.arange(len(DF)) & 1).astype(np.uint8)}


def raw_idf(df, ndf, ndocs, min_df, max_df, keep, out):
    """jb_idf itself, its return code included (out: a float32 array or None)."""
    return J.lib().jb_idf(df.ctypes.data if df is not None else None, ndf, ndocs, min_df, max_df,
                          keep.ctypes.data if keep is not None else None, out.ctypes.data if out is not None else None)


def test_exports():
    L = J.lib()
    for name in NEW:
        assert name in J.EXPORTS and hasattr(L, name), name
    assert J.JB_DF_NOMAX == DR.NOMAX == 0xFFFFFFFF


@pytest.mark.parametrize("ndocs", NDOCS)
def test_idf_matches_the_reference_bit_for_bit(ndocs):
    base = DR.smoothed(DF, ndocs)  # (the unfiltered weights, once per ndocs)
    assert np.isfinite(base).all()
    for min_df, max_df, kname in itertools.product(MIN_DF, MAX_DF, KEEP):
        keep = KEEP[kname]
        want = DR.idf(DF, ndocs, min_df, max_df, keep, base=base)
        out = np.full(len(DF) + 8, np.nan, np.float32)  # every slot is written, and none after them
        assert raw_idf(DF, len(DF), ndocs, min_df, max_df, keep, out) == J.JB_OK
        label = (ndocs, min_df, max_df, kname)
        assert np.isnan(out[len(DF):]).all(), label
        got = out[:len(DF)]
        assert not np.isnan(got).any(), label
        if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            raise AssertionError(f"{label}: {len(bad)} weights differ; first df={DF[bad[0]]}: got {got[bad[0]]!r} "
                                 f"want {want[bad[0]]!r}")
        # the wrapper is the same call
        assert np.array_equal(J.idf(DF, ndocs, min_df, None if max_df == J.JB_DF_NOMAX else max_df, keep).view(np.uint32),
                              want.view(np.uint32)), label


def test_the_rule_by_hand():
    # 3 documents; df 0 -> 0; df 1 -> ln(4/2) + 1; df 3 -> ln(4/4) + 1 = 1; df 7 > ndocs -> ln(4/8) + 1, no clamp
    w = J.idf(np.array([0, 1, 3, 7], np.uint32), 3)
    assert w[0] == 0.0 and w[2] == 1.0
    assert w[1] == np.float32(np.log(2.0) + 1.0) and w[3] == np.float32(1.0 - np.log(2.0))
    # filters: min_df 2 drops df 1, max_df 3 drops df 7, keep drops id 2
    w = J.idf(np.array([0, 1, 3, 7], np.uint32), 3, min_df=2, max_df=3, keep=[1, 1, 0, 1])
    assert w.tolist() == [0.0, 0.0, 0.0, 0.0]
    w = J.idf(np.array([0, 1, 3, 7], np.uint32), 3, min_df=2, max_df=3)
    assert w.tolist() == [0.0, 0.0, 1.0, 0.0]
    # a negative weight comes out as it is (downstream it is no candidate)
    assert J.idf(np.array([2**32 - 1], np.uint32), 0)[0] == np.float32(1.0 - 32 * np.log(2.0)) < 0


def test_error_codes_and_no_ids():
    one = np.ones(4, np.uint32)
    out = np.full(4, np.nan, np.float32)
    assert raw_idf(one, 4, 2**53, 1, J.JB_DF_NOMAX, None, out) == J.JB_ELIMIT
    assert "2^53" in J.lib().jb_last_error().decode() and np.isnan(out).all()
    assert raw_idf(one, 4, 2**53 - 1, 1, J.JB_DF_NOMAX, None, out) == J.JB_OK
    out[:] = np.nan
    assert raw_idf(None, 4, 3, 1, J.JB_DF_NOMAX, None, out) == J.JB_EINVAL
    assert "df" in J.lib().jb_last_error().decode()
    assert raw_idf(one, 4, 3, 1, J.JB_DF_NOMAX, None, None) == J.JB_EINVAL
    assert "weight" in J.lib().jb_last_error().decode() and np.isnan(out).all()
    # ndf = 0: valid, nothing is written (with or without pointers)
    assert raw_idf(one, 0, 3, 1, J.JB_DF_NOMAX, None, out) == J.JB_OK and np.isnan(out).all()
    assert raw_idf(None, 0, 3, 1, J.JB_DF_NOMAX, None, None) == J.JB_OK
    assert len(J.idf(np.zeros(0, np.uint32), 5)) == 0
    with pytest.raises(J.JbError) as ei:
        J.idf(one, 2**53)
    assert ei.value.code == J.JB_ELIMIT


def test_null_arguments_of_the_device_calls():
    L = J.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    # (a null ctx: nothing can be queued)
    assert L.jb_df_device(None, p, p, 1, p, 1, None) == J.JB_EINVAL
    assert "null" in L.jb_last_error().decode()
    assert L.jb_idf_device(None, p, 1, 1, 1, J.JB_DF_NOMAX, None, None, p) == J.JB_EINVAL
    assert L.jb_df_batch(None, p, p, 1, 1, p, 1) == J.JB_EINVAL
