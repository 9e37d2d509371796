"""Reference for the document-frequency and IDF calls (jb_df_device, jb_idf, jb_idf_device; jiebahip.h):
np.bincount over the flat term list, and the IDF rule in Python with the library's restatement of Go's
math.Log (jiebahip.go_log) and numpy's float32 narrowing.  A helper, not a test."""
import numpy as np

import jiebahip as J

NOMAX = 0xFFFFFFFF


def df(term_id, nterms, cap, ndf):
    """u32[ndf]: how many of the entries term_id[:min(nterms, cap)] carry each id < ndf."""
    x = np.asarray(term_id, np.uint32)[:min(int(nterms), int(cap))].astype(np.int64)
    return np.bincount(x[x < ndf], minlength=ndf).astype(np.uint32)


def smoothed(df, ndocs):
    """f32[len(df)], no filter: float32(go_log((ndocs + 1) / (df + 1)) + 1).  The sums are exact integers;
    the divide, the add and the narrowing are each rounded once (Python's float is the f64 of the C rule)."""
    u, inv = np.unique(np.asarray(df, np.uint32), return_inverse=True)
    num = float(int(ndocs) + 1)
    vals = np.array([np.float32(J.go_log(num / float(f + 1)) + 1.0) for f in u.tolist()], np.float32)
    return vals[inv]


def idf(df, ndocs, min_df=1, max_df=NOMAX, keep=None, base=None):
    """f32[len(df)]: 0 where df is 0, below min_df, above max_df (NOMAX: no upper bound) or where keep is 0;
    smoothed(df, ndocs) elsewhere (base: that array, when the caller already has it)."""
    df = np.asarray(df, np.uint32)
    w = np.array(smoothed(df, ndocs) if base is None else base, np.float32)
    zero = (df == 0) | (df < min_df) | (df > max_df)
    if keep is not None:
        zero |= np.asarray(keep) == 0
    w[zero] = 0.0
    return w
