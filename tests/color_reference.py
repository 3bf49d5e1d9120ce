"""The NumPy definition of what color_predictive returns, on given model values Y[f, t, s] (filters x times x samples):
colours, their percentiles and valid counts, and first-occurrence peaks.  The device is held to this; the helper itself
is checked against a brute-force loop in tests/test_color_host.py."""
import warnings

import numpy as np


def colors(Y, pairs, dzp):
    """C[c, t, s] = dzp[c] - 2.5 log10(Y[a] / Y[b]) where both values are finite and > 0, else NaN."""
    Y = np.asarray(Y, dtype=np.float64)
    out = np.full((len(pairs),) + Y.shape[1:], np.nan)
    for c, (a, b) in enumerate(pairs):
        ya, yb = Y[a], Y[b]
        ok = np.isfinite(ya) & np.isfinite(yb) & (ya > 0.) & (yb > 0.)
        ratio = np.divide(ya, yb, out=np.ones_like(ya), where=ok)
        out[c] = np.where(ok, dzp[c] - 2.5 * np.log10(ratio), np.nan)
    return out


def color_bands(Y, pairs, dzp, percentiles):
    """``(color[q, c, t], n_valid[c, t])``: np.nanpercentile of the colours over the samples, NaN where none has one."""
    C = colors(Y, pairs, dzp)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)   # (all-NaN slices: NaN)
        bands = np.nanpercentile(C, np.asarray(percentiles, dtype=np.float64), axis=-1)
    return bands, np.sum(~np.isnan(C), axis=-1)


def peaks(Y):
    """``(y_peak[s, f], peak_index[s, f])``: the largest non-NaN Y[f, :, s] and the first time index it is attained at
    (strict >, in index order); NaN and -1 where every value is NaN."""
    Y = np.asarray(Y, dtype=np.float64)
    valid = ~np.isnan(Y)
    none = ~np.any(valid, axis=1)                             # (f, s)
    top = np.max(np.where(valid, Y, -np.inf), axis=1, keepdims=True)
    index = np.argmax(valid & (Y == top), axis=1)             # the first occurrence of the maximum
    y = np.take_along_axis(Y, index[:, None, :], axis=1)[:, 0, :]
    y = np.where(none, np.nan, y)
    index = np.where(none, -1, index).astype(np.int32)
    return y.T.copy(), index.T.copy()
