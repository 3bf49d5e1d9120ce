"""An extended-precision reference of emcee's integrated autocorrelation time, and the inputs of
tests/test_gpu_autocorr_edges.py (tests/test_autocorr_reference_host.py checks both without a GPU).

The reference restates the estimator by direct sums in np.longdouble, with no FFT.  Per parameter: ``y = x - mean(x)``
of every walker, ``acf_w[k] = sum_t y_t y_{t+k}``, ``f[k] = mean_w(acf_w[k] / acf_w[0])``, ``taus = 2 cumsum(f) - 1``,
``window = argmin(k < c taus)`` if any is true, else ``n_t - 1``, and ``tau = taus[window]``.  Lags are computed one at
a time and only up to the one that decides the window.  The mean is taken of ``x - x_0`` (in np.longdouble that
difference is exact for the columns used here), so a large offset costs the reference nothing.

Beside ``tau`` and ``window`` the reference returns the **decision margin** ``min_k |k - c taus[k]| / max(1, k)`` over
the lags it examined: an exact window is a fair demand of the device only where no comparison ``k < c taus[k]`` is
nearly a tie, and every case asserts that before it looks at the device."""
import numpy as np

from helpers import LD, LD_OK
from test_autocorr_host import ar1, oracle_autocorr

TAU_TOL = 1e-10        # |tau - want| <= TAU_TOL max(|want|, 1), the bound of tests/test_gpu_autocorr.py
MIN_MARGIN = 1e-6      # the smallest decision margin at which the window is compared exactly

# the device's lag slabs (csrc/lcf_autocorr.hip): [0, 64) [64, 128) [128, 256) [256, 512) [512, 1024), then 512 wide
SLAB_FIRST, SLAB_MAX = 64, 512


def slab_of(k):
    """Index of the lag slab that holds lag ``k``: 0 for [0, 64), 1 for [64, 128), ... 5 for [1024, 1536), ..."""
    lo, width, i = 0, SLAB_FIRST, 0
    while k >= lo + width:
        lo += width
        width = min(lo, SLAB_MAX)
        i += 1
    return i


class Reference:
    """The estimator on one chain (n_t, n_w, n_d); the normalised autocorrelations are kept, so several ``c`` on one
    chain cost no more than the largest window among them."""

    def __init__(self, x):
        x = np.asarray(x, dtype=np.float64)
        assert x.ndim == 3 and x.shape[0] >= 1
        self.x = x
        self.n_t, self.n_w, self.n_d = x.shape
        # a series that is constant or holds a non-finite value: its parameter is NaN with window n_t - 1
        self.bad = (~np.isfinite(x).all(axis=0) | (x == x[0]).all(axis=0)).any(axis=0)
        self._y, self._a0, self._taus = {}, {}, {d: [] for d in range(self.n_d)}

    def taus(self, d, n):
        """``taus[0:n]`` of parameter ``d``, np.longdouble."""
        return np.array(self._extend(d, n)[:n], dtype=LD)

    def _extend(self, d, n):
        assert not self.bad[d] and n <= self.n_t
        if d not in self._y:
            r = self.x[:, :, d].astype(LD) - self.x[0, :, d].astype(LD)
            self._y[d] = r - r.sum(axis=0) / LD(self.n_t)
            self._a0[d] = (self._y[d] * self._y[d]).sum(axis=0)
        y, a0, t = self._y[d], self._a0[d], self._taus[d]
        for k in range(len(t), n):
            f = ((y[:self.n_t - k] * y[k:]).sum(axis=0) / a0).sum() / LD(self.n_w)
            t.append((t[-1] if t else LD(-1)) + 2 * f)
        return t

    def _one(self, d, c):
        n_t, c = self.n_t, LD(c)
        any_true, first_false, margin = False, -1, np.inf
        for k in range(n_t):
            t = self._extend(d, k + 1)[k]
            margin = min(margin, float(abs(k - c * t) / max(1, k)))
            if k < c * t:
                any_true = True
            elif first_false < 0:
                first_false = k
            if any_true and first_false >= 0:     # (the window is decided: argmin of m is the first false)
                break
        window = (first_false if first_false >= 0 else 0) if any_true else n_t - 1
        return float(self._extend(d, window + 1)[window]), window, margin

    def result(self, c=5.):
        """``(tau[n_d], window[n_d], margin)``; the margin is the smallest over the parameters that have one."""
        tau, window, margin = np.full(self.n_d, np.nan), np.full(self.n_d, self.n_t - 1, dtype=np.int64), np.inf
        for d in np.nonzero(~self.bad)[0]:
            tau[d], window[d], m = self._one(d, c)
            margin = min(margin, m)
        return tau, window, margin


_refs = {}


def reference_of(x):
    """The :class:`Reference` of a chain, built once per array object (the inputs below are built once, too)."""
    if isinstance(x, Reference):
        return x
    if id(x) not in _refs:
        _refs[id(x)] = (x, Reference(x))      # (the array is held, so its id stays its own)
    return _refs[id(x)][1]


def reference(x, c=5.):
    """``(tau, window, margin)`` of the chain ``x`` (n_t, n_w, n_d) in np.longdouble arithmetic."""
    return reference_of(x).result(c)


def expected(x, c=5.):
    """What the device is compared with: the reference, or the float64 oracle where np.longdouble is float64 (the
    margin is the reference's either way)."""
    tau, window, margin = reference(x, c)
    if not LD_OK:
        tau, window = oracle_autocorr(np.asarray(x, dtype=np.float64), c)
    return tau, window, margin


def tau_error(tau, want):
    """Largest ``|tau - want| / max(|want|, 1)``; NaNs must coincide."""
    tau, want = np.asarray(tau, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert tau.shape == want.shape and np.array_equal(np.isnan(tau), np.isnan(want)), (tau, want)
    ok = ~np.isnan(want)
    return float(np.max(np.abs(tau[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1.), initial=0.))


def ar1_phis(n_t, n_w, phis, seed):
    """An AR(1) chain (n_t, n_w, len(phis)) with its own ``phi`` per parameter."""
    return np.concatenate([ar1(n_t, n_w, 1, phi, seed + 1000 * d) for d, phi in enumerate(phis)], axis=2)


def c_for_window(x, d, k):
    """A ``c`` for which the reference's window of parameter ``d`` is exactly ``k``.  Lag ``k`` must be the first to
    fail ``k < c taus[k]``, so ``(k - 1) / taus[k - 1] < c <= k / taus[k]``.  ``(k - 0.5) / taus[k]`` is tried first;
    it lies below that interval where ``taus`` still grows fast at ``k``, and then the interval's middle is taken.
    The reference confirms the window (the lags before ``k - 1`` have a say, too); ValueError if it is another."""
    ref = reference_of(x)
    assert 1 <= k < ref.n_t
    t = ref.taus(d, k + 1)
    lower, upper = (k - 1) / t[k - 1], k / t[k]
    c = (k - LD(0.5)) / t[k]
    if not lower < c:
        c = (lower + upper) / 2
    c = float(c)
    window = ref.result(c)[1]
    if window[d] != k:
        raise ValueError('no c puts the window of parameter %d at lag %d (c = %g gives %d)' % (d, k, c, window[d]))
    return c


# --- the inputs of tests/test_gpu_autocorr_edges.py ------------------------------------------------------------------
_built = {}


def _once(key, make):
    if key not in _built:
        _built[key] = make()
    return _built[key]


#: fewer steps than t-chunks (8), around the register window (16), at the first slabs' ends (64, 128)
SHORT_NT = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
SHORT_C = (5., -1.)     # (c = -1: no lag passes the window rule, so every lag is computed and window = n_t - 1)


def short_chain(n_t):
    return _once(('short', n_t), lambda: ar1(n_t, 5, 2, 0.5, seed=40 + n_t))


#: (n_w, n_d) for 1, 63, 64, 65, 128 and 129 series, at n_t = 200; every parameter its own phi, so that the rows of a
#: tile are decided in different slabs
TILING = ((1, 1), (21, 3), (64, 1), (13, 5), (32, 4), (43, 3))
TILING_NT = 200
TILING_PHIS = (0.97, 0.3, 0.9, 0.6, 0.95)


def tiling_chain(n_w, n_d):
    return _once(('tiling', n_w, n_d), lambda: ar1_phis(TILING_NT, n_w, TILING_PHIS[:n_d], seed=7 + n_w))


#: windows placed on both sides of every slab boundary of one chain (and its window at c = 5)
BOUNDARIES = (64, 128, 256, 512, 1024, 1536)
BOUNDARY_WINDOWS = tuple(b + s for b in BOUNDARIES for s in (-1, 0, 1))
BOUNDARY_SEED = 2


def boundary_chain():
    return _once('boundary', lambda: ar1(2600, 4, 1, 0.995, seed=BOUNDARY_SEED))


#: every lag (c = -1) of chains that end in, at the end of and just behind a 512-wide slab
CAPPED_NT = (1024, 1025, 1536, 1537, 2100)


def capped_chain(n_t):
    return _once(('capped', n_t), lambda: ar1(n_t, 3, 1, 0.9, seed=n_t))


#: four parameters of one call whose windows lie in four different slabs, in both orders
MIXED_PHIS = (0.3, 0.9, 0.97, 0.99)
MIXED_SEED = 8


def mixed_chain(reverse=False):
    """phi per parameter as in MIXED_PHIS; ``reverse``: the same columns in the opposite order."""
    if reverse:
        return _once(('mixed', True), lambda: np.ascontiguousarray(mixed_chain()[:, :, ::-1]))
    return _once(('mixed', False), lambda: ar1_phis(4000, 6, MIXED_PHIS, seed=MIXED_SEED))


#: (offset, scale) of columns offset + scale * ar1: an explosion time in MJD, and two that nobody fits
CONDITIONING_REAL = (58000.3, 0.05)
CONDITIONING_MEASURED = ((1e6, 1e-3), (1e9, 1e-3))


def conditioning_chain(offset, scale):
    return _once(('conditioning', offset, scale), lambda: offset + scale * ar1(3000, 8, 2, 0.9, seed=21))


#: a non-finite value in walker 2 of parameter 1, at these steps
NONFINITE_VALUES = (np.nan, np.inf, -np.inf)
NONFINITE_T = (0, 150)
NONFINITE_AT = (2, 1)
SCALE_POWERS = (-100, 100)


def plain_chain():
    return _once('plain', lambda: ar1_phis(300, 5, (0.5, 0.8, 0.9), seed=31))


def nonfinite_chain(value, t):
    def make():
        x = plain_chain().copy()
        x[(t,) + NONFINITE_AT] = value
        return x
    return _once(('nonfinite', repr(value), t), make)
