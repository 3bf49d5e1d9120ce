"""The extended-precision reference of the autocorrelation time (tests/autocorr_reference.py) and the inputs of
tests/test_gpu_autocorr_edges.py, checked on the host before any GPU sees them: the reference agrees with the NumPy
restatement of emcee's FFT estimator and with the AR(1) answer, and every input has what the GPU test relies on -- a
decision margin far above the tolerance, windows in the intended lag slabs, a ``c`` that puts the window where it is
meant to be."""
import numpy as np
import pytest

import autocorr_reference as R
from test_autocorr_host import ar1, oracle_autocorr

pytestmark = pytest.mark.skipif(not R.LD_OK, reason='np.longdouble is no wider than float64 here: eps = %.1e, the '
                                'reference needs eps < 1e-18' % np.finfo(np.longdouble).eps)

#: the AR(1) shapes of tests/test_gpu_autocorr.py
AR1_SHAPES = [(1000, 7, 3, 0.9, 5.), (999, 16, 1, 0.8, 5.), (50, 8, 2, 0.5, 5.), (3001, 9, 2, 0.9, 1.),
              (3001, 9, 2, 0.9, 10.), (20000, 8, 1, 0.98, 5.), (300, 70, 2, 0.99, 5.), (700, 5, 2, 0.5, -1.)]


def _fair(x, c):
    """The reference's result of a case, after the precondition of every case: no comparison is nearly a tie."""
    tau, window, margin = R.reference(x, c)
    assert margin >= R.MIN_MARGIN, margin
    return tau, window


@pytest.mark.parametrize('n_t,n_w,n_d,phi,c', AR1_SHAPES)
def test_reference_equals_the_fft_oracle(n_t, n_w, n_d, phi, c):
    x = ar1(n_t, n_w, n_d, phi, seed=n_t + n_w)
    tau, window = _fair(x, c)
    want, want_window = oracle_autocorr(x, c)
    assert R.tau_error(want, tau) <= 1e-12
    assert np.array_equal(window, want_window)


def test_reference_gives_the_ar1_answer():
    x = ar1(20000, 48, 2, 0.9, seed=1)
    tau, window, _ = R.reference(x)
    np.testing.assert_allclose(tau, 19., rtol=0.03)
    assert np.all(window >= 5 * tau - 1) and np.all(window <= 5 * tau + 5)


def test_one_and_two_steps():
    rng = np.random.default_rng(0)
    for c in (5., -1.):
        tau, window, _ = R.reference(rng.standard_normal((1, 4, 3)), c)      # one step: a constant series
        assert np.isnan(tau).all() and np.array_equal(window, [0, 0, 0])
        tau, window, margin = R.reference(rng.standard_normal((2, 4, 3)), c)  # y = (-h, h): f = (1, -1/2), taus (1, 0)
        assert np.array_equal(tau, [0., 0., 0.]) and np.array_equal(window, [1, 1, 1]) and margin == 1.


def test_constant_and_non_finite_series():
    x = R.plain_chain()
    tau, window = _fair(x, 5.)
    assert not np.isnan(tau).any() and np.all(window < len(x) - 1)
    w, d = R.NONFINITE_AT
    flat = x.copy()
    flat[:, w, d] = 2.5
    for y in [flat] + [R.nonfinite_chain(v, t) for v in R.NONFINITE_VALUES for t in R.NONFINITE_T]:
        assert not np.array_equal(y[:, w, d], x[:, w, d], equal_nan=True)
        got, got_window = _fair(y, 5.)
        assert np.isnan(got[d]) and got_window[d] == len(x) - 1
        keep = np.arange(x.shape[2]) != d
        assert np.array_equal(got[keep], tau[keep]) and np.array_equal(got_window[keep], window[keep])
    for k in R.SCALE_POWERS:        # (an exact scaling changes nothing in the reference either)
        got, got_window = _fair(x * 2. ** k, 5.)
        assert R.tau_error(got, tau) <= 1e-17 and np.array_equal(got_window, window)


def test_slab_of():
    edges = [0, 64, 128, 256, 512, 1024, 1536, 2048, 2560]
    for i, (lo, hi) in enumerate(zip(edges, edges[1:])):
        assert R.slab_of(lo) == i and R.slab_of(hi - 1) == i and R.slab_of(hi) == i + 1


def test_ar1_phis():
    x = R.ar1_phis(50, 3, (0.3, 0.9), seed=5)
    assert x.shape == (50, 3, 2) and np.array_equal(x, R.ar1_phis(50, 3, (0.3, 0.9), seed=5))
    assert np.array_equal(x[:, :, :1], ar1(50, 3, 1, 0.3, 5)) and np.array_equal(x[:, :, 1:], ar1(50, 3, 1, 0.9, 1005))


# --- the inputs of the GPU test ----------------------------------------------------------------------------------
@pytest.mark.parametrize('n_t', R.SHORT_NT)
def test_short_chains(n_t):
    x = R.short_chain(n_t)
    assert x.shape == (n_t, 5, 2)
    for c in R.SHORT_C:
        tau, window = _fair(x, c)
        if n_t == 1:
            assert np.isnan(tau).all() and np.all(window == 0)
        elif c < 0:     # every lag: the whole sum, which is 0 but for rounding
            assert np.all(window == n_t - 1) and np.all(np.abs(tau) < 1e-15)
        else:
            assert not np.isnan(tau).any()


@pytest.mark.parametrize('n_w,n_d', R.TILING)
def test_tiling_chains(n_w, n_d):
    x = R.tiling_chain(n_w, n_d)
    assert x.shape == (R.TILING_NT, n_w, n_d)
    _, window = _fair(x, 5.)
    slabs = {R.slab_of(k) for k in window}
    assert np.all(window < R.TILING_NT - 1) and (slabs == {0, 1} if n_d > 1 else slabs <= {0, 1}), window
    assert sorted(n_w * n_d for n_w, n_d in R.TILING) == [1, 63, 64, 65, 128, 129]


def test_boundary_windows():
    x = R.boundary_chain()
    assert x.shape == (2600, 4, 1)
    _, window = _fair(x, 5.)
    assert R.slab_of(window[0]) == 5       # (1063 at BOUNDARY_SEED)
    assert sorted(R.BOUNDARY_WINDOWS) == sorted({b + s for b in (64, 128, 256, 512, 1024, 1536) for s in (-1, 0, 1)})
    taus = []
    for k in R.BOUNDARY_WINDOWS:
        tau, window = _fair(x, R.c_for_window(x, 0, k))
        assert window[0] == k
        taus.append(tau[0])
    assert len(set(taus)) == len(taus)      # 18 different prefix sums
    with pytest.raises(ValueError):
        R.c_for_window(R.short_chain(9), 0, 8)   # taus[8] is 0 but for rounding, and an earlier lag fails first


@pytest.mark.parametrize('n_t', R.CAPPED_NT)
def test_capped_chains(n_t):
    x = R.capped_chain(n_t)
    assert x.shape == (n_t, 3, 1)
    tau, window = _fair(x, -1.)
    assert window[0] == n_t - 1 and R.slab_of(n_t - 1) >= 4 and abs(tau[0]) < 1e-15


def test_mixed_chains():
    x, r = R.mixed_chain(), R.mixed_chain(reverse=True)
    assert x.shape == (4000, 6, 4) and np.array_equal(r, x[:, :, ::-1])
    tau, window = _fair(x, 5.)
    assert [R.slab_of(k) for k in window] == [0, 1, 2, 4], window
    rtau, rwindow = _fair(r, 5.)
    assert np.array_equal(rtau, tau[::-1]) and np.array_equal(rwindow, window[::-1])


def test_conditioning_chains():
    base = R.conditioning_chain(0., 1.)
    tau, window = _fair(base, 5.)
    for offset, scale in (R.CONDITIONING_REAL,) + R.CONDITIONING_MEASURED:
        x = R.conditioning_chain(offset, scale)
        assert x.shape == (3000, 8, 2)
        got, got_window, margin = R.reference(x, 5.)
        # the column is the centred one but for the rounding of offset + scale * ar1 to float64, which moves tau by
        # something of the order of ulp(offset) / scale
        assert R.tau_error(got, tau) <= 100. * np.spacing(offset) / scale and np.array_equal(got_window, window)
        err = R.tau_error(oracle_autocorr(x, 5.)[0], got)
        print('offset %g scale %g: margin %.2e, float64 FFT oracle against the reference %.2e' %
              (offset, scale, margin, err))
        assert margin >= R.MIN_MARGIN
        if (offset, scale) == R.CONDITIONING_REAL:
            assert err <= R.TAU_TOL     # (emcee's own arithmetic meets the tolerance on the column of a real fit)
