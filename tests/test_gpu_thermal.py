"""thermal_predictive on the device against the CPU oracle + NumPy: T and R are the oracle's temperature_radius of the
very samples the call used, L its stefan_boltzmann of each pair, want = np.nanpercentile(..., axis=samples).

Tolerances: TOL = 1e-11 for T and R, the project's bound for single evaluations (tests/test_gpu_parity.py); order
statistics and their convex combinations inherit it.  6 TOL for L: T enters to the fourth power and R squared.  relerr
also demands identical NaN patterns.  Every count is compared exactly -- which is only meaningful where no oracle
temperature lies within 1e-9 (relative) of the floor and no grid time within 1e-9 of a window bound: the tests that
compare counts with the oracle assert that first."""
import numpy as np
import pytest

from conftest import relerr
from lightcurve_fitting_amd import bolometric as B, models as M
from lightcurve_fitting_amd.fitting import thermal_predictive
from helpers import config2_case
from oracle import lcf_oracle as O
from test_gpu_predictive import SEVEN, _companion_rows, _fit, _lc, _one_sample_cases, _rows

pytestmark = pytest.mark.gpu

TOL = 1e-11
FLOOR = 8.12
FIELDS = ('temperature', 'radius', 'luminosity', 'n_valid', 'n_cold', 'n_inside')


def _window(m, P):
    """(t_min, t_max) of every row from the package's host methods (kappa = 1); no lower bound: -inf."""
    with np.errstate(all='ignore'):
        lo, hi = m.t_min(P.T), m.t_max(P.T)
    if lo is NotImplemented:
        lo = np.full(len(P), -np.inf)
    return np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)


def _clear_of(times, bounds, eps=1e-9):
    """No time within eps (relative) of a finite bound."""
    b = bounds[np.isfinite(bounds)]
    return bool(np.all(np.abs(times[:, None] - b) > eps * np.abs(b)))


def _check(res, T, R, m=None, P=None, tol=(TOL, TOL, 6 * TOL), floor_eps=1e-9, stefan_boltzmann=O.stefan_boltzmann):
    """T, R: (nt, S) reference values.  With (m, P): n_inside against the package's t_min / t_max."""
    T, R = np.asarray(T).reshape(len(res.t), -1), np.asarray(R).reshape(len(res.t), -1)
    with np.errstate(all='ignore'):
        L = stefan_boltzmann(T, R)
        want = [np.nanpercentile(X, res.percentiles, axis=-1) for X in (T, R, L)]
    for name, got, w, bound in zip('TRL', (res.temperature, res.radius, res.luminosity), want, tol):
        err = relerr(got, w)
        print(f'thermal_predictive {name} vs reference + nanpercentile: max rel err {err:.3e} over {got.shape}')
        assert err <= bound, name
    assert np.array_equal(res.n_valid, [np.sum(~np.isnan(X), axis=-1) for X in (T, R, L)])
    assert np.all(np.abs(T / FLOOR - 1.) > floor_eps)
    assert np.array_equal(res.n_cold, np.sum(T < FLOOR, axis=-1))
    if m is not None:
        lo, hi = _window(m, P)
        assert _clear_of(res.t, lo) and _clear_of(res.t, hi)
        assert np.array_equal(res.n_inside, np.sum((lo <= res.t[:, None]) & (res.t[:, None] <= hi), axis=-1))
    return want


@pytest.fixture(scope='module')
def case_4096():
    """4096 rows x 50 times x 7 percentiles, the call with the default workspace and the oracle's T, R."""
    P = _rows(4096)
    m = M.ShockCooling(redshift=0.01)
    res = thermal_predictive(_lc(), m, P, percentiles=SEVEN, num=50)
    T, R = O.ShockCoolingOracle(0.01).temperature_radius(res.t, *P.T)
    return P, m, res, T, R


def test_shockcooling_4096_rows_seven_percentiles(case_4096):
    """More samples than the 2048 keys a search sorts and than one 512-lane trip: refinement and the sample loop run."""
    P, m, res, T, R = case_4096
    assert res.temperature.shape == res.radius.shape == res.luminosity.shape == (7, 50)
    assert res.n_valid.shape == (3, 50) and res.n_cold.shape == res.n_inside.shape == (50,) and res.n_samples == 4096
    assert np.array_equal(res.t, np.linspace(0.3, 12., 50)) and np.array_equal(res.percentiles, SEVEN)
    _check(res, T, R, m, P)
    for X in (res.temperature, res.radius, res.luminosity):
        assert np.all(np.diff(X, axis=0) >= 0.)
    # both counters are exercised away from 0 and from n
    assert res.n_cold.min() == 0 and 2048 < res.n_cold.max() < 4096
    assert 0 < res.n_inside[0] < 4096 and res.n_inside.max() == 4096 and 0 < res.n_inside[-1] < 4096
    assert np.array_equal(res.frac_cold, res.n_cold / 4096) and np.array_equal(res.frac_inside, res.n_inside / 4096)


def test_ties_at_exact_zero():
    """Before its t_0 a sample's T, R and L are exactly 0 (the reference's power()): at 0.1 d the second group's k rows
    tie, and every one of them is cold."""
    S = 4096
    rng = np.random.default_rng(7)
    P = _rows(S, seed=8)
    second = np.arange(S) >= int(0.6 * S)
    P[:, 4] = np.where(second, rng.uniform(0.12, 0.14, S), rng.uniform(0.07, 0.09, S))
    P = P[rng.permutation(S)]
    k = int(np.sum(P[:, 4] > 0.1))
    assert k == S - int(0.6 * S)
    times = np.array([0.05, 0.1, 0.2])
    T, R = O.ShockCoolingOracle(0.01).temperature_radius(times, *P.T)
    L = O.stefan_boltzmann(T, R)
    inside, edge = 100. * (k // 2) / (S - 1), 100. * (k - 0.5) / (S - 1)
    m = M.ShockCooling(redshift=0.01)
    res = thermal_predictive(_lc(), m, P, percentiles=[0., inside, edge, 50., 84.14, 100.], t=times)
    assert res.n_cold[0] == S and res.n_cold[1] >= k
    for got, Y in ((res.temperature, T), (res.radius, R), (res.luminosity, L)):
        assert np.all(Y[0] == 0.) and np.sum(Y[1] == 0.) == k and np.all(Y[2] > 0.)
        assert np.all(got[:, 0] == 0.)                      # every sample is 0 at 0.05 d
        assert got[1, 1] == 0.                               # inside the tie
        smallest = np.min(Y[1][Y[1] > 0.])
        assert relerr(got[2:3, 1], [0.5 * smallest]) <= 6 * TOL  # half way from the last zero to the first value
    _check(res, T, R, m, P)


def _oracle_tr(name, orc, times, P):
    """The oracle's (T, R), (nt, S), for rows P of the model `name` of _one_sample_cases."""
    cols = P.T
    if name == 'ShockCooling2':
        return orc[1].temperature_radius2(times, *cols)
    if name == 'ShockCooling3':      # ShockCooling's T and R of (v_s, M_env, f_rho M, R, t_0)
        return orc[1].temperature_radius(times, *cols[[0, 1, 2, 3, 6]])
    if name == 'CompanionShocking':  # the shock component's
        return O.kasen_temperature_radius(times, *cols[:3])
    return orc[1].temperature_radius(times, *cols)


def test_one_sample_every_model():
    """With one sample no interpolation happens: all percentiles are the value itself, the counts are 0 or 1."""
    times = np.linspace(0.3, 12., 23)
    for name, m, orc, p in _one_sample_cases():
        res = thermal_predictive(_lc(), m, p[None, :], percentiles=(0., 15.87, 50., 100.), t=times)
        for X in (res.temperature, res.radius, res.luminosity):
            assert np.all(X == X[0]), name
        assert np.all(res.n_valid == 1) and res.n_samples == 1, name
        assert set(np.unique(res.n_cold)) <= {0, 1} and set(np.unique(res.n_inside)) <= {0, 1}, name
        T, R = _oracle_tr(name, orc, times, p[None, :])
        print(name, end=': ')
        _check(res, T, R, m, p[None, :])


def _window_cases():
    g, lc2 = config2_case()
    rng = np.random.default_rng(21)
    sc = O.ShockCoolingOracle(0.01)
    yield ('ShockCooling2', M.ShockCooling2(redshift=0.01), ('ShockCooling2', sc),
           np.array([20., 3., 20., 0.1]) * (1. + 0.2 * rng.uniform(-1., 1., (512, 4))))
    yield 'ShockCooling4', M.ShockCooling4(redshift=0.01), ('ShockCooling4', O.ShockCooling4Oracle(0.01)), _rows(512, seed=5)
    yield 'CompanionShocking', M.CompanionShocking(lc2, redshift=0.003), None, _companion_rows(512, 1)


def test_windows_of_the_other_models():
    """n_inside of the models whose window is not ShockCooling's.  The times lie strictly between the smallest and the
    largest t_min, and between the smallest and the largest t_max, of the rows: every count is then neither 0 nor n."""
    for name, m, orc, P in _window_cases():
        lo, hi = _window(m, P)
        assert np.all(np.isfinite(hi)) and (name == 'ShockCooling2') == bool(np.all(lo == -np.inf))
        times = np.linspace(hi.min(), hi.max(), 9)[1:-1]
        if name != 'ShockCooling2':
            assert lo.max() < hi.min()
            times = np.concatenate([np.linspace(lo.min(), lo.max(), 9)[1:-1], times])
        res = thermal_predictive(_lc(), m, P, t=times)
        T, R = _oracle_tr(name, orc, times, P)
        print(name, end=': ')
        _check(res, T, R, m, P)
        assert 0 < res.n_inside.min() and res.n_inside.max() < 512 and len(np.unique(res.n_inside)) > 4, name


def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in FIELDS)


@pytest.mark.parametrize('use_sigma', [False, True])
def test_sampler_in_place_equals_the_array_form(use_sigma):
    lc, m, s = _fit(64, 40, use_sigma)
    assert len(s._chain_host) == 0 and s._chain_on_device == 40           # read where it lies
    a = thermal_predictive(lc, m, s, discard=7, thin=3, num=30, use_sigma=use_sigma)
    assert len(s._chain_host) == 0 and s._chain_on_device == 40           # ... and it still lies there
    flat = s.get_chain(discard=7, thin=3, flat=True)
    assert a.n_samples == len(flat) == 11 * 64
    b = thermal_predictive(lc, m, flat, num=30, use_sigma=use_sigma)
    assert _same(a, b)
    T, R = O.ShockCoolingOracle(0.).temperature_radius(a.t, *flat[:, :5].T)
    _check(a, T, R, m, flat[:, :5])
    s.run_mcmc(None, 10)                                                   # the chain is now partly on the host
    c = thermal_predictive(lc, m, s, discard=7, thin=3, num=30, use_sigma=use_sigma)
    d = thermal_predictive(lc, m, s.get_chain(discard=7, thin=3, flat=True), num=30, use_sigma=use_sigma)
    assert c.n_samples == 15 * 64 and _same(c, d)
    with pytest.raises(ValueError, match='columns'):
        thermal_predictive(lc, m, s, use_sigma=not use_sigma)


def test_tiling_and_determinism(case_4096):
    P, m, one, _, _ = case_4096
    # seven percentiles x three series keep 21 * 2048 keys of 8 bytes per time: 2 MiB hold four of the 50 times
    tiled = thermal_predictive(_lc(), m, P, percentiles=SEVEN, num=50, workspace_bytes=2 << 20)
    two = thermal_predictive(_lc(), m, P, percentiles=SEVEN, num=50)
    assert _same(one, two) and _same(one, tiled)
    with pytest.raises(Exception, match='workspace_bytes too small'):
        thermal_predictive(_lc(), m, P, percentiles=SEVEN, num=50, workspace_bytes=1 << 16)


def test_repeated_times_and_many_percentiles():
    """Times the caller repeats, or gives out of order, come back where they were given; more percentiles than one
    native call takes (170) are split over several."""
    P = _rows(300, seed=2)
    m = M.ShockCooling(redshift=0.01)
    times = np.array([5., 0.6, 5., 2.5])
    q = np.linspace(0., 100., 173)
    res = thermal_predictive(_lc(), m, P, percentiles=q, t=times)
    assert res.temperature.shape == (173, 4) and np.array_equal(res.t, times)
    T, R = O.ShockCoolingOracle(0.01).temperature_radius(times, *P.T)
    _check(res, T, R, m, P)
    assert np.array_equal(res.temperature[:, 0], res.temperature[:, 2]) and res.n_cold[0] == res.n_cold[2]


def test_every_pass_loops_and_refines_more_than_once():
    """S = 1024 x 100 rows of a fit on 100 times: every pass loops over samples and a bin of the first histogram holds
    far more keys than a search sorts.  Against the package's own temperature_radius in slices + np.nanpercentile (the
    oracle is too slow here): both sides are within 1e-11 of the oracle, so they are held to 2e-11 of each other, L
    included (it is the same product of the same T and R on both sides).  The counts are NumPy's on those same values:
    the temperatures are the device's own, so n_cold needs no margin about the floor; and as a fit's 1e7 (row, time)
    pairs cannot all be 1e-9 clear of a window bound, the times only have to be 1e-12 clear here -- a thousand
    roundings of the bound's arithmetic."""
    lc, m, s = _fit(1024, 100)
    res = thermal_predictive(lc, m, s, num=100)
    flat = s.get_chain(flat=True)
    assert res.n_samples == len(flat) == 102400
    T, R = np.empty((100, len(flat))), np.empty((100, len(flat)))
    for k in range(0, len(flat), 8192):
        T[:, k:k + 8192], R[:, k:k + 8192] = m.temperature_radius(res.t, *flat[k:k + 8192].T)
    _check(res, T, R, tol=(2 * TOL,) * 3, floor_eps=-1., stefan_boltzmann=B.stefan_boltzmann)
    lo, hi = _window(m, flat)
    assert _clear_of(res.t, lo, 1e-12) and _clear_of(res.t, hi, 1e-12)
    assert np.array_equal(res.n_inside, np.sum((lo <= res.t[:, None]) & (res.t[:, None] <= hi), axis=-1))
