"""posterior_predictive on the device against the CPU oracle + NumPy: want = np.nanpercentile(Y, q, axis=-1) with
Y[f, t, s] the oracle's evaluation of the very samples the call used.  Tolerance: the 1e-11 of tests/test_gpu_parity.py
for single evaluations -- if every value is within a relative eps of the oracle's and non-negative, so is every order
statistic and every convex combination of two of them; relerr also demands identical NaN patterns.  n_valid must be
equal exactly."""
import numpy as np
import pytest

from conftest import relerr
from helpers import config2_case, lc_dict, small_problem
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.fitting import lightcurve_mcmc, posterior_predictive
from oracle import lcf_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-11
TRUTH = np.array([1.2, 0.5, 3.0, 2.0, 0.1])
UFILTS = list('UBVgri')
SEVEN = (0., 2.5, 15.87, 50., 84.14, 97.5, 100.)


def _lc(t0=0.3, t1=12.):
    """A light curve that only gives the grid its range and filters."""
    t = np.repeat([t0, t1], 6)
    return lc_dict(t, UFILTS * 2, np.full(12, 1e20), np.full(12, 1e18))


def _rows(n, seed=12):
    """The recipe of test_model_grid_at_plotting_size: 20 % scatter about the truth."""
    rng = np.random.default_rng(seed)
    return TRUTH * (1. + 0.2 * rng.uniform(-1., 1., (n, 5)))


def _oracle_grid(orc, times, names, P):
    """Y[f, t, s] for models whose oracle takes blocks of parameter vectors."""
    return np.stack([O.evaluate(orc, times, [O.band(f)] * len(times), P.T).reshape(len(times), -1) for f in names])


def _check(res, Y, q=None):
    want = np.nanpercentile(Y, res.percentiles if q is None else q, axis=-1)
    err = relerr(res.quantiles, want)
    print(f'posterior_predictive vs oracle + nanpercentile: max rel err {err:.3e} over {res.quantiles.shape}')
    assert err <= TOL
    assert np.array_equal(res.n_valid, np.sum(~np.isnan(Y), axis=-1))
    return want


def test_shockcooling_4096_rows_seven_percentiles():
    P = _rows(4096)
    m = M.ShockCooling(redshift=0.01)
    res = posterior_predictive(_lc(), m, P, percentiles=SEVEN, num=50)
    assert res.quantiles.shape == (7, 6, 50) and res.n_valid.shape == (6, 50) and res.n_samples == 4096
    names = [f.name for f in res.filters]      # the light curve's filters in the registry's order
    assert np.array_equal(res.t, np.linspace(0.3, 12., 50)) and res.filters == sorted(res.filters)
    assert sorted(names) == sorted(UFILTS)
    Y = _oracle_grid(('ShockCooling', O.ShockCoolingOracle(0.01)), res.t, names, P)
    _check(res, Y)
    # q = 0 and q = 100 are evaluated values themselves: within TOL of the oracle's extremes, and ordered
    assert np.all(np.diff(res.quantiles, axis=0) >= 0.)


def test_ties_at_exact_zero():
    """Before its t_0 a sample's model is exactly 0 (the reference's power()): at 0.1 d the second group's k rows tie."""
    S = 4096
    rng = np.random.default_rng(7)
    P = _rows(S, seed=8)
    second = np.arange(S) >= int(0.6 * S)
    P[:, 4] = np.where(second, rng.uniform(0.12, 0.14, S), rng.uniform(0.07, 0.09, S))
    P = P[rng.permutation(S)]
    k = int(np.sum(P[:, 4] > 0.1))
    times = np.array([0.05, 0.1, 0.2])
    Y = _oracle_grid(('ShockCooling', O.ShockCoolingOracle(0.01)), times, UFILTS, P)
    assert np.all(Y[:, 0] == 0.) and np.all(np.sum(Y[:, 1] == 0., axis=-1) == k) and np.all(Y[:, 2] > 0.)
    assert k == S - int(0.6 * S)
    inside, edge = 100. * (k // 2) / (S - 1), 100. * (k - 0.5) / (S - 1)
    q = [0., inside, edge, 50., 84.14, 100.]
    m = M.ShockCooling(redshift=0.01)
    res = posterior_predictive(_lc(), m, P, percentiles=q, t=times, filters_to_model=UFILTS)
    assert np.all(res.quantiles[:, :, 0] == 0.)                 # every sample is 0 at 0.05 d
    assert np.all(res.quantiles[1, :, 1] == 0.)                 # inside the tie
    smallest = np.min(np.where(Y[:, 1] > 0., Y[:, 1], np.inf), axis=-1)
    assert relerr(res.quantiles[2, :, 1], 0.5 * smallest) <= TOL   # half way from the last zero to the first value
    _check(res, Y)


def _one_sample_cases():
    g, lc2 = config2_case()
    sc = O.ShockCoolingOracle(0.01)
    yield 'ShockCooling', M.ShockCooling(redshift=0.01), ('ShockCooling', sc), TRUTH
    yield 'ShockCooling2', M.ShockCooling2(redshift=0.01), ('ShockCooling2', sc), np.array([20., 3., 20., 0.1])
    yield 'ShockCooling4', M.ShockCooling4(redshift=0.01), ('ShockCooling4', O.ShockCooling4Oracle(0.01)), TRUTH
    yield ('ShockCooling3', M.ShockCooling3(redshift=0.01), ('ShockCooling3', sc),
           np.array([1.2, 0.5, 3.0, 2.0, 30., 0.1, 0.1]))
    bands = [O.band(n) for n in lc2['filter']]
    yield ('CompanionShocking', M.CompanionShocking(lc2, redshift=0.003),
           ('CompanionShocking', O.CompanionShockingOracle(bands, lc2['lum'], z=0.003, variant=1)),
           np.array([0.2, 0.5, 1.2, 12., 1.05, 0.95, 0.9, 0.6]))


def test_one_sample_every_model():
    """With one sample no interpolation happens: all percentiles of a call are the value itself."""
    times = np.linspace(0.3, 12., 23)
    for name, m, orc, p in _one_sample_cases():
        res = posterior_predictive(_lc(), m, p[None, :], percentiles=(0., 15.87, 50., 100.), t=times,
                                   filters_to_model=UFILTS)
        assert np.all(res.quantiles == res.quantiles[0]), name
        assert np.all(res.n_valid == 1) and res.n_samples == 1
        if name == 'CompanionShocking':
            want = np.stack([orc[1].evaluate(times, [O.band(f)] * len(times), *p) for f in UFILTS])
        else:
            want = np.stack([O.evaluate(orc, times, [O.band(f)] * len(times), p) for f in UFILTS])
        err = relerr(res.quantiles[0], want)
        print(f'{name}: one sample vs oracle {err:.3e}')
        assert err <= TOL, name


def _companion_rows(n, variant, seed=3):
    rng = np.random.default_rng(seed)
    centre = {1: [0.2, 0.5, 1.2, 12., 1.05, 0.95, 0.9, 0.6], 2: [0.2, 0.5, 1.2, 12., 1.05, 0.8, -0.6]}[variant]
    return np.array(centre) * (1. + 0.1 * rng.uniform(-1., 1., (n, len(centre))))


@pytest.mark.parametrize('variant', [1, 2])
def test_companion_model_and_sifto_component(variant):
    g, lc = config2_case()
    cls = {1: M.CompanionShocking, 2: M.CompanionShocking2}[variant]
    m = cls(lc, redshift=0.003)
    orc = O.CompanionShockingOracle([O.band(n) for n in lc['filter']], lc['lum'], z=0.003, variant=variant)
    P = _companion_rows(512, variant)
    res = posterior_predictive(lc, m, P, num=40)
    names = [f.name for f in res.filters]
    assert sorted(names) == sorted(UFILTS) and len(res.t) == 40
    bands = [[O.band(f)] * 40 for f in names]
    Y = np.stack([np.stack([orc.evaluate(res.t, b, *p) for p in P], axis=-1) for b in bands])
    _check(res, Y)
    sif = posterior_predictive(lc, m, P, num=40, component='sifto')

    def sifto(b, p):
        if variant == 2:
            return orc.stretched_sifto(res.t, b, p[3], p[4], p[5], p[6])
        fac = p[5] if b[0].char == 'r' else p[6] if b[0].char == 'i' else 1.
        return orc.stretched_sifto(res.t, b, p[3], p[4]) * fac
    Y1 = np.stack([np.stack([sifto(b, p) for p in P], axis=-1) for b in bands])
    _check(sif, Y1)
    assert relerr(sif.quantiles[1], np.median(Y1, axis=-1)) <= TOL   # what fitting.py:422 plots
    with pytest.raises(ValueError, match='sifto'):
        posterior_predictive(lc, M.ShockCooling(redshift=0.), _rows(4), component='sifto')


def _fit(nwalkers, nsteps, use_sigma=False):
    pb = small_problem()
    lc = lc_dict(pb['t'], pb['names'], pb['y'], pb['dy'])
    priors = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.5)] + ([M.UniformPrior(0., 2.)] if use_sigma else [])
    p_lo = list(0.9 * TRUTH[:4]) + [0.05] + ([0.1] if use_sigma else [])
    p_up = list(1.1 * TRUTH[:4]) + [0.15] + ([0.5] if use_sigma else [])
    m = M.ShockCooling(redshift=0.)
    np.random.seed(4)
    s = lightcurve_mcmc(lc, m, priors=priors, p_lo=p_lo, p_up=p_up, nwalkers=nwalkers, nsteps=nsteps,
                        nsteps_burnin=50, use_sigma=use_sigma, seed=9)
    return lc, m, s


@pytest.mark.parametrize('use_sigma', [False, True])
def test_sampler_in_place_equals_the_array_form(use_sigma):
    lc, m, s = _fit(64, 40, use_sigma)
    assert len(s._chain_host) == 0 and s._chain_on_device == 40           # read where it lies
    a = posterior_predictive(lc, m, s, discard=7, thin=3, num=30, use_sigma=use_sigma)
    assert len(s._chain_host) == 0 and s._chain_on_device == 40           # ... and it still lies there
    flat = s.get_chain(discard=7, thin=3, flat=True)
    assert a.n_samples == len(flat) == 11 * 64
    b = posterior_predictive(lc, m, flat, num=30, use_sigma=use_sigma)
    assert np.array_equal(a.quantiles, b.quantiles, equal_nan=True) and np.array_equal(a.n_valid, b.n_valid)
    Y = _oracle_grid(('ShockCooling', O.ShockCoolingOracle(0.)), a.t, [f.name for f in a.filters], flat[:, :5])
    _check(a, Y)
    s.run_mcmc(None, 10)                                                   # the chain is now partly on the host
    c = posterior_predictive(lc, m, s, discard=7, thin=3, num=30, use_sigma=use_sigma)
    d = posterior_predictive(lc, m, s.get_chain(discard=7, thin=3, flat=True), num=30, use_sigma=use_sigma)
    assert c.n_samples == 15 * 64
    assert np.array_equal(c.quantiles, d.quantiles, equal_nan=True) and np.array_equal(c.n_valid, d.n_valid)
    with pytest.raises(ValueError, match='columns'):
        posterior_predictive(lc, m, s, use_sigma=not use_sigma)


def test_tiling_and_determinism():
    P = _rows(4096)
    m = M.ShockCooling(redshift=0.01)
    # seven percentiles x six filters keep 7 * 6 * 2048 keys of 8 bytes per time: 4 MiB hold at most six of the 50 times
    tiled = posterior_predictive(_lc(), m, P, percentiles=SEVEN, num=50, workspace_bytes=4 << 20)
    one = posterior_predictive(_lc(), m, P, percentiles=SEVEN, num=50)
    two = posterior_predictive(_lc(), m, P, percentiles=SEVEN, num=50)
    assert np.array_equal(one.quantiles, two.quantiles) and np.array_equal(one.n_valid, two.n_valid)
    assert np.array_equal(one.quantiles, tiled.quantiles) and np.array_equal(one.n_valid, tiled.n_valid)
    with pytest.raises(Exception, match='workspace_bytes too small'):
        posterior_predictive(_lc(), m, P, percentiles=SEVEN, num=50, workspace_bytes=1 << 16)


def test_every_pass_loops_and_refines_more_than_once():
    """S = 1024 x 100 rows of a fit on 6 x 100 points (6e7 values, 0.5 GB on the host): every pass loops over samples and
    a bin of the first histogram holds far more keys than a search sorts.  Against the project's own model(...) in
    slices + np.nanpercentile (the oracle is too slow here): both sides are within 1e-11 of the oracle, so they are held
    to 2e-11 of each other."""
    lc, m, s = _fit(1024, 100)
    res = posterior_predictive(lc, m, s, num=100)
    flat = s.get_chain(flat=True)
    assert res.n_samples == len(flat) == 102400
    Y = np.empty((6, 100, len(flat)))
    for k in range(0, len(flat), 8192):
        Y[:, :, k:k + 8192] = m(res.t, res.filters, *flat[k:k + 8192].T)
    want = np.nanpercentile(Y, res.percentiles, axis=-1)
    err = relerr(res.quantiles, want)
    print(f'102400 samples x 600 points vs model(...) + nanpercentile: max rel err {err:.3e}')
    assert err <= 2 * TOL
    assert np.array_equal(res.n_valid, np.sum(~np.isnan(Y), axis=-1))


def test_companion_shocking_term_alone():
    """BaseCompanionShocking.companion_shocking (models.py:757-784): the shock term on the dense filters x times grid,
    with and without an opacity other than 1."""
    g, lc = config2_case()
    m = M.CompanionShocking(lc, redshift=0.003)
    t = np.linspace(0.5, 10., 17)
    for kappa in (1., 0.7):
        got = m.companion_shocking(t, UFILTS, 0.2, 0.5, 1.2, kappa=kappa)
        T, R = O.kasen_temperature_radius(t, 0.2, 0.5, 1.2, kappa)
        want = np.stack([O.blackbody_to_filters_batch([O.band(f)] * len(t), T, R, 0.003) for f in UFILTS])
        assert got.shape == (6, 17) and relerr(got, want) <= TOL
