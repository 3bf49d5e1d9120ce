"""Integrated autocorrelation time on the GPU against the NumPy restatement of emcee's estimator: seeded AR(1) chains of
many shapes, the input forms of integrated_time, the tol check, a real fit whose chain stays on the device, a chain of
two runs, populations and determinism."""
import logging

import numpy as np
import pytest

from helpers import shockcooling_case
from lightcurve_fitting_amd import engine as E
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.autocorr import AutocorrError, integrated_time
from lightcurve_fitting_amd.fitting import lightcurve_mcmc
from lightcurve_fitting_amd.sampler import EnsembleSampler, PopulationSampler
from test_autocorr_host import ar1, oracle_autocorr

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]), initial=0.))


@pytest.mark.parametrize('n_t,n_w,n_d,phi,c', [
    (1000, 7, 3, 0.9, 5.),       # odd n_w
    (999, 16, 1, 0.8, 5.),       # n_d = 1, n_t not a power of two
    (50, 8, 2, 0.5, 5.),         # n_t below the first lag block
    (3001, 9, 2, 0.9, 1.),
    (3001, 9, 2, 0.9, 10.),      # window past the first two lag blocks
    (20000, 8, 1, 0.98, 5.),     # window of several hundred lags
    (300, 70, 2, 0.99, 5.),      # tau comparable to n_t
    (700, 5, 2, 0.5, -1.),       # no lag satisfies the window rule: every lag computed, window n_t - 1
])
def test_matches_oracle_on_ar1_chains(n_t, n_w, n_d, phi, c):
    x = ar1(n_t, n_w, n_d, phi, seed=n_t + n_w)
    tau, window = E.autocorr_time(x, c)
    want, want_window = oracle_autocorr(x, c)
    # (relative to max(|tau|, 1): with window n_t - 1, tau is the sum of all normalised autocorrelations, which is 0
    # up to rounding, and f[0] = 1 sets the scale of that rounding)
    assert np.all(np.abs(tau - want) <= 1e-10 * np.maximum(np.abs(want), 1.)), (tau, want)
    assert np.array_equal(window, want_window)


def test_known_answer_ar1():
    x = ar1(20000, 128, 2, 0.9, seed=7)
    tau = integrated_time(x)
    np.testing.assert_allclose(tau, 19., rtol=0.03)
    assert _rel(tau, oracle_autocorr(x)[0]) <= 1e-10


def test_input_forms():
    x = ar1(2000, 6, 3, 0.7, seed=3)
    tau = integrated_time(x[:, 0, 0], quiet=True)                         # 1-D: (n_t, 1, 1)
    assert tau.shape == (1,) and _rel(tau, oracle_autocorr(x[:, :1, :1])[0]) <= 1e-10
    tau = integrated_time(x[:, :, 1], quiet=True)                         # 2-D with walkers: (n_t, n_w, 1)
    assert tau.shape == (1,) and _rel(tau, oracle_autocorr(x[:, :, 1:2])[0]) <= 1e-10
    tau = integrated_time(x[:, 2, :], quiet=True, has_walkers=False)      # 2-D without: (n_t, 1, n_d)
    assert tau.shape == (3,) and _rel(tau, oracle_autocorr(x[:, 2:3, :])[0]) <= 1e-10
    y = x.copy()
    y[:, 4, 1] = 2.5                                                      # a constant walker: NaN tau, no exception
    tau = integrated_time(y)
    want, want_window = oracle_autocorr(y)
    assert np.isnan(tau[1]) and not np.isnan(tau[0]) and _rel(tau, want) <= 1e-10
    assert np.array_equal(E.autocorr_time(y)[1], want_window) and want_window[1] == len(y) - 1


def test_non_convergence(caplog):
    x = ar1(400, 10, 2, 0.95, seed=11)
    with pytest.raises(AutocorrError) as err:
        integrated_time(x)
    with caplog.at_level(logging.WARNING, logger='lightcurve_fitting_amd.autocorr'):
        tau = integrated_time(x, quiet=True)
    assert np.array_equal(err.value.tau, tau, equal_nan=True)
    assert any('shorter than 50 times' in r.getMessage() for r in caplog.records)
    assert _rel(tau, oracle_autocorr(x)[0]) <= 1e-10


def _fit(nsteps=400, burnin=100, seed=5):
    _, lc = shockcooling_case()
    priors = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.2)]
    return lightcurve_mcmc(lc, M.ShockCooling(redshift=0.01), priors=priors, p_lo=[1., 0.5, 2., 1., -0.5],
                           p_up=[2., 1.5, 4., 3., 0.], nwalkers=64, nsteps=nsteps, nsteps_burnin=burnin, seed=seed)


def test_real_fit_reads_the_chain_on_the_device():
    sampler = _fit()
    assert sampler._chain_on_device == 400 and len(sampler._chain_host) == 0
    got = sampler.get_autocorr_time(quiet=True)
    again = sampler.get_autocorr_time(quiet=True)
    thinned = sampler.get_autocorr_time(discard=37, thin=3, quiet=True)
    assert sampler._chain_on_device == 400, 'the chain was copied to the host'
    assert np.array_equal(got, again, equal_nan=True)   # determinism
    chain = sampler.get_chain()
    assert _rel(got, oracle_autocorr(chain)[0]) <= 1e-10
    # device-resident entry == host entry, bitwise
    host = integrated_time(sampler.get_chain(discard=37, thin=3), quiet=True)
    assert np.array_equal(thinned, 3 * host, equal_nan=True)
    assert np.array_equal(got, integrated_time(chain, quiet=True), equal_nan=True)
    # (the chain is on the host now: the host entry)
    assert np.array_equal(thinned, sampler.get_autocorr_time(discard=37, thin=3, quiet=True), equal_nan=True)
    with pytest.raises(ValueError):
        sampler.get_autocorr_time(discard=400)


def test_two_stored_runs_use_the_host_path():
    sampler = _fit(nsteps=200, burnin=50, seed=9)
    sampler.run_mcmc(None, 150)
    assert len(sampler._chain_host) == 200 and sampler._chain_on_device == 150
    got = sampler.get_autocorr_time(discard=20, quiet=True)
    chain = sampler.get_chain(discard=20)
    assert chain.shape == (330, 64, 5)
    assert _rel(got, oracle_autocorr(chain)[0]) <= 1e-10


def test_population_equals_each_transient():
    _, lc = shockcooling_case()
    pri1 = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.2)]
    pri2 = [M.UniformPrior(0., 100.), M.UniformPrior(0., 20.), M.UniformPrior(0., 100.), M.UniformPrior(-1., 0.2)]
    problems = [(M.ShockCooling(redshift=0.01), lc, pri1), (M.ShockCooling2(redshift=0.01), lc, pri2),
                (M.ShockCooling(redshift=0.02), lc, pri1)]
    rng = np.random.default_rng(4)
    x0 = {0: rng.uniform([1., 0.5, 2., 1., -0.5], [2., 1.5, 4., 3., 0.], (48, 5)),
          1: rng.uniform([10., 2., 10., -0.5], [30., 6., 30., 0.], (48, 4)),
          2: rng.uniform([1., 0.5, 2., 1., -0.5], [2., 1.5, 4., 3., 0.], (48, 5))}
    pop = PopulationSampler(problems, 48, seed=3)
    pop.run_mcmc(x0, 300)
    assert all(pop[k]._chain_on_device == 300 for k in range(3))
    for kw in ({}, {'discard': 50, 'thin': 2}):
        got = pop.get_autocorr_time(quiet=True, **kw)
        assert sorted(got) == [0, 1, 2] and got[1].shape == (4,) and got[0].shape == (5,)
        for k in range(3):
            assert np.array_equal(got[k], pop[k].get_autocorr_time(quiet=True, **kw), equal_nan=True)
        assert all(pop[k]._chain_on_device == 300 for k in range(3))
    plain = pop.get_autocorr_time(quiet=True)
    with pytest.raises(AutocorrError) as err:
        pop.get_autocorr_time(tol=1e6)
    assert sorted(err.value.tau) == [0, 1, 2]
    assert all(np.array_equal(err.value.tau[k], plain[k], equal_nan=True) for k in range(3))
    for k in range(3):
        assert _rel(plain[k], oracle_autocorr(pop[k].get_chain())[0]) <= 1e-10
    # the 4-D transient behind a 5-D one samples its own posterior: its chain is that of a solo run
    model, lc2, pri = problems[1]
    solo = EnsembleSampler(48, 4, model.engine_for(lc2, priors=pri), seed=3 + 1)
    solo.run_mcmc(x0[1], 300)
    assert np.array_equal(pop[1].get_chain(), solo.get_chain())
    np.testing.assert_allclose(pop[1].get_log_prob(), solo.get_log_prob(), rtol=1e-12, atol=1e-9)
