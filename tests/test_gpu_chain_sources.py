"""What the chain analyses share: ONE list of samplers with different parameter counts, walker counts and run lengths,
read in place by every analysis, against the same analysis of each sampler's chain passed as a host array.  Both forms
run the same kernels on the same numbers, so nothing here has a tolerance.  discard = 3, thin = 3 keep steps 3, 6, 9 of
the 11-step run and 3, 6, 9, 12 of the 14-step run: neither run length divides."""
import numpy as np
import pytest

from lightcurve_fitting_amd import engine as E, models as M
from lightcurve_fitting_amd.engine import LcfError
from lightcurve_fitting_amd.fitting import _thermal_filter
from lightcurve_fitting_amd.sampler import EnsembleSampler
from helpers import shockcooling_case

pytestmark = pytest.mark.gpu

DISCARD, THIN = 3, 3
Q = np.array([2.5, 50., 84.14])


def _sampler(model, lc, priors, nwalkers, nsteps, lo, hi, seed):
    sampler = EnsembleSampler(nwalkers, len(priors), model.engine_for(lc, priors=priors), seed=seed)
    sampler.run_mcmc(np.random.default_rng(seed).uniform(lo, hi, (nwalkers, len(priors))), nsteps)
    return sampler


@pytest.fixture(scope='module')
def fits():
    """(model, light curve, sampler) twice: ShockCooling, 5 columns, 16 walkers, 11 steps; ShockCooling2, 4 columns,
    24 walkers, 14 steps."""
    _, lc = shockcooling_case()
    m1, m2 = M.ShockCooling(redshift=0.01), M.ShockCooling2(redshift=0.01)
    pri1 = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.2)]
    pri2 = [M.UniformPrior(0., 100.), M.UniformPrior(0., 20.), M.UniformPrior(0., 100.), M.UniformPrior(-1., 0.2)]
    s1 = _sampler(m1, lc, pri1, 16, 11, [1., 0.5, 2., 1., -0.5], [2., 1.5, 4., 3., 0.], seed=3)
    s2 = _sampler(m2, lc, pri2, 24, 14, [10., 2., 10., -0.5], [30., 6., 30., 0.], seed=4)
    return [(m1, lc, s1), (m2, lc, s2)]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=True)


def test_a_mixed_list_equals_each_chain_as_a_host_array(fits):
    natives = [s._native for _, _, s in fits]
    tau = E.samplers_autocorr_time(natives, discard=DISCARD, thin=THIN)
    rng_ = E.chain_range(natives, discard=DISCARD, thin=THIN)
    edges = [np.linspace(lo - 1., hi + 1., 8).T.copy() for lo, hi, _ in rng_]    # (n_dim, 7 + 1) each
    shifts = [np.zeros(len(e)) for e in edges]
    hist = E.chain_hist(natives, shifts, edges, discard=DISCARD, thin=THIN)
    history = E.chain_history(natives, Q, discard=DISCARD, thin=THIN)
    raster = E.chain_raster(natives, 2, edges, discard=DISCARD, thin=THIN)
    assert len(tau) == len(rng_) == len(hist) == len(history) == len(raster) == 2
    for i, (_, _, s) in enumerate(fits):
        chain, lp = s.get_chain(), s.get_log_prob()
        n_t, n_w, n_dim = chain.shape
        assert (n_t, n_w, n_dim) == [(11, 16, 5), (14, 24, 4)][i] and lp.shape == (n_t, n_w)
        kept = chain[DISCARD::THIN]
        assert len(kept) == [3, 4][i]
        flat = kept.reshape(-1, n_dim)
        _same(tau[i], E.autocorr_time(kept))
        _same(rng_[i], E.chain_range(flat))
        _same(hist[i], E.chain_hist(flat, shifts[i], edges[i]))
        _same(history[i], E.chain_history(chain, Q, log_prob=lp, discard=DISCARD, thin=THIN))
        _same([raster[i]], [E.chain_raster(chain, 2, edges[i], discard=DISCARD, thin=THIN)])
        assert history[i][0].shape == (len(Q), len(kept), n_dim + 1) and raster[i].sum() == flat.size


def test_predictive_bands_of_a_stored_run_equal_its_rows_as_a_host_array(fits):
    model, lc, s = fits[0]
    times = np.linspace(0.5, 9., 7)
    rows = s.get_chain()[DISCARD::THIN].reshape(-1, s.ndim)
    grid, _ = M.Model._eval_engine(model, times, ['U', 'r'], False)
    _same(E.predict_quantiles(grid, s._native, Q, discard=DISCARD, thin=THIN), E.predict_quantiles(grid, rows, Q))
    filt = _thermal_filter(model)
    grid, _ = M.Model._eval_engine(model, times, [filt] * len(times))
    _same(E.predict_thermal(grid, s._native, Q, discard=DISCARD, thin=THIN), E.predict_thermal(grid, rows, Q))


def test_what_a_list_is_refused_for(fits):
    model, lc, s1 = fits[0]
    s2 = fits[1][2]
    priors = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.2)]
    fresh = EnsembleSampler(16, 5, model.engine_for(lc, priors=priors), seed=5)
    natives = [s1._native, s2._native]
    calls = [lambda n, d: E.samplers_autocorr_time(n, discard=d, thin=THIN),
             lambda n, d: E.chain_range(n, discard=d, thin=THIN),
             lambda n, d: E.chain_history(n, Q, discard=d, thin=THIN)]
    for call in calls:
        with pytest.raises(LcfError) as err:     # a sampler without a stored run: LCF_ERR_STATE
            call(natives + [fresh._native], DISCARD)
        assert err.value.status == 7 and 'no stored chain' in str(err.value)
        with pytest.raises(LcfError) as err:     # discard at the shorter run's length
            call(natives, 11)
        assert err.value.status == 1 and 'discard leaves no chain' in str(err.value)
        call(natives, 10)                        # ... and one step short of it
