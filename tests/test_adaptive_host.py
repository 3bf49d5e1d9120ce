"""Host side of the adaptive ladder and the stepping-stone estimator: the new entry points are declared, bound and
exported; the ladder rule of the NumPy restatement (tests/adaptive_reference.py); ``stepping_stone`` against a closed
form; and every ``ValueError`` of the new interface, raised before the device is reached.  No GPU."""
import os
import re

import numpy as np
import pytest

import adaptive_reference as A
from lightcurve_fitting_amd import engine as E, fitting as Fit, models as M, sampler as S
from lightcurve_fitting_amd.sampler import LogEvidence, TemperedSampler, stepping_stone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lcf_tempered_run_adaptive', 'lcf_tempered_get_betas', 'lcf_tempered_get_beta_history',
         'lcf_tempered_stepping_stones')


def test_symbols_are_declared_and_bound_and_the_abi_is_8():
    header = open(os.path.join(ROOT, 'include', 'lcf.h')).read()
    declared = set(re.findall(r'\b(lcf_[a-z_0-9]+)\s*\(', header))
    bound = {name for name, _, _ in E.SIGNATURES}
    lib = E.load_library()
    for name in NAMES:
        assert name in declared and name in bound and hasattr(lib, name)
    for name in ('run_adaptive', 'get_betas', 'get_beta_history', 'stepping_stones'):
        assert callable(getattr(E.NativeTempered, name))
    assert E.LCF_ABI_VERSION == 8 and lib.lcf_abi_version() == 8
    assert re.search(r'#define LCF_ABI_VERSION 8\b', header)


# ---- the ladder rule ---------------------------------------------------------------------------------------------------
LADDERS = (np.array([1., .5, .1, 0.]), np.array([1., .6, .3, .1, 0.]), S.default_betas(5, 12, np.inf), np.array([1., .5, 0.]))


@pytest.mark.parametrize('betas', LADDERS, ids=lambda b: f'K{len(b)}')
def test_equal_swap_fractions_leave_the_ladder(betas):
    for a in (0., .25, 1.):
        got = A.adapt_ladder(betas, np.full(len(betas) - 1, a), t=1, lag=10., time=2.)
        np.testing.assert_allclose(got, betas, rtol=1e-15, atol=0.)
        assert got[0] == 1. and got[-1] == 0.


def test_a_pair_that_swaps_more_than_the_next_moves_apart():
    betas = np.array([1., .6, .3, .1, 0.])
    gaps = lambda b: np.diff(1. / b[:-1])                  # T_{k+1} - T_k of the finite rungs
    for k in range(3):
        acc = np.full(4, .3)
        acc[k] = .6                                         # A_k > A_{k+1}: gap k widens; A_{k-1} < A_k: gap k - 1 narrows
        got = A.adapt_ladder(betas, acc, t=3, lag=10., time=2.)
        ratio = gaps(got) / gaps(betas)
        kappa = 10. / 13. / 2.
        want = np.ones(3)
        want[k] = np.exp(kappa * .3)
        if k:
            want[k - 1] = np.exp(-kappa * .3)
        np.testing.assert_allclose(ratio, want, rtol=1e-13)
        assert ratio[k] > 1.


def test_the_ends_never_move_and_descent_is_preserved():
    rng = np.random.default_rng(5)
    for betas in LADDERS:
        b = betas.copy()
        for t in range(1, 200):
            b = A.adapt_ladder(b, rng.random(len(b) - 1), t=t, lag=5., time=1.)
            assert b[0] == 1. and b[-1] == 0.
            assert np.all(np.diff(b) < 0.)
    # kappa falls with t: the same fractions move a late ladder less
    early = A.adapt_ladder(LADDERS[1], [.9, .1, .5, .5], t=1, lag=10., time=2.)
    late = A.adapt_ladder(LADDERS[1], [.9, .1, .5, .5], t=1000, lag=10., time=2.)
    assert abs(late[1] - .6) < abs(early[1] - .6)
    for bad in ((1., .5), (1., .5, .1)):
        with pytest.raises(ValueError, match='at least 3 rungs'):
            A.adapt_ladder(bad, np.zeros(len(bad) - 1), 1, 10., 2.)


# ---- stepping stones ---------------------------------------------------------------------------------------------------
def _gaussian_case(seed):
    """Prior N(0, 1), L = exp(-x^2 / 2 sigma^2), sigma = 0.1: rung beta is N(0, 1 / (1 + beta / sigma^2)) exactly, and
    lnZ = -ln(1 + 1 / sigma^2) / 2."""
    sigma = .1
    betas = np.append(np.geomspace(1., 1e-4, 16), 0.)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((64, 17, 32)) / np.sqrt(1. + betas / sigma ** 2)[None, :, None]
    return betas, -.5 * x ** 2 / sigma ** 2, -.5 * np.log(1. + 1. / sigma ** 2)


def test_stepping_stone_against_a_closed_form():
    betas, lnL, exact = _gaussian_case(0)
    assert exact == pytest.approx(-2.30756, abs=1e-5)
    ev = stepping_stone(betas, A.stone_partials(lnL, betas, 8))
    print(f'lnZ = {ev.lnZ:.5f} +- {ev.dlnZ:.5f}; exact {exact:.5f}')
    assert isinstance(ev, LogEvidence) and ev.reaches_prior and tuple(ev) == (ev.lnZ, ev.dlnZ)
    assert abs(ev.lnZ - exact) < .1
    assert .005 < ev.dlnZ < .05
    # the function is the estimator restated sample by sample
    want = A.stepping_stone(lnL, betas, 8)
    assert ev.lnZ == pytest.approx(want[0], rel=1e-13) and ev.dlnZ == pytest.approx(want[1], rel=1e-10)
    # a ladder that stops above 0: the stones of the rungs there are, and it says so
    cut = stepping_stone(betas[:9], A.stone_partials(lnL[:, :9], betas[:9], 8))
    assert not cut.reaches_prior
    assert cut.lnZ == pytest.approx(A.stepping_stone(lnL[:, :9], betas[:9], 8)[0], rel=1e-13)
    assert cut.lnZ == pytest.approx(-.5 * np.log((1. + 100.) / (1. + 100. * betas[8])), abs=.1)


def test_stepping_stone_partials_by_hand():
    # one pair, dbeta = 0.5, two batches of two samples: ln L = (0, -2) and (-4, -4)
    m, s, n = np.array([[0., -4.]]), np.array([[1. + np.exp(-1.), 2.]]), np.array([[2., 2.]])
    ev = stepping_stone([.5, 0.], (m, s, n))
    r = np.array([np.log((1. + np.exp(-1.)) / 2.), -2.])
    assert ev.lnZ == pytest.approx(np.log((1. + np.exp(-1.) + 2. * np.exp(-2.)) / 4.), rel=1e-14)
    assert ev.dlnZ == pytest.approx(np.sqrt(np.var(r, ddof=1) / 2.), rel=1e-14)
    # a batch that never left ln L = -inf (max -inf, sum 0) weighs nothing in the pair's average
    ev = stepping_stone([.5, 0.], (np.array([[0., -np.inf]]), np.array([[1. + np.exp(-1.), 0.]]), n))
    assert ev.lnZ == pytest.approx(np.log((1. + np.exp(-1.)) / 4.), rel=1e-14)
    for bad in (([1., 0.], (m[:, :1], s[:, :1], n[:, :1])), ([1., .5, 0.], (m, s, n)), ([1.], (m[:0], s[:0], n[:0])),
                ([1., 0.], (m, s))):
        with pytest.raises(ValueError):
            stepping_stone(*bad)


def test_restated_partials_have_the_batches_edges():
    assert np.array_equal(A.batch_edges(12, 4), [0, 3, 6, 9, 12]) and np.array_equal(A.batch_edges(13, 4), [0, 3, 6, 9, 13])
    assert np.array_equal(A.batch_edges(8, 8), np.arange(9))
    rng = np.random.default_rng(2)
    lnL = -50. * rng.random((14, 3, 5))
    m, s, n = A.stone_partials(lnL, [1., .4, 0.], 4, discard=1)
    assert np.array_equal(n, [[15., 15., 15., 20.]] * 2)
    assert m[1, 3] == lnL[10:, 2].max() and s[0, 0] == pytest.approx(np.sum(np.exp(.6 * (lnL[1:4, 1] - m[0, 0]))), rel=1e-14)
    with pytest.raises(ValueError, match='batches'):
        A.stone_partials(lnL, [1., .4, 0.], 15)


# ---- errors before the device ------------------------------------------------------------------------------------------
class _Engine:
    ndim, device = 5, 0
    priors = [p.descriptor() for p in [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., .5)]]


class _NoDevice:
    """Stands in for ``NativeTempered``: it holds a ladder and a stored-step count, and anything that would enqueue work
    on the device fails the test."""

    def __init__(self, engine, betas, nwalkers, seed=0, a=2.):
        self.betas, self.shape = np.array(betas, dtype=np.float64), (len(betas), int(nwalkers), engine.ndim)
        self.history = None

    def _reached(self, *a, **k):
        raise AssertionError('the device was reached')

    set_state = run = run_adaptive = get_chain = mean_loglike = stepping_stones = get_state = counts = _reached

    def get_betas(self):
        return self.betas.copy()

    def get_beta_history(self, nstored):
        return np.tile(self.betas, (nstored, 1)) if self.history is None else self.history

    def close(self):
        pass


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(E, 'NativeTempered', _NoDevice)
    monkeypatch.setattr(E, 'load_library', _NoDevice._reached)


def _stored(sampler, nsteps, history=None):
    """As after a stored run of ``nsteps`` steps."""
    sampler._stored, sampler._state = nsteps, object()
    sampler._tempered.history = history
    return sampler


def test_adapting_needs_three_rungs_and_a_prior_rung(no_device):
    x0 = np.zeros((2, 12, 5))
    for kw in (dict(betas=(1., 0.)), dict(ntemps=2, Tmax=np.inf)):                    # K < 3
        s = TemperedSampler(12, 5, _Engine(), **kw)
        with pytest.raises(ValueError, match='at least 3 rungs'):
            s.run_mcmc(x0, 4, adapt=True)
    for kw in (dict(betas=(1., .5, .1)), dict(ntemps=4), dict(ntemps=4, Tmax=100.)):   # last beta != 0
        s = TemperedSampler(12, 5, _Engine(), **kw)
        with pytest.raises(ValueError, match='last rung at beta = 0'):
            s.run_mcmc(np.zeros((s.ntemps, 12, 5)), 4, adapt=True)
        assert s.adaptation_steps == 0
    for kw in (dict(adaptation_lag=0.), dict(adaptation_time=-1.), dict(adaptation_lag=np.inf)):
        with pytest.raises(ValueError, match='adaptation_lag and adaptation_time'):
            TemperedSampler(12, 5, _Engine(), ntemps=4, Tmax=np.inf, **kw)
    s = TemperedSampler(12, 5, _Engine(), ntemps=4, Tmax=np.inf)
    assert (s.adaptation_lag, s.adaptation_time, s.adaptation_steps) == (10000., 100., 0)   # ptemcee's defaults


def test_log_evidence_errors_come_before_the_device(no_device):
    s = _stored(TemperedSampler(12, 5, _Engine(), betas=(1., .5, .1, 0.)), 6)
    for method in ('harmonic', None, 'stepping stone'):
        with pytest.raises(ValueError, match='method'):
            s.log_evidence(method=method)
    for batches in (1, 0, -3, 2.5):
        with pytest.raises(ValueError, match='batches >= 2'):
            s.log_evidence(method='stepping_stone', batches=batches)
    with pytest.raises(ValueError, match='batches=7 is more than the 6 stored'):
        s.log_evidence(method='stepping_stone', batches=7)
    with pytest.raises(ValueError, match='batches=5 is more than the 4 stored'):
        s.log_evidence(method='stepping_stone', batches=5, discard=2)
    with pytest.raises(ValueError, match='leaves no steps'):
        s.log_evidence(method='stepping_stone', discard=6)
    # a ladder that moved while the chain was stored: either method refuses
    moved = np.tile(s.betas, (6, 1))
    moved[2:, 1] = .45
    s = _stored(TemperedSampler(12, 5, _Engine(), betas=(1., .5, .1, 0.)), 6, moved)
    assert s.get_betas().shape == (6, 4) and np.array_equal(s.get_betas(discard=1, thin=2), moved[1::2])
    for kw in (dict(), dict(method='thermodynamic'), dict(method='stepping_stone', batches=2), dict(discard=1)):
        with pytest.raises(ValueError, match='the ladder moved'):
            s.log_evidence(**kw)
    with pytest.raises(AssertionError, match='device was reached'):   # rows 2: are one ladder: the reduction is asked for
        s.log_evidence(discard=2, method='stepping_stone', batches=2)
    with pytest.raises(AssertionError, match='device was reached'):
        s.log_evidence(discard=2)
    empty = TemperedSampler(12, 5, _Engine(), betas=(1., .5, 0.))
    with pytest.raises(ValueError, match='no chain'):
        empty.log_evidence(method='stepping_stone')


def test_lightcurve_mcmc_adapt_needs_tempering(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(E, 'load_library', no_device)
    monkeypatch.setattr(Fit, '_prepare_photometry', no_device)
    m = M.ShockCooling(redshift=0.)
    with pytest.raises(ValueError, match='adapt=True'):
        Fit.lightcurve_mcmc({}, m, p_lo=np.zeros(5), p_up=np.ones(5), adapt=True)
