"""Host side of the parallel-tempered sampler: the ladder, its validation, the proper-prior rule, thermodynamic
integration, and the swap step of the NumPy restatement (tests/tempered_reference.py).  No GPU."""
import numpy as np
import pytest

import tempered_reference as R
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.sampler import (check_betas, check_proper_priors, default_betas,
                                            thermodynamic_integration)


def test_default_ladders():
    c = 1. + 2. * np.sqrt(np.log(4.)) / np.sqrt(5.)
    assert np.allclose(default_betas(5, 4), [1., 1. / c, c ** -2., c ** -3.], rtol=1e-15)
    assert np.allclose(default_betas(5, 4, Tmax=1000.), [1., 0.1, 0.01, 0.001], rtol=1e-14)
    hot = default_betas(5, 4, Tmax=np.inf)
    assert np.allclose(hot[:3], [1., 1. / c, c ** -2.], rtol=1e-15) and hot[3] == 0.
    for ladder in (default_betas(5, 4), default_betas(5, 4, 1000.), hot, default_betas(3, 1), default_betas(3, 1, 50.)):
        assert ladder[0] == 1. and np.array_equal(check_betas(ladder), ladder)
    assert 1. / default_betas(1, 2)[1] == pytest.approx(1. + 2. * np.sqrt(np.log(4.)))


@pytest.mark.parametrize('bad', [(0.9, 0.5), (1., 1.), (1., 0.5, 0.6), (1., -0.1), (1., np.nan), (), ((1., 0.5),),
                                 tuple(np.linspace(1., 0., 65))])
def test_betas_are_validated(bad):
    with pytest.raises(ValueError, match='betas'):
        check_betas(bad)


def test_betas_accepted():
    assert np.array_equal(check_betas((1, .5, 0)), [1., .5, 0.])
    assert np.array_equal(check_betas([1.]), [1.])
    assert len(check_betas(np.linspace(1., 0., 64))) == 64


def test_prior_rung_needs_proper_priors():
    names = ['v', 'M', 'f', 'R', 't0']
    proper = [M.UniformPrior(0., 10.), M.LogUniformPrior(1e-3, 10.), M.GaussianPrior(mean=1., stddev=2.),
              M.GaussianPrior(0., 5., 1., 2.), M.UniformPrior(-1., 0.5)]
    check_proper_priors([p.descriptor() for p in proper], names)
    cases = [(M.UniformPrior(0., np.inf), 'bounds'), (M.UniformPrior(), 'bounds'), (M.LogUniformPrior(0., 10.), 'p_min'),
             (M.LogUniformPrior(1., np.inf), 'bounds')]
    for k, (prior, what) in enumerate(cases):
        mixed = list(proper)
        mixed[k] = prior
        with pytest.raises(ValueError, match=f'prior of {names[k]} is improper.*{what}'):
            check_proper_priors([p.descriptor() for p in mixed], names)
        with pytest.raises(ValueError, match=f'prior of p{k} is improper'):
            check_proper_priors([p.descriptor() for p in mixed])
    with pytest.raises(ValueError, match='no priors'):
        check_proper_priors(None)


def test_thermodynamic_integration_is_exact_for_a_linear_integrand():
    for betas in (np.array([1., .7, .4, .15, 0.]), default_betas(5, 6, np.inf)):
        ev = thermodynamic_integration(betas, -3. + 8. * betas)
        assert ev.reaches_prior and ev.lnZ == pytest.approx(1., abs=1e-14) and ev.dlnZ == pytest.approx(0., abs=1e-14)
        assert tuple(ev) == (ev.lnZ, ev.dlnZ)


def test_thermodynamic_integration_by_hand():
    # with a prior rung: trapezoids -7.5 - 7.5 - 17.5; coarse ladder (1, .25, 0): -18.75 - 17.5
    lnZ, dlnZ = ev = thermodynamic_integration([1., .5, .25, 0.], [-10., -20., -40., -100.])
    assert ev.reaches_prior and lnZ == -32.5 and dlnZ == 3.75
    # without: (0, m_3) is appended: -7.5 - 7.5 - 7.5 - 10; coarse ladder (1, .25, 0) of the five: -18.75 - 15
    lnZ, dlnZ = ev = thermodynamic_integration([1., .5, .25, .125], [-10., -20., -40., -80.])
    assert not ev.reaches_prior and lnZ == -32.5 and dlnZ == 1.25
    # one rung: the integrand is its mean all the way
    ev = thermodynamic_integration([1.], [-7.])
    assert not ev.reaches_prior and tuple(ev) == (-7., 0.)
    with pytest.raises(ValueError):
        thermodynamic_integration([1., .5], [-1.])


@pytest.mark.parametrize('step', [0, 1])
def test_restated_swaps_conserve_every_slot(step):
    rng = np.random.default_rng(11 + step)
    K, W, D = 5, 7, 3
    x, ll, lpr = rng.normal(size=(K, W, D)), -50. * rng.random((K, W)), rng.normal(size=(K, W))
    betas = np.array([1., .5, .2, .05, 0.])
    before = (x.copy(), ll.copy(), lpr.copy())
    acc, prop, margin = R.swap_step(x, ll, lpr, betas, 123456789, step)
    pairs = np.arange(step & 1, K - 1, 2)
    assert np.array_equal(prop[pairs], [W] * len(pairs)) and prop.sum() == W * len(pairs)
    assert 0 < acc.sum() < prop.sum() and margin > 0.       # (both outcomes occur in this draw)
    rows = lambda a, b, c, i: sorted(map(tuple, np.column_stack([a[:, i], b[:, i], c[:, i]])))
    for i in range(W):
        assert rows(x, ll, lpr, i) == rows(*before, i)
    moved = np.any(x != before[0], axis=2)
    assert moved.sum() == 2 * acc.sum()
    idle = np.setdiff1d(np.arange(K), np.concatenate([pairs, pairs + 1]))
    assert not moved[idle].any()
