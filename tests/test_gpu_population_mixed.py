"""Populations of DIFFERENT transients -- models, fit dimensions, a fitted sigma, stretch scales -- in every form a
population run can take: each transient's chain must be the chain of that transient run alone (same seed, same stretch
scale) and the oracle-driven chain.  Transient 0's sampler shapes the population's shared launches, so the order of
the transients matters: P1 puts the lowest dimension first, P2 the highest."""
import numpy as np
import pytest

from conftest import relerr
from helpers import lc_dict, oracle_log_posterior
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.sampler import EnsembleSampler, PopulationSampler
from oracle import lcf_oracle as O

pytestmark = pytest.mark.gpu

SEED = 61
STEPS = (6, 3)   # run_mcmc(x0, 6) then run_mcmc(None, 3): a continuation with first_step > 0
Z = 0.01

# kind -> (truth, priors); t_exp prior bounds keep the explosion in front of the first epoch
SHAPES = {
    'ShockCooling': ([1.2, 0.5, 3.0, 2.0, 0.1], [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.29)]),
    'ShockCooling4': ([1.2, 0.5, 3.0, 2.0, 0.1], [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.29)]),
    'ShockCooling2': ([30., 3., 30., 0.2], [M.UniformPrior(0., 100.)] * 3 + [M.UniformPrior(-1., 0.29)]),
    'ShockCooling3': ([1.1, 0.6, 2.5, 1.8, 25., 0.15, 0.05],   # E(B-V) free inside a fixed range
                      [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(1., 100.), M.UniformPrior(0., 0.6),
                                                       M.UniformPrior(-1., 0.29)]),
    'CompanionShocking': ([57001., 0.5, 1.2, 57018., 1.05, 0.95, 0.9, 0.6],
                          [M.UniformPrior(56999., 57001.4), M.UniformPrior(0., 10.), M.UniformPrior(0., 10.),
                           M.UniformPrior(57008., 57028.), M.UniformPrior(0.5, 2.), M.UniformPrior(0., 5.),
                           M.UniformPrior(0., 5.), M.UniformPrior(0., 5.)]),
}
ORACLES = {'ShockCooling': O.ShockCoolingOracle, 'ShockCooling2': O.ShockCoolingOracle,
           'ShockCooling3': O.ShockCoolingOracle, 'ShockCooling4': O.ShockCooling4Oracle}

# id -> (walkers, [(kind, fitted sigma, stretch scale a, light-curve seed)]); transient 0 first
P1 = [('ShockCooling2', False, 2., 1), ('ShockCooling', False, 2., 2), ('ShockCooling', True, 2., 3),
      ('ShockCooling2', True, 2., 4)]
POPULATIONS = {
    'P1': (27, P1),                                           # mixed dimensions 4, 5, 6, 5: the lowest first
    'P2': (34, P1[::-1]),                                     # ... the highest first
    'P3': (27, [('ShockCooling', False, 2., 5), ('ShockCooling2', True, 2., 6), ('ShockCooling4', False, 2., 7)]),
    'P4': (34, [('ShockCooling', False, 2., 8), ('ShockCooling', False, 1.5, 9), ('ShockCooling', False, 3., 10)]),
    'P5': (27, [('CompanionShocking', False, 2., 11), ('CompanionShocking', True, 2., 12), ('ShockCooling', False, 2., 13)]),
    'P6': (34, [('ShockCooling', False, 2., 14), ('ShockCooling3', False, 2., 15)]),
}

# form -> (environment, random split, batched)
FORMS = {
    'population-run': ({}, True, True),
    'population': ({'LCF_NO_POP_RUN': '1'}, True, True),
    'population-phases': ({'LCF_NO_POP': '1'}, True, True),
    'blocks of 2 steps': ({'LCF_DRAW_BLOCK': '2'}, True, True),
    'identity split': ({}, False, True),
    'unbatched': ({}, True, False),
}
ENV = ('LCF_NO_POP_RUN', 'LCF_NO_POP', 'LCF_DRAW_BLOCK', 'LCF_RUN_GRID', 'LCF_POP_ITAB_LDS', 'LCF_NO_RUN_KERNEL')

# what pop[0]._native.last_run_kernel() reports for each form (unbatched: transient 0's own run)
KERNELS = {form: form for form in ('population-run', 'population', 'population-phases')}
KERNELS.update({'blocks of 2 steps': 'population-run', 'identity split': 'population-run', 'unbatched': 'run'})
EXPECTED = {pop_id: dict(KERNELS) for pop_id in POPULATIONS}
# ShockCooling3's reddened tables depend on the proposal: no one-launch form, the population takes the two launches
EXPECTED['P6'].update({form: 'population-phases' for form in FORMS if form != 'unbatched'})


def _transient(kind, sigma, a, seed, nw):
    """A transient on shared epochs (3 or 4 filters, a different epoch count per seed) with data from the oracle."""
    rng = np.random.default_rng(1000 + seed)
    truth, priors = (np.array(SHAPES[kind][0]), list(SHAPES[kind][1]))
    filts = list('UBri' if seed % 2 else 'Bgr') if kind == 'CompanionShocking' else list('BVgr')[:3 + seed % 2]
    if kind == 'CompanionShocking':
        epochs = 57001.5 + np.sort(rng.uniform(0., 40., 18 + 3 * seed))
    else:
        epochs = np.sort(rng.uniform(0.4, 16., 16 + 5 * seed))
    t, names = np.repeat(epochs, len(filts)), list(np.tile(filts, len(epochs)))
    bands = [O.band(n) for n in names]
    if kind == 'CompanionShocking':   # (the template is scaled to the observed peak: data from a smooth stand-in first)
        guess = 2e20 * np.exp(-0.5 * ((t - 57018.) / 12.) ** 2)
        ytrue = O.evaluate((kind, O.CompanionShockingOracle(bands, guess, Z, 1)), t, bands, truth)
    else:
        ytrue = O.evaluate((kind, ORACLES[kind](Z)), t, bands, truth)
    y = ytrue * (1 + 0.05 * rng.standard_normal(len(t)))
    dy = 0.05 * np.abs(ytrue)
    if kind == 'CompanionShocking':
        om = (kind, O.CompanionShockingOracle(bands, y, Z, 1))
        model = M.CompanionShocking(lc_dict(t, names, y, dy), redshift=Z)
        spread = np.array([0.05, 0.02, 0.05, 0.2, 0.01, 0.02, 0.02, 0.02])
    else:
        om = (kind, ORACLES[kind](Z))
        model = getattr(M, kind)(redshift=Z)
        spread = 0.03 * np.abs(truth)
    lc = lc_dict(t, names, y, dy)
    if kind == 'ShockCooling3':   # (fits 'flux')
        lc = {'MJD': lc['MJD'], 'filter': lc['filter'], 'flux': y, 'dflux': dy}
    if sigma:
        truth, spread, priors = np.append(truth, 0.5), np.append(spread, 0.05), priors + [M.UniformPrior(0., 5.)]
    x0 = truth + spread * rng.standard_normal((nw, len(truth)))
    pb = dict(model=om, t=t, bands=bands, y=y, dy=dy, priors=[p.descriptor() for p in priors], use_sigma=sigma)
    return dict(problem=(model, lc, priors) + (({'use_sigma': True},) if sigma else ()), ndim=len(truth), a=a, x0=x0,
                pb=pb, model=model, lc=lc, priors=priors, sigma=sigma)


def _run(sampler, x0, **kw):
    sampler.run_mcmc(x0, STEPS[0], **kw)
    sampler.run_mcmc(None, STEPS[1], **kw)


_REFS = {}


def _references(pop_id, random_split):
    """Per transient: its solo run and its oracle chain (computed once per population and split)."""
    key = (pop_id, random_split)
    if key not in _REFS:
        nw, specs = POPULATIONS[pop_id]
        refs = []
        for k, spec in enumerate(specs):
            tr = _transient(*spec, nw)
            eng = tr['model'].engine_for(tr['lc'], priors=tr['priors'], use_sigma=tr['sigma'])
            solo = EnsembleSampler(nw, tr['ndim'], eng, seed=SEED + k, a=tr['a'], randomize_split=random_split)
            _run(solo, tr['x0'])
            oracle = O.stretch_move_run(oracle_log_posterior(tr['pb']), tr['x0'], sum(STEPS), SEED + k, a=tr['a'],
                                        randomize_split=random_split)
            refs.append(((solo.get_chain(), solo.get_log_prob(), solo.acceptance_fraction), oracle))
        _REFS[key] = refs
    return _REFS[key]


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('pop_id', list(POPULATIONS))
def test_mixed_population_equals_solo_runs_and_oracle(pop_id, form, monkeypatch):
    nw, specs = POPULATIONS[pop_id]
    env, random_split, batched = FORMS[form]
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    refs = _references(pop_id, random_split)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    ts = [_transient(*spec, nw) for spec in specs]
    pop = PopulationSampler([tr['problem'] for tr in ts], nw, seed=SEED)
    for k, tr in enumerate(ts):
        assert pop[k].ndim == tr['ndim']
        if tr['a'] != 2.:   # (PopulationSampler takes one stretch scale: the transient's own sampler instead)
            pop.samplers[k] = EnsembleSampler(nw, tr['ndim'], pop[k].engine, seed=SEED + k, a=tr['a'])
        pop[k].randomize_split = random_split
    _run(pop, {k: tr['x0'] for k, tr in enumerate(ts)}, batched=batched)
    assert pop[0]._native.last_run_kernel() == EXPECTED[pop_id][form]
    if form == 'blocks of 2 steps' and EXPECTED[pop_id][form] == 'population-run':
        assert pop[0]._native.last_run_launches() == 2   # (the continuation's 3 steps: two blocks of draw records)
    n = sum(STEPS)
    for k, ((chain, lp, acc), (ref, ref_lp, ref_acc)) in enumerate(refs):
        got = (pop[k].get_chain(), pop[k].get_log_prob(), pop[k].acceptance_fraction)
        assert got[0].shape == (n, nw, ts[k]['ndim'])
        assert np.array_equal(got[0], chain), (pop_id, form, k)
        np.testing.assert_allclose(got[1], lp, rtol=1e-12, atol=1e-9, err_msg=f'{pop_id} {form} {k}')
        assert np.array_equal(got[2], acc), (pop_id, form, k)
        assert relerr(got[0], ref) < 1e-9 and relerr(got[1], ref_lp) < 1e-9, (pop_id, form, k)
        assert np.array_equal(np.round(got[2] * n).astype(int), ref_acc), (pop_id, form, k)
        # the accept test decides in both directions, so a wrong (n_dim - 1) ln z or z would move the chain
        assert 0.1 * nw * n < ref_acc.sum() < 0.9 * nw * n, (pop_id, k, ref_acc.sum())
