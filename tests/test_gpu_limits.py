"""Censored non-detections on the GPU (``nondet='censored'``): the device's ``ln Phi`` alone against 60 digits; whole
log-likelihoods of every shock model and a ``CustomModel`` against ``limits_reference`` to the project's 1e-11
(``conftest.relerr``); batch independence bit for bit; the untouched default; the edges; sampling through the tempered
driver decision for decision, a ladder, and the resident samplers' refusal."""
import numpy as np
import pytest

import limits_reference as L
import tempered_reference as R
from conftest import relerr
from test_gpu_custom import BOX_HI, BOX_LO, MCMC, SEED, floor_model, mcmc_priors, sc2_model, sc2_state
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.engine import LcfError
from lightcurve_fitting_amd.fitting import lightcurve_mcmc, make_log_posterior
from lightcurve_fitting_amd.sampler import EnsembleSampler, PopulationSampler, TemperedSampler

pytestmark = pytest.mark.gpu

Z = L.Z
TOL = 1e-11
SIGMA_MODES = ((False, 'relative'), (True, 'relative'), (True, 'absolute'))
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def device_model(kind, c):
    """The package's model of the case (one per kind: it keeps its engines), and the reference's."""
    def make():
        if kind == 'custom':
            return sc2_model()
        if kind == 'CompanionShocking':
            return M.CompanionShocking(c['lc'], redshift=Z)
        return getattr(M, kind)(redshift=Z)
    return memo(('model', kind, len(c['t'])), make), (('custom', sc2_state, Z) if kind == 'custom' else c['model'])


# ---- 1. ln Phi alone ------------------------------------------------------------------------------------------------------
def phi_case(use_sigma):
    """A Blackbody engine on one detection with 130 limits attached, all in one filter: dy fixed, L_lim = m0 + z dy."""
    def make():
        bb = M.Blackbody(redshift=Z)
        p = (12., 1.5)
        z = L.z_sweep()
        t, f = np.linspace(1., 2., len(z)), ['r'] * len(z)
        m = bb(t, f, *p)                                             # the device's own model values
        assert m.shape == (130,) and np.all(m == m[0]) and np.isfinite(m[0]) and m[0] > 0.
        dy = np.full(len(z), 1e-3 * m[0])
        L_lim = m[0] + z * dy
        eng = bb.make_engine([1.5], ['r'], [m[0]], [0.05 * m[0]], use_sigma=use_sigma)
        at = bb.make_engine(t, f, np.zeros(len(z)), dy, use_sigma=use_sigma)
        eng.set_limits(at, L_lim, dy)
        return dict(bb=bb, p=p, m=m, dy=dy, L_lim=L_lim, eng=eng, at=at, t=t, f=f)
    return memo(('phi', use_sigma), make)


@pytest.mark.parametrize('use_sigma', [False, True])
def test_log_ndtr_of_the_device_against_60_digits(use_sigma):
    c = phi_case(use_sigma)
    s = np.array([0., 0.3, 2.5])
    P = np.column_stack([np.full(3, c['p'][0]), np.full(3, c['p'][1])] + ([s] if use_sigma else []))
    got = c['eng'].limit_terms(P)
    assert got.shape == (3, 130)
    sigma = np.sqrt(c['dy'] ** 2. + (s[:, None] * c['dy']) ** 2.) if use_sigma else c['dy'][None, :]
    z = np.broadcast_to((c['L_lim'] - c['m']) / sigma, got.shape)    # rebuilt from the device's own m: one -, one /
    assert abs(z.min() + 1e4) < 1e-6 and z.max() > 36.9 and np.any(z == 0.) and np.any((z < -38.5) & (z > -38.7)) \
        and np.any((z > -38.5) & (z < -38.3))
    want = L.log_ndtr_exact(z)
    naive = L.log_ndtr_naive(z)
    err = np.abs(got / want - 1.)
    print(f'use_sigma={use_sigma}: device ln Phi vs 60 digits over z in [{z.min():.3g}, {z.max():.3g}]: max rel err '
          f'{err.max():.2e} at z = {z.ravel()[np.argmax(err)]:.4g}; left of 0: {err[z <= 0].max():.2e}, right: '
          f'{err[z > 0].max():.2e}; the naive form: {np.max(np.abs(naive[np.isfinite(naive)] / want[np.isfinite(naive)] - 1.)):.2e}, '
          f'{np.sum(~np.isfinite(naive))} of {z.size} -inf')
    assert relerr(got, want) < TOL
    assert np.all(got < 0.) and np.all(np.diff(got, axis=1) >= 0.)   # increasing with z, never rounded to 0


# ---- 2. whole log-likelihoods ---------------------------------------------------------------------------------------------
CASES = [(kind, 13) for kind in ('ShockCooling2', 'custom', 'ShockCooling', 'ShockCooling3', 'ShockCooling4',
                                 'CompanionShocking')] + \
        [(kind, n) for kind in ('ShockCooling2', 'custom') for n in (1, 64, 65, 130)]


@pytest.mark.parametrize('kind,n_lim', CASES)
@pytest.mark.parametrize('use_sigma,sigma_type', SIGMA_MODES)
def test_log_likelihood_against_the_reference(kind, n_lim, use_sigma, sigma_type):
    c = L.case('ShockCooling2' if kind == 'custom' else kind, n_lim)
    model, ref_model = device_model(kind, c)
    P = L.rows(c, use_sigma)
    kw = dict(use_sigma=use_sigma, sigma_type=sigma_type)
    got = model.log_likelihood(c['lc'], P, nondet='censored', **kw)
    want = L.log_likelihood(ref_model, c['t'], c['bands'], c['y'], c['dy'], c['nondet'], P, **kw)
    terms = model.limit_terms(c['lc'], P, **kw)
    want_terms = L.limit_terms(ref_model, c['t'], c['bands'], c['dy'], c['nondet'], P, **kw)
    detections = model.log_likelihood(L.without_limits(c), P, **kw)
    assert terms.shape == (L.N_ROWS, n_lim) and np.all(terms <= 0.)
    e_ref, e_sum = relerr(got, want), relerr(terms.sum(axis=1) + detections, got)
    share = np.abs(terms.sum(axis=1) / got)
    print(f'{kind}, {n_lim} limits, sigma {use_sigma}/{sigma_type}: vs reference {e_ref:.2e}; terms + detections vs total '
          f'{e_sum:.2e}; terms vs reference {relerr(terms.sum(axis=1), want_terms.sum(axis=1)):.2e}; the limits are '
          f'{share.min():.1e} ... {share.max():.1e} of |ln L|, z of both signs: '
          f'{bool(np.any(terms > np.log(0.5)) and np.any(terms < np.log(0.5)))}')
    assert np.all(np.isfinite(want)) and not np.array_equal(got, detections)
    assert e_ref < TOL and e_sum < TOL
    # the default treatment is another number: the limits as measurements of zero
    assert relerr(model.log_likelihood(c['lc'], P, **kw), got) > 1e-6


# ---- 3. batch independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ShockCooling2', 'custom'])
def test_batch_independence_bit_for_bit(kind):
    c = L.case('ShockCooling2', 65)
    model, _ = device_model(kind, c)
    P37 = L.rows(c, False)
    rng = np.random.default_rng(5)
    P300 = np.concatenate([P37, P37[rng.integers(0, L.N_ROWS, 263)] * rng.uniform(0.9, 1.1, (263, 4))])
    eng = model.engine_for(c['lc'], nondet='censored')
    assert eng.nlimits == 65
    l37, l300 = eng.log_likelihood(P37), eng.log_likelihood(P300)
    t37, t300 = eng.limit_terms(P37), eng.limit_terms(P300)
    alone = np.array([eng.log_likelihood(P37[k:k + 1])[0] for k in range(L.N_ROWS)])
    t_alone = np.concatenate([eng.limit_terms(P37[k:k + 1]) for k in range(L.N_ROWS)])
    assert np.array_equal(alone, l37) and np.array_equal(l37, l300[:L.N_ROWS]) and not np.any(np.isnan(l300))
    assert np.array_equal(t_alone, t37) and np.array_equal(t37, t300[:L.N_ROWS]) and t300.shape == (300, 65)


# ---- 4. nothing changes without limits ------------------------------------------------------------------------------------
def test_nothing_changes_without_limits():
    c = L.case('ShockCooling2', 13)
    model, _ = device_model('ShockCooling2', c)
    P = L.rows(c, False)
    plain = L.without_limits(c)
    for lc in (plain, dict(plain, nondet=np.zeros(60, dtype=bool))):
        assert model.engine_for(lc, nondet='censored') is model.engine_for(plain)          # the same engine, the same route
        assert np.array_equal(model.log_likelihood(lc, P, nondet='censored'), model.log_likelihood(plain, P))
        assert model.limit_terms(lc, P).shape == (L.N_ROWS, 0) and model.limit_terms(lc, P[0]).shape == (0,)
    # the default on the light curve WITH limits is the call without the keyword: the rows as measurements of zero
    assert np.array_equal(model.log_likelihood(c['lc'], P, nondet='gaussian'), model.log_likelihood(c['lc'], P))
    assert model.engine_for(c['lc'], nondet='gaussian') is model.engine_for(c['lc'])
    assert model.engine_for(c['lc'], nondet='censored') is not model.engine_for(c['lc'])
    # a fit of a light curve without limits is the resident sampler's, the same chain
    runs = []
    for kw in ({}, {'nondet': 'censored'}):
        np.random.seed(3)
        runs.append(lightcurve_mcmc(plain, model, priors=mcmc_priors(), p_lo=BOX_LO, p_up=BOX_HI, seed=SEED, nwalkers=16,
                                    nsteps=10, nsteps_burnin=10, **kw))
    assert all(isinstance(s, EnsembleSampler) for s in runs) and np.array_equal(runs[0].chain, runs[1].chain)
    # detaching gives an engine its old values bit for bit
    det = np.nonzero(~c['nondet'])[0]
    lim = np.nonzero(c['nondet'])[0]
    names = c['lc']['filter']
    eng = model.make_engine(c['t'][det], [names[k] for k in det], c['y'][det], c['dy'][det])
    at = model.make_engine(c['t'][lim], [names[k] for k in lim], np.zeros(13), c['dy'][lim])
    before = eng.log_likelihood(P)
    eng.set_limits(at, 3. * c['dy'][lim], c['dy'][lim])
    with_limits = eng.log_likelihood(P)
    eng.set_limits(None, None, None)
    assert np.array_equal(eng.log_likelihood(P), before) and not np.array_equal(with_limits, before)
    assert np.array_equal(with_limits, model.log_likelihood(c['lc'], P, nondet='censored'))
    with pytest.raises(LcfError) as exc:
        eng.limit_terms(P)
    assert exc.value.status == 7


# ---- 5. edges -------------------------------------------------------------------------------------------------------------
def test_edges_of_the_rows():
    c = L.case('ShockCooling2', 13)
    model, _ = device_model('ShockCooling2', c)
    P = L.rows(c, False)
    priors = [M.UniformPrior(0., 50.), M.UniformPrior(-5., 2.5), M.UniformPrior(0., 100.), M.UniformPrior(-4., 1.5)]
    excluded = (P[:, 1] >= 2.5) | (P[:, 3] >= 1.5)
    assert 3 < excluded.sum() < 30
    post = make_log_posterior(c['lc'], model, priors=priors, nondet='censored')(P)
    like = model.log_likelihood(c['lc'], P, nondet='censored')
    assert np.all(post[excluded] == -np.inf) and np.array_equal(post[~excluded], like[~excluded])
    # a negative luminosity scale is a NaN model value wherever the row has exploded (the reference's sqrt(L)): NaN, as
    # for a detection; outside the prior the row stays -inf
    bad = P[:4].copy()
    bad[:, 1], bad[:, 3] = -1., -3.5
    lim = np.nonzero(c['nondet'])[0]
    assert np.all(np.isnan(model(c['t'][lim], [c['lc']['filter'][k] for k in lim], *bad[1])))
    assert np.all(np.isnan(model.log_likelihood(c['lc'], bad, nondet='censored')))
    assert np.all(np.isnan(model.limit_terms(c['lc'], bad)))
    bad[0, 3] = 2.
    out = make_log_posterior(c['lc'], model, priors=priors, nondet='censored')(bad)
    assert out[0] == -np.inf and np.all(np.isnan(out[1:]))


def test_edges_of_the_terms():
    c = phi_case(False)
    bb, m0 = c['bb'], c['m'][0]
    t, f = c['t'][:4], c['f'][:4]
    eng = bb.make_engine([1.5], ['r'], [m0], [0.05 * m0])
    at = bb.make_engine(t, f, np.zeros(4), np.ones(4))
    dy = np.array([1e-3 * m0, 1e-160 * m0, 1e-150 * m0, 1e-3 * m0])
    eng.set_limits(at, np.array([m0, 0., 0., 2. * m0]), dy)
    P = np.array([c['p'], (c['p'][0], 1e200), (c['p'][0], np.nan)])
    assert bb(t, f, *P[1])[0] == np.inf and np.isnan(bb(t, f, *P[2])[0])     # (a model at +inf, a NaN model)
    got = eng.limit_terms(P)
    z0 = (np.array([m0, 0., 0., 2. * m0]) - m0) / dy
    assert z0[0] == 0. and z0[1] < -1e154 and -1e154 < z0[2] < -1e149 and z0[3] == 1e3
    assert got[0, 0] == np.log(0.5) and got[0, 1] == -np.inf and got[0, 3] == 0.   # z^2 overflows; ln Phi(1000) = -0.
    assert np.isfinite(got[0, 2]) and relerr(got[0, 2:3], L.log_ndtr_exact(z0[2:3])) < TOL
    assert np.all(got[1] == -np.inf) and np.all(np.isnan(got[2]))
    like = eng.log_likelihood(P)
    assert like[0] == -np.inf and like[1] == -np.inf and np.isnan(like[2])


def test_what_cannot_be_attached_is_refused():
    c = L.case('ShockCooling2', 13)
    lim = np.nonzero(c['nondet'])[0]
    det = np.nonzero(~c['nondet'])[0]
    names = c['lc']['filter']
    dy = c['dy'][lim]

    def engines(model, at_model, **at_kw):
        return (model.make_engine(c['t'][det], [names[k] for k in det], c['y'][det], c['dy'][det]),
                at_model.make_engine(c['t'][lim], [names[k] for k in lim], np.zeros(13), dy, **at_kw))
    sc2 = M.ShockCooling2(redshift=Z)
    for model, at_model, kw in ((sc2, M.ShockCooling(redshift=Z), {}),                   # another model (and n_par)
                                (M.ShockCooling(redshift=Z), M.ShockCooling4(redshift=Z), {}),   # ... the same n_par
                                (sc2_model(), floor_model(), {}),                        # another n_par of one model id
                                (sc2, sc2, dict(use_sigma=True)),                        # another use_sigma
                                (sc2, M.ShockCooling2(redshift=Z, n=3.), {})):           # other constants
        eng, at = engines(model, at_model, **kw)
        with pytest.raises(LcfError, match="limits' engine") as exc:
            eng.set_limits(at, 3. * dy, dy)
        assert exc.value.status == 1
    eng, at = engines(sc2, sc2)
    for L_lim, d in ((3. * dy, np.where(np.arange(13) == 5, 0., dy)), (3. * dy, -dy), (3. * dy, dy * np.inf),
                     (np.where(np.arange(13) == 12, np.nan, 3. * dy), dy), (3. * dy[:12], dy[:12])):
        with pytest.raises(LcfError) as exc:
            eng.set_limits(at, L_lim, d)
        assert exc.value.status == 1
    with pytest.raises(LcfError) as exc:                                 # (nothing was attached by the refused calls)
        eng.limit_terms(L.rows(c, False))
    assert exc.value.status == 7
    # a live resident sampler computes the likelihood itself: no limits under it
    sampler = EnsembleSampler(16, 4, eng)
    with pytest.raises(LcfError, match='tempered') as exc:
        eng.set_limits(at, 3. * dy, dy)
    assert exc.value.status == 5
    del sampler
    # a bolometric table has no non-detections
    arnett = M.Arnett()
    mjd = np.linspace(5., 60., 12)
    a = arnett.make_engine(mjd, np.full(12, 1e35), np.full(12, 1e34))
    b = arnett.make_engine(mjd[:3], np.zeros(3), np.ones(3))
    with pytest.raises(LcfError, match='bolometric') as exc:
        a.set_limits(b, np.full(3, 1e34), np.full(3, 1e33))
    assert exc.value.status == 5
    with pytest.raises(LcfError, match='bolometric') as exc:
        arnett.engine_for({'MJD': mjd, 'L_bol': np.full(12, 1e35), 'dL_bol': np.full(12, 1e34),
                           'nondet': np.arange(12) < 2}, nondet='censored')
    assert exc.value.status == 5


# ---- 6. sampling, decision for decision -----------------------------------------------------------------------------------
def mcmc_reference(monkeypatch):
    """The start ``lightcurve_mcmc`` draws under np.random.seed(3), and 40 steps of the restatement from it, with the
    censored likelihood and -- for the precondition -- without the limits."""
    c = L.case('ShockCooling2', 13)
    np.random.seed(3)
    x0 = BOX_LO + (BOX_HI - BOX_LO) * np.random.rand(1, MCMC['nwalkers'], 4)
    pb = dict(c, priors=[p.descriptor() for p in mcmc_priors()])

    def run(log_like):
        monkeypatch.setattr(R, 'log_like', log_like)
        return R.run(pb, x0, (1.,), 40, SEED)
    return c, x0, memo('mcmc_ref', lambda: run(L.censored_log_like)), memo('mcmc_plain', lambda: run(L.gaussian_log_like))


def test_lightcurve_mcmc_makes_the_restatements_decisions(monkeypatch):
    c, x0, ref, plain = mcmc_reference(monkeypatch)
    final = L.limit_terms(c['model'], c['t'], c['bands'], c['dy'], c['nondet'], ref['chain'][-1, 0]).sum(axis=1)
    print(f'smallest accept margin of the restatement: {ref["move_margin"]:.3g}; moves accepted: {ref["nacc"].sum()} '
          f'(without the limits: {plain["nacc"].sum()}); NaN proposals: {ref["nan_proposals"]}; the censored term over the '
          f'final ensemble: {final.min():.2f} ... {final.max():.2f}')
    assert ref['move_margin'] > 1e-6                                     # the preconditions, on the restatement alone:
    assert not np.array_equal(ref['chain'], plain['chain'])              # ... and the limits decide moves
    model, _ = device_model('ShockCooling2', c)
    np.random.seed(3)
    s = lightcurve_mcmc(c['lc'], model, priors=mcmc_priors(), p_lo=BOX_LO, p_up=BOX_HI, seed=SEED, nondet='censored',
                        **MCMC)
    assert isinstance(s, TemperedSampler) and s.ntemps == 1 and np.array_equal(s.betas, [1.])
    assert s.chain.shape == (16, 20, 4) and s.flatchain.shape == (320, 4) and s.acceptance_fraction.shape == (1, 16)
    assert np.array_equal(np.round(s.acceptance_fraction * 40).astype(int), ref['nacc'])     # identical move counts
    np.testing.assert_allclose(s.get_chain(temp=None), ref['chain'][20:], rtol=1e-12, atol=0.)
    np.testing.assert_allclose(s.get_log_like(), ref['lnL'][20:], rtol=TOL, atol=0.)
    assert np.all(np.isfinite(s.get_autocorr_time(quiet=True)))
    # the CustomModel restatement through the same call: decision for decision
    np.random.seed(3)
    b = lightcurve_mcmc(c['lc'], sc2_model(), priors=mcmc_priors(), p_lo=BOX_LO, p_up=BOX_HI, seed=SEED,
                        nondet='censored', **MCMC)
    assert isinstance(b, TemperedSampler) and np.array_equal(b.acceptance_fraction, s.acceptance_fraction)
    np.testing.assert_allclose(b.get_chain(temp=None), s.get_chain(temp=None), rtol=1e-12, atol=0.)


# ---- 7. a ladder ----------------------------------------------------------------------------------------------------------
def test_a_ladder_tempers_the_term_with_the_likelihood():
    c = L.case('ShockCooling2', 13)
    model, _ = device_model('ShockCooling2', c)
    np.random.seed(3)
    s = lightcurve_mcmc(c['lc'], model, priors=mcmc_priors(), p_lo=BOX_LO, p_up=BOX_HI, seed=SEED, ntemps=3,
                        Tmax=np.inf, nondet='censored', **MCMC)
    assert s.ntemps == 3 and s.chain.shape == (16, 20, 4) and np.all(np.isfinite(s.chain))
    ev = s.log_evidence()
    assert np.isfinite(ev.lnZ) and np.isfinite(ev.dlnZ) and ev.reaches_prior
    cold = np.ascontiguousarray(s.get_chain(temp=0).reshape(-1, 4))
    stored = s.get_log_like(temp=0).reshape(-1)
    e_cold = relerr(stored, model.log_likelihood(c['lc'], cold, nondet='censored'))
    terms = model.limit_terms(c['lc'], cold).sum(axis=1)
    print(f'stored ln L of the cold rung vs log_likelihood of its rows: {e_cold:.2e}; lnZ = {ev.lnZ:.3f} +- {ev.dlnZ:.3f}; '
          f'the censored terms of the stored rows: {terms.min():.2f} ... {terms.max():.2f}')
    assert e_cold < TOL and terms.min() < -0.5       # the term is in the tempered likelihood, and it is not negligible


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------
def test_the_resident_samplers_refuse_with_the_route():
    c = L.case('ShockCooling2', 13)
    model, _ = device_model('ShockCooling2', c)
    eng = model.engine_for(c['lc'], priors=mcmc_priors(), nondet='censored')
    with pytest.raises(LcfError, match='tempered') as exc:
        EnsembleSampler(16, 4, eng)
    assert exc.value.status == 5
    with pytest.raises(LcfError, match='tempered') as exc:
        PopulationSampler([(model, c['lc'], mcmc_priors(), {'nondet': 'censored'})] * 2, 16)
    assert exc.value.status == 5
    with pytest.raises(LcfError, match='tempered') as exc:
        eng.profile_loglike_kernel(L.rows(c, False))
    assert exc.value.status == 5
    assert np.all(np.isfinite(eng.log_posterior(L.rows(c, False)[:1])))          # (the engine is as it was)
