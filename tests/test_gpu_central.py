"""Central-engine models on the GPU: ``Arnett`` and ``Magnetar`` against the NumPy restatement of their definition
(``central_reference``) to the project's 1e-11 (``conftest.relerr``); batch independence bit for bit; NaN rows and rows
the prior excludes; sampling through the tempered driver decision for decision; recovery of a known truth; the
direction of a model comparison by the log-evidence; what is compiled per photometric model refusing with the route."""
import numpy as np
import pytest

import central_reference as C
import tempered_reference as R
from conftest import relerr
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.engine import LcfError
from lightcurve_fitting_amd.fitting import (chain_history, lightcurve_mcmc, make_log_posterior, posterior_corner,
                                            posterior_predictive, thermal_predictive)
from lightcurve_fitting_amd.sampler import EnsembleSampler, PopulationSampler, TemperedSampler

pytestmark = pytest.mark.gpu

TOL = 1e-11
Z = 0.02
SIGMA_MODES = ((False, 'relative'), (True, 'relative'), (True, 'absolute'))
# Epoch counts: one wave's share, a workgroup's share, and both sides of where the kernel splits a light curve into
# parts (lcf_central.hip: one part up to 64 epochs, four up to 256, eight beyond)
EPOCH_COUNTS = (1, 3, 64, 65, 256, 257, 300)
ROW_COUNTS = (1, 37, 300)
KINDS = [('arnett', False), ('arnett', True), ('magnetar', False), ('magnetar', True)]

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def model_of(kind, leak, z=Z):
    return memo(('model', kind, leak, z), lambda: (M.Arnett if kind == 'arnett' else M.Magnetar)(redshift=z, gamma_leakage=leak))


def rows_case(kind, leak):
    """300 epochs in random order over 130 days, data about a truth with 2 % errors, 300 rows (sigma last) scattered
    about it whose explosion times run from before the first epoch to after some of them, and the restatement's
    L (300 rows, 300 epochs), computed once."""
    def make():
        rng = np.random.default_rng(7 + 2 * (kind == 'magnetar') + leak)
        n = max(EPOCH_COUNTS)
        mjd = rng.permutation(np.linspace(1., 130., n) + rng.uniform(-0.2, 0.2, n))
        mjd[:3] = 3., 70., 6.5                           # (the shortest light curves too have epochs before an explosion)
        if kind == 'arnett':
            truth = [0.07, 12.]
            cols = [rng.uniform(0.03, 0.15, 300), rng.uniform(5., 25., 300)]
        else:
            truth = [1., 8., 20.]
            cols = [rng.uniform(0.5, 2., 300), rng.uniform(2., 20., 300), rng.uniform(10., 40., 300)]
        if leak:
            truth.append(45.)
            cols.append(rng.uniform(20., 80., 300))
        truth += [-4., 0.5]
        cols += [rng.uniform(-10., 8., 300), rng.uniform(0.1, 1., 300)]
        P = np.column_stack(cols)
        P[0] = truth
        y_true = C.luminosity(kind, mjd, [truth], Z, leak, True)[0]
        y = y_true * (1. + 0.02 * rng.standard_normal(n))
        dy = 0.02 * y_true * rng.uniform(0.7, 1.4, n)
        L = C.luminosity(kind, mjd, P, Z, leak, True)
        early = mjd[None, :] <= P[:, -2, None]
        assert early[:, :3].any() and (~early[:, :1]).any() and np.all(L[early] == 0.) and np.all(L[~early] > 0.)
        return dict(mjd=mjd, y=y, dy=dy, P=P, L=L)
    return memo(('rows', kind, leak), make)


def lc_of(c, n=None):
    return {'MJD': c['mjd'][:n], 'L_bol': c['y'][:n], 'dL_bol': c['dy'][:n]}


@pytest.mark.parametrize('kind,leak', KINDS)
def test_likelihood_parity(kind, leak):
    c = rows_case(kind, leak)
    m = model_of(kind, leak)
    worst = 0.
    for n in EPOCH_COUNTS:
        for use_sigma, sigma_type in SIGMA_MODES:
            P = np.ascontiguousarray(c['P'] if use_sigma else c['P'][:, :-1])
            want = C.gaussian_log_likelihood(c['L'][:, :n], c['y'][:n], c['dy'][:n], P[:, -1] if use_sigma else None,
                                             sigma_type)
            assert np.all(np.isfinite(want))              # (epochs before a row's explosion included: L = 0 there)
            eng = m.make_engine(c['mjd'][:n], c['y'][:n], c['dy'][:n], use_sigma, sigma_type)
            for rows in ROW_COUNTS:
                got = eng.log_likelihood(P[:rows])
                err = relerr(got, want[:rows])
                worst = max(worst, err)
                assert err <= TOL, (kind, leak, n, use_sigma, sigma_type, rows, err)
            eng.close()
    print(f'{kind}, leakage {leak}: worst relative error of the log-likelihood {worst:.2e}')


@pytest.mark.parametrize('kind,leak', KINDS)
def test_evaluation_parity(kind, leak):
    m = model_of(kind, leak, 0.)
    # explosion at MJD 5: epochs before it and at it; t = 0.01 d (with tau_m = 60); t = 400 d (with tau_m = 2, where
    # the range of the quadrature is cut)
    mjd = np.array([-20., 4.99, 5., 5.01, 6., 17., 55., 105., 405.])
    tau_m = np.array([60., 2., 12.])
    src = [np.array([0.07, 0.2, 0.05])] if kind == 'arnett' else [np.array([1., 0.3, 2.]), np.array([1., 100., 10.])]
    cols = src + [tau_m] + ([np.array([30., 50., 70.])] if leak else []) + [np.full(3, 5.)]
    want = C.luminosity(kind, mjd, np.column_stack(cols), 0., leak).T
    got = m(mjd, *cols)
    assert got.shape == (9, 3) and np.all(got[:3] == 0.) and not np.any(np.signbit(got[:3])) and np.all(got[3:] > 0.)
    s_lo, _ = C.pieces(400., 2.)
    assert s_lo > 399.                                    # the cut is active at (t, tau_m) = (400, 2)
    err = relerr(got, want)
    print(f'{kind}, leakage {leak}: L(t) against the restatement {err:.2e}')
    assert err <= TOL
    one = m(mjd, *[col[0] for col in cols])               # scalar parameters: (ntimes,)
    assert one.shape == (9,) and np.array_equal(one, got[:, 0])
    z = model_of(kind, leak)                              # ... and with a redshift
    assert relerr(z(mjd, *cols), C.luminosity(kind, mjd, np.column_stack(cols), Z, leak).T) <= TOL


def test_batch_independence_bit_for_bit():
    c = rows_case('arnett', True)
    m = model_of('arnett', True)
    lc = lc_of(c, 257)                                    # eight parts
    P300 = np.ascontiguousarray(c['P'][:, :-1])
    P37 = P300[:37]
    eng = m.engine_for(lc)
    l37, l300 = eng.log_likelihood(P37), eng.log_likelihood(P300)
    alone = np.array([eng.log_likelihood(P37[k:k + 1])[0] for k in range(37)])
    assert np.array_equal(alone, l37) and np.array_equal(l37, l300[:37]) and np.all(np.isfinite(l300))
    # ... and through the log-posterior with priors that exclude some rows: -inf there, the same bits elsewhere
    priors = [M.UniformPrior(0., 0.1), M.UniformPrior(0., 100.), M.UniformPrior(0., 100.), M.UniformPrior(-20., 4.)]
    excluded = (P300[:, 0] >= 0.1) | (P300[:, 3] >= 4.)
    assert 20 < excluded.sum() < 280 and 0 < excluded[:37].sum() < 37
    post = make_log_posterior(lc, m, priors)(P300)
    assert np.all(post[excluded] == -np.inf) and np.array_equal(post[~excluded], l300[~excluded])
    assert np.array_equal(m.engine_for(lc, priors=priors).log_posterior(P37), post[:37])
    assert m.log_likelihood(lc, P300[5]) == l300[5]       # (the model's own front end, one row)


def test_nan_rows_and_excluded_rows():
    c = rows_case('magnetar', False)
    m = model_of('magnetar', False)
    lc = lc_of(c, 65)
    P = np.ascontiguousarray(c['P'][:40, :-1])
    clean = m.log_likelihood(lc, P)
    bad = P.copy()
    bad[3, 0], bad[7, 2], bad[11, 1], bad[20, 3], bad[21, 2] = np.nan, -1., 0., np.inf, np.nan
    hit = np.zeros(40, dtype=bool)
    hit[[3, 7, 11, 20, 21]] = True
    got = m.log_likelihood(lc, bad)
    assert np.all(np.isnan(got[hit])) and np.array_equal(got[~hit], clean[~hit])
    assert relerr(got, C.log_likelihood('magnetar', lc['MJD'], lc['L_bol'], lc['dL_bol'], bad, Z)) <= TOL
    # the prior keeps t_p and tau_m positive: those rows are -inf, not NaN; a NaN inside the prior stays NaN
    priors = [M.UniformPrior(0., 10.), M.UniformPrior(0., 100.), M.UniformPrior(0., 100.), M.UniformPrior(-50., 50.)]
    post = m.engine_for(lc, priors=priors).log_posterior(bad)
    outside = np.zeros(40, dtype=bool)
    outside[[3, 7, 11, 20, 21]] = True                    # (a NaN or infinite coordinate is outside every interval)
    assert np.all(post[outside] == -np.inf) and np.array_equal(post[~outside], clean[~outside])
    free = m.engine_for(lc, priors=[M.UniformPrior(-np.inf, np.inf)] * 4).log_posterior(bad)
    assert np.all(np.isnan(free[[7, 11]])) and np.array_equal(free[~hit], clean[~hit])


# ---- sampling ---------------------------------------------------------------------------------------------------------
TRUTH = np.array([0.07, 12., -5.])           # M_Ni, tau_m, t_0: five days before the first epoch (MJD 0)
MCMC = dict(nwalkers=16, nsteps=30, nsteps_burnin=30)
BOX_LO, BOX_HI = np.array([0.05, 9., -7.]), np.array([0.09, 15., -3.])
MAG_LO, MAG_HI = np.array([0.1, 5., 8., -7.]), np.array([0.4, 20., 16., -3.])
SEED, START_SEED = 2026, 5


def arnett_priors():
    return [M.UniformPrior(0.001, 1.), M.UniformPrior(2., 60.), M.UniformPrior(-30., -0.01)]


def magnetar_priors():
    return [M.UniformPrior(0.001, 10.), M.UniformPrior(1., 100.), M.UniformPrior(2., 60.), M.UniformPrior(-30., -0.01)]


def arnett_curve(noise):
    """40 epochs from MJD 0 to 90 of the exact Arnett curve (``central_reference.truth``) at TRUTH, with Gaussian
    noise of the relative size ``noise`` from a seeded generator (the same deviates at every size)."""
    def make():
        mjd = np.linspace(0., 90., 40)
        exact = memo('exact', lambda: np.array([C.truth('arnett', t - TRUTH[2], TRUTH[:1], TRUTH[1]) for t in mjd]))
        deviates = np.random.default_rng(11).standard_normal(40)
        return {'MJD': mjd, 'L_bol': exact * (1. + noise * deviates), 'dL_bol': noise * exact}
    return memo(('curve', noise), make)


def restatement_log_like(pb, block):
    return C.log_likelihood('arnett', pb['t'], pb['y'], pb['dy'], np.atleast_2d(block))


def test_lightcurve_mcmc_makes_the_restatements_decisions(monkeypatch):
    lc = arnett_curve(0.02)
    np.random.seed(START_SEED)
    x0 = BOX_LO + (BOX_HI - BOX_LO) * np.random.rand(1, MCMC['nwalkers'], 3)
    pb = dict(t=lc['MJD'], y=lc['L_bol'], dy=lc['dL_bol'], priors=[p.descriptor() for p in arnett_priors()])
    monkeypatch.setattr(R, 'log_like', restatement_log_like)
    ref = memo('mcmc_ref', lambda: R.run(pb, x0, (1.,), 60, SEED))
    print(f'smallest accept margin of the restatement: {ref["move_margin"]:.3g}; moves accepted: {ref["nacc"].sum()}')
    assert ref['move_margin'] > 1e-6                      # the precondition, on the restatement alone
    np.random.seed(START_SEED)
    s = lightcurve_mcmc(lc, M.Arnett(), priors=arnett_priors(), p_lo=BOX_LO, p_up=BOX_HI, seed=SEED, **MCMC)
    assert isinstance(s, TemperedSampler) and s.ntemps == 1 and np.array_equal(s.betas, [1.])
    assert s.chain.shape == (16, 30, 3) and s.flatchain.shape == (480, 3) and s.acceptance_fraction.shape == (1, 16)
    assert np.array_equal(np.round(s.acceptance_fraction * 60).astype(int), ref['nacc'])     # identical move counts
    np.testing.assert_allclose(s.get_chain(temp=None), ref['chain'][30:], rtol=1e-9, atol=0.)
    np.testing.assert_allclose(s.get_log_like(), ref['lnL'][30:], rtol=1e-9, atol=0.)
    # the chain is a host array like any other
    assert posterior_corner(M.Arnett(), s.flatchain) is not None
    assert chain_history(M.Arnett(), np.ascontiguousarray(s.get_chain())) is not None


def test_recovery_of_the_truth():
    lc = arnett_curve(0.02)
    np.random.seed(START_SEED)
    s = lightcurve_mcmc(lc, M.Arnett(), priors=arnett_priors(), p_lo=BOX_LO, p_up=BOX_HI, seed=SEED, nwalkers=64,
                        nsteps=400, nsteps_burnin=400)
    flat = s.flatchain
    med, std = np.median(flat, axis=0), np.std(flat, axis=0)
    print('posterior medians', med, 'standard deviations', std, 'truth', TRUTH)
    assert flat.shape == (64 * 400, 3) and np.all(np.isfinite(flat))
    assert np.all(np.abs(med - TRUTH) < 4. * std)
    assert np.all(np.isfinite(s.get_autocorr_time(quiet=True)))


def evidence(kind, noise):
    def make():
        lc = arnett_curve(noise)
        arnett = kind == 'arnett'
        model = M.Arnett() if arnett else M.Magnetar()
        np.random.seed(START_SEED)
        s = lightcurve_mcmc(lc, model, priors=arnett_priors() if arnett else magnetar_priors(),
                            p_lo=BOX_LO if arnett else MAG_LO, p_up=BOX_HI if arnett else MAG_HI, seed=SEED, nwalkers=32,
                            nsteps=300, nsteps_burnin=300, ntemps=4, Tmax=np.inf)
        assert s.ntemps == 4 and s.betas[-1] == 0. and np.all(np.isfinite(s.chain))
        return s.log_evidence()
    return memo(('evidence', kind, noise), make)


def test_model_comparison_by_the_log_evidence():
    ev = {(kind, noise): evidence(kind, noise) for kind in ('arnett', 'magnetar') for noise in (0.02, 0.002)}
    for key, e in ev.items():
        print(key, f'ln Z = {e.lnZ:.2f} +- {e.dlnZ:.2f}')
        assert np.isfinite(e.lnZ) and np.isfinite(e.dlnZ) and e.reaches_prior
    coarse = ev['arnett', 0.02].lnZ - ev['magnetar', 0.02].lnZ
    fine = ev['arnett', 0.002].lnZ - ev['magnetar', 0.002].lnZ
    print(f'ln Z(Arnett) - ln Z(Magnetar): {coarse:.2f} at 2 % noise, {fine:.2f} at 0.2 %')
    assert coarse < fine                                  # the data tell the models apart better when they are better


def test_what_is_compiled_per_model_refuses_with_the_route():
    lc = arnett_curve(0.02)
    m = M.Arnett()
    eng = m.engine_for(lc, priors=arnett_priors())
    with pytest.raises(LcfError, match='tempered') as exc:
        EnsembleSampler(16, 3, eng)
    assert exc.value.status == 5
    with pytest.raises(LcfError, match='tempered') as exc:
        PopulationSampler([(M.Magnetar(), lc, magnetar_priors())], 16)
    assert exc.value.status == 5
    samples = np.tile(TRUTH, (8, 1))
    for fn in (posterior_predictive, thermal_predictive):
        with pytest.raises(LcfError, match='tempered') as exc:
            fn(lc, m, samples, num=5)
        assert exc.value.status == 5
    with pytest.raises(LcfError, match='tempered') as exc:
        m.temperature_radius(lc['MJD'], *TRUTH)
    assert exc.value.status == 5
    with pytest.raises(LcfError, match='tempered') as exc:           # the library's own refusal, below the model class
        eng.temperature_radius(TRUTH)
    assert exc.value.status == 5
    with pytest.raises(LcfError, match='tempered') as exc:
        eng.profile_loglike_kernel(TRUTH[None, :])
    assert exc.value.status == 5
    assert np.isfinite(eng.log_posterior(TRUTH)[0])       # the engine itself is fine
