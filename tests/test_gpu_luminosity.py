"""``luminosity_predictive`` on the GPU: the percentile bands of ``L(t)`` of the central-engine models against
``np.nanpercentile`` of the NumPy restatement (``central_reference``) to the project's 1e-11, and bit for bit against
the project's own evaluation; the valid and dark counts; a tie of more than ``kPqCap`` equal keys; NaN rows; the peaks
against the NumPy rule of ``test_luminosity_host.peak_rule``; independence of the tiling; a fit; the refusals."""
import numpy as np
import pytest

import central_reference as C
from conftest import relerr
from test_luminosity_host import peak_rule
from lightcurve_fitting_amd import engine as E
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.fitting import (lightcurve_mcmc, luminosity_predictive, posterior_predictive, quantile_lerp,
                                            quantile_ranks)

pytestmark = pytest.mark.gpu

TOL = 1e-11
Z = 0.02
KINDS = [('arnett', False), ('arnett', True), ('magnetar', False), ('magnetar', True)]
TIMES = np.concatenate([[-10., 1.], np.linspace(5., 150., 30)])   # before every explosion, between the groups', after
LC = {'MJD': TIMES, 'L_bol': np.ones(len(TIMES)), 'dL_bol': np.ones(len(TIMES))}
FIELDS = ('t', 'percentiles', 'luminosity', 'n_valid', 'n_dark', 'peak_index', 'L_peak', 't_peak', 't_rise')

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def model_of(kind, leak, z=Z):
    return (M.Arnett if kind == 'arnett' else M.Magnetar)(redshift=z, gamma_leakage=leak)


def rows(kind, leak, S, rng):
    """S parameter rows in random order: 40 % explode between MJD -6 and -4, the rest between 2 and 4."""
    U = lambda lo, hi: rng.uniform(lo, hi, S)
    late = np.arange(S) >= int(0.4 * S)
    t0 = np.where(late, rng.uniform(2., 4., S), rng.uniform(-6., -4., S))
    cols = [U(0.03, 0.15), U(5., 25.)] if kind == 'arnett' else [U(0.5, 2.), U(2., 20.), U(10., 40.)]
    if leak:
        cols.append(U(20., 80.))
    return np.column_stack(cols + [t0])[rng.permutation(S)]


def case1(kind, leak):
    """4096 rows, three of them NaN at every time, the restatement's L (rows, times), the percentiles -- one strictly
    inside the tie of zeros at MJD 1 and one at its edge -- and the default call's result, all computed once."""
    def make():
        S = 4096
        P = rows(kind, leak, S, np.random.default_rng(11))
        P[5, C.N_SOURCE[kind]] = -1.
        P[77, 0] = np.nan
        P[4000, -1] = np.inf
        Y = C.luminosity(kind, TIMES, P, Z, leak)
        k = int(np.sum(Y[:, 1] == 0.))
        inside, edge = 100. * (k // 2) / (S - 4), 100. * (k - 0.5) / (S - 4)
        q = np.array([0., 2.5, 15.87, 50., 84.14, 97.5, 100., inside, edge])
        res = luminosity_predictive(LC, model_of(kind, leak), P, percentiles=q, t=TIMES)
        return dict(P=P, Y=Y, q=q, k=k, res=res)
    return memo(('case1', kind, leak), make)


def assert_same(a, b):
    for name in FIELDS:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    assert (a.n_samples, a.n_peak_first, a.n_peak_last) == (b.n_samples, b.n_peak_first, b.n_peak_last)


@pytest.mark.parametrize('kind,leak', [('arnett', False), ('magnetar', True)])
def test_values_ties_nan_rows_and_peaks(kind, leak):
    c = case1(kind, leak)
    P, Y, q, res = c['P'], c['Y'], c['q'], c['res']
    S = len(P)
    # the preconditions, on the restatement alone
    nan_rows = np.all(np.isnan(Y), axis=1)
    assert nan_rows.sum() == 3 and np.array_equal(np.nonzero(nan_rows)[0], [5, 77, 4000])
    assert not np.any(np.isnan(Y[~nan_rows]))
    assert np.array_equal((Y == 0.).sum(0)[:4], [S - 3, 2455 if kind == 'arnett' else 2457, 0, 0])
    assert c['k'] > 2048                                  # more equal keys than a search sorts: the tie path
    want_idx, want_L, want_t, want_rise = peak_rule(Y, TIMES, P[:, -1], Z)
    ok = ~nan_rows
    assert np.all((want_idx[ok] > 0) & (want_idx[ok] < len(TIMES) - 1))   # no valid row peaks at a grid edge
    top2 = np.sort(Y[ok], axis=1)[:, -2:]
    gap = np.min((top2[:, 1] - top2[:, 0]) / top2[:, 1])
    print(f'{kind}: smallest relative gap between a row\'s two largest values {gap:.2e}')
    assert gap > 1e-6                                     # the restatement's peak index is unambiguous at 1e-11

    want = np.nanpercentile(Y, q, axis=0)
    err = relerr(res.luminosity, want)
    print(f'{kind}, leakage {leak}: bands against np.nanpercentile of the restatement {err:.2e}')
    assert err <= TOL
    assert res.luminosity.shape == (len(q), len(TIMES)) and res.n_samples == S
    assert np.array_equal(res.n_valid, np.full(len(TIMES), S - 3))
    assert np.array_equal(res.n_dark, (Y == 0.).sum(0))
    assert np.array_equal(res.frac_dark, (Y == 0.).sum(0) / (S - 3))
    assert np.all(res.luminosity[:, 0] == 0.) and not np.any(np.signbit(res.luminosity[:, 0]))
    assert res.luminosity[7, 1] == 0.                     # strictly inside the tie
    smallest = np.min(np.where(Y[:, 1] > 0., Y[:, 1], np.inf))
    assert relerr(res.luminosity[8:9, 1], [0.5 * smallest]) <= TOL   # half way from the last zero to the first value
    order = np.argsort(q)
    assert np.all(np.diff(res.luminosity[order], axis=0) >= 0.)

    assert res.peak_index.dtype == np.int32 and np.array_equal(res.peak_index, want_idx)
    assert np.array_equal(res.peak_index[nan_rows], [-1, -1, -1])
    err = relerr(res.L_peak, want_L)
    print(f'{kind}, leakage {leak}: L_peak against the restatement {err:.2e}')
    assert err <= TOL
    assert np.array_equal(res.t_peak, want_t, equal_nan=True)
    assert np.array_equal(res.t_rise, want_rise, equal_nan=True)
    assert res.n_peak_first == np.sum(want_idx == 0) == 0 and res.n_peak_last == np.sum(want_idx == len(TIMES) - 1) == 0
    summary = res.peak_summary((50.,))
    assert relerr(summary['L_peak'], np.nanpercentile(want_L, [50.])) <= TOL
    assert np.array_equal(summary['t_rise'], np.nanpercentile(want_rise, [50.]))


def test_bit_for_bit_against_the_models_own_evaluation():
    """102 400 samples: every pass loops over the samples of its workgroup, and the searches refine more than once."""
    S = 102400
    m = model_of('arnett', False)
    times = np.concatenate([[-10., 1.], np.linspace(5., 150., 38)])
    P = rows('arnett', False, S, np.random.default_rng(12))
    q = np.array([0., 2.5, 15.87, 50., 84.14, 97.5, 100.])
    Yd = np.concatenate([m(times, *P[k:k + 16384].T) for k in range(0, S, 16384)], axis=1)   # (times, samples)
    assert Yd.shape == (40, S) and not np.any(np.isnan(Yd))
    res = luminosity_predictive(LC, m, P, percentiles=q, t=times)
    srt = np.sort(Yd, axis=1)
    lo, hi, gamma = quantile_ranks(np.full((1, 40), S), q[:, None])
    at = np.arange(40)[None, :]
    assert np.array_equal(res.luminosity, quantile_lerp(srt[at, lo], srt[at, hi], gamma))
    assert relerr(res.luminosity, np.nanpercentile(Yd, q, axis=1)) <= TOL
    assert np.array_equal(res.n_valid, np.full(40, S)) and np.array_equal(res.n_dark, (Yd == 0.).sum(1))
    assert res.n_dark[0] == S and 2048 < res.n_dark[1] < S and res.n_dark[2] == 0
    want_idx, want_L, want_t, want_rise = peak_rule(Yd.T, times, P[:, -1], Z)
    assert np.array_equal(res.peak_index, want_idx) and np.array_equal(res.L_peak, want_L)
    assert np.array_equal(res.t_peak, want_t) and np.array_equal(res.t_rise, want_rise)


@pytest.mark.parametrize('kind,leak', KINDS)
def test_one_sample(kind, leak):
    """With one sample no interpolation happens: every percentile is the value itself."""
    m = model_of(kind, leak)
    p = rows(kind, leak, 4, np.random.default_rng(13))[0]
    times = np.array([150., 1., 30., -10., 12., 30., 60.])     # unsorted, one time twice
    want = m(times, *p)
    assert np.all(want[[0, 2, 4, 5, 6]] > 0.) and want[3] == 0.
    res = luminosity_predictive(LC, m, p[None, :], percentiles=(0., 15.87, 50., 100.), t=times)
    assert np.array_equal(res.luminosity, np.tile(want, (4, 1)))
    assert np.array_equal(res.n_valid, np.ones(7)) and res.n_samples == 1
    assert np.array_equal(res.n_dark, (want == 0.).astype(int))
    distinct = np.unique(times)
    assert res.peak_index[0] == np.nanargmax(m(distinct, *p)) and res.L_peak[0] == want.max()
    assert res.t_peak[0] == distinct[res.peak_index[0]]
    none = luminosity_predictive(LC, m, p[None, :], t=times, peak=False)
    assert none.peak_index is None and none.L_peak is None and none.t_rise is None and none.n_peak_first is None
    assert np.array_equal(none.luminosity, np.tile(want, (3, 1)))


def test_tiling_and_determinism():
    c = case1('arnett', False)
    P, q, res = c['P'], c['q'], c['res']
    m = model_of('arnett', False)
    # the documented memory formula (DESIGN.md "Luminosity bands and peaks"; engine.luminosity_workspace states it
    # too, and must agree): fixed part + per time of a tile.  Room for three times and a half: tiles of at most 3.
    n, nt, nq = len(P), len(TIMES), len(q)
    b = 4
    while b < 11 and (nq << (b + 1)) * 4 <= 48 * 1024:
        b += 1
    fixed = 12 * n + 8 * (nq + 1) * nt + 12 * nt + 4096
    per_time = 8 * n + nq * (56 + 8 * 2048) + 4 * max(2048, nq << b)
    assert E.luminosity_workspace(n, nt, nq, tile=3) == fixed + 3 * per_time
    tiled = luminosity_predictive(LC, m, P, percentiles=q, t=TIMES, workspace_bytes=fixed + 3 * per_time + per_time // 2)
    again = luminosity_predictive(LC, m, P, percentiles=q, t=TIMES)
    assert_same(tiled, res)
    assert_same(again, res)
    with pytest.raises(E.LcfError, match='workspace_bytes too small') as exc:
        luminosity_predictive(LC, m, P, percentiles=q, t=TIMES, workspace_bytes=1 << 12)
    assert exc.value.status == 1
    # one byte less than one time needs is refused, exactly that much is enough: the formula is the library's
    with pytest.raises(E.LcfError, match=f'at least {fixed + per_time} bytes'):
        luminosity_predictive(LC, m, P, percentiles=q, t=TIMES, workspace_bytes=fixed + per_time - 1)
    assert_same(luminosity_predictive(LC, m, P, percentiles=q, t=TIMES, workspace_bytes=fixed + per_time), res)


# ---- from a fit ---------------------------------------------------------------------------------------------------------
TRUTH = np.array([0.07, 12., -5.])           # M_Ni, tau_m, t_0 (tests/test_gpu_central.py)


def arnett_curve(noise=0.02):
    mjd = np.linspace(0., 90., 40)
    exact = np.array([C.truth('arnett', t - TRUTH[2], TRUTH[:1], TRUTH[1]) for t in mjd])
    deviates = np.random.default_rng(11).standard_normal(40)
    return {'MJD': mjd, 'L_bol': exact * (1. + noise * deviates), 'dL_bol': noise * exact}


def test_from_a_fit():
    lc = arnett_curve()
    m = M.Arnett()
    priors = [M.UniformPrior(0.001, 1.), M.UniformPrior(2., 60.), M.UniformPrior(-30., -0.01), M.UniformPrior(0., 10.)]
    np.random.seed(5)
    s = lightcurve_mcmc(lc, m, priors=priors, p_lo=[0.05, 9., -7., 0.1], p_up=[0.09, 15., -3., 1.], seed=2026,
                        nwalkers=32, nsteps=60, nsteps_burnin=60, use_sigma=True)
    res = luminosity_predictive(lc, m, s, discard=7, thin=3, use_sigma=True, num=50)
    flat = s.get_chain(discard=7, thin=3, flat=True)
    assert flat.shape == (18 * 32, 4) and res.n_samples == 18 * 32
    assert_same(res, luminosity_predictive(lc, m, flat, use_sigma=True, num=50))
    assert res.t.shape == (50,) and res.luminosity.shape == (3, 50) and np.all(res.n_valid == 18 * 32)
    assert np.all(np.isfinite(res.luminosity)) and np.all(res.luminosity[1, 1:] > 0.)
    assert np.all(res.t_rise > 0.) and res.n_peak_first == 0 and res.n_peak_last == 0
    with pytest.raises(ValueError, match='columns'):
        luminosity_predictive(lc, m, s, discard=7, thin=3, use_sigma=False)
    with pytest.raises(ValueError, match='discard'):
        luminosity_predictive(lc, m, s, discard=60)


def test_refusals_on_the_device():
    sc = M.ShockCooling(redshift=0.01)
    grid, _ = M.Model._eval_engine(sc, np.array([1., 2., 3.]), ['g'], False)
    with pytest.raises(E.LcfError, match='lcf_predict_quantiles') as exc:
        E.predict_luminosity(grid, np.ones((4, 5)), [50.])
    assert exc.value.status == 5
    with pytest.raises(E.LcfError, match='tempered') as exc:
        posterior_predictive(arnett_curve(), M.Arnett(), np.tile(TRUTH, (8, 1)), num=5)
    assert exc.value.status == 5
    # the library's own argument checks: too few columns, a percentile out of range
    eng = M.Arnett()._grid_engine(np.array([1., 2., 3.]))
    for args in ((np.ones((4, 2)), [50.]), (np.ones((4, 3)), [101.])):
        with pytest.raises(E.LcfError) as exc:
            E.predict_luminosity(eng, *args)
        assert exc.value.status == 1
