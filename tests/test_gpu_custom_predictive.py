"""``custom_predictive`` on the GPU: the percentile bands of a custom model's light curves against ``np.nanpercentile`` of
the oracle around the NumPy restatement of its state function, those of T, R and L against the restatement itself, to
the project's 1e-11 (``L``: 6e-11, T enters to the fourth power and R squared); bit for bit against the model's own
evaluation; the counts; one and two samples; independence of the samples a sample is evaluated beside, of the tiling
and of the run; more percentiles than one native call takes; a fit; the refusals."""
import warnings

import numpy as np
import pytest

from conftest import relerr
from oracle import lcf_oracle as O
from test_gpu_custom import BOX_HI, BOX_LO, SEED, Z, floor_model, floor_state, memo, mcmc_priors, sc2_case, sc2_model
from lightcurve_fitting_amd import engine as E
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.fitting import (custom_predictive, lightcurve_mcmc, quantile_lerp, quantile_ranks)

pytestmark = pytest.mark.gpu

TOL = 1e-11
FILTERS = ['U', 'g', 'i']
DISTINCT = np.array([0.3, 0.8, 1.5, 2.5, 4., 6., 9.])
TIMES = np.concatenate([DISTINCT, [2.5]])                     # ... and one of them twice
Q = np.array([0., 2.5, 15.87, 50., 84.14, 97.5, 100.])
LC = {'MJD': TIMES, 'filter': ['g'] * len(TIMES), 'lum': np.ones(len(TIMES)), 'dlum': np.ones(len(TIMES))}
FLOORS = np.array([0.2, 0.4, 7., 9.])                          # [kK] two below every power law, two above the late ones
T_FLOOR = 0.5
NAN_ROWS = (5, 2050, 4097)                                     # first, a middle and the last wave of 4099 rows
HOT_ROWS = (70, 1000, 2100, 3000, 4090)                        # explode 1e-3 d before a grid time: T above 256 kK there
FIELDS = ('t', 'percentiles', 'quantiles', 'n_valid', 'n_dark', 'temperature', 'radius', 'luminosity', 'n_valid_thermal',
          'n_cold')


def bands():
    return [O.band(n) for n in FILTERS]


def draw_rows(n, rng, t0_lo=-0.5, t0_hi=3.):
    """Rows of the floor model as ``sc2_case`` draws them, the floor from four values."""
    return np.column_stack([rng.uniform(15., 25., n), rng.uniform(1., 3., n), rng.uniform(5., 15., n),
                            rng.uniform(t0_lo, t0_hi, n), rng.choice(FLOORS, n)])


def restate(times, P):
    """The restatement on ``times`` for rows ``P``: light curves (nf, nt, n) from the oracle, T, R (nt, n), L (nt, n)."""
    T, R = floor_state(times, P)
    with np.errstate(all='ignore'):
        Y = np.array([O.blackbody_to_filters_batch([b] * len(times), T, R, Z) for b in bands()])
        return Y, T, R, O.stefan_boltzmann(T, R)


def nanpct(a, q, axis):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)   # (every sample NaN: NaN)
        return np.nanpercentile(a, q, axis=axis)


def case1():
    """4099 rows -- a prime: no multiple of a wave or a workgroup, several chunks of samples per time -- three of them
    with NaNs, five hot ones; the restatement on the grid; the default call's result.  Computed once."""
    def make():
        n = 4099
        P = draw_rows(n, np.random.default_rng(21))
        for k, row in enumerate(HOT_ROWS):
            P[row, 3] = DISTINCT[1 + k % 4] - 1e-3
        # The row with a NaN T_1 has a NaN floor and a NaN L_1 too: fmax in the model's source returns the floor where
        # the power law is NaN, np.maximum of the restatement a NaN; and for a NaN temperature with a finite radius
        # (pw(NaN, -2) = 0) the library's light curve is NaN (include/lcf.h, "custom models"), the oracle's 0.  With
        # the three NaN the source and the restatement agree on T, R (NaN) and the library and the oracle on the rest.
        P[NAN_ROWS[0], [0, 1, 4]] = np.nan
        P[NAN_ROWS[1], 1] = np.nan
        P[NAN_ROWS[2], :] = np.nan
        Y, T, R, L = restate(TIMES, P)
        res = custom_predictive(LC, floor_model(), P, percentiles=Q, t=TIMES, filters_to_model=FILTERS, T_floor=T_FLOOR)
        return dict(P=P, Y=Y, T=T, R=R, L=L, res=res)
    return memo('cp_case1', make)


def assert_same(a, b):
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), name
    assert a.n_samples == b.n_samples and [f.name for f in a.filters] == [f.name for f in b.filters]


def test_values_ties_and_nan_rows():
    c = case1()
    P, Y, T, R, L, res = c['P'], c['Y'], c['T'], c['R'], c['L'], c['res']
    n = len(P)
    # the preconditions, on the inputs and the restatement alone
    assert n == 4099 and n % 64 != 0 and n % 256 != 0
    t0 = P[:, 3]
    assert np.nanmin(t0) < DISTINCT[0] and np.nanmax(t0) > DISTINCT[3]            # before the first, after the fourth time
    dark = (Y == 0.) & ~np.signbit(Y)
    assert np.all(dark[:, 0].sum(-1) > 2048) and np.all(dark[:, 3].sum(-1) > 100)    # ties at 0: more than a search sorts
    assert np.all(dark[:, 6].sum(-1) == 0)
    late = T[6][~np.isnan(T[6])]
    assert len(np.unique(late)) < len(late) - 100 and np.sum(late == 7.) > 50 and np.sum(late == 9.) > 50   # ties in T
    assert np.array_equal(np.nonzero(np.isnan(T).all(0))[0], [NAN_ROWS[0], NAN_ROWS[2]])
    assert np.array_equal(np.nonzero(np.isnan(L).all(0))[0], sorted(NAN_ROWS))
    assert np.array_equal(np.nonzero(np.isnan(Y).all((0, 1)))[0], sorted(NAN_ROWS))
    assert np.array_equal(np.nonzero(np.isnan(R).all(0))[0], sorted(NAN_ROWS))
    assert not np.any(np.isnan(T[:, NAN_ROWS[1]])) and np.isnan(P[NAN_ROWS[1]]).sum() == 1
    assert [k // 64 for k in NAN_ROWS] == [0, 32, 64] and (n - 1) // 64 == 64
    assert np.nanmax(T[:, list(HOT_ROWS)]) > 256. * (1. + Z)                        # beyond the interpolants: the tables
    with np.errstate(invalid='ignore'):
        assert not np.any(np.abs(T - T_FLOOR) <= 1e-9 * T_FLOOR)                    # no temperature at the floor's edge

    assert res.n_samples == n and res.quantiles.shape == (len(Q), 3, len(TIMES))
    assert [f.name for f in res.filters] == [O.band(f).name for f in FILTERS]
    e_y = relerr(res.quantiles, nanpct(Y, Q, -1))
    e_T, e_R = relerr(res.temperature, nanpct(T, Q, -1)), relerr(res.radius, nanpct(R, Q, -1))
    e_L = relerr(res.luminosity, nanpct(L, Q, -1))
    print(f'bands against np.nanpercentile of the restatement: light curves {e_y:.2e}, T {e_T:.2e}, R {e_R:.2e}, '
          f'L {e_L:.2e}')
    assert e_y <= TOL and e_T <= TOL and e_R <= TOL and e_L <= 6 * TOL
    assert np.array_equal(res.n_valid, (~np.isnan(Y)).sum(-1))
    assert np.array_equal(res.n_valid_thermal, [(~np.isnan(v)).sum(-1) for v in (T, R, L)])
    assert np.array_equal(res.n_dark, dark.sum(-1))
    with np.errstate(invalid='ignore'):
        cold = (T < T_FLOOR).sum(-1)
    assert np.array_equal(res.n_cold, cold) and cold[0] > 100 and cold[6] == 0
    assert np.array_equal(res.frac_cold, cold / (~np.isnan(T)).sum(-1))
    assert np.all(res.quantiles[0, :, 0] == 0.) and not np.any(np.signbit(res.quantiles[0, :, 0]))
    for name in ('quantiles', 'temperature', 'radius', 'luminosity'):
        v = getattr(res, name)
        assert np.all(np.diff(v, axis=0) >= 0.), name                                  # Q ascends
        assert np.array_equal(v[..., 3], v[..., 7]), name                              # the repeated time
    assert np.array_equal(res.n_cold[3], res.n_cold[7]) and np.array_equal(res.n_valid[:, 3], res.n_valid[:, 7])


def test_bit_for_bit_against_the_models_own_evaluation():
    """2053 rows that have all exploded before the first grid time: every temperature is where the interpolant or the
    main form of the band sum applies, so the model's evaluation -- which chooses the form per wavefront -- and the
    per-sample choice coincide."""
    m = floor_model()
    n = 2053
    rng = np.random.default_rng(22)
    P = draw_rows(n, rng, -0.5, 0.2)
    P[:, 4] = rng.uniform(0.1, 1., n)
    T, _ = floor_state(TIMES, P)
    a_max = np.max(M.PackedTables(FILTERS, z=Z).a)
    print(f'temperatures {T.min():.3g} ... {T.max():.3g} kK; a_max / T at most {a_max / T.min():.3g}')
    assert np.all(a_max / T < 170.)
    Yd = m(TIMES, FILTERS, *P.T)                                   # (nf, nt, n)
    Td, Rd = m.temperature_radius(TIMES, *P.T)                     # (nt, n) each
    assert Yd.shape == (3, len(TIMES), n) and Td.shape == (len(TIMES), n) and not np.any(np.isnan(Yd))
    res = custom_predictive(LC, m, P, percentiles=Q, t=TIMES, filters_to_model=FILTERS)
    lo, hi, gamma = quantile_ranks(n, Q)
    for got, values in ((res.quantiles, Yd), (res.temperature, Td), (res.radius, Rd)):
        srt = np.moveaxis(np.sort(values, axis=-1), -1, 0)
        assert np.array_equal(got, quantile_lerp(srt[lo], srt[hi], gamma.reshape((-1,) + (1,) * (srt.ndim - 1))))
    assert np.array_equal(res.n_valid, np.full((3, len(TIMES)), n)) and np.all(res.n_dark == 0) and res.n_cold is None


def test_one_sample_two_samples():
    m = floor_model()
    a, b = np.array([20., 2., 10., 0.1, 0.4]), np.array([22., 1.5, 12., 1., 0.2])
    one = custom_predictive(LC, m, a[None, :], percentiles=Q, t=TIMES, filters_to_model=FILTERS, T_floor=T_FLOOR)
    want = m(TIMES, FILTERS, *a)
    wT, wR = m.temperature_radius(TIMES, *a)
    assert one.n_samples == 1 and np.array_equal(one.quantiles, np.tile(want, (len(Q), 1, 1)))
    assert np.array_equal(one.temperature, np.tile(wT, (len(Q), 1))) and np.array_equal(one.radius, np.tile(wR, (len(Q), 1)))
    assert np.all(one.luminosity == one.luminosity[0]) and relerr(one.luminosity[0], O.stefan_boltzmann(wT, wR)) <= 6 * TOL
    assert np.all(one.n_valid == 1) and np.all(one.n_valid_thermal == 1)
    assert np.array_equal(one.n_dark, (want == 0.).astype(int)) and one.n_dark[0, 0] == 0
    assert np.array_equal(one.n_cold, (wT < T_FLOOR).astype(int)) and not np.any(one.n_cold)
    other = custom_predictive(LC, m, b[None, :], percentiles=(0., 100.), t=TIMES, filters_to_model=FILTERS, T_floor=T_FLOOR)
    assert np.array_equal(other.n_dark[:, :2], np.ones((3, 2))) and np.array_equal(other.n_cold, [1, 1, 0, 0, 0, 0, 0, 0])
    two = custom_predictive(LC, m, np.array([a, b]), percentiles=(0., 50., 100.), t=TIMES, filters_to_model=FILTERS,
                            T_floor=T_FLOOR)
    for name in ('quantiles', 'temperature', 'radius', 'luminosity'):
        x, y, got = getattr(one, name)[0], getattr(other, name)[0], getattr(two, name)
        assert np.array_equal(got[0], np.minimum(x, y)) and np.array_equal(got[2], np.maximum(x, y)), name
        assert np.array_equal(got[1], quantile_lerp(got[0], got[2], 0.5)), name
        assert relerr(got[1], 0.5 * (x + y)) <= TOL, name
    assert np.all(two.n_valid == 2) and np.array_equal(two.n_cold, other.n_cold)


def test_a_samples_values_do_not_depend_on_the_samples_beside_it():
    """The rows of the first test as they are and reversed: the same values in other wavefronts, so every order
    statistic is the same bits.  Then 130 of them -- the five hot ones among them, whose band sums at one time are the
    main form over the sample tables -- interleaved with 127 rows so cold that theirs are the safe form: 257 rows, every
    order statistic of which is a percentile (rank k is percentile 100 k / 256, exactly), and the values of five probe
    rows, evaluated alone, must be among them bit for bit.  A form chosen per wavefront fails here."""
    c = case1()
    m = floor_model()
    kw = dict(t=TIMES, filters_to_model=FILTERS)
    assert_same(custom_predictive(LC, m, c['P'][::-1], percentiles=Q, T_floor=T_FLOOR, **kw), c['res'])

    rng = np.random.default_rng(23)
    ok = np.setdiff1d(np.arange(len(c['P'])), NAN_ROWS + HOT_ROWS)
    subset = np.concatenate([HOT_ROWS, rng.choice(ok, 125, replace=False)])
    cold = draw_rows(127, rng, -0.5, 0.2)
    cold[:, 0], cold[:, 4] = 0.02, 0.01
    Tc, _ = floor_state(TIMES, cold)
    a = M.PackedTables(FILTERS, z=Z).a
    a_max, a_min = np.max(a), np.min(a)
    print(f'cold rows: {Tc.min():.3g} ... {Tc.max():.3g} kK, a / T at least {a_min / Tc.max():.3g}')
    assert np.all(a_min / Tc >= 170.)                              # every band sum of a cold row: the safe form
    rows = np.empty((257, 5))
    rows[1:254:2], rows[np.setdiff1d(np.arange(257), np.arange(1, 254, 2))] = cold, c['P'][subset]
    where = {int(k): i for i, k in zip(np.setdiff1d(np.arange(257), np.arange(1, 254, 2)), subset)}
    q_all = 100. * np.arange(257) / 256.
    lo, _, gamma = quantile_ranks(257, q_all)
    assert np.array_equal(lo, np.arange(257)) and np.all(gamma == 0.)
    mixed = custom_predictive(LC, m, rows, percentiles=q_all, **kw)
    assert np.all(mixed.n_valid == 257)
    hot_main = 0
    for k in HOT_ROWS:
        assert where[k] % 2 == 0 and where[k] < 64                # its wavefront: every other row a cold one
        alone = custom_predictive(LC, m, c['P'][k:k + 1], percentiles=(0., 100.), **kw)
        assert np.array_equal(alone.quantiles[0], alone.quantiles[1])
        for name in ('quantiles', 'temperature', 'radius', 'luminosity'):
            value, among = getattr(alone, name)[0], getattr(mixed, name)
            assert np.all(np.any(among == value[None], axis=0)), (k, name)
        Tk = c['T'][:, k]
        hot_main += int(np.sum((Tk > 256. * (1. + Z)) & (a_max / Tk < 170.)))
    assert hot_main >= 5                                           # each probe has a time on the sample tables' main form


def test_tiling_and_determinism():
    c = case1()
    P, res = c['P'], c['res']
    m = floor_model()
    kw = dict(percentiles=Q, t=TIMES, filters_to_model=FILTERS, T_floor=T_FLOOR)
    n, nt, nf, nq = len(P), len(DISTINCT), len(FILTERS), len(Q)
    one = E.custom_workspace(n, nt, nf, nq, tile=1)
    per_time = E.custom_workspace(n, nt, nf, nq, tile=2) - one
    b = 4
    while b < 11 and (nq << (b + 1)) * 4 <= 48 * 1024:
        b += 1
    assert per_time == (nf + 3) * (8 * n + nq * (56 + 8 * 2048) + 4 * max(2048, nq << b))
    assert one - per_time == 8 * (nq + 1) * (nf + 3) * nt + 20 * (nf + 3) * nt + 4096
    assert_same(custom_predictive(LC, m, P, workspace_bytes=one, **kw), res)                        # one time per tile
    assert_same(custom_predictive(LC, m, P, workspace_bytes=one + 2 * per_time + per_time // 2, **kw), res)   # 3.5
    assert_same(custom_predictive(LC, m, P, **kw), res)                                             # the default, again
    with pytest.raises(E.LcfError, match=f'workspace_bytes too small.*at least {one} bytes') as exc:
        custom_predictive(LC, m, P, workspace_bytes=one - 1, **kw)
    assert exc.value.status == 1
    with pytest.raises(E.LcfError, match='workspace_bytes too small'):
        custom_predictive(LC, m, P, workspace_bytes=1 << 12, **kw)


def test_more_percentiles_than_one_call_takes():
    c = case1()
    P = c['P'][:600]
    m = floor_model()
    kw = dict(t=TIMES, filters_to_model=FILTERS, T_floor=T_FLOOR)
    q = np.linspace(0., 100., 700)
    res = custom_predictive(LC, m, P, percentiles=q, **kw)
    first, second = custom_predictive(LC, m, P, percentiles=q[:512], **kw), custom_predictive(LC, m, P, percentiles=q[512:], **kw)
    for name in ('quantiles', 'temperature', 'radius', 'luminosity'):
        v = getattr(res, name)
        assert v.shape[0] == 700
        assert np.array_equal(v, np.concatenate([getattr(first, name), getattr(second, name)]), equal_nan=True), name
        assert np.array_equal(v[..., 3], v[..., 7], equal_nan=True), name
    for name in ('n_valid', 'n_dark', 'n_valid_thermal', 'n_cold'):
        assert np.array_equal(getattr(res, name), getattr(first, name)), name
        assert np.array_equal(getattr(res, name), getattr(second, name)), name


def test_use_sigma_and_the_sampler_as_the_source():
    m = floor_model()
    kw = dict(t=TIMES, filters_to_model=FILTERS)
    P = case1()['P'][:300]
    plain = custom_predictive(LC, m, P, **kw)
    assert plain.n_cold is None and plain.frac_cold is None
    with_sigma = np.column_stack([P, np.random.default_rng(24).uniform(0.1, 1., len(P))])
    assert_same(custom_predictive(LC, m, with_sigma, use_sigma=True, **kw), plain)

    lc = sc2_case(60)['lc']
    priors = mcmc_priors() + [M.UniformPrior(0., 5.)]
    np.random.seed(3)
    s = lightcurve_mcmc(lc, m, priors=priors, p_lo=np.append(BOX_LO, 0.2), p_up=np.append(BOX_HI, 0.9), seed=SEED,
                        nwalkers=16, nsteps=12, nsteps_burnin=12)
    assert hasattr(s, 'get_chain') and s.ntemps == 1
    flat = s.get_chain(discard=2, thin=3, flat=True)
    assert flat.shape == (4 * 16, 5)
    res = custom_predictive(lc, m, s, discard=2, thin=3, num=20)
    assert res.n_samples == 64 and res.quantiles.shape == (3, len(res.filters), 20) and res.n_cold is None
    assert_same(res, custom_predictive(lc, m, flat, num=20))
    assert np.all(res.n_valid == 64) and np.all(np.isfinite(res.temperature))


def test_refusals_on_the_device():
    sc = M.ShockCooling2(redshift=Z)
    with pytest.raises(E.LcfError, match='posterior_predictive') as exc:
        custom_predictive(LC, sc, np.tile([20., 2., 10., 0.1], (8, 1)), t=TIMES, filters_to_model=FILTERS)
    assert exc.value.status == 5
    grid, _ = M.Model._eval_engine(sc, DISTINCT, FILTERS, False)
    with pytest.raises(E.LcfError, match='lcf_predict_quantiles.*lcf_predict_luminosity') as exc:
        E.predict_custom(grid, np.ones((4, 4)), [50.])
    assert exc.value.status == 5
    m = sc2_model()
    t = np.tile(DISTINCT, 3)
    names = [f for f in FILTERS for _ in DISTINCT]
    bare = M.Model.make_engine(m, t, names, np.zeros(len(t)), np.ones(len(t)))     # a custom engine, no program attached
    with pytest.raises(E.LcfError, match='lcf_engine_set_custom') as exc:
        E.predict_custom(bare, np.ones((4, 4)), [50.])
    assert exc.value.status == 7
    twice = m.make_engine(np.append(t, t[0]), names + [names[0]], np.zeros(len(t) + 1), np.ones(len(t) + 1))
    with pytest.raises(E.LcfError, match='twice') as exc:
        E.predict_custom(twice, np.ones((4, 4)), [50.])
    assert exc.value.status == 1
    sparse = m.make_engine(t[:-1], names[:-1], np.zeros(len(t) - 1), np.ones(len(t) - 1))
    with pytest.raises(E.LcfError, match='every filter at every distinct time') as exc:
        E.predict_custom(sparse, np.ones((4, 4)), [50.])
    assert exc.value.status == 1
    # the library's own argument checks: too few columns, a percentile out of range, too many percentiles
    good, _ = M.Model._eval_engine(m, DISTINCT, FILTERS, False)
    for args in ((np.ones((4, 3)), [50.]), (np.ones((4, 4)), [101.]), (np.ones((4, 4)), np.linspace(0., 100., 513))):
        with pytest.raises(E.LcfError) as exc:
            E.predict_custom(good, *args)
        assert exc.value.status == 1
