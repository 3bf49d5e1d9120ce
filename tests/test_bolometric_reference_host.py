"""The bolometric kernels' reference earns its trust without a GPU (tests/bolometric_reference.py): ``lstsq_ref``
against the reference project's own ``curve_fit`` on the 300 recorded epochs, ``pseudo_ref`` against the host's
``pseudo``, and every generated input of tests/test_gpu_bolometric_edges.py against the active set its name claims."""
import numpy as np

import bolometric_reference as BR
from conftest import golden
from helpers import LD_OK
from lightcurve_fitting_amd import bolometric as B

PG_ZERO = 1e-12 if LD_OK else 1e-7   # "zero to rounding" of the relative projected gradient (measured: <= 1e-14)


def test_lstsq_ref_is_at_least_as_good_as_the_recorded_curve_fit():
    """On the fixture's 300 epochs: the reference's cost is never above scipy's, its projected gradient is zero, and
    where it is not better than scipy by more than 1e-10 relative it agrees with the recorded T, R, dT, dR, cov within
    the tolerances of test_gpu_bolometric.py; the better ones (scipy stopped early) stay within that test's cap."""
    g = golden('bolometric')
    off, setup, result = g['ls/ep_off'], g['ls/setup'], g['ls/result']
    early = 0
    for e in range(len(setup)):
        f, y = g['ls/freq'][off[e]:off[e + 1]], g['ls/lum'][off[e]:off[e + 1]]
        z, cut, lo, hi = setup[e][0], setup[e][1], setup[e][[4, 5]], setup[e][[6, 7]]
        rT, rR, rdT, rdR, _, _, _, rcov, rcost = result[e]
        T, R, cost, pg = BR.lstsq_ref(f, y, z, cut, setup[e][2:4], lo, hi)
        m = len(f)
        floor = 1e-24 * np.sum(y ** 2)   # (m = 2: an exact fit, both costs are rounding)
        assert float(cost) <= rcost * (1 + 1e-9) + floor, (e, float(cost), rcost)
        assert lo[0] <= T <= hi[0] and lo[1] <= R <= hi[1]
        if m > 2:
            assert np.all(np.abs(pg) < PG_ZERO), (e, pg)
        if float(cost) < rcost * (1 - 1e-10) and m > 2:
            early += 1
            continue
        cov = BR.curve_fit_cov(f, z, cut, T, R, cost, m)
        if m <= 2:
            assert np.all(np.isinf(cov))
            assert abs(float(T) - rT) <= 1e-5 * rT and abs(float(R) - rR) <= 1e-5 * rR
            continue
        assert abs(float(T) - rT) <= max(1e-4 * rdT, 1e-5 * rT) and abs(float(R) - rR) <= max(1e-4 * rdR, 1e-5 * rR), e
        for got, want in ((np.sqrt(cov[0, 0]), rdT), (np.sqrt(cov[1, 1]), rdR), (cov[0, 1], rcov)):
            assert abs(got / want - 1.) <= 1e-4, (e, got, want)
    assert early <= 10, early


def test_pseudo_ref_equals_the_host_pseudo():
    T = np.concatenate([[0.3, 300., 0., -1., np.inf, np.nan], np.exp(np.linspace(np.log(0.3), np.log(300.), 400))])
    R = np.concatenate([[2., 2., 2., 2., 2., 2.], np.exp(np.linspace(np.log(0.01), np.log(100.), 400))])
    freq0, n_grid = BR.lum_grids()[0]
    assert (freq0, n_grid) == B._grid()
    for z, cut in BR.LUM_SETTINGS:
        want = B.pseudo(T, R, z, cutoff_freq=cut)
        got = BR.pseudo_ref(T, R, z, freq0, n_grid, cut)
        zero = want == 0.
        assert np.array_equal(zero, got == 0) and zero.sum() == 4
        assert np.max(np.abs(got[~zero] / want[~zero] - 1)) < 1e-13


def test_pseudo_ref_small_grids():
    T, R = np.array([5., 20.]), np.array([2., 3.])
    assert np.all(BR.pseudo_ref(T, R, 0., 300.5, 0, np.inf) == 0)
    one = BR.planck(300.5, T, R, np.inf) * 1e12
    assert np.allclose((BR.pseudo_ref(T, R, 0., 300.5, 1, np.inf) / (one / 2)).astype(float), 1., rtol=1e-15)
    two = (one + BR.planck(301.5, T, R, np.inf) * 1e12) / 2
    assert np.allclose((BR.pseudo_ref(T, R, 0., 300.5, 2, np.inf) / two).astype(float), 1., rtol=1e-15)


def test_curve_fit_cov_is_scipys_rule():
    """Against ``scipy.optimize.curve_fit`` itself on one well-conditioned epoch, and the rank-one / m <= 2 rules."""
    from scipy.optimize import curve_fit
    c = BR.fit_cases()[1]
    T, R, cost, _ = c.reference()
    model = lambda nu, T, R: BR.planck(nu, T, R, c.cut).astype(np.float64) / c.lum.max()
    p, pcov = curve_fit(model, c.freq * (1 + c.z), c.lum / c.lum.max(), p0=[float(T), float(R)],
                        bounds=(c.lo, c.hi), xtol=1e-14, ftol=1e-14, gtol=1e-14)
    cov = BR.curve_fit_cov(c.freq, c.z, c.cut, T, R, cost, c.m)
    assert np.max(np.abs(cov / pcov - 1)) < 1e-5    # (curve_fit's Jacobian is a finite difference)
    assert np.all(np.isinf(BR.curve_fit_cov(c.freq[:2], c.z, c.cut, T, R, cost, 2)))
    r1 = BR.rank_one_cases()[0]
    cov = BR.curve_fit_cov(r1.freq, r1.z, r1.cut, 8., 3., 1e38, r1.m)
    assert np.linalg.matrix_rank(cov) == 1 and np.all(np.isfinite(cov))


def test_fit_cases_land_on_the_active_set_they_claim():
    cases = BR.fit_cases()
    kinds = {}
    for k, c in enumerate(cases):
        T, R, cost, pg = c.reference()
        assert BR.active_set(T, R, c.lo, c.hi) == c.active, (k, c.kind, float(T), float(R), c.lo, c.hi)
        assert np.all(np.abs(pg) < PG_ZERO), (k, c.kind, pg)
        assert 3 <= c.m <= 20 and np.all(c.lo <= c.p0) and np.all(c.p0 <= c.hi)
        kinds[c.kind] = kinds.get(c.kind, 0) + 1
    assert kinds == {**{k: BR.N_PER_KIND for k in BR.ACTIVE_KINDS}, **{k: BR.N_PER_START for k in BR.START_KINDS}}
    assert {(c.z, c.cut) for c in cases} == set(BR.SETTINGS)
    assert all(c.cut < np.min(c.freq) for c in cases if c.cut == BR.CUT_BELOW)
    for kind in BR.START_KINDS:   # the start really is on the bounds named
        for c in (c for c in cases if c.kind == kind):
            on = BR.active_set(c.p0[0], c.p0[1], c.lo, c.hi)
            assert on == frozenset(kind[3:].split(',')), (kind, c.p0)


def test_special_cases_are_what_their_names_say():
    for c in BR.noiseless_cases():
        T, R, cost, _ = c.reference()
        assert abs(float(T) / c.truth[0] - 1) < 1e-12 and abs(float(R) / c.truth[1] - 1) < 1e-12
    for c in BR.rank_one_cases():
        assert 3 <= c.m <= 6 and np.all(c.freq == c.freq[0])
        _, dT, dR = BR.planck_jac(c.freq * (1 + c.z), 8., 3., c.cut)
        assert np.linalg.matrix_rank(np.column_stack([dT, dR]).astype(np.float64)) == 1
    for c in BR.zero_jacobian_cases():
        for T in (c.lo[0], c.p0[0], c.hi[0]):
            assert not np.any(BR.planck_jac(c.freq, T, c.hi[1], c.cut))
    for c in BR.hard_cases():   # the start is far from the optimum, which is interior
        T, R, _, pg = c.reference()
        assert BR.active_set(T, R, c.lo, c.hi) == frozenset() and np.all(np.abs(pg) < PG_ZERO)
        assert c.p0[0] / float(T) > 100 and c.p0[1] / float(R) > 1000
    for c in BR.zero_and_negative_cases():
        T, R, cost, _ = c.reference()
        if c.kind == 'zero':
            assert not c.lum.any() and R == c.lo[1]
        else:
            assert np.any(c.lum < 0)
    kinds = [c.kind for c in BR.mixed_cases()]
    assert set(kinds) == set(BR.MIXED_KINDS) and len(kinds) > 64
    for c in BR.mixed_cases():
        assert c.m == {'m0': 0, 'm1': 1, 'm2': 2}.get(c.kind, c.m)
        bad = not (np.isfinite(c.lum).all() and np.isfinite(c.freq).all())
        assert bad == (c.kind not in ('good', 'm0', 'm1', 'm2'))
    for c in BR.singular_cases():   # J^T J underflows to 0 somewhere in the box while J^T r does not
        _, dT, dR = (v.astype(np.float64) / c.lum.max() for v in BR.planck_jac(c.freq, c.p0[0], c.p0[1], c.cut))
        assert np.any(dR != 0) and not np.any(dR * dR) and not np.any(dT * dT)
    T, R = BR.lum_samples()
    assert len(T) == BR.LUM_N and (T == 0).any() and (T < 0).any() and np.isinf(T).any() and np.isnan(T).any()
    assert (R == 0).any() and (R < 0).any() and T[np.isfinite(T)].max() == 1e5 and T[T > 0].min() == 0.05
    for f0, ng in BR.lum_grids():
        assert BR.LUM_SETTINGS[-1][1] < f0
