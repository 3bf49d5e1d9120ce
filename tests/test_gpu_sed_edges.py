"""The per-epoch SED engine's paths that the golden epochs never reach: the list of candidates outside the interpolants'
range and k_sed_rest, the list's state from call to call, per-filter validity, the grid stride of k_sed_interp, small
shapes, the zero model, band tables outside LDS with more filters than the interpolants' LDS holds, and a fuzz sweep.

Everything is compared with helpers.sed_reference (np.longdouble; tests/test_sed_reference_host.py checks it and the
input families on the host).  Tolerance (helpers.sed_tolerances): the project's 1e-11 wherever the float64 oracle is
within 1e-12 of the reference; for candidates colder than 0.937 kK (1 + z) ``max(1e-11, 10 d_cold)`` with ``d_cold`` the
oracle's own deviation from the reference on the same candidates.  Where np.longdouble is float64 the float64 oracle
stands in for the reference (``H.LD_OK`` is False then, and every message says so).

Measured on an MI355X: every docstring below gives the worst |device - reference| / |reference| of its family over both
float64 precisions, both kinds of band table and the three forms; the tests print the same figures per call.
The largest d_cold is 2.3e-12 (fuzz seed 0, z = 0.3) and 2.2e-12 (listed candidates, no sigma)."""
import numpy as np
import pytest

import helpers as H
from lightcurve_fitting_amd import bolometric as B, engine as E

pytestmark = pytest.mark.gpu

AGAINST = 'the np.longdouble reference' if H.LD_OK else 'the float64 oracle (np.longdouble is float64 here)'
ITEMS_OF_LARGEST_LAUNCH = 8192   # k_sed_interp: at most 512 workgroups of 16 waves, one (epoch, 64 candidates) item each


def _like(case):
    like = B.SpectrumLikelihood(case.epochs, z=case.z, cutoff_freq=case.cutoff_freq)
    if hasattr(case, 'itab'):   # the range's boundaries that the family was built around are the engine's own
        assert np.array_equal(like.itab_tmin, case.itab[1])
    return like


def _compare(fn, case, label, forms=H.SED_FORMS, precisions=('f64', 'f64-tables')):
    """``fn(candidates, sigma_type, precision, compressed)`` against the reference for every form, precision and both
    kinds of band table.  Prints and returns the worst error; asserts every candidate's own tolerance."""
    worst = 0.
    for form in forms:
        tol, d_cold = H.sed_tolerances(case, form)
        for precision in precisions:
            for compressed in (True, False):
                got = fn(case.candidates(form), form or 'relative', precision, compressed)
                err, ratio = H.sed_worst(got, case, form)
                print(f'{label} [{form}, {precision}, compressed={compressed}]: worst error {err:.2e} against '
                      f'{AGAINST}; tolerance {tol.min():.1e} (cold candidates: {tol.max():.1e}, d_cold = {d_cold:.1e})')
                assert ratio < 1., (label, form, precision, compressed, err)
                worst = max(worst, err)
    return worst


def _epoch_tmin(case, tmin):
    """(n_epochs, 1): the largest ``t_min`` of the epoch's filters -- what the fast kernel compares with."""
    uniq = case.unique
    return np.array([[max([tmin[uniq.index(n)] for n in ep], default=0.)] for ep in case.names])


def test_listed_candidates_cold_and_hot():
    """Candidates below and above the interpolants' range in every wave, one epoch all cold, one with one cold lane,
    the range's edges and their neighbours.
    MI355X: worst error 2.9e-12, in the cold candidates without sigma (their tolerance: 2.2e-11 = 10 d_cold, d_cold =
    2.2e-12); 'relative' 6.2e-13 (d_cold 9.8e-13, tolerance 1e-11), 'absolute' 8.9e-13 (d_cold 1.5e-12, 1.5e-11)."""
    case = H.sed_case('listed')
    like = _like(case)
    T = case.cand[..., 0]
    t_lo, t_hi = H.sed_range(case.itab)
    assert np.all(np.abs(like.itab_tmin / t_lo - 1.) < 1e-15)         # (all seven are proved from the table's start)
    listed = H.sed_listed(T, _epoch_tmin(case, like.itab_tmin), case.itab)
    clear = (np.abs(T / t_lo - 1.) > 1e-12) & (np.abs(T / t_hi - 1.) > 1e-12)     # (not the edges' neighbours)
    assert np.array_equal(listed[clear], ((T < t_lo) | (T >= t_hi))[clear])
    print(f'listed: {listed.sum()} of {listed.size} candidates, per epoch {listed.sum(axis=1)}')
    assert listed[2].all() and listed[6].sum() == 1
    for e in set(range(len(T))) - {2, 6}:      # listed and unlisted lanes in both waves
        for wave in (slice(0, 64), slice(64, None)):
            assert listed[e, wave].any() and not listed[e, wave].all()
    assert (listed & (T < t_lo)).sum() > 100 and (listed & (T >= t_hi)).sum() > 100
    # the full-table branch of compressed=True: candidates below a filter's compressed table's range, and above it
    ctmin = case.tabs.ctmin
    fin = np.isfinite(ctmin)
    assert fin.sum() >= 4 and np.all((ctmin[fin] >= 0.2) & (ctmin[fin] <= 1.0))
    cold = T[listed & (T < t_lo)]
    for t in ctmin[fin]:
        assert (cold < t).sum() >= 10 and (cold >= t).sum() >= 10
    # edges: both neighbours of t_lo and t_hi are there
    for t in (t_lo, t_hi):
        assert {np.nextafter(t, 0.), t, np.nextafter(t, 1e9)} <= set(T[0])
    _compare(like, case, 'listed')


def test_list_state_across_calls_on_one_engine():
    """half listed -> none listed -> all listed with more candidates (the list and the results are reallocated) ->
    the first again, on one engine: every result is right, the first and the fourth are the same bits.
    MI355X: worst error of the four calls 1.5e-13 against 1e-11 (d_cold at the most 7.1e-14)."""
    half, none, every = H.sed_case('state')
    like = _like(half)
    tmin = _epoch_tmin(half, like.itab_tmin)
    share = [float(H.sed_listed(c.cand[..., 0], tmin, c.itab).mean()) for c in (half, none, every)]
    assert 0.3 < share[0] < 0.7 and share[1] == 0. and share[2] == 1.
    assert every.cand.shape[1] > half.cand.shape[1]
    for compressed in (True, False):
        for form in H.SED_FORMS:
            got = [like(c.candidates(form), form or 'relative', 'f64', compressed) for c in (half, none, every, half)]
            for k, (g, c) in enumerate(zip(got, (half, none, every, half))):
                err, ratio = H.sed_worst(g, c, form)
                print(f'state, call {k + 1} [{form}, compressed={compressed}]: worst error {err:.2e} against {AGAINST}')
                assert ratio < 1., (k, form, compressed, err)
            assert np.array_equal(got[0], got[3])
    _compare(like, every, 'state (all listed)')


def _engine(case, tmin):
    """A SedEngine made directly from the case's PackedTables, its interpolants' ``t_min`` replaced by ``tmin``."""
    tabs, (coef, _, u0, h) = case.tabs, case.itab
    assert [f.name for f in tabs.filters] == [B.as_filter(n).name for n in case.unique]
    eng = E.SedEngine(tabs.off, tabs.a, tabs.w, ctab=(tabs.coff, tabs.ca, tabs.cw, tabs.ctmin), itab=(coef, tmin, u0, h))
    eng.set_observations(np.concatenate([[0], np.cumsum([len(n) for n in case.names])]),
                         np.array([case.unique.index(n) for ep in case.names for n in ep], dtype=np.int32),
                         np.concatenate(case.y), np.concatenate(case.dy))
    return eng


def test_per_filter_validity():
    """Interpolants that hold from 3 kK (U), from 10 kK (g) and not at all (i): a listed candidate takes, filter by
    filter, the interpolant where it holds and the sample table where it does not.  Every route is exact.
    MI355X: worst error 1.3e-13 against 1e-11 (d_cold 6.3e-14)."""
    case = H.sed_case('validity')
    tmin = np.array(case.itab[1])
    for name, t in H.SED_ALTERED.items():
        tmin[case.unique.index(name)] = t
    assert (tmin == case.itab[1]).sum() == len(tmin) - 3
    plain, altered = _engine(case, case.itab[1]), _engine(case, tmin)
    T = case.cand[..., 0]
    has = {n: np.array([[n in ep] for ep in case.names]) for n in H.SED_ALTERED}
    assert (~has['i']).sum() >= 1
    for n in ('U', 'g'):     # candidates on both sides of the threshold, in epochs that do and do not have the filter i
        for with_i in (has['i'], ~has['i']):
            sel = has[n] & with_i
            assert (T[sel[:, 0]] < H.SED_ALTERED[n]).sum() >= 20 and (T[sel[:, 0]] > H.SED_ALTERED[n]).sum() >= 20
    listed = H.sed_listed(T, _epoch_tmin(case, tmin), case.itab)
    was = H.sed_listed(T, _epoch_tmin(case, case.itab[1]), case.itab)
    assert listed[has['i'][:, 0]].all() and (~listed).sum() >= 50 and (listed & ~was).sum() > (listed & was).sum() > 0
    prec = {'f64': 2, 'f64-tables': 0}

    def call(eng):
        return lambda c, st, p, comp: eng.log_likelihood(c, E.SIGMA_RELATIVE if st == 'relative' else E.SIGMA_ABSOLUTE,
                                                         prec[p], comp)
    _compare(call(altered), case, 'validity', precisions=('f64',))
    _compare(call(plain), case, 'validity (thresholds as shipped)', precisions=('f64',))
    for form in H.SED_FORMS:     # above every threshold nothing has changed: the same bits
        a, b = (call(e)(case.candidates(form), form or 'relative', 'f64', True) for e in (altered, plain))
        assert np.array_equal(a[~listed], b[~listed])
        assert not np.array_equal(a[listed & ~was], b[listed & ~was])     # (and below one, another route was taken)


def test_grid_stride_and_prefetch():
    """More (epoch, 64 candidates) items than the largest launch has waves: some waves walk two items, the second
    one's candidate requested while the first is computed.
    MI355X: worst error 5.1e-13 ('f64'), 6.1e-13 ('f64-tables') against 1e-11 (d_cold 6.5e-15)."""
    case = H.sed_case('stride')
    n_ep, n_c = case.cand.shape[:2]
    items = n_ep * ((n_c + 63) // 64)
    assert ITEMS_OF_LARGEST_LAUNCH < items < 2 * ITEMS_OF_LARGEST_LAUNCH     # waves with two items AND with one
    assert {len(n) for n in case.names} == {1, 2, 3}
    like = _like(case)
    listed = H.sed_listed(case.cand[..., 0], _epoch_tmin(case, like.itab_tmin), case.itab)
    where = np.nonzero(listed.any(axis=1))[0]
    assert 24 <= listed.sum() <= 60 and where[0] == 0 and where[-1] == n_ep - 1
    # (listed candidates among each wave's first items and among the second ones)
    first = where * ((n_c + 63) // 64) < ITEMS_OF_LARGEST_LAUNCH
    assert first.sum() >= 5 and (~first).sum() >= 1
    _compare(like, case, 'stride')


@pytest.mark.parametrize('n_cand', [1, 63, 64, 65, 129])
def test_shapes(n_cand):
    """Epochs with 0, 1, 2 (the same filter twice) and 7 observations, candidate counts around the wave's width.
    MI355X: worst error 6.4e-13 against 1e-11 (d_cold 5.8e-13)."""
    case = H.sed_case('shapes', n_cand)
    assert {len(n) for n in case.names} == {0, 1, 2, 7} and ['g', 'g'] in case.names
    like = _like(case)
    _compare(like, case, f'shapes, n_cand = {n_cand}')
    for form in H.SED_FORMS:
        for precision in like.PRECISIONS:
            got = like(case.candidates(form), form or 'relative', precision)
            for e in np.nonzero(case.empty()[:, 0])[0]:      # an empty epoch: exactly -0.0
                assert np.all(got[e] == 0.) and np.all(np.signbit(got[e]))


def test_zero_model():
    """T in {0, -1, +inf, NaN} and R in {0, -2} among ordinary candidates, in all three precisions: such a T (and R = 0)
    gives -1/2 sum [ln(2 pi sigma^2) + (y / sigma)^2]; R < 0 gives what |R| gives.
    MI355X: the zero model is within 2.5e-16 of the closed form in the float64 precisions (bound 1e-14) and 2.3e-7 in
    float32 (bound 3e-5); ordinary candidates 1.1e-13 against 1e-11 (d_cold 5.7e-14)."""
    case = H.sed_case('zero')
    like = _like(case)
    zero = case.zero_model()
    T = case.cand[..., 0]
    for v in (0., -1., np.inf):
        assert np.all((T == v).sum(axis=1) == 4)
    assert np.all(np.isnan(T).sum(axis=1) == 4)
    for wave in (slice(0, 64), slice(64, 128)):      # mixed into waves of ordinary candidates
        assert np.all(zero[:, wave].any(axis=1) & ~zero[:, wave].all(axis=1))
    _compare(like, case, 'zero model')
    for form in H.SED_FORMS:
        want = np.empty(zero.shape)
        for e, (_, y, dy) in enumerate(case.epochs):
            s = case.cand[e, :, 2] if form else np.zeros(zero.shape[1])
            var = dy[:, None] ** 2 + ((dy[:, None] if form != 'absolute' else np.median(dy)) * s[None, :]) ** 2
            want[e] = -0.5 * np.sum(np.log(2 * np.pi * var) + y[:, None] ** 2 / var, axis=0)
        for precision in like.PRECISIONS:
            for compressed in (True, False):
                got = like(case.candidates(form), form or 'relative', precision, compressed)
                assert not np.isnan(got).any()
                err = float(np.max(np.abs(got[zero] - want[zero]) / np.abs(want[zero])))
                print(f'zero model [{form}, {precision}, compressed={compressed}]: {err:.2e} from the closed form')
                # float32: the bound test_sed_float32_mode_error_is_bounded holds that mode to
                assert err < (3e-5 if precision == 'f32' else 1e-14)
                for e, (neg, pos) in enumerate(case.mirror):
                    assert np.all(case.cand[e, neg, 1] < 0) and np.array_equal(got[e, neg], got[e, pos])


def test_more_filters_than_fit_and_tables_outside_lds():
    """14 filters: their sample tables exceed what k_sed stages in LDS (it reads them from memory), and their
    interpolants exceed what k_sed_interp stages (precision 'f64' falls back to the sample tables, and says so).
    MI355X: 14 filters 1.3e-13, 13 filters 5.5e-13 against 1e-11 (d_cold 6.5e-14); float32 against float64 1.0e-5
    (bound 3e-5)."""
    case = H.sed_case('many')
    tabs = case.tabs
    assert len(case.unique) == 14
    padded = sum(int(n + 3) // 4 * 4 for off in (tabs.off, tabs.coff) for n in np.diff(off))
    assert padded > 3500                                   # kSedLdsMax: the tables stay in global memory
    m = case.itab[0].shape[1]
    assert E.SedEngine.interpolants_fit(13, m) and not E.SedEngine.interpolants_fit(14, m)
    like = _like(case)
    assert not like.engine.has_interpolants
    _compare(like, case, '14 filters')
    # the fall-back runs the sample-table kernel: the same bits as 'f64-tables'.  With 13 filters it does not.
    few = H.SedCase([[n for n in ep if n != 'y'] for ep in case.names],
                    [np.asarray(y)[np.array(ep) != 'y'] for ep, y in zip(case.names, case.y)],
                    [np.asarray(dy)[np.array(ep) != 'y'] for ep, dy in zip(case.names, case.dy)], case.cand, case.z)
    like13 = _like(few)
    assert len(few.unique) == 13 and like13.engine.has_interpolants
    for form in H.SED_FORMS:
        c = case.candidates(form)
        assert np.array_equal(like(c, form or 'relative', 'f64'), like(c, form or 'relative', 'f64-tables'))
        assert not np.array_equal(like13(c, form or 'relative', 'f64'), like13(c, form or 'relative', 'f64-tables'))
    _compare(like13, few, '13 filters')
    # float32 is specified for the priors of configs[3], 1-100 kK: the epochs whose truth lies there
    sel = (case.truth_T >= 1.) & (case.truth_T <= 100.)
    assert sel.sum() == 4
    for form in H.SED_FORMS:
        c = case.candidates(form)
        f64, f32 = like(c, form or 'relative', 'f64'), like(c, form or 'relative', 'f32')
        err = float(np.max(np.abs(f32[sel] - f64[sel]) / np.abs(f64[sel])))
        print(f'14 filters [{form}]: float32 against float64 {err:.2e}')
        assert err < 3e-5


@pytest.mark.parametrize('seed', range(8))
def test_sed_fuzz(seed):
    """Random redshift, cut-off frequency, filters, epochs, candidate count and sigma form; truths log-uniform over
    0.3-2000 kK, candidates scattered about them.
    MI355X: seed 0 (z = 0.3, 'absolute') 7.0e-12 in its cold candidates (tolerance 2.3e-11 = 10 d_cold, d_cold =
    2.3e-12); the other seeds 3.0e-13 at the most against 1e-11."""
    case = H.sed_case('fuzz', seed)
    like = _like(case)
    print(f'fuzz {seed}: z = {case.z}, cut-off {case.cutoff_freq}, {len(case.unique)} filters {case.unique}, '
          f'{case.cand.shape[0]} epochs x {case.cand.shape[1]} candidates, form {case.form}, interpolants from '
          f'{like.itab_tmin} kK')
    _compare(like, case, f'fuzz {seed}', forms=(case.form,))
