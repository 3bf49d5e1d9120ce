"""color_predictive on the device against the CPU oracle + the NumPy definition of tests/color_reference.py: ``want`` is
color_bands / peaks of Y[f, t, s], the oracle's evaluation of the very samples the call used.

Tolerance of a colour, absolute: every model value is within a relative 1e-11 of the oracle's (tests/test_gpu_parity.py),
so the ratio of two is within 2e-11 and -2.5 log10 of it within (2.5 / ln 10) * 2e-11 = 2.2e-11 mag; so is every order
statistic and every convex combination of two.  Held to 2.5e-11.  n_valid must be equal exactly.  (Measured maxima are
printed and recorded in DESIGN.md, "Colour bands and peaks".)"""
import numpy as np
import pytest

import color_reference as R
from conftest import relerr
from helpers import config2_case
from lightcurve_fitting_amd import engine as E
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.filters import filtdict
from lightcurve_fitting_amd.fitting import color_predictive, posterior_predictive
from oracle import lcf_oracle as O
from test_gpu_predictive import SEVEN, UFILTS, _companion_rows, _fit, _lc, _one_sample_cases, _oracle_grid, _rows

pytestmark = pytest.mark.gpu

TOL_MAG = 2.5e-11
TOL = 1e-11
FOUR = ('U-B', 'B-V', 'g-r', 'r-i')
SORTED = [f.name for f in sorted(filtdict[c] for c in UFILTS)]     # the grid's filters: the registry's order
_cache = {}


def _shared(key):
    """The rows and the oracle's Y[f, t, s] of the two 4096-row cases, computed once and left unchanged."""
    if key not in _cache:
        P = _rows(4096)
        if key == 'peaks':          # eight rows explode after the grid's last time; the grid ends inside the red peaks
            P[::512, 4] = 12.5
            times = np.linspace(0.3, 6., 50)
        else:
            times = np.linspace(0.3, 12., 50)
        Y = _oracle_grid(('ShockCooling', O.ShockCoolingOracle(0.01)), times, SORTED, P)
        for a in (P, times, Y):
            a.setflags(write=False)
        _cache[key] = (P, times, Y)
    return _cache[key]


def _index(res):
    where = {f: i for i, f in enumerate(res.filters)}
    return [(where[a], where[b]) for a, b in res.colors]


def _check(res, Y, tol=TOL_MAG, what=''):
    pairs = _index(res)
    dzp = [a.m0 - b.m0 for a, b in res.colors]
    want, n_valid = R.color_bands(Y, pairs, dzp, res.percentiles)
    assert res.color.shape == want.shape and np.array_equal(np.isnan(res.color), np.isnan(want)), 'NaN pattern differs'
    err = float(np.nanmax(np.abs(res.color - want))) if np.any(~np.isnan(want)) else 0.
    print(f'color_predictive vs oracle + nanpercentile {what}: max abs err {err:.3e} mag over {res.color.shape}')
    assert err <= tol
    assert np.array_equal(res.n_valid, n_valid)
    return want


def _same(a, b):
    assert np.array_equal(a.color, b.color, equal_nan=True) and np.array_equal(a.n_valid, b.n_valid)
    if a.peak_index is not None:
        assert np.array_equal(a.y_peak, b.y_peak, equal_nan=True) and np.array_equal(a.peak_index, b.peak_index)
        assert np.array_equal(a.M_peak, b.M_peak, equal_nan=True) and np.array_equal(a.t_peak, b.t_peak, equal_nan=True)


def test_shockcooling_4096_rows_seven_percentiles():
    P, times, Y = _shared('bands')
    res = color_predictive(_lc(), M.ShockCooling(redshift=0.01), P, colors=FOUR, percentiles=SEVEN, num=50)
    assert res.color.shape == (7, 4, 50) and res.n_valid.shape == (4, 50) and res.n_samples == 4096
    assert res.y_peak.shape == res.peak_index.shape == res.t_peak.shape == res.M_peak.shape == (4096, 6)
    assert np.array_equal(res.t, times) and [f.name for f in res.filters] == SORTED and res.color_names == list(FOUR)
    _check(res, Y, what='(4096 rows)')
    assert np.all(np.diff(res.color, axis=0) >= 0.)
    assert np.all(res.n_valid == 4096)


def test_dark_samples_and_empty_points():
    """The recipe of test_ties_at_exact_zero: at 0.05 d no sample has exploded, at 0.1 d k of them have not."""
    S = 4096
    rng = np.random.default_rng(7)
    P = _rows(S, seed=8)
    second = np.arange(S) >= int(0.6 * S)
    P[:, 4] = np.where(second, rng.uniform(0.12, 0.14, S), rng.uniform(0.07, 0.09, S))
    P = P[rng.permutation(S)]
    k = int(np.sum(P[:, 4] > 0.1))
    times = np.array([0.05, 0.1, 0.2])
    Y = _oracle_grid(('ShockCooling', O.ShockCoolingOracle(0.01)), times, SORTED, P)
    assert np.all(Y[:, 0] == 0.) and np.all(np.sum(Y[:, 1] == 0., axis=-1) == k) and np.all(Y[:, 2] > 0.)
    res = color_predictive(_lc(), M.ShockCooling(redshift=0.01), P, colors=FOUR, percentiles=(0., 15.87, 50., 100.),
                           t=times)
    assert np.all(np.isnan(res.color[:, :, 0])) and np.all(res.n_valid[:, 0] == 0)
    assert np.all(res.n_valid[:, 1] == S - k) and np.all(res.n_valid[:, 2] == S)
    _check(res, Y, what='(dark samples)')
    want, _ = R.color_bands(Y[:, :, P[:, 4] <= 0.1], _index(res), [a.m0 - b.m0 for a, b in res.colors], res.percentiles)
    assert np.nanmax(np.abs(res.color[:, :, 1] - want[:, :, 1])) <= TOL_MAG      # ... those of the remaining samples
    # no sample is dark on the whole grid, and none peaks before it has exploded
    assert np.all(res.y_peak > 0.) and np.all(res.peak_index >= 1)


def test_one_sample_every_model():
    times = np.linspace(0.3, 12., 23)
    for name, m, orc, p in _one_sample_cases():
        res = color_predictive(_lc(), m, p[None, :], colors=FOUR, percentiles=(0., 15.87, 50., 100.), t=times)
        assert np.array_equal(res.color, np.broadcast_to(res.color[0], res.color.shape), equal_nan=True), name
        assert res.n_samples == 1 and np.all(res.n_valid <= 1)
        if name == 'CompanionShocking':
            Y = np.stack([orc[1].evaluate(times, [O.band(f)] * len(times), *p) for f in SORTED])[:, :, None]
        else:
            Y = np.stack([O.evaluate(orc, times, [O.band(f)] * len(times), p) for f in SORTED])[:, :, None]
        _check(res, Y, what=f'({name}, one sample)')
        y_peak, index = R.peaks(Y)
        assert np.array_equal(res.peak_index, index), name
        err = relerr(res.y_peak, y_peak)
        print(f'{name}: y_peak vs oracle {err:.3e}')
        assert err <= TOL, name
        zero = np.array([f.m0 if name == 'ShockCooling3' else f.M0 for f in res.filters])
        assert m.output_quantity == ('flux' if name == 'ShockCooling3' else 'lum')
        assert np.allclose(res.M_peak, zero - 2.5 * np.log10(y_peak), rtol=0., atol=TOL_MAG)
        assert np.array_equal(res.t_peak, times[index])


@pytest.mark.parametrize('variant', [1, 2])
def test_companion_models(variant):
    g, lc = config2_case()
    cls = {1: M.CompanionShocking, 2: M.CompanionShocking2}[variant]
    m = cls(lc, redshift=0.003)
    orc = O.CompanionShockingOracle([O.band(n) for n in lc['filter']], lc['lum'], z=0.003, variant=variant)
    P = _companion_rows(512, variant)
    res = color_predictive(lc, m, P, colors=FOUR, num=40)
    assert [f.name for f in res.filters] == SORTED and len(res.t) == 40
    Y = np.stack([np.stack([orc.evaluate(res.t, [O.band(f)] * 40, *p) for p in P], axis=-1) for f in SORTED])
    _check(res, Y, what=f'(companion variant {variant})')
    y_peak, _ = R.peaks(Y)
    assert relerr(res.y_peak, y_peak) <= TOL


def test_peaks():
    P, times, Y = _shared('peaks')
    nt = len(times)
    res = color_predictive(_lc(), M.ShockCooling(redshift=0.01), P, colors=FOUR, tmin=0.3, tmax=6., num=50)
    assert np.array_equal(res.t, times)
    y_peak, index = R.peaks(Y)
    err = relerr(res.y_peak, y_peak)
    print(f'y_peak vs the oracle\'s nanmax: max rel err {err:.3e} over {y_peak.shape}')
    assert err <= TOL
    top2 = np.sort(Y, axis=1)[:, -2:, :]                                  # (no NaN in this case)
    clear = ((top2[:, 1] - top2[:, 0]) > 1e-9 * np.abs(top2[:, 1])).T     # (s, f)
    print(f'peak_index compared for {clear.mean():.4%} of the (sample, filter) pairs')
    assert np.mean(~clear) <= 0.01
    assert np.array_equal(res.peak_index[clear], index[clear])
    dark = P[:, 4] > times[-1]
    assert dark.sum() == 8 and np.all(res.y_peak[dark] == 0.) and np.all(res.peak_index[dark] == 0)
    assert np.array_equal(res.n_peak_first, np.sum(res.peak_index == 0, axis=0))
    assert np.array_equal(res.n_peak_last, np.sum(res.peak_index == nt - 1, axis=0))
    assert np.all(res.n_peak_first == 8)
    inside = np.sum((res.peak_index > 0) & (res.peak_index < nt - 1), axis=0)
    u, i = SORTED.index('U'), SORTED.index('i')
    assert inside[u] > 4000 and res.n_peak_last[u] == 0                   # the blue peaks lie inside the grid ...
    assert res.n_peak_last[i] > 1000 and inside[i] > 1000                 # ... many of the red ones on its edge
    assert np.array_equal(res.t_peak, times[res.peak_index])
    s = res.peak_summary()
    assert s['M_peak'].shape == (3, 6) and np.all(np.diff(s['M_peak'], axis=0) >= 0.)
    # the colours of the same call: the dark rows have none
    _check(res, Y, what='(peaks case)')
    assert np.all(res.n_valid == 4088)


def test_peaks_equal_the_device_own_maxima_bit_for_bit():
    """max over samples of y_peak[:, f] and max over times of the 100th percentile of posterior_predictive are maxima
    of the same pq_point values."""
    P, times, _ = _shared('peaks')
    m = M.ShockCooling(redshift=0.01)
    res = color_predictive(_lc(), m, P, colors=FOUR, tmin=0.3, tmax=6., num=50, percentiles=(50.,))
    top = posterior_predictive(_lc(), m, P, percentiles=(100.,), tmin=0.3, tmax=6., num=50, filters_to_model=res.filters)
    assert top.filters == res.filters
    for f in range(6):
        assert np.max(res.y_peak[:, f]) == np.max(top.quantiles[0, f])


@pytest.mark.parametrize('use_sigma', [False, True])
def test_sampler_in_place_equals_the_array_form(use_sigma):
    lc, m, s = _fit(64, 40, use_sigma)
    assert len(s._chain_host) == 0 and s._chain_on_device == 40           # read where it lies
    a = color_predictive(lc, m, s, colors=FOUR, discard=7, thin=3, num=30, use_sigma=use_sigma)
    assert len(s._chain_host) == 0 and s._chain_on_device == 40           # ... and it still lies there
    flat = s.get_chain(discard=7, thin=3, flat=True)
    assert a.n_samples == len(flat) == 11 * 64 and a.y_peak.shape == (11 * 64, 6)
    b = color_predictive(lc, m, flat, colors=FOUR, num=30, use_sigma=use_sigma)
    _same(a, b)
    Y = _oracle_grid(('ShockCooling', O.ShockCoolingOracle(0.)), a.t, SORTED, flat[:, :5])
    _check(a, Y, what='(sampler in place)')
    assert relerr(a.y_peak, R.peaks(Y)[0]) <= TOL
    with pytest.raises(ValueError, match='columns'):
        color_predictive(lc, m, s, use_sigma=not use_sigma)


def test_tiling_and_determinism():
    P, times, Y = _shared('bands')
    m = M.ShockCooling(redshift=0.01)
    colors = FOUR + ('B-V',)                                               # a colour given twice
    # five colours x seven percentiles keep 35 * 2048 keys of 8 bytes per time: 4 MiB hold at most six of the 50 times
    small = 4 << 20
    n_tiles = -(-50 // ((small - E.color_workspace(4096, 50, 5, 7, tile=0)) //
                        (E.color_workspace(4096, 50, 5, 7, tile=1) - E.color_workspace(4096, 50, 5, 7, tile=0))))
    assert n_tiles >= 3
    tiled = color_predictive(_lc(), m, P, colors=colors, percentiles=SEVEN, num=50, workspace_bytes=small)
    one = color_predictive(_lc(), m, P, colors=colors, percentiles=SEVEN, num=50)
    two = color_predictive(_lc(), m, P, colors=colors, percentiles=SEVEN, num=50)
    _same(one, two)
    _same(one, tiled)
    assert np.array_equal(one.color[:, 1], one.color[:, 4]) and np.array_equal(one.n_valid[1], one.n_valid[4])
    _check(tiled, Y, what='(tiled)')
    with pytest.raises(Exception, match='workspace_bytes too small'):
        color_predictive(_lc(), m, P, colors=colors, percentiles=SEVEN, num=50, workspace_bytes=1 << 16)
    # without the peaks the bands are the same bits
    bare = color_predictive(_lc(), m, P, colors=colors, percentiles=SEVEN, num=50, peak=False)
    assert bare.y_peak is None and np.array_equal(bare.color, one.color)


def test_every_pass_loops_and_refines_more_than_once():
    """The recipe of the light-curve form's test of that name: 1024 x 100 rows of a fit, whose colours crowd into a few
    bins of the first histogram.  Against the project's own model(...) in slices + the NumPy definition (the oracle is
    too slow here), held to the tolerance of a colour against the oracle itself."""
    lc, m, s = _fit(1024, 100)
    res = color_predictive(lc, m, s, colors=FOUR, num=100)
    flat = s.get_chain(flat=True)
    assert res.n_samples == len(flat) == 102400
    Y = np.empty((6, 100, len(flat)))
    for k in range(0, len(flat), 8192):
        Y[:, :, k:k + 8192] = m(res.t, res.filters, *flat[k:k + 8192].T)
    _check(res, Y, what='(102400 samples, vs model(...))')
    err = relerr(res.y_peak, R.peaks(Y)[0])
    print(f'y_peak vs model(...): max rel err {err:.3e}')
    assert err <= 2 * TOL                                       # (both sides within 1e-11 of the oracle)


def test_refusals_through_the_c_abi():
    lib = E.load_library()
    m = M.ShockCooling(redshift=0.01)
    times = np.linspace(0.3, 12., 5)
    grid, _ = M.Model._eval_engine(m, times, [filtdict[c] for c in SORTED], False)
    P = _rows(8)
    out, nv = np.full((600, 5), -7.), np.full((600, 5), -7, dtype=np.int64)
    q = np.linspace(0., 100., 300)

    def call(engine, pairs, n_q):
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        dzp = np.zeros(len(pairs))
        st = lib.lcf_predict_colors(engine.handle, E._ptr(P), 8, 5, len(pairs), E._ptr(pairs, E._ip), E._ptr(dzp), E._ptr(q),
                                    n_q, 1 << 30, E._ptr(out), E._i64p(nv), None, None)
        return st, lib.lcf_last_error().decode()

    for bad in ([[0, 6]], [[-1, 2]], [[0, 1], [2, 3], [6, 0]]):
        st, msg = call(grid, bad, 3)
        assert st == 1 and 'not a filter of the grid engine' in msg
    st, msg = call(grid, [[0, 1], [1, 2]], 257)
    assert st == 5 and 'must not exceed 512' in msg
    st, msg = call(grid, [[0, 1], [1, 2]], 0)
    assert st == 1
    # y_peak without peak_index
    pairs, dzp, y = np.array([[0, 1]], dtype=np.int32), np.zeros(1), np.empty((6, 8))
    assert lib.lcf_predict_colors(grid.handle, E._ptr(P), 8, 5, 1, E._ptr(pairs, E._ip), E._ptr(dzp), E._ptr(q), 1, 1 << 30,
                                  E._ptr(out), E._i64p(nv), E._ptr(y), None) == 1
    assert 'together' in lib.lcf_last_error().decode()
    central = M.Arnett()._grid_engine(times)
    st, msg = call(central, [[0, 1]], 3)
    assert st == 5 and 'lcf_predict_colors' in msg and 'compiled per photometric model' in msg and 'lcf_tempered' in msg
    assert np.all(out == -7.) and np.all(nv == -7)                          # nothing was launched or written
    # ... and the same call goes through once its arguments are right
    st, msg = call(grid, [[0, 1], [1, 2]], 256)
    assert st == 0 and np.all(nv[:2] == 8)
