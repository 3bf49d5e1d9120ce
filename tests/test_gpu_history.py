"""chain_history on the device against NumPy on the same array.  Nothing here has a tolerance: the order statistics
must EQUAL np.sort's picks, the percentiles np.nanpercentile (the device selects, the interpolation is NumPy's own
arithmetic), the moves the comparison of chain.view(np.int64) rows, and the raster np.histogram per step-bin slab."""
import warnings

import numpy as np
import pytest

from lightcurve_fitting_amd import engine as E, models as M
from lightcurve_fitting_amd.engine import LcfError
from lightcurve_fitting_amd.fitting import HISTORY_PERCENTILES, chain_history, lightcurve_mcmc, quantile_ranks
from lightcurve_fitting_amd.sampler import EnsembleSampler, PopulationSampler
from helpers import lc_dict, small_problem
from test_gpu_corner import _posterior_like
from test_gpu_population_mixed import P1, _transient
from test_gpu_predictive import TRUTH, _fit

pytestmark = pytest.mark.gpu

Q5 = np.array(HISTORY_PERCENTILES)


def _chain(n_t, n_w, n_dim, seed):
    """A chain (n_t, n_w, n_dim) with columns of very different scale, one near 58000, and its log-probabilities."""
    x = _posterior_like(n_t * n_w, n_dim, seed).reshape(n_t, n_w, n_dim)
    lp = -0.5 * np.random.default_rng(seed + 1).chisquare(n_dim, (n_t, n_w))
    return x, lp


def _numpy_moves(x, steps):
    bits = np.ascontiguousarray(x).view(np.int64)
    return np.array([-1 if t == 0 else np.any(bits[t] != bits[t - 1], axis=1).sum() for t in steps])


def _numpy_bands(x, lp, q, steps):
    """(percentiles[nq, n_keep, n_dim + 1], n_valid) of the kept steps, the log-probability as the last column (NaN
    without one)."""
    lp = np.full(x.shape[:2], np.nan) if lp is None else lp
    cols = np.concatenate([x, lp[:, :, None]], axis=2)[steps]
    with np.errstate(invalid='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return np.nanpercentile(cols, q, axis=1), (~np.isnan(cols)).sum(axis=1), cols


def _numpy_raster(x, steps, step_edges, edges):
    kept = x[steps]
    with np.errstate(invalid='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return np.array([[np.histogram(kept[a:b, :, d].ravel(), bins=edges[d])[0]
                          for a, b in zip(step_edges[:-1], step_edges[1:])] for d in range(x.shape[2])])


def _check_native_picks(x, lp, q, discard=0, thin=1):
    """engine.chain_history: the two order statistics are np.sort's picks at the ranks of quantile_ranks."""
    steps = np.arange(discard, len(x), thin)
    stat_lo, stat_hi, n_valid, n_moved = E.chain_history(x, q, log_prob=lp, discard=discard, thin=thin)
    _, nv, cols = _numpy_bands(x, lp, q, steps)
    assert stat_lo.shape == stat_hi.shape == (len(q), len(steps), x.shape[2] + 1)
    assert np.array_equal(n_valid, nv) and n_valid.dtype == np.int64
    srt = np.sort(cols, axis=1)                                            # NaNs last
    lo, hi, _ = quantile_ranks(np.maximum(nv, 1)[None], np.asarray(q, dtype=float)[:, None, None])
    for k in range(len(steps)):
        for c in range(cols.shape[2]):
            want_lo, want_hi = srt[k, lo[:, k, c], c], srt[k, hi[:, k, c], c]
            if nv[k, c] == 0:
                want_lo = want_hi = np.full(len(q), np.nan)
            assert np.array_equal(stat_lo[:, k, c], want_lo, equal_nan=True), (k, c)
            assert np.array_equal(stat_hi[:, k, c], want_hi, equal_nan=True), (k, c)
    assert np.array_equal(n_moved, _numpy_moves(x, steps))
    return stat_lo, stat_hi, n_valid, n_moved


def _check(res, x, lp, q=Q5, discard=0, thin=1, default_range=True):
    """Every field of a ChainHistory against NumPy on the whole chain x (n_t, n_w, n_dim) and lp (n_t, n_w) or None."""
    n_t, n_w, n_dim = x.shape
    steps = np.arange(discard, n_t, thin)
    n_keep = len(steps)
    assert np.array_equal(res.steps, steps) and np.array_equal(res.percentiles, q) and res.n_walkers == n_w
    want, nv, _ = _numpy_bands(x, lp, q, steps)
    assert res.quantiles.shape == (len(q), n_keep, n_dim) and res.log_prob_quantiles.shape == (len(q), n_keep)
    assert np.array_equal(res.quantiles, want[:, :, :n_dim], equal_nan=True)
    assert np.array_equal(res.log_prob_quantiles, want[:, :, n_dim], equal_nan=True)
    assert np.array_equal(res.n_valid, nv)
    moved = _numpy_moves(x, steps)
    assert np.array_equal(res.n_moved, moved) and res.n_moved.dtype == np.int64
    assert np.array_equal(res.frac_moved, np.where(moved < 0, np.nan, moved / n_w), equal_nan=True)
    t_bins, v_bins = res.counts.shape[1:]
    assert res.counts.shape == (n_dim, t_bins, v_bins) and res.counts.dtype == np.int64
    k = np.arange(n_keep)
    assert np.array_equal(np.searchsorted(res.step_edges, k, 'right') - 1, (k * t_bins) // n_keep)
    if default_range:
        kept = x[steps].reshape(-1, n_dim)
        lo, hi = np.nanmin(kept, axis=0), np.nanmax(kept, axis=0)
        same = lo == hi
        assert np.array_equal(res.range, np.stack([np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)], axis=1))
    for d in range(n_dim):
        assert np.array_equal(res.edges[d], np.linspace(res.range[d, 0], res.range[d, 1], v_bins + 1))   # bitwise
    assert np.array_equal(res.counts, _numpy_raster(x, steps, res.step_edges, res.edges))
    return want


@pytest.mark.parametrize('with_lp', [False, True])
@pytest.mark.parametrize('n_w', [1, 2, 63, 64, 65, 1000, 1025])
def test_sizes_that_break_the_sort_and_the_ballots(n_w, with_lp):
    """One walker (nothing to sort), a wave less one, a wave, a wave and one, 1000 (24 keys of padding) and 1025 (1023
    of them, two sweeps of the workgroup); one step (no predecessor at all), two and five."""
    for n_t in (1, 2, 5):
        x, lp = _chain(n_t, n_w, 5, seed=10 * n_w + n_t)
        lp = lp if with_lp else None
        x[n_t // 2, ::3] = x[0, ::3] if n_t == 1 else x[n_t // 2 - 1, ::3]   # a third of the walkers stay
        _check_native_picks(x, lp, Q5)
        res = chain_history(None, x, log_prob=lp)
        _check(res, x, lp)
        assert res.counts.shape[1] == n_t and np.all(res.counts.sum(axis=(1, 2)) == n_t * n_w)
        if not with_lp:
            assert np.all(np.isnan(res.log_prob_quantiles)) and np.all(res.n_valid[:, 5] == 0)


def test_largest_and_too_large_ensembles():
    x, lp = _chain(2, 16384, 2, seed=3)                                    # 128 KiB of keys in LDS
    _check_native_picks(x, lp, Q5)
    res = chain_history(None, x, log_prob=lp, v_bins=7)
    _check(res, x, lp)
    big = np.zeros((1, 16385, 1))
    with pytest.raises(LcfError) as err:
        E.chain_history(big, Q5)
    assert err.value.status == 5
    with pytest.raises(LcfError) as err:
        E.chain_raster(big, 1, np.array([[0., 1.]]))
    assert err.value.status == 5
    with pytest.raises(ValueError, match='16384'):
        chain_history(None, big)


@pytest.mark.parametrize('n_dim', [1, 16])
def test_column_and_percentile_limits(n_dim):
    """16 percentiles: 0, 100, a repeated value and one whose rank is an integer (25 % of 321 - 1 = 80)."""
    x, lp = _chain(3, 321, n_dim, seed=20 + n_dim)
    q = np.array([0., 100., 50., 50., 25., 1., 2.5, 15.87, 33.3, 66.6, 84.14, 97.5, 99., 99.9, 0.1, 75.])
    assert len(q) == 16 and (321 - 1) * 0.25 == 80.
    _check_native_picks(x, lp, q)
    res = chain_history(None, x, percentiles=q, log_prob=lp)
    _check(res, x, lp, q)
    assert np.array_equal(res.quantiles[0], x.min(axis=1)) and np.array_equal(res.quantiles[1], x.max(axis=1))
    assert np.array_equal(res.quantiles[2], res.quantiles[3]) and np.array_equal(res.quantiles[4], np.sort(x, axis=1)[:, 80])
    for call in (lambda: E.chain_history(x, np.linspace(0., 100., 17)), lambda: E.chain_history(np.zeros((2, 40, 17)), q),
                 lambda: E.chain_history(x, [])):
        with pytest.raises(LcfError) as err:
            call()
        assert err.value.status == 1


def test_moves():
    n_w = 130
    x, lp = _chain(7, n_w, 4, seed=30)
    stay = np.arange(n_w) % 3 == 0
    x[1, stay] = x[0, stay]                                                # walkers that keep their row
    x[2] = x[1]
    last = np.arange(n_w) % 5 == 1
    x[2, last, 3] += 1.                                                    # rows that change only in the last column
    x[3] = x[2]                                                            # nobody moves
    x[4, 7, 1] = -0.                                                       # (step 4: everybody moves)
    x[5] = x[4]
    x[5, 7, 1] = 0.                                                        # -0.0 -> +0.0: equal as numbers, a move in bits
    x[6] = x[5]
    x[6, 129, 0] = np.nextafter(x[5, 129, 0], np.inf)                      # the last walker, by one bit
    want = [-1, n_w - stay.sum(), last.sum(), 0, n_w, 1, 1]
    res = chain_history(None, x, log_prob=lp)
    assert np.array_equal(res.n_moved, want) and np.array_equal(_numpy_moves(x, np.arange(7)), want)
    assert np.isnan(res.frac_moved[0]) and res.frac_moved[4] == 1. and res.frac_moved[3] == 0.
    _check(res, x, lp)
    for discard in (1, 2, 6):
        part = chain_history(None, x, discard=discard)
        assert np.array_equal(part.n_moved, want[discard:]) and np.all(part.n_moved >= 0)
    # thin = 3: the predecessor is the stored step before, not the kept step before
    thinned = chain_history(None, x, discard=1, thin=3)
    assert np.array_equal(thinned.steps, [1, 4]) and np.array_equal(thinned.n_moved, [want[1], want[4]])
    _check(thinned, x, None, discard=1, thin=3)
    thinned = chain_history(None, x, thin=3)
    assert np.array_equal(thinned.steps, [0, 3, 6]) and np.array_equal(thinned.n_moved, [-1, 0, 1])
    # a NaN keeps its bits: not a move
    y = x.copy()
    y[2:4, 5, 2] = np.nan
    assert np.array_equal(chain_history(None, y, range=[(-1e5, 1e5)] * 4).n_moved[3:4], [0])


def test_ties_nans_and_infinities():
    n_w = 500
    x, lp = _chain(4, n_w, 4, seed=40)
    rng = np.random.default_rng(41)
    x[0, rng.permutation(n_w)[:300], 1] = x[0, 0, 1]                       # 60 % of a step's walkers on one value
    x[1, rng.permutation(n_w)[:123], 2] = np.nan                           # NaNs in some cells
    x[2, :, 0] = np.nan                                                    # an all-NaN cell
    x[3, 1:, 3] = np.nan                                                   # a cell of one value
    lp[1, ::7] = np.nan
    q = np.array([0., 10., 50., 59.9, 60.1, 100.])
    _check_native_picks(x, lp, q)
    outside = lp.copy()
    outside[2, ::2] = -np.inf                                              # walkers outside the prior: values, the lowest
    _check_native_picks(x, outside, q)
    res = chain_history(None, x, percentiles=q, log_prob=lp)
    with np.errstate(invalid='ignore'):
        _check(res, x, lp, q)
    assert res.n_valid[1, 2] == n_w - 123 and res.n_valid[2, 0] == 0 and res.n_valid[3, 3] == 1
    assert np.all(np.isnan(res.quantiles[:, 2, 0])) and np.all(res.quantiles[:, 3, 3] == x[3, 0, 3])
    assert res.n_valid[1, 4] == n_w - len(lp[1, ::7]) and res.n_valid[2, 4] == n_w
    # +-inf and both zeros in one column: the keys order -inf < ... < -0 < +0 < ... < +inf, and the percentiles 0 and
    # 100 are NumPy's minimum and maximum.  (np.nanpercentile itself interpolates inf - inf = NaN next to an infinity,
    # also at 0 and 100: there the order statistics are compared with np.sort's instead.)
    z, _ = _chain(2, 257, 3, seed=42)
    z[:, :, 1] = np.where(rng.random((2, 257)) < 0.5, -1., 1.) * 10. ** rng.uniform(-300., 300., (2, 257))
    z[0, 3, 1], z[0, 4, 1], z[0, 5, 1], z[0, 6, 1] = np.inf, -np.inf, -0., 0.
    z[1, 8, 1], z[1, 9, 1] = -0., 0.
    stat_lo, stat_hi, _, _ = _check_native_picks(z, None, q)
    both = E.chain_history(np.array([0., -0., 1., -1.]).reshape(1, 4, 1), [50.])   # ranks 1 and 2: -0, then +0
    assert both[0][0, 0, 0] == 0. and np.signbit(both[0][0, 0, 0])
    assert both[1][0, 0, 0] == 0. and not np.signbit(both[1][0, 0, 0])
    res = chain_history(None, z, percentiles=q, range=[None, (-1., 1.), None])
    assert np.array_equal(res.quantiles[0, :, 1], z[:, :, 1].min(axis=1)) and res.quantiles[0, 0, 1] == -np.inf
    assert np.array_equal(res.quantiles[-1, :, 1], z[:, :, 1].max(axis=1)) and res.quantiles[-1, 0, 1] == np.inf
    with np.errstate(invalid='ignore'):
        want = np.nanpercentile(z, q, axis=1)
    assert np.array_equal(res.quantiles[:, 1], want[:, 1]) and np.array_equal(res.quantiles[:, :, ::2], want[:, :, ::2])
    assert np.array_equal(res.quantiles[1:-1, 0, 1], want[1:-1, 0, 1], equal_nan=True)   # (interior: as NumPy has them)


def test_raster_step_bins():
    x, lp = _chain(11, 77, 3, seed=50)
    for t_bins in (4, 11, 1):
        res = chain_history(None, x, t_bins=t_bins, v_bins=9)
        _check(res, x, None)
        assert res.counts.shape == (3, t_bins, 9) and np.all(res.counts.sum(axis=(1, 2)) == 11 * 77)
        if t_bins == 4:
            assert np.array_equal(res.step_edges, [0, 3, 6, 9, 11])
            assert np.array_equal(res.counts.sum(axis=2), np.tile([3 * 77, 3 * 77, 3 * 77, 2 * 77], (3, 1)))
        if t_bins == 1:   # the shared bin rule: one step bin is the corner histogram of the same rows on the same edges
            hist1d, _ = E.chain_hist(x.reshape(-1, 3), np.zeros(3), res.edges)
            assert np.array_equal(res.counts[:, 0], hist1d)
    # discard and thin: the step bins are bins of KEPT steps
    res = chain_history(None, x, t_bins=2, v_bins=9, discard=2, thin=4)
    assert np.array_equal(res.steps, [2, 6, 10]) and np.array_equal(res.step_edges, [0, 2, 3])
    _check(res, x, None, discard=2, thin=4)


def test_raster_edge_membership_and_ranges():
    """Values on, just below and just above every edge; NaN and the neighbours outside [lo, hi] are in no bin."""
    e = np.linspace(0., 1., 21)
    col = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                          [1., np.nextafter(1., np.inf), np.nextafter(0., -np.inf), np.nan, np.nan]])
    assert len(col) == 68
    rng = np.random.default_rng(60)
    x = np.stack([col.reshape(4, 17), rng.uniform(0.2, 0.8, (4, 17))], axis=2)
    res = chain_history(None, x, t_bins=1, v_bins=20, range=[(0., 1.), (0., 1.)])
    assert np.array_equal(res.edges[0], e)
    inside = col[(col >= 0.) & (col <= 1.)]
    want = np.bincount(np.minimum(np.searchsorted(e, inside, 'right') - 1, 19), minlength=20)
    assert np.array_equal(res.counts[0, 0], want) and np.all(want[:19] == 3) and want[19] == 5
    assert res.counts[0].sum() == 68 - 6
    _check(res, x, None, default_range=False)
    _check(chain_history(None, x, t_bins=4, v_bins=20, range=[(0., 1.), (0., 1.)]), x, None, default_range=False)
    # a range narrower than the data, on some columns
    y, _ = _chain(9, 130, 4, seed=61)
    flat = y.reshape(-1, 4)
    lo, hi = np.percentile(flat, 20., axis=0), np.percentile(flat, 85., axis=0)
    rng_ = [(lo[0], hi[0]), None, (lo[2], hi[2]), (lo[3], hi[3])]
    res = chain_history(None, y, t_bins=3, range=rng_)
    assert np.array_equal(res.range[1], [flat[:, 1].min(), flat[:, 1].max()]) and np.array_equal(res.range[2], rng_[2])
    _check(res, y, None, default_range=False)
    within = (flat >= res.range[:, 0]) & (flat <= res.range[:, 1])
    assert np.array_equal(res.counts.sum(axis=(1, 2)), within.sum(axis=0)) and not within[:, 0].all()
    for v_bins in (1, 256):
        res = chain_history(None, y, v_bins=v_bins)
        _check(res, y, None)
        assert res.counts.shape == (4, 9, v_bins) and np.all(res.counts.sum(axis=(1, 2)) == 9 * 130)
    for call in (lambda: E.chain_raster(y, 10, res.edges), lambda: E.chain_raster(y, 0, res.edges),
                 lambda: E.chain_raster(y, 3, np.tile(np.linspace(0., 1., 258), (4, 1))),
                 lambda: E.chain_raster(y, 3, res.edges[:, ::-1].copy())):
        with pytest.raises(LcfError) as err:
            call()
        assert err.value.status == 1


FIELDS = ('steps', 'percentiles', 'quantiles', 'log_prob_quantiles', 'n_valid', 'n_moved', 'frac_moved', 'counts',
          'step_edges', 'edges', 'range')


def _same(a, b):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    assert a.names == b.names and a.labels == b.labels and a.n_walkers == b.n_walkers


def test_chain_in_place():
    lc, m, fitted = _fit(64, 40)
    x0 = fitted.get_chain()[-1]
    # seed 3, picked once: no accepted proposal of this run reproduces its walker's bits, so that the moves counted in
    # the chain are the sampler's own accept counters
    s = EnsembleSampler(64, 5, fitted.engine, seed=3)
    s.run_mcmc(x0, 40)
    assert len(s._chain_host) == 0 and s._chain_on_device == 40           # read where it lies
    whole = chain_history(m, s)
    part = chain_history(m, s, discard=7, thin=3, t_bins=4, v_bins=13)
    with pytest.raises(ValueError, match='leaves no steps'):
        chain_history(m, s, discard=40)
    for call in (lambda: E.chain_history(s._native, Q5, discard=40),
                 lambda: E.chain_raster(s._native, 1, whole.edges, discard=40)):
        with pytest.raises(LcfError) as err:
            call()
        assert err.value.status == 1
    idle = EnsembleSampler(64, 5, s.engine, seed=2)
    with pytest.raises(ValueError, match='no chain is stored'):
        chain_history(m, idle)
    for call in (lambda: E.chain_history(idle._native, Q5), lambda: E.chain_raster(idle._native, 1, whole.edges)):
        with pytest.raises(LcfError) as err:
            call()
        assert err.value.status == 7
    assert len(s._chain_host) == 0 and s._chain_on_device == 40           # ... and it still lies there: no download
    x, lp = s.get_chain(), s.get_log_prob()
    assert x.shape == (40, 64, 5) and lp.shape == (40, 64)
    assert whole.names == m.input_names and whole.labels == m.axis_labels  # t_0 and its label as they are
    _check(whole, x, lp)
    _check(part, x, lp, discard=7, thin=3)
    assert whole.counts.shape == (5, 40, 64) and part.counts.shape == (5, 4, 13) and len(part.steps) == 11
    _same(whole, chain_history(m, x, log_prob=lp))                          # the array form, uploaded
    _same(part, chain_history(m, x, log_prob=lp, discard=7, thin=3, t_bins=4, v_bins=13))
    # the sampler's own accept counters: an independent check of the moves
    first = _numpy_moves(np.stack([x0, x[0]]), [1])[0]
    assert whole.n_moved[0] == -1 and first + whole.n_moved[1:].sum() == s._naccepted.sum()
    s.run_mcmc(None, 10)                                                   # the chain is now partly on the host
    later = chain_history(m, s, discard=7, thin=3)
    x, lp = s.get_chain(), s.get_log_prob()
    assert len(later.steps) == 15 and later.n_moved[-1] >= 0
    _check(later, x, lp, discard=7, thin=3)


def test_population_in_one_call():
    """Three transients of 4, 5 and 6 columns (the last with a fitted sigma): one call, each equal to its own."""
    nw = 32
    ts = [_transient(*spec, nw) for spec in P1[:3]]
    pop = PopulationSampler([tr['problem'] for tr in ts], nw, seed=17)
    pop.run_mcmc({k: tr['x0'] for k, tr in enumerate(ts)}, 12)
    models = [tr['model'] for tr in ts]
    assert [pop[k].ndim for k in range(3)] == [4, 5, 6]
    got = pop.history(models, discard=2, v_bins=11)
    assert sorted(got) == [0, 1, 2] and all(pop[k]._chain_on_device == 12 and len(pop[k]._chain_host) == 0 for k in got)
    for k in got:
        _same(got[k], chain_history(models[k], pop[k], discard=2, v_bins=11, use_sigma=ts[k]['sigma']))
        assert (got[k].names[-1] == '\\sigma') == ts[k]['sigma'] and len(got[k].names) == pop[k].ndim
    assert all(pop[k]._chain_on_device == 12 for k in got)
    for k in got:
        _check(got[k], pop[k].get_chain(), pop[k].get_log_prob(), discard=2)
    # the chains are now on the host: the call that uploads them gives the same
    again = pop.history(models, discard=2, v_bins=11)
    for k in got:
        _same(again[k], got[k])
    with pytest.raises(ValueError, match='transient 0'):
        pop.history(models, discard=12)


def test_reproducible_and_independent_of_the_chunks(monkeypatch):
    x, lp = _chain(23, 1025, 5, seed=70)
    a = chain_history(None, x, log_prob=lp, t_bins=3)
    b = chain_history(None, x, log_prob=lp, t_bins=3)
    monkeypatch.setenv('LCF_HISTORY_CHUNK', '1000')                        # a step bin's samples in nine workgroups
    c = chain_history(None, x, log_prob=lp, t_bins=3)
    monkeypatch.setenv('LCF_HISTORY_CHUNK', '100000')                      # ... and in one
    d = chain_history(None, x, log_prob=lp, t_bins=3)
    for other in (b, c, d):
        _same(a, other)
    _check(a, x, lp)


def test_lightcurve_mcmc_keeps_the_burn_in_history():
    pb = small_problem()
    lc = lc_dict(pb['t'], pb['names'], pb['y'], pb['dy'])
    priors = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.5)]
    p_lo, p_up = np.array(list(0.9 * TRUTH[:4]) + [0.05]), np.array(list(1.1 * TRUTH[:4]) + [0.15])
    m = M.ShockCooling(redshift=0.)
    kw = dict(priors=priors, p_lo=p_lo, p_up=p_up, nwalkers=16, nsteps=10, nsteps_burnin=12, seed=5)
    np.random.seed(4)
    with pytest.warns(UserWarning, match='chain plots are not produced by the MI355X engine'):
        s = lightcurve_mcmc(lc, m, show=True, **kw)
    h = s.burnin_history
    assert len(h.steps) == 12 and h.n_walkers == 16 and h.quantiles.shape == (5, 12, 5) and h.counts.shape == (5, 12, 64)
    assert h.names == m.input_names and s.chain.shape == (16, 10, 5)
    # the same burn-in by hand: the same start (NumPy's generator), the same seed
    np.random.seed(4)
    start = p_lo + (p_up - p_lo) * np.random.rand(16, 5)
    hand = EnsembleSampler(16, 5, s.engine, seed=5)
    hand.run_mcmc(start, 12)
    _same(h, chain_history(m, hand))
    _check(h, hand.get_chain(), hand.get_log_prob())
    assert np.array_equal(h.n_moved[1:] >= 0, np.ones(11, dtype=bool)) and h.n_moved[0] == -1
    # the post-burn-in half is chain_history(model, sampler)
    after = chain_history(m, s)
    _check(after, s.get_chain(), s.get_log_prob())
    np.random.seed(4)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        plain = lightcurve_mcmc(lc, m, **kw)
    assert not hasattr(plain, 'burnin_history') and not any('chain plots' in str(w.message) for w in seen)
    np.random.seed(4)
    with pytest.warns(UserWarning, match='chain plots are not produced'):
        saved = lightcurve_mcmc(lc, m, save_plot_as='chains.pdf', **kw)
    _same(saved.burnin_history, h)
