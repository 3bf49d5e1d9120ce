"""posterior_corner on the device against NumPy: every count must EQUAL np.histogram / np.histogram2d on the same
samples and ranges (integers: np.array_equal, no tolerance), every edge table must be np.linspace's bit for bit, and
the extremes of the range pass must be NumPy's minimum and maximum."""
import warnings

import numpy as np
import pytest

from lightcurve_fitting_amd import engine as E, models as M
from lightcurve_fitting_amd.engine import LcfError
from lightcurve_fitting_amd.fitting import CORNER_LEVELS, corner_contour_levels, posterior_corner
from lightcurve_fitting_amd.sampler import EnsembleSampler, PopulationSampler
from test_gpu_population_mixed import P1, _transient
from test_gpu_predictive import _fit

pytestmark = pytest.mark.gpu


def _posterior_like(n, n_dim, seed):
    """Correlated columns of very different scale (and one far from zero), as a chain's are."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, n_dim))
    z[:, 1:] += 0.7 * z[:, :-1]
    return z * np.geomspace(1e-3, 1e4, n_dim) + np.linspace(-5., 58000., n_dim)


def _numpy_counts(x, rng, bins):
    """np.histogram of every column and np.histogram2d of every pair b < a, on the ranges rng (P, 2)."""
    n_dim = x.shape[1]
    with np.errstate(invalid='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        h1 = np.array([np.histogram(x[:, d], bins=bins, range=tuple(rng[d]))[0] for d in range(n_dim)])
        h2 = np.zeros((n_dim, n_dim, bins, bins), dtype=np.int64)
        for a in range(1, n_dim):
            for b in range(a):
                h2[a, b] = np.histogram2d(x[:, b], x[:, a], bins=bins, range=[tuple(rng[b]), tuple(rng[a])])[0]
    return h1, h2


def _check(res, x, bins=20, shifted=None):
    """res against NumPy on the samples x (shifted: what NumPy histograms, default x itself)."""
    v = x if shifted is None else shifted
    n_dim = x.shape[1]
    assert res.hist1d.shape == (n_dim, bins) and res.hist2d.shape == (n_dim, n_dim, bins, bins)
    assert res.hist1d.dtype == res.hist2d.dtype == np.int64 and res.n_samples == len(x)
    assert np.array_equal(res.n_nan, np.isnan(x).sum(axis=0))
    for d in range(n_dim):
        assert np.array_equal(res.edges[d], np.linspace(res.range[d, 0], res.range[d, 1], bins + 1))   # bitwise
    h1, h2 = _numpy_counts(v, res.range, bins)
    assert np.array_equal(res.hist1d, h1)
    assert np.array_equal(res.hist2d, h2)
    for a in range(1, n_dim):
        for b in range(a):
            assert np.array_equal(res.contour_levels[a, b], corner_contour_levels(h2[a, b], res.levels), equal_nan=True)
    return h1, h2


def _default_range(res, v):
    assert np.array_equal(res.range, np.stack([np.nanmin(v, axis=0), np.nanmax(v, axis=0)], axis=1))


@pytest.mark.parametrize('n', [1, 63, 65, 4097])
def test_sizes_that_break_the_chunking(n):
    """Fewer samples than a wave, one more than a wave, and a workgroup's sweep (1024) four times and one over."""
    x = _posterior_like(n, 5, seed=n)
    if n == 1:
        res = posterior_corner(None, x, range=[(v - 1., v + 2.) for v in x[0]])
    else:
        res = posterior_corner(None, x)
        _default_range(res, x)
    _check(res, x)
    assert np.all(res.hist1d.sum(axis=1) == n) and res.hist2d[4, 0].sum() == n
    assert res.names == res.labels == ['p0', 'p1', 'p2', 'p3', 'p4'] and np.all(res.offsets == 0.)
    assert np.array_equal(res.levels, CORNER_LEVELS)


@pytest.mark.parametrize('n_dim,bins', [(2, 20), (9, 20), (16, 20), (3, 64), (3, 128)])
def test_dimensions_and_bins(n_dim, bins):
    """9 columns: 36 pairs in one group; 16 columns: 120 pairs in more than one; 128 bins: one pair is 64 KiB."""
    x = _posterior_like(3001, n_dim, seed=10 * n_dim + bins)
    res = posterior_corner(None, x, bins=bins)
    _default_range(res, x)
    _check(res, x, bins)


def test_one_column_needs_no_pair_storage():
    x = _posterior_like(777, 1, seed=3)
    res = posterior_corner(None, x)
    _check(res, x)
    lo, hi, n_nan = E.chain_range(x)
    assert lo[0] == x.min() and hi[0] == x.max() and n_nan[0] == 0
    h1, h2 = E.chain_hist(x, np.zeros(1), res.edges)      # (the wrapper passes a NULL hist2d: there are no pairs)
    assert h2.shape == (0, 20, 20) and np.array_equal(h1, res.hist1d)


def test_native_limits_are_invalid_arguments():
    x = _posterior_like(100, 3, seed=4)
    ok = np.array([np.linspace(c.min(), c.max(), 130) for c in x.T])
    for edges in (ok, ok[:, ::-1][:, :21].copy(), np.full((3, 21), np.nan)):   # 129 bins; descending; NaN
        with pytest.raises(LcfError) as err:
            E.chain_hist(x, np.zeros(3), edges)
        assert err.value.status == 1
    wide = np.zeros((10, 17))
    for call in (lambda: E.chain_range(wide), lambda: E.chain_hist(wide, np.zeros(17), np.tile(np.linspace(-1., 1., 21), (17, 1)))):
        with pytest.raises(LcfError) as err:
            call()
        assert err.value.status == 1
    with pytest.raises(ValueError, match='no dynamic range'):                  # corner refuses a constant column
        posterior_corner(None, np.column_stack([x, np.full(100, 2.5)]))


def test_edge_membership():
    """Values on, just below and just above every edge: bin i holds edges[i] <= v < edges[i + 1], the last bin also
    v == hi; NaN and the neighbours outside [lo, hi] are in no bin."""
    e = np.linspace(0., 1., 21)
    col = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                          [1., np.nextafter(1., np.inf), np.nextafter(0., -np.inf), np.nan, np.nan]])
    rng = np.random.default_rng(5)
    x = np.column_stack([col, rng.uniform(0.2, 0.8, len(col))])
    x[3, 1] = np.nan
    res = posterior_corner(None, x, range=[(0., 1.), (0., 1.)])
    assert np.array_equal(res.edges[0], e) and np.array_equal(res.n_nan, [2, 1])
    # the definition, bin by bin
    inside = col[(col >= 0.) & (col <= 1.)]
    idx = np.minimum(np.searchsorted(e, inside, 'right') - 1, 19)
    want = np.bincount(idx, minlength=20)
    assert np.array_equal(res.hist1d[0], want)
    # every interior edge: itself and its upper neighbour in its bin, its lower neighbour in the bin below
    assert np.all(want[:19] == 3) and want[19] == 5                          # (the last: also hi, given twice)
    assert res.hist1d[0].sum() == len(col) - 2 - 2 - 2                       # NaN, below lo, above hi: two of each
    _check(res, x)
    # a pair counts a row only with both coordinates in a bin
    both = (x[:, 0] >= 0.) & (x[:, 0] <= 1.) & ~np.isnan(x[:, 1])
    assert res.hist2d[1, 0].sum() == both.sum()


def test_range_narrower_than_the_data():
    x = _posterior_like(4097, 4, seed=6)
    lo, hi = np.percentile(x, 20., axis=0), np.percentile(x, 85., axis=0)
    rng = [(lo[0], hi[0]), None, (lo[2], hi[2]), (lo[3], hi[3])]
    res = posterior_corner(None, x, range=rng)
    assert np.array_equal(res.range[1], [x[:, 1].min(), x[:, 1].max()]) and np.array_equal(res.range[2], rng[2])
    _check(res, x)
    inside = (x >= res.range[:, 0]) & (x <= res.range[:, 1])
    assert np.array_equal(res.hist1d.sum(axis=1), inside.sum(axis=0)) and not inside[:, 0].all()
    for a in range(1, 4):
        for b in range(a):
            assert res.hist2d[a, b].sum() == np.sum(inside[:, a] & inside[:, b])


def test_ties_concentration_and_key_order():
    """60 % of the rows are one exact row (one LDS counter takes most of a workgroup's adds); a column of both signs
    from 1e-300 to 1e300 with both zeros orders the range pass's keys."""
    n = 4096
    rng = np.random.default_rng(7)
    x = _posterior_like(n, 5, seed=8)
    x[rng.permutation(n)[:int(0.6 * n)]] = x[0]
    mag = 10. ** rng.uniform(-300., 300., n)
    x[:, 4] = np.where(rng.random(n) < 0.5, -mag, mag)
    x[5, 4], x[6, 4] = -0., 0.
    res = posterior_corner(None, x)
    _default_range(res, x)
    h1, h2 = _check(res, x)
    assert h1[0].max() >= int(0.6 * n) and h2[1, 0].max() >= int(0.6 * n)
    # zeros only: the smallest is -0.0 or +0.0, equal under ==; then the smallest positive and largest negative values
    z = np.zeros((n, 2))
    z[::2, 0], z[:, 1] = -0., np.abs(x[:, 4])
    lo, hi, n_nan = E.chain_range(z)
    assert lo[0] == 0. and hi[0] == 0. and lo[1] == z[:, 1].min() and hi[1] == z[:, 1].max()
    lo, hi, n_nan = E.chain_range(-z)
    assert lo[1] == -z[:, 1].max() and hi[1] == -z[:, 1].min()
    # infinities are values (the extremes), NaNs are not; a column of NaNs alone has no extremes
    w = np.column_stack([x[:, 4], np.full(n, np.nan), x[:, 0]])
    w[1, 0], w[2, 0], w[3, 0], w[4, 2] = np.inf, -np.inf, np.nan, np.nan
    lo, hi, n_nan = E.chain_range(w)
    assert lo[0] == -np.inf and hi[0] == np.inf and np.isnan(lo[1]) and np.isnan(hi[1])
    assert lo[2] == np.nanmin(w[:, 2]) and hi[2] == np.nanmax(w[:, 2]) and np.array_equal(n_nan, [1, n, 1])


def test_chain_in_place():
    lc, m, s = _fit(64, 40)
    assert len(s._chain_host) == 0 and s._chain_on_device == 40           # read where it lies
    a = posterior_corner(m, s, discard=7, thin=3)
    whole = posterior_corner(m, s)
    assert len(s._chain_host) == 0 and s._chain_on_device == 40           # ... and it still lies there: no download
    with pytest.raises(ValueError, match='leaves no steps'):
        posterior_corner(m, s, discard=40)
    with pytest.raises(LcfError) as err:
        E.chain_range(s._native, discard=40)
    assert err.value.status == 1
    idle = EnsembleSampler(64, 5, s.engine, seed=2)
    with pytest.raises(ValueError, match='no chain is stored'):
        posterior_corner(m, idle)
    with pytest.raises(LcfError) as err:
        E.chain_range(idle._native)
    assert err.value.status == 7
    assert len(s._chain_host) == 0 and s._chain_on_device == 40
    flat = s.get_chain(discard=7, thin=3, flat=True)
    assert a.n_samples == len(flat) == 11 * 64 and a.names == m.input_names
    off = np.floor(flat[:, 4].min())
    assert a.offsets[4] == off and np.all(a.offsets[:4] == 0.)
    shifted = flat - a.offsets
    _default_range(a, shifted)
    _check(a, flat, shifted=shifted)
    everything = s.get_chain(flat=True)
    assert whole.n_samples == 40 * 64
    _check(whole, everything, shifted=everything - whole.offsets)
    b = posterior_corner(m, flat)                                          # the array form, uploaded
    for f in ('offsets', 'range', 'edges', 'hist1d', 'hist2d', 'contour_levels', 'n_nan'):
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    s.run_mcmc(None, 10)                                                   # the chain is now partly on the host
    c = posterior_corner(m, s, discard=7, thin=3)
    flat = s.get_chain(discard=7, thin=3, flat=True)
    assert c.n_samples == 15 * 64
    _check(c, flat, shifted=flat - c.offsets)


def test_shift_of_the_explosion_time():
    """t_0 near MJD 58000.3: counted as x - floor(min), the label says so, the other columns are untouched."""
    rng = np.random.default_rng(9)
    m = M.ShockCooling(redshift=0.)
    x = np.array([1.2, 0.5, 3.0, 2.0, 0.]) * (1. + 0.2 * rng.uniform(-1., 1., (5000, 5)))
    x[:, 4] = 58000.3 + 0.05 * rng.standard_normal(5000)
    res = posterior_corner(m, x)
    assert np.array_equal(res.offsets, [0., 0., 0., 0., 58000.]) and res.labels[4] == '$t_0 - 58000$ (d)'
    assert res.labels[:4] == m.axis_labels[:4]
    shifted = x.copy()
    shifted[:, 4] -= 58000.
    _default_range(res, shifted)
    _check(res, x, shifted=shifted)
    # the caller's offset and a range in shifted coordinates
    res = posterior_corner(m, x, t0_offset=58000.25, range=[None] * 4 + [(0., 0.1)], bins=13)
    shifted = x.copy()
    shifted[:, 4] -= 58000.25
    assert res.labels[4] == '$t_0 - 58000.25$ (d)' and np.array_equal(res.range[4], [0., 0.1])
    _check(res, x, bins=13, shifted=shifted)
    assert 0 < res.hist1d[4].sum() < 5000


def test_population_in_one_call():
    """Three transients of 4, 5 and 6 columns (the last with a fitted sigma): one call, each equal to its own."""
    nw = 32
    ts = [_transient(*spec, nw) for spec in P1[:3]]
    pop = PopulationSampler([tr['problem'] for tr in ts], nw, seed=17)
    pop.run_mcmc({k: tr['x0'] for k, tr in enumerate(ts)}, 12)
    models = [tr['model'] for tr in ts]
    assert [pop[k].ndim for k in range(3)] == [4, 5, 6]
    got = pop.corner(models, discard=2, bins=11)
    assert sorted(got) == [0, 1, 2] and all(pop[k]._chain_on_device == 12 and len(pop[k]._chain_host) == 0 for k in got)
    solo = {k: posterior_corner(models[k], pop[k], discard=2, bins=11, use_sigma=ts[k]['sigma']) for k in got}
    for k in got:
        for f in ('offsets', 'range', 'edges', 'hist1d', 'hist2d', 'contour_levels', 'n_nan'):
            assert np.array_equal(getattr(got[k], f), getattr(solo[k], f), equal_nan=True), (k, f)
        assert got[k].names == solo[k].names and got[k].labels == solo[k].labels
        assert (got[k].names[-1] == '\\sigma') == ts[k]['sigma']
    for k in got:
        flat = pop[k].get_chain(discard=2, flat=True)
        assert got[k].n_samples == len(flat) == 10 * nw
        _check(got[k], flat, bins=11, shifted=flat - got[k].offsets)
    # the chains are now on the host: the call that uploads them gives the same
    again = pop.corner(models, discard=2, bins=11)
    for k in got:
        assert np.array_equal(again[k].hist2d, got[k].hist2d) and np.array_equal(again[k].hist1d, got[k].hist1d)


def test_reproducible_and_independent_of_the_pair_groups(monkeypatch):
    x = _posterior_like(4097, 9, seed=11)
    a, b = posterior_corner(None, x), posterior_corner(None, x)
    monkeypatch.setenv('LCF_CORNER_GROUP_PAIRS', '1')                      # 36 groups of one pair each
    c = posterior_corner(None, x)
    monkeypatch.setenv('LCF_CORNER_GROUP_PAIRS', '7')                      # 6 groups, the last of one pair
    d = posterior_corner(None, x)
    for other in (b, c, d):
        for f in ('range', 'edges', 'hist1d', 'hist2d', 'contour_levels', 'n_nan'):
            assert np.array_equal(getattr(a, f), getattr(other, f), equal_nan=True), f
    _check(a, x)
