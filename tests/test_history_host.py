"""The host half of chain_history: the four entry points are declared and bound, argument errors come before any device
call, the native limits are decided before any HIP call, the step bins follow (k * t_bins) // n_keep, the percentiles
assembled from order statistics are NumPy's bit for bit, and names and labels follow posterior_corner's rule."""
import os
import re

import numpy as np
import pytest

from lightcurve_fitting_amd import engine as E, fitting as Fit, models as M
from lightcurve_fitting_amd.engine import LcfError
from lightcurve_fitting_amd.fitting import ChainHistory, chain_history

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lcf_chain_history', 'lcf_chain_raster', 'lcf_samplers_chain_history', 'lcf_samplers_chain_raster')


def test_symbols_are_declared_and_bound_and_the_abi_is_8():
    header = open(os.path.join(ROOT, 'include', 'lcf.h')).read()
    declared = set(re.findall(r'\b(lcf_[a-z_0-9]+)\s*\(', header))
    bound = {name for name, _, _ in E.SIGNATURES}
    lib = E.load_library()
    for name in NAMES:
        assert name in declared and name in bound and hasattr(lib, name)
    assert E.LCF_ABI_VERSION == 8 and lib.lcf_abi_version() == 8
    assert re.search(r'#define LCF_ABI_VERSION 8\b', header)


def _chain(n_t=12, n_w=10, n_dim=5, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_t, n_w, n_dim)) * np.geomspace(1e-3, 1e4, n_dim) + np.linspace(-5., 58000., n_dim)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    for name in ('chain_history', 'chain_raster', 'chain_range', 'chain_hist', 'load_library'):
        monkeypatch.setattr(E, name, no_device)
    m = M.ShockCooling(redshift=0.)
    x = _chain()
    with pytest.raises(ValueError, match='columns'):                       # a wrong column count for the model
        chain_history(m, x[:, :, :4])
    with pytest.raises(ValueError, match='columns'):
        chain_history(m, x, use_sigma=True)
    with pytest.raises(ValueError, match='from 1 to 16 columns'):
        chain_history(None, np.zeros((3, 40, 17)))
    for v_bins in (0, 257, 2.5, True):
        with pytest.raises(ValueError, match='v_bins'):
            chain_history(m, x, v_bins=v_bins)
    for t_bins in (0, 13, 1.5):                                            # 12 kept steps
        with pytest.raises(ValueError, match='t_bins'):
            chain_history(m, x, t_bins=t_bins)
    with pytest.raises(ValueError, match='t_bins'):                        # discard = 4, thin = 2: 4 kept steps
        chain_history(m, x, t_bins=5, discard=4, thin=2)
    with pytest.raises(ValueError, match='t_bins'):
        chain_history(None, np.zeros((5000, 2, 1)), t_bins=4097)
    for bad in ((1.5, 1.5), (2., 1.), (0., np.inf), (np.nan, 1.)):         # a range without extent
        with pytest.raises(ValueError, match='no extent'):
            chain_history(m, x, range=[None, bad, None, None, None])
    with pytest.raises(ValueError, match='range needs one entry per column'):
        chain_history(m, x, range=[(0., 1.)] * 4)
    for discard in (12, 100):
        with pytest.raises(ValueError, match='leaves no steps'):
            chain_history(m, x, discard=discard)
    for kw in (dict(discard=-1), dict(thin=0)):
        with pytest.raises(ValueError, match='discard >= 0 and thin >= 1'):
            chain_history(m, x, **kw)
    for q in ((-0.1, 50.), (50., 100.5), (np.nan,)):
        with pytest.raises(ValueError, match=r'range \[0, 100\]'):
            chain_history(m, x, percentiles=q)
    with pytest.raises(ValueError, match='empty'):
        chain_history(m, x, percentiles=())
    with pytest.raises(ValueError, match='at most 16 percentiles'):
        chain_history(m, x, percentiles=np.linspace(0., 100., 17))
    for lp in (np.zeros((12, 9)), np.zeros((11, 10)), np.zeros(120), np.zeros((12, 10, 1))):
        with pytest.raises(ValueError, match='log_prob must have shape'):
            chain_history(m, x, log_prob=lp)
    with pytest.raises(ValueError, match='16384'):                         # the bound is named
        chain_history(None, np.zeros((1, 16385, 1)))
    for bad in (np.zeros((10, 5)), np.zeros(7), np.zeros((2, 3, 4, 5))):
        with pytest.raises(ValueError, match='shape'):
            chain_history(None, bad)
    with pytest.raises(ValueError, match='at least one'):
        chain_history(None, np.zeros((0, 4, 2)))


def test_the_wrappers_check_shapes_before_the_library(monkeypatch):
    monkeypatch.setattr(E, 'load_library', lambda *a, **k: None)
    x = np.zeros((6, 10, 3))
    with pytest.raises(ValueError, match='shape'):
        E.chain_history(np.zeros((10, 3)), [50.])
    with pytest.raises(ValueError, match='log_prob must have shape'):
        E.chain_history(x, [50.], log_prob=np.zeros((6, 9)))
    with pytest.raises(ValueError, match='shape'):
        E.chain_raster(x, 2, np.zeros((2, 5)))
    with pytest.raises(ValueError, match='shape'):
        E.chain_raster(x, 2, np.zeros(5))


def _status(call):
    with pytest.raises(LcfError) as err:
        call()
    return err.value.status


def test_native_limits_are_decided_before_any_hip_call():
    """Without a GPU a valid call ends in LCF_ERR_NO_DEVICE (3); every limit must be refused before that is found out --
    status 1, and 5 for more walkers than the sort takes."""
    no_gpu = E.load_library().lcf_device_count() <= 0

    def _valid(call):   # (with a GPU the call runs: tests/test_gpu_history.py checks what it returns)
        return _status(call) if no_gpu else (call(), 3)[1]
    x = _chain(6, 8, 3)
    q = [0., 50., 100.]
    edges = np.array([np.linspace(c.min(), c.max(), 9) for c in x.reshape(-1, 3).T])
    assert _valid(lambda: E.chain_history(x, q)) == 3
    assert _valid(lambda: E.chain_history(x, q, log_prob=x[:, :, 0])) == 3
    assert _valid(lambda: E.chain_raster(x, 6, edges)) == 3
    # the steps pass
    assert _status(lambda: E.chain_history(np.zeros((2, 4, 17)), q)) == 1               # n_dim
    assert _status(lambda: E.chain_history(np.zeros((2, 16385, 1)), q)) == 5            # n_w
    assert _status(lambda: E.chain_history(x, [])) == 1                                 # n_q
    assert _status(lambda: E.chain_history(x, np.linspace(0., 100., 17))) == 1
    assert _status(lambda: E.chain_history(x, [50., 100.1])) == 1
    assert _status(lambda: E.chain_history(x, [np.nan])) == 1
    assert _status(lambda: E.chain_history(x, q, discard=6)) == 1
    assert _status(lambda: E.chain_history(x, q, discard=-1)) == 1
    assert _status(lambda: E.chain_history(x, q, thin=0)) == 1
    assert _status(lambda: E.chain_history(np.zeros((0, 4, 2)), q)) == 1
    # the raster pass
    assert _status(lambda: E.chain_raster(np.zeros((2, 4, 17)), 1, np.tile(np.linspace(0., 1., 9), (17, 1)))) == 1
    assert _status(lambda: E.chain_raster(np.zeros((2, 16385, 1)), 1, np.linspace(0., 1., 9)[None])) == 5
    assert _status(lambda: E.chain_raster(x, 0, edges)) == 1                             # t_bins
    assert _status(lambda: E.chain_raster(x, 7, edges)) == 1                             # ... above n_keep
    assert _status(lambda: E.chain_raster(x, 3, edges, discard=2, thin=2)) == 1          # (2 kept steps)
    assert _valid(lambda: E.chain_raster(x, 2, edges, discard=2, thin=2)) == 3
    assert _status(lambda: E.chain_raster(np.zeros((4098, 1, 1)), 4097, np.linspace(0., 1., 9)[None])) == 1
    assert _valid(lambda: E.chain_raster(np.zeros((4098, 1, 1)), 4096, np.linspace(0., 1., 9)[None])) == 3
    assert _status(lambda: E.chain_raster(x, 2, np.tile(np.linspace(0., 1., 258), (3, 1)))) == 1   # v_bins = 257
    assert _valid(lambda: E.chain_raster(x, 2, np.tile(np.linspace(0., 1., 257), (3, 1)))) == 3   # v_bins = 256
    assert _status(lambda: E.chain_raster(x, 2, np.zeros((3, 1)))) == 1                            # v_bins = 0
    assert _status(lambda: E.chain_raster(x, 2, edges[:, ::-1].copy())) == 1             # descending
    assert _status(lambda: E.chain_raster(x, 2, np.full((3, 9), np.nan))) == 1
    assert _status(lambda: E.chain_raster(x, 2, np.zeros((3, 9)))) == 1                  # no extent
    assert _status(lambda: E.chain_raster(x, 2, edges, discard=6)) == 1


def _plan(n_t, t_bins=None, discard=0, thin=1, n_w=7, n_col=3, model=None, use_sigma=None, **kw):
    return Fit._HistoryPlan(model, n_t, n_w, n_col, kw.pop('percentiles', Fit.HISTORY_PERCENTILES), t_bins,
                            kw.pop('v_bins', 64), kw.pop('range', None), discard, thin, use_sigma)


@pytest.mark.parametrize('n_keep,t_bins', [(11, 4), (11, 11), (11, 1), (2000, 512), (7, 3)])
def test_step_edges_follow_the_rule(n_keep, t_bins):
    plan = _plan(n_keep, t_bins)
    k = np.arange(n_keep)
    which = (k * t_bins) // n_keep
    e = plan.step_edges
    assert e.shape == (t_bins + 1,) and e.dtype == np.int64 and e[0] == 0 and e[-1] == n_keep
    for i in range(t_bins):
        assert np.array_equal(k[which == i], np.arange(e[i], e[i + 1])) and e[i + 1] > e[i]
    if (n_keep, t_bins) == (11, 4):
        assert np.array_equal(e, [0, 3, 6, 9, 11])


def test_kept_steps_and_default_step_bins():
    plan = _plan(40, discard=7, thin=3)
    assert np.array_equal(plan.steps, np.arange(7, 40, 3)) and plan.t_bins == 11
    assert _plan(2000).t_bins == 512 and _plan(2000, discard=1600).t_bins == 400
    assert _plan(5000, 4096).t_bins == 4096


def test_assembled_percentiles_are_numpys_bit_for_bit():
    """What the device returns -- the order statistics of ranks lo and hi and n_valid -- taken here from np.sort; the
    assembly must give np.nanpercentile exactly, NaN cells and cells of one value included."""
    rng = np.random.default_rng(1)
    n_keep, n_w, n_col = 9, 257, 3
    x = _chain(n_keep, n_w, n_col, seed=2)
    lp = -0.5 * rng.chisquare(5, (n_keep, n_w))
    x[1, rng.permutation(n_w)[:100], 0] = np.nan
    x[2, :, 1] = np.nan                                                    # an all-NaN cell
    x[3, 1:, 2] = np.nan                                                   # one value left
    x[4, rng.permutation(n_w)[:150], 2] = x[4, 0, 2]                       # ties
    q = np.array([0., 2.5, 15.87, 50., 50., 84.14, 25., 100.])            # 25: an integer rank (n = 257)
    plan = _plan(n_keep, n_w=n_w, n_col=n_col, percentiles=q)
    cols = np.concatenate([x, lp[:, :, None]], axis=2)                     # the log-probability as column n_dim
    srt = np.sort(cols, axis=1)                                            # NaNs last
    n_valid = (~np.isnan(cols)).sum(axis=1)
    lo, hi, _ = Fit.quantile_ranks(np.maximum(n_valid, 1)[None], q[:, None, None])
    stat_lo, stat_hi = np.empty(lo.shape), np.empty(lo.shape)
    for k in range(n_keep):
        for c in range(n_col + 1):
            stat_lo[:, k, c], stat_hi[:, k, c] = srt[k, lo[:, k, c], c], srt[k, hi[:, k, c], c]
    stat_lo, stat_hi = (np.where(n_valid[None] > 0, s, np.nan) for s in (stat_lo, stat_hi))
    n_moved = np.array([-1] + [n_w] * (n_keep - 1))
    rng_, edges = plan.settle(np.nanmin(x.reshape(-1, n_col), axis=0), np.nanmax(x.reshape(-1, n_col), axis=0))
    res = plan.data(stat_lo, stat_hi, n_valid, n_moved, np.zeros((n_col, plan.t_bins, 64), dtype=np.int64), rng_, edges)
    assert isinstance(res, ChainHistory)
    with np.errstate(invalid='ignore'), pytest.warns(RuntimeWarning):
        want = np.nanpercentile(cols, q, axis=1)
    assert want.shape == (len(q), n_keep, n_col + 1)
    assert np.array_equal(res.quantiles, want[:, :, :n_col], equal_nan=True)
    assert np.array_equal(res.log_prob_quantiles, want[:, :, n_col], equal_nan=True)
    assert np.all(np.isnan(res.quantiles[:, 2, 1])) and res.n_valid[2, 1] == 0 and res.n_valid[1, 0] == n_w - 100
    assert np.all(res.quantiles[:, 3, 2] == x[3, 0, 2])
    assert np.isnan(res.frac_moved[0]) and np.all(res.frac_moved[1:] == 1.)
    assert res.n_walkers == n_w and np.array_equal(res.steps, np.arange(n_keep))
    assert res.quantiles.shape == (len(q), n_keep, n_col) and res.log_prob_quantiles.shape == (len(q), n_keep)
    for d in range(n_col):
        assert np.array_equal(res.edges[d], np.linspace(res.range[d, 0], res.range[d, 1], 65))
    assert 'ChainHistory' in repr(res) and not hasattr(res, '__dict__')


def test_default_range_of_a_constant_column_is_widened_as_numpy_widens_it():
    plan = _plan(5, n_col=2, range=[None, (1., 3.)], v_bins=4)
    assert plan.needs_extremes
    rng_, edges = plan.settle(np.array([2.5, 0.]), np.array([2.5, 9.]))
    assert np.array_equal(rng_, [[2., 3.], [1., 3.]]) and np.array_equal(edges[1], [1., 1.5, 2., 2.5, 3.])
    assert np.array_equal(edges[0], np.histogram_bin_edges([2.5], bins=4))
    with pytest.raises(ValueError, match='no finite range'):
        plan.settle(np.array([np.nan, 0.]), np.array([np.nan, 1.]))
    assert not _plan(5, n_col=2, range=[(0., 1.), (1., 3.)]).needs_extremes


def test_names_and_labels_follow_the_corner_rule():
    m = M.ShockCooling(redshift=0.)
    plain = _plan(5, n_col=5, model=m)
    assert plain.names == m.input_names == ['v_\\mathrm{s*}', 'M_\\mathrm{env}', 'f_\\rho M', 'R', 't_0']
    assert plain.labels == m.axis_labels and plain.labels[4] == '$t_0$ (d)'           # t_0: no offset, label untouched
    for use_sigma in (True, None):                                        # None: one column more than the model takes
        sig = _plan(5, n_col=6, model=m, use_sigma=use_sigma)
        assert sig.names == plain.names + ['\\sigma'] and sig.labels == plain.labels + ['$\\sigma$']
    assert m.input_names[-1] == 't_0'                                     # (the model is left as it was)
    with pytest.raises(ValueError, match='columns'):
        _plan(5, n_col=6, model=m, use_sigma=False)
    with pytest.raises(ValueError, match='columns'):
        _plan(5, n_col=7, model=m)
    none = _plan(5, n_col=3)
    assert none.names == none.labels == ['p0', 'p1', 'p2']
