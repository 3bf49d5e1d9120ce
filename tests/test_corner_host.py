"""The host half of posterior_corner: contour levels (corner.hist2d's rule), the reference's t0_offset and label
rewriting (fitting.py:241-251), argument errors that must come before any device call, and the pair accessor."""
import numpy as np
import pytest

from conftest import golden
from lightcurve_fitting_amd import engine as E, fitting as Fit, models as M
from lightcurve_fitting_amd.fitting import CornerData, corner_contour_levels, posterior_corner


def _companion():
    c = golden('companion')
    lc = {'MJD': c['csb/t'], 'filter': [str(x) for x in c['csb/names']], 'lum': c['csb/lum'], 'dlum': c['csb/dlum']}
    return M.CompanionShocking(lc, redshift=0.003)


def test_contour_levels_follow_corner_hist2d():
    H = np.array([[4, 3], [2, 1]])
    # sorted 4 3 2 1, cumulative shares 0.4 0.7 0.9 1: the last share <= 0.5 belongs to 4, the last <= 0.8 to 3
    assert np.array_equal(corner_contour_levels(H, (0.5, 0.8)), [3., 4.])
    assert np.array_equal(corner_contour_levels(H, (0.3,)), [4.])          # no share <= 0.3: the largest count
    # both levels pick 4: the first of the equal neighbours is multiplied by 1 - 1e-4
    assert np.array_equal(corner_contour_levels(H, (0.4, 0.45)), [4. * (1. - 1e-4), 4.])
    # three equal values: nudged until no two neighbours are equal, ascending
    V = corner_contour_levels(H, (0.4, 0.45, 0.5))
    assert np.all(np.diff(V) > 0.) and V[-1] == 4. and V[0] == pytest.approx(4. * (1. - 1e-4) ** 2, rel=1e-15)
    assert np.all(np.isnan(corner_contour_levels(np.zeros((3, 3)), (0.5, 0.9))))
    assert np.allclose(Fit.CORNER_LEVELS, 1. - np.exp(-0.5 * np.array([0.5, 1., 1.5, 2.]) ** 2), rtol=0, atol=1e-16)


def _settle(model, x, **kw):
    """The plan's offsets / range / edges / labels from NumPy's column extremes (what the range pass returns)."""
    plan = Fit._CornerPlan(model, x.shape[1], kw.pop('bins', 20), kw.pop('range', None), None, kw.pop('t0_offset', None),
                           kw.pop('use_sigma', False))
    return plan, plan.settle(np.nanmin(x, axis=0), np.nanmax(x, axis=0))


def test_t0_offset_and_labels():
    rng = np.random.default_rng(0)
    m = M.ShockCooling(redshift=0.)
    x = rng.uniform(1., 2., (50, 5))
    x[:, 4] = 58000.3 + rng.uniform(0., 0.5, 50)
    plan, (offsets, rng_, edges, labels) = _settle(m, x)
    assert plan.names == m.input_names == ['v_\\mathrm{s*}', 'M_\\mathrm{env}', 'f_\\rho M', 'R', 't_0']
    assert np.array_equal(offsets, [0., 0., 0., 0., 58000.])              # floor(min)
    assert labels[:4] == m.axis_labels[:4] and labels[4] == '$t_0 - 58000$ (d)'
    shifted = x - offsets
    assert np.array_equal(rng_, np.stack([shifted.min(axis=0), shifted.max(axis=0)], axis=1))
    for d in range(5):
        assert np.array_equal(edges[d], np.linspace(rng_[d, 0], rng_[d, 1], 21))
    # an explicit offset is formatted as the reference formats it; an explicit range is in shifted coordinates
    _, (offsets, rng_, edges, labels) = _settle(m, x, t0_offset=57999.25, range=[None] * 4 + [(1., 2.)], bins=4)
    assert offsets[4] == 57999.25 and labels[4] == '$t_0 - 57999.25$ (d)'
    assert np.array_equal(rng_[4], [1., 2.]) and np.array_equal(edges[4], [1., 1.25, 1.5, 1.75, 2.])
    # a zero offset -- given, or the floor of a small minimum -- leaves column and label alone
    for kw in (dict(t0_offset=0.), dict()):
        y = x.copy()
        y[:, 4] -= 58000.
        _, (offsets, rng_, _, labels) = _settle(m, y, **kw)
        assert np.all(offsets == 0.) and labels == m.axis_labels
        assert np.array_equal(rng_[4], [y[:, 4].min(), y[:, 4].max()])
    # use_sigma: one more column, named and labelled as lightcurve_mcmc names it
    plan, (_, _, _, labels) = _settle(m, np.column_stack([x, rng.uniform(0., 1., 50)]), use_sigma=True)
    assert plan.names[-1] == '\\sigma' and labels[-1] == '$\\sigma$' and len(labels) == 6
    assert m.input_names[-1] == 't_0'                                     # (the model is left as it was)
    # no model: plain names, nothing shifted
    plan, (offsets, _, _, labels) = _settle(None, x)
    assert plan.names == labels == ['p0', 'p1', 'p2', 'p3', 'p4'] and np.all(offsets == 0.)


def test_companion_shocking_time_columns_share_one_offset():
    m = _companion()
    rng = np.random.default_rng(1)
    x = rng.uniform(0.5, 1.5, (40, 8))
    x[:, 0] = 57001.7 + rng.uniform(0., 1., 40)       # t_0
    x[:, 3] = 57018.2 + rng.uniform(0., 1., 40)       # t_max
    _, (offsets, rng_, _, labels) = _settle(m, x)
    assert np.array_equal(offsets, [57001., 0., 0., 57001., 0., 0., 0., 0.])   # floor(min t_0) for both
    assert labels[0] == '$t_0 - 57001$ (d)' and labels[3] == '$t_\\mathrm{max} - 57001$ (d)'
    assert labels[1] == m.axis_labels[1]
    assert np.array_equal(rng_[3], [(x[:, 3] - 57001.).min(), (x[:, 3] - 57001.).max()])


def test_argument_errors_come_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(E, 'chain_range', no_device)
    monkeypatch.setattr(E, 'chain_hist', no_device)
    monkeypatch.setattr(E, 'load_library', no_device)
    m = M.ShockCooling(redshift=0.)
    x = np.random.default_rng(2).uniform(1., 2., (30, 5))
    for bins in (0, 129, 2.5):
        with pytest.raises(ValueError, match='bins'):
            posterior_corner(m, x, bins=bins)
    with pytest.raises(ValueError, match='no dynamic range'):
        posterior_corner(m, x, range=[None, (1.5, 1.5), None, None, None])
    with pytest.raises(ValueError, match='columns'):
        posterior_corner(m, x[:, :4])
    with pytest.raises(ValueError, match='columns'):
        posterior_corner(m, x, use_sigma=True)
    with pytest.raises(ValueError, match='sigma'):
        posterior_corner(m, np.column_stack([x, x, x[:, :1]]), use_sigma=True)
    with pytest.raises(ValueError, match='discard and thin'):
        posterior_corner(m, x, discard=3)
    with pytest.raises(ValueError, match='discard and thin'):
        posterior_corner(m, x, thin=2)
    for bad in ([(0., 3.)] * 4, [(0., 3.)] * 6):
        with pytest.raises(ValueError, match='range needs one entry per column'):
            posterior_corner(m, x, range=bad)
    with pytest.raises(ValueError, match='lo <= hi'):
        posterior_corner(m, x, range=[(2., 1.)] + [None] * 4)
    with pytest.raises(ValueError, match='levels'):
        posterior_corner(m, x, levels=[0.5, 1.5])
    with pytest.raises(ValueError, match='from 1 to 16 columns'):
        posterior_corner(None, np.zeros((4, 17)))
    with pytest.raises(ValueError, match='t0_offset needs a model'):
        posterior_corner(None, x, t0_offset=3.)
    with pytest.raises(ValueError, match='shape'):
        posterior_corner(None, np.zeros(7))


def test_pair_accessor_index_and_orientation():
    """hist2d[a, b] for b < a is np.histogram2d(x[:, b], x[:, a]); pair() serves either order."""
    rng = np.random.default_rng(3)
    x = rng.normal(size=(500, 3)) * [1., 5., 0.1] + [0., 2., 7.]
    bins = 6
    plan = Fit._CornerPlan(None, 3, bins, None, (0.5, 0.9), None, False)
    offsets, rng_, edges, labels = plan.settle(x.min(axis=0), x.max(axis=0))
    hist1d = np.array([np.histogram(x[:, d], bins=edges[d])[0] for d in range(3)])
    pairs = np.array([np.histogram2d(x[:, b], x[:, a], bins=(edges[b], edges[a]))[0]
                      for a in range(1, 3) for b in range(a)]).astype(np.int64)      # index a (a - 1) / 2 + b
    res = plan.data(offsets, rng_, edges, labels, hist1d, pairs, len(x), np.zeros(3, dtype=np.int64))
    assert isinstance(res, CornerData) and res.hist2d.shape == (3, 3, bins, bins) and res.hist2d.dtype == np.int64
    assert res.contour_levels.shape == (3, 3, 2) and res.n_samples == 500
    for a in range(3):
        for b in range(3):
            if b < a:
                want = np.histogram2d(x[:, b], x[:, a], bins=(edges[b], edges[a]))[0]
                assert np.array_equal(res.hist2d[a, b], want) and want.sum() == 500
                assert np.array_equal(res.contour_levels[a, b], corner_contour_levels(want, (0.5, 0.9)))
                H, xe, ye, V = res.pair(a, b)
                assert np.array_equal(H, want) and np.array_equal(xe, edges[b]) and np.array_equal(ye, edges[a])
                # the other order: column a on the first axis
                Ht, xe, ye, Vt = res.pair(b, a)
                assert np.array_equal(Ht, want.T) and np.array_equal(xe, edges[a]) and np.array_equal(ye, edges[b])
                assert np.array_equal(Ht, np.histogram2d(x[:, a], x[:, b], bins=(edges[a], edges[b]))[0])
                assert np.array_equal(V, Vt)
            else:
                assert not res.hist2d[a, b].any() and np.all(np.isnan(res.contour_levels[a, b]))
    # marginals of a pair are the columns' histograms (every sample is inside both ranges)
    assert np.array_equal(res.hist2d[2, 1].sum(axis=1), res.hist1d[1])
    assert np.array_equal(res.hist2d[2, 1].sum(axis=0), res.hist1d[2])
    for bad in ((1, 1), (3, 0), (0, -1)):
        with pytest.raises(IndexError):
            res.pair(*bad)


def test_the_wrappers_check_shapes_before_the_library(monkeypatch):
    monkeypatch.setattr(E, 'load_library', lambda *a, **k: None)
    x = np.zeros((10, 3))
    with pytest.raises(ValueError, match='shape'):
        E.chain_hist(x, np.zeros(2), np.zeros((3, 5)))
    with pytest.raises(ValueError, match='shape'):
        E.chain_hist(x, np.zeros(3), np.zeros((2, 5)))
    with pytest.raises(ValueError, match='shape'):
        E.chain_range(np.zeros(5))
