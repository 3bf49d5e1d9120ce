"""``fitting.template_predictive`` on the GPU: the bands of the sum, the base and the template term of every built-in base
and template against the NumPy definition (``template_predictive_reference``) to the project's 1e-11
(``conftest.relerr``), the valid and dark counts as integers; NaN rows; the per-sample features index for index; tiling
and component subsets bit for bit; the product's own host route; end to end from a ``TemperedSampler``; the refusals."""
import numpy as np
import pytest

import template_predictive_reference as R
import template_reference as T
from conftest import relerr
from test_gpu_template import BOX_HI, BOX_LO, KW, MCMC, SEED, device_model, mcmc_priors
from lightcurve_fitting_amd import engine as E
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.engine import LcfError
from lightcurve_fitting_amd.fitting import lightcurve_mcmc, template_predictive
from lightcurve_fitting_amd.sampler import TemperedSampler

pytestmark = pytest.mark.gpu

TOL = 1e-11
Q = R.PERCENTILES
GRID = dict(t=R.GRID_T, filters_to_model=R.FILTERS)
_models = {}


def grid_model(kind, template):
    """One ``WithTemplate`` per case (it keeps its engines), with a template column for all six filters."""
    if (kind, template) not in _models:
        c = R.grid_case(kind, template)
        kw = dict(KW) if c['scale'] is None else dict(KW, scale=c['scale'])
        _models[kind, template] = M.WithTemplate(getattr(M, kind)(redshift=T.Z), c['template'], c['lc'], **kw)
    return _models[kind, template]


def assert_not_degenerate(B, Tm, Y, n_rows):
    """What the issue's fixture has, asserted on the reference alone (per 37 distinct rows)."""
    B, Tm, Y = B[..., :n_rows], Tm[..., :n_rows], Y[..., :n_rows]
    _, idx = R.features(B, Tm)
    assert not np.any(np.isnan(Y))
    assert np.sum(R.n_dark(B)) > 0
    assert np.sum(idx[2] < 0) >= 10 and np.sum(idx[2] >= 0) >= 150          # without / with a crossing
    assert np.sum(idx[3] >= 0) >= 150                                      # with a dip
    assert len(np.unique(idx[:2])) >= 4                                    # distinct peak indices


def compare_bands(res, B, Tm, Y, label):
    worst = 0.
    for name, V in (('total', Y), ('base', B), ('template', Tm)):
        want, want_valid = R.bands(V, Q)
        err = relerr(res.quantiles[name], want)
        print(f'{label}, {name}: {err:.2e}')
        worst = max(worst, err)
        assert np.array_equal(res.n_valid[name], want_valid) and res.n_valid[name].dtype == np.int64
        assert err < TOL
    assert np.array_equal(res.n_dark, R.n_dark(B))
    return worst


# ---- 1. bands ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('template', R.TEMPLATES)
@pytest.mark.parametrize('kind', R.KINDS)
def test_bands_against_the_reference(kind, template):
    model = grid_model(kind, template)
    for rows in ('tiled', 'jitter'):
        c, P, B, Tm, Y = R.reference_values(kind, template, rows)
        if rows == 'tiled':
            assert_not_degenerate(B, Tm, Y, T.N_ROWS)
        res = template_predictive(c['lc'], model, P, Q, features=False, **GRID)
        assert res.total.shape == (len(Q), 6, len(R.GRID_T)) and res.n_samples == 2100 and res.i_cross is None
        assert res.components == R.COMPONENTS and res.base is res.quantiles['base']
        compare_bands(res, B, Tm, Y, f'{kind}, {template}, {rows}')
        assert np.sum(res.n_dark) > 0


# ---- 2. NaN rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,template', [('ShockCooling2', 'sifto'), ('ShockCooling4', 'bump'), ('ShockCooling3', 'four')])
def test_nan_rows(kind, template):
    c, P, B, Tm, Y = R.reference_values(kind, template, 'nan')
    n = len(P)
    assert n == T.N_ROWS + 2 and np.all(np.isnan(B[..., -2])) and not np.any(np.isnan(Tm[..., -2]))
    assert np.all(np.isnan(Tm[R.FILTERS.index('r'), :, -1])) and not np.any(np.isnan(B[..., -1]))
    res = template_predictive(c['lc'], grid_model(kind, template), P, Q, **GRID)
    compare_bands(res, B, Tm, Y, f'{kind}, {template}, NaN rows')
    r = R.FILTERS.index('r')
    assert np.all(res.n_valid['base'] == n - 1) and np.all(res.n_valid['template'][r] == n - 1)
    assert np.all(res.n_valid['total'][r] == n - 2) and np.all(np.delete(res.n_valid['total'], r, 0) == n - 1)
    vals, idx = R.features(B, Tm)
    for k, name in enumerate(res.FEATURE_INDICES):
        assert np.array_equal(getattr(res, name), idx[k]), name
    assert np.all(res.i_peak_base[:, -2] == -1) and np.all(res.i_dip[:, -2] == -1) and np.all(np.isnan(res.y_peak_base[:, -2]))
    assert res.i_peak_template[r, -1] == -1 and res.i_cross[r, -1] == -1 and np.all(res.i_peak_template[:, -2] >= 0)


# ---- 3. features ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('template', R.TEMPLATES)
@pytest.mark.parametrize('kind', R.KINDS)
def test_features_against_the_reference(kind, template):
    c, P, B, Tm, Y = R.reference_values(kind, template, 'plain')
    assert_not_degenerate(B, Tm, Y, T.N_ROWS)
    vals, idx = R.features(B, Tm)
    res = template_predictive(c['lc'], grid_model(kind, template), P, (50.,), components='total', **GRID)
    for k, name in enumerate(res.FEATURE_INDICES):
        got = getattr(res, name)
        assert got.dtype == np.int32 and got.shape == (6, T.N_ROWS) and np.array_equal(got, idx[k]), name
    for k, (name, i_name) in enumerate(zip(res.FEATURE_VALUES, ('i_peak_base', 'i_peak_template', 'i_dip'))):
        err = relerr(getattr(res, name), vals[k])
        print(f'{kind}, {template}, {name}: {err:.2e}')
        assert err < TOL and np.array_equal(np.isnan(getattr(res, name)), getattr(res, i_name) < 0)
    t = R.GRID_T
    assert np.array_equal(res.t_cross, np.where(idx[2] < 0, np.nan, t[np.maximum(idx[2], 0)]), equal_nan=True)
    assert np.array_equal(res.t_dip, np.where(idx[3] < 0, np.nan, t[np.maximum(idx[3], 0)]), equal_nan=True)
    assert np.array_equal(res.n_cross_none, np.sum(idx[2] < 0, axis=1)) and np.array_equal(res.n_dip_none, np.sum(idx[3] < 0, axis=1))
    s = res.feature_summary(Q)
    assert s['t_dip'].shape == (len(Q), 6) and relerr(s['y_dip'], np.nanpercentile(vals[2], Q, axis=1)) < TOL
    assert np.array_equal(s['t_cross'], np.nanpercentile(res.t_cross, Q, axis=1), equal_nan=True)


# ---- 4. tiling and component subsets ------------------------------------------------------------------------------------------
def test_tiling_and_component_subsets_bit_for_bit():
    kind, template = 'ShockCooling4', 'sifto'
    c, P, _, _, _ = R.reference_values(kind, template, 'jitter')
    model = grid_model(kind, template)
    nt, nq = len(R.GRID_T), len(Q)
    ws3, ws1 = E.template_workspace(len(P), nt, 6, 3, nq, tile=1), E.template_workspace(len(P), nt, 6, 1, nq, tile=1)
    assert ws1 < ws3 < E.template_workspace(len(P), nt, 6, 3, nq, tile=2) < E.PREDICT_WORKSPACE_BYTES
    whole = template_predictive(c['lc'], model, P, Q, **GRID)
    tiled = template_predictive(c['lc'], model, P, Q, workspace_bytes=ws3, **GRID)
    total = template_predictive(c['lc'], model, P, Q, components=('total',), features=False, **GRID)
    total_tiled = template_predictive(c['lc'], model, P, Q, components='total', features=False, workspace_bytes=ws1, **GRID)
    assert total.components == ('total',) and total.base is None and total.template is None
    for name in R.COMPONENTS:
        assert np.array_equal(whole.quantiles[name], tiled.quantiles[name], equal_nan=True), name
        assert np.array_equal(whole.n_valid[name], tiled.n_valid[name])
    for other in (total, total_tiled):
        assert np.array_equal(whole.total, other.total, equal_nan=True) and np.array_equal(whole.n_dark, other.n_dark)
        assert np.array_equal(whole.n_valid['total'], other.n_valid['total'])
    assert np.array_equal(whole.n_dark, tiled.n_dark)
    for name in whole.FEATURE_INDICES + whole.FEATURE_VALUES:
        assert np.array_equal(getattr(whole, name), getattr(tiled, name), equal_nan=True), name
    with pytest.raises(LcfError, match=f'at least {ws3} bytes') as exc:
        template_predictive(c['lc'], model, P, Q, workspace_bytes=ws3 - 1, **GRID)
    assert exc.value.status == 1
    with pytest.raises(LcfError, match=f'at least {ws1} bytes'):
        template_predictive(c['lc'], model, P, Q, components='total', workspace_bytes=ws1 - 1, **GRID)


# ---- 5. the product's own host route --------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,template', [('ShockCooling2', 'sifto'), ('ShockCooling', 'bump'), ('ShockCooling4', 'four'),
                                           ('ShockCooling3', 'sifto')])
def test_against_model_and_components_on_the_host(kind, template):
    c, P, _, _, _ = R.reference_values(kind, template, 'jitter')
    P = P[:500]
    model = grid_model(kind, template)
    res = template_predictive(c['lc'], model, P, Q, **GRID)
    Y = model(R.GRID_T, R.FILTERS, *P.T)
    B, Tm = model.components(R.GRID_T, R.FILTERS, *P.T)
    assert Y.shape == (6, len(R.GRID_T), 500)
    bitwise = True
    for name, V in (('total', Y), ('base', B), ('template', Tm)):
        want, want_valid = R.bands(V, Q)
        err = relerr(res.quantiles[name], want)
        same = np.array_equal(res.quantiles[name], want, equal_nan=True)
        bitwise = bitwise and same
        print(f'{kind}, {template}, {name} vs np.nanpercentile of the host route: {err:.2e}, bitwise {same}')
        assert err < TOL and np.array_equal(res.n_valid[name], want_valid)
    assert np.array_equal(res.n_dark, R.n_dark(B))
    vals, idx = R.features(B, Tm)
    same = all(np.array_equal(getattr(res, n), idx[k]) for k, n in enumerate(res.FEATURE_INDICES)) and \
        all(np.array_equal(getattr(res, n), vals[k], equal_nan=True) for k, n in enumerate(res.FEATURE_VALUES))
    print(f'{kind}, {template}: bands bitwise {bitwise}, features bitwise {same}')
    for k, n in enumerate(res.FEATURE_INDICES):
        assert np.array_equal(getattr(res, n), idx[k]), n
    for k, n in enumerate(res.FEATURE_VALUES):
        assert relerr(getattr(res, n), vals[k]) < TOL


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------
def test_from_the_sampler_lightcurve_mcmc_returns():
    model, c, _ = device_model('ShockCooling2')
    np.random.seed(3)
    s = lightcurve_mcmc(c['lc'], model, priors=mcmc_priors(), p_lo=BOX_LO, p_up=BOX_HI, seed=SEED, **MCMC)
    assert isinstance(s, TemperedSampler)
    got = template_predictive(c['lc'], model, s, discard=5, thin=2, t=R.GRID_T)
    rows = s.get_chain(discard=5, thin=2, flat=True)
    want = template_predictive(c['lc'], model, rows, t=R.GRID_T)
    assert rows.shape == (8 * 16, 8) and got.n_samples == want.n_samples == len(rows)
    assert [f.name for f in got.filters] == sorted(set(c['lc']['filter']), key=lambda n: M.as_filter(n))
    for name in R.COMPONENTS:
        assert np.array_equal(got.quantiles[name], want.quantiles[name], equal_nan=True)
        assert np.array_equal(got.n_valid[name], want.n_valid[name])
    assert np.all(np.isfinite(got.total)) and np.array_equal(got.n_dark, want.n_dark)
    for name in got.FEATURE_INDICES + got.FEATURE_VALUES + got.FEATURE_TIMES:
        assert np.array_equal(getattr(got, name), getattr(want, name), equal_nan=True), name
    with pytest.raises(ValueError, match='leaves no steps'):
        template_predictive(c['lc'], model, s, discard=20, t=R.GRID_T)
    # repeated and unsorted times, a repeated filter: scattered back from the distinct ones
    t2 = np.array([8., 0.5, 8., 3.])
    a = template_predictive(c['lc'], model, rows, t=t2, filters_to_model=['r', 'U', 'r'])
    b = template_predictive(c['lc'], model, rows, t=np.array([0.5, 3., 8.]), filters_to_model=['U', 'r'])
    assert np.array_equal(a.total, b.total[:, [1, 0, 1]][..., [2, 0, 2, 1]]) and a.n_dark.shape == (3, 4)
    assert np.array_equal(a.y_peak_base, b.y_peak_base[[1, 0, 1]])
    assert np.array_equal(a.t_dip, b.t_dip[[1, 0, 1]], equal_nan=True) and set(np.unique(a.i_peak_base)) <= {0, 1, 3}


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_route():
    c = R.grid_case('ShockCooling2', 'sifto')
    P = T.rows(c, False)
    custom, _, _ = device_model('custom')
    with pytest.raises(LcfError, match=r'model\(t, f, \*p\) and model.components\(t, f, \*p\) on a thinned chain') as exc:
        template_predictive(c['lc'], custom, P, **GRID)
    assert exc.value.status == 5
    base = M.ShockCooling2(redshift=T.Z)
    with pytest.raises(LcfError, match='posterior_predictive') as exc:
        template_predictive(c['lc'], base, P[:, :4], **GRID)
    assert exc.value.status == 5
    with pytest.raises(LcfError, match='luminosity_predictive') as exc:
        template_predictive(c['lc'], M.Arnett(), P[:, :3], **GRID)
    assert exc.value.status == 5
    # the C entry points: an engine without a template (a call-sequence error, as for lcf_template_evaluate), a
    # central-engine model, too many searches
    tt, ff = np.tile(R.GRID_T, 6), np.repeat(R.FILTERS, len(R.GRID_T))
    plain = base.make_engine(tt, list(ff), np.zeros(len(tt)), np.ones(len(tt)))
    for call in (lambda: E.predict_template(plain, P, [50.]), lambda: E.template_features(plain, P)):
        with pytest.raises(LcfError, match='lcf_engine_set_template') as exc:
            call()
        assert exc.value.status == 7
    mjd = np.linspace(5., 60., 12)
    with pytest.raises(LcfError, match='compiled per photometric model') as exc:
        E.predict_template(M.Arnett().make_engine(mjd, np.full(12, 1e35), np.full(12, 1e34)), P, [50.])
    assert exc.value.status == 5
    grid_engine, _ = M.Model._eval_engine(grid_model('ShockCooling2', 'sifto'), R.GRID_T, [M.as_filter(f) for f in R.FILTERS], False)
    with pytest.raises(LcfError, match='must not exceed 512, this call has 522') as exc:
        E.predict_template(grid_engine, P, np.linspace(0., 100., 29))
    assert exc.value.status == 5
    with pytest.raises(LcfError, match='ld is smaller') as exc:
        E.predict_template(grid_engine, P[:, :5], [50.])
    assert exc.value.status == 1
    many = template_predictive(c['lc'], grid_model('ShockCooling2', 'sifto'), P, np.linspace(0., 100., 61), features=False, **GRID)
    assert many.total.shape == (61, 6, len(R.GRID_T)) and np.all(np.diff(many.total, axis=0) >= 0.)      # split over calls
