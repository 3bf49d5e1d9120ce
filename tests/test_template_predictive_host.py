"""``template_predictive`` without a device: the NumPy reference's features against a restatement, the argument checks
and refusals that come before an engine is built, the workspace arithmetic, and the C entry points' null checks."""
import os
import re

import numpy as np
import pytest

import template_predictive_reference as R
from lightcurve_fitting_amd import engine as E
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.fitting import TemplatePredictive, template_predictive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lcf_predict_template', 'lcf_template_features')
LC = {'MJD': np.array([0.3, 12.]), 'filter': np.array(['B', 'V'], dtype=object), 'lum': np.ones(2), 'dlum': np.ones(2)}
CUSTOM = '__device__ void lcf_user_state(double, const double*, const double*, double, double& T, double& R) { T = R = 1.; }'
nan = np.nan


def _no_engine(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError('an engine was built')
    monkeypatch.setattr(E, 'Engine', no_engine)


def _model(base=None):
    return M.WithTemplate(base or M.ShockCooling2(redshift=0.01), M.sifto_template(), LC, factors=('V',))


def test_reference_features_against_a_restatement():
    rng = np.random.default_rng(12)
    nf, nt, n = 3, 9, 60
    B = np.round(rng.lognormal(0., 1., (nf, nt, n)), 1)          # (rounded: ties along time and between the two terms)
    Tm = np.round(rng.lognormal(0., 1., (nf, nt, n)), 1)
    for V in (B, Tm):
        V[rng.uniform(size=V.shape) < 0.1] = nan
        V[rng.uniform(size=V.shape) < 0.1] = 0.
        V[rng.uniform(size=V.shape) < 0.05] = -0.
    Tm[rng.uniform(size=Tm.shape) < 0.05] *= -1.                 # a negative template tail
    B[0, :, 0] = nan                                             # no base value anywhere: no peak, no dip
    Tm[0, :, 1] = nan                                            # no template value anywhere
    B[1, :, 2], Tm[1, :, 2] = 0., -0.                            # all ties, +0 against -0: index 0, never a crossing
    B[2, :, 3] = np.arange(nt, 0, -1.)                           # the base peaks first, the template last: the whole grid
    Tm[2, :, 3] = np.arange(nt) * 0.5
    B[2, :, 4], Tm[2, :, 4] = np.arange(nt) + 1., np.arange(nt, 0, -1.) * 0.1   # the template peaks first: no dip
    B[1, :, 5] = [1., 5., 5., 2., nan, 1., 2., 3., 3.]
    Tm[1, :, 5] = [0., 0., 1., 1., 1., nan, 1., 7., 7.]          # NaN sums inside the range, a tie at the dip
    vals, idx = R.features(B, Tm)
    b_vals, b_idx = R.features_brute(B, Tm)
    assert idx.dtype == np.int32 and np.array_equal(idx, b_idx) and np.array_equal(vals, b_vals, equal_nan=True)
    assert list(idx[:, 0, 0]) == [-1, idx[1, 0, 0], idx[2, 0, 0], -1] and np.isnan(vals[0, 0, 0]) and np.isnan(vals[2, 0, 0])
    assert idx[1, 0, 1] == -1 and idx[3, 0, 1] == -1 and idx[2, 0, 1] == -1
    assert list(idx[:, 1, 2]) == [0, 0, -1, -1] and vals[0, 1, 2] == 0. and not np.signbit(vals[0, 1, 2])
    assert np.signbit(vals[1, 1, 2])
    assert list(idx[:, 2, 3]) == [0, nt - 1, 7, nt - 1] and vals[2, 2, 3] == 1. + 4.        # (the sum falls throughout)
    assert list(idx[:, 2, 4]) == [nt - 1, 0, -1, -1]
    assert list(idx[:, 1, 5]) == [1, 7, 7, 3] and vals[2, 1, 5] == 3.      # (sums 5, 6, 3, NaN, NaN, 3, 10: the first 3)
    assert np.array_equal(np.isnan(vals[0]), idx[0] < 0) and np.array_equal(np.isnan(vals[2]), idx[3] < 0)
    assert 0 < np.sum(idx[2] < 0) < nf * n and 0 < np.sum(idx[3] < 0) < nf * n
    # the bands: np.nanpercentile, the valid and the dark counts
    q, n_valid = R.bands(B, (0., 50., 100.))
    assert q.shape == (3, nf, nt) and np.array_equal(n_valid, np.sum(~np.isnan(B), axis=-1))
    assert np.array_equal(q[0], np.nanmin(B, axis=-1)) and np.array_equal(q[2], np.nanmax(B, axis=-1))
    dark = R.n_dark(B)
    assert dark[1, 0] == sum(1 for v in B[1, 0] if v == 0. and not np.signbit(v)) and 0 < dark.sum() < np.sum(B == 0.)


def test_the_dip_of_one_hand_written_sample():
    """Base peak at 1 (the first 5), template peak at 7 (the first 7), the sums between them 5, 6, 3, NaN, NaN, 2, 10."""
    b = [1., 5., 5., 2., nan, 1., 1., 3., 3.]
    tm = [0., 0., 1., 1., 1., nan, 1., 7., 7.]
    vals, idx = R.features_of(b, tm)
    assert idx == (1, 7, 7, 6) and vals == (5., 7., 2.)


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'lcf.h')).read()
    sigs = {name: args for name, _, args in E.SIGNATURES}
    lib = E.load_library()
    for name, n_args in zip(NAMES, (11, 6)):
        assert re.search(r'lcf_status\s+%s\s*\(' % name, header)
        assert len(sigs[name]) == n_args and getattr(lib, name).argtypes == sigs[name]
    assert int(re.search(r'#define LCF_ABI_VERSION (\d+)', header).group(1)) == 8 == E.LCF_ABI_VERSION == lib.lcf_abi_version()
    masks = dict(re.findall(r'LCF_TEMPLATE_MASK_(\w+) = (\d+)', header))
    assert {k.lower(): int(v) for k, v in masks.items()} == E.TEMPLATE_MASK
    # argument errors come before any device call
    assert lib.lcf_predict_template(None, None, 1, 8, 7, None, 1, 1 << 20, None, None, None) == 1
    assert b'null' in lib.lcf_last_error()
    assert lib.lcf_template_features(None, None, 1, 8, None, None) == 1
    assert b'null' in lib.lcf_last_error()
    for text, word in (('INTEGRATION.md', 'lcf_predict_template'), ('DESIGN.md', 'k_tq_pass'),
                       ('README.md', 'template_predictive')):
        assert word in open(os.path.join(ROOT, text)).read()


def test_every_refusal_comes_before_an_engine_is_built(monkeypatch):
    _no_engine(monkeypatch)
    m, P = _model(), np.ones((8, 7))
    assert m.n_model_params == 7
    with pytest.raises(ValueError, match="out of 'total', 'base', 'template', not 'sifto'"):
        template_predictive(LC, m, P, components=('total', 'sifto'))
    with pytest.raises(ValueError, match='non-empty selection of distinct names'):
        template_predictive(LC, m, P, components=())
    with pytest.raises(ValueError, match='distinct names'):
        template_predictive(LC, m, P, components=('base', 'base'))
    with pytest.raises(ValueError, match='must not be empty'):
        template_predictive(LC, m, P, percentiles=())
    with pytest.raises(ValueError, match=r'\[0, 100\]'):
        template_predictive(LC, m, P, percentiles=(50., 101.))
    with pytest.raises(ValueError, match='the samples have 6 columns, the model takes 7'):
        template_predictive(LC, m, np.ones((8, 6)))
    with pytest.raises(ValueError, match='the samples have 7 columns, the model takes 7 and one for sigma'):
        template_predictive(LC, m, P, use_sigma=True)
    with pytest.raises(ValueError, match='discard and thin'):
        template_predictive(LC, m, P, discard=2)
    with pytest.raises(ValueError, match='xscale'):
        template_predictive(LC, m, P, xscale='cubic')
    assert E.TEMPLATE_MAX_FILTERS == 16
    from lightcurve_fitting_amd.filters import filtdict
    many = sorted(set(filtdict.values()))[:17]
    with pytest.raises(ValueError, match='17 distinct filters: template_predictive takes at most 16'):
        template_predictive(LC, m, P, filters_to_model=many)
    assert E.template_components('base') == (('base',), 2)
    assert E.template_components(('template', 'total')) == (('total', 'template'), 5)


def test_other_models_are_refused_with_their_route(monkeypatch):
    _no_engine(monkeypatch)
    with pytest.raises(E.LcfError, match=r'CustomModel.*model\(t, f, \*p\) and model.components\(t, f, \*p\) on a thinned chain') as exc:
        template_predictive(LC, _model(M.CustomModel(CUSTOM, ['a'])), np.ones((4, 4)))
    assert exc.value.status == 5
    with pytest.raises(E.LcfError, match='takes a WithTemplate model.*posterior_predictive gives the bands of a ShockCooling2') as exc:
        template_predictive(LC, M.ShockCooling2(redshift=0.01), np.ones((4, 4)))
    assert exc.value.status == 5
    with pytest.raises(E.LcfError, match='takes a WithTemplate model.*luminosity_predictive') as exc:
        template_predictive(LC, M.Arnett(), np.ones((4, 3)))
    assert exc.value.status == 5
    with pytest.raises(E.LcfError, match='takes a WithTemplate model.*custom_predictive') as exc:
        template_predictive(LC, M.CustomModel(CUSTOM, ['a']), np.ones((4, 1)))
    assert exc.value.status == 5


def test_workspace_arithmetic():
    # three components x six filters, three percentiles: 9 bits for the 18 series' histograms (36 KiB), 7 for the 54
    # searches' (27 KiB)
    n, nt, nf, nc, nq = 2_048_000, 1000, 6, 3, 3
    fixed = 64 * n + 8 * 4 * 18 * nt + (4 * 18 + 8 * 6) * nt + 4096
    per_time = 54 * (56 + 8 * 2048) + 4 * max(18 << 9, 54 << 7)
    assert E.template_workspace(n, nt, nf, nc, nq) == fixed + per_time
    assert E.template_workspace(n, nt, nf, nc, nq, tile=7) == fixed + 7 * per_time
    assert E.template_workspace(n, nt, nf, nc, nq, tile=1000) < 1 << 30      # the headline chain in one tile, by default
    sizes = [E.template_workspace(5000, 40, 6, 3, 5, tile=k) for k in range(1, 42)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))                       # monotone in the tile
    assert E.template_workspace(10, 2, 1, 1, 1) == 640 + 32 + 24 + 4096 + (56 + 16384) + 4 * 2048
    with pytest.raises(ValueError, match='shape'):
        E.predict_template(None, np.ones(5), [50.])


def test_result_object_and_host_side_of_the_features():
    t = np.array([1., 2., 4., 8.])
    res = TemplatePredictive(t, ['f0', 'f1'], np.array([50.]), 3, ('total', 'template'),
                             {'total': np.zeros((1, 2, 4)), 'template': np.ones((1, 2, 4))},
                             {'total': np.full((2, 4), 3), 'template': np.full((2, 4), 3)}, np.zeros((2, 4), dtype=np.int64))
    assert res.base is None and res.total.shape == (1, 2, 4) and np.all(res.template == 1.)
    assert res.i_cross is None and 'features' not in repr(res)
    with pytest.raises(ValueError, match='features=True'):
        res.feature_summary()
    values = np.array([[[3., 2., nan], [1., 1., 1.]], [[5., nan, 4.], [2., 2., 2.]], [[1., nan, nan], [nan, 0.5, nan]]])
    indices = np.array([[[0, 1, -1], [0, 0, 0]], [[3, -1, 2], [1, 2, 3]], [[1, -1, 0], [-1, -1, 1]],
                        [[2, -1, -1], [-1, 1, -1]]], dtype=np.int32)
    res.set_features(values, indices)
    assert np.array_equal(res.t_peak_base, [[1., 2., nan], [1., 1., 1.]], equal_nan=True)
    assert np.array_equal(res.t_cross, [[2., nan, 1.], [nan, nan, 2.]], equal_nan=True)
    assert np.array_equal(res.t_dip, [[4., nan, nan], [nan, 2., nan]], equal_nan=True)
    assert list(res.n_cross_none) == [1, 2] and list(res.n_dip_none) == [2, 2]
    assert np.array_equal(res.y_dip, values[2], equal_nan=True) and np.array_equal(res.i_dip, indices[3])
    s = res.feature_summary((0., 50., 100.))
    assert set(s) == set(res.FEATURE_TIMES + res.FEATURE_VALUES) and s['t_dip'].shape == (3, 2)
    assert np.array_equal(s['t_peak_template'][:, 0], [4., 6., 8.]) and np.array_equal(s['y_dip'][:, 1], [0.5, 0.5, 0.5])
    assert 'with features' in repr(res)
