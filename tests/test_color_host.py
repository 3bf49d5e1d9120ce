"""``color_predictive`` without a GPU: the NumPy definition the device is held to (``tests/color_reference.py``) against
a brute-force loop; how colours are parsed and what is refused, all before an engine is built; the workspace
arithmetic; and what the result object derives on the host from the two arrays the device returns."""
import math
import os
import re

import numpy as np
import pytest

import color_reference as R
from lightcurve_fitting_amd import engine as E
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.filters import Filter, filtdict
from lightcurve_fitting_amd.fitting import ColorPredictive, color_predictive, parse_colors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lcf_predict_colors', 'lcf_sampler_predict_colors')
LC = {'MJD': np.array([0.3, 12.]), 'filter': np.array(['B', 'V'], dtype=object), 'lum': np.ones(2), 'dlum': np.ones(2)}
nan = np.nan


def _no_engine(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError('an engine was built')
    monkeypatch.setattr(E, 'Engine', no_engine)


def _brute(Y, pairs, dzp, q):
    """The definition, one number at a time."""
    nf, nt, n = Y.shape
    color = np.full((len(q), len(pairs), nt), nan)
    n_valid = np.zeros((len(pairs), nt), dtype=np.int64)
    for c, (a, b) in enumerate(pairs):
        for t in range(nt):
            vals = []
            for s in range(n):
                ya, yb = Y[a, t, s], Y[b, t, s]
                if math.isfinite(ya) and math.isfinite(yb) and ya > 0. and yb > 0.:
                    vals.append(dzp[c] - 2.5 * np.log10(ya / yb))
            n_valid[c, t] = len(vals)
            vals.sort()
            for j, qq in enumerate(q):
                if not vals:
                    continue
                h = (len(vals) - 1) * (qq / 100.)
                lo = int(math.floor(h))
                g, x, y = h - lo, vals[lo], vals[min(lo + 1, len(vals) - 1)]
                color[j, c, t] = x if g == 0. else (y - (y - x) * (1. - g) if g >= 0.5 else x + (y - x) * g)
    y_peak, index = np.full((n, nf), nan), np.full((n, nf), -1, dtype=np.int32)
    for s in range(n):
        for f in range(nf):
            for t in range(nt):
                v = Y[f, t, s]
                if v == v and (index[s, f] < 0 or v > y_peak[s, f]):
                    y_peak[s, f], index[s, f] = v, t
    return color, n_valid, y_peak, index


def test_reference_helper_against_a_brute_force_loop():
    rng = np.random.default_rng(5)
    Y = rng.lognormal(0., 1., (4, 7, 33))
    Y[rng.uniform(size=Y.shape) < 0.1] = nan
    Y[rng.uniform(size=Y.shape) < 0.1] = 0.
    Y[rng.uniform(size=Y.shape) < 0.05] = -1.5
    Y[1, :, :5] = Y[1, 2:3, :5]                 # exact ties along time: the first occurrence
    Y[2, :, 7] = nan                            # a sample that is NaN everywhere in a filter
    Y[3, 4, :] = nan                            # a time at which no sample has the colours of filter 3
    Y[0, :, 9] = 0.                             # not exploded on the whole grid
    Y[:, :, 11] = Y[:, :, 10]                   # two samples with identical colours
    pairs, dzp = [(0, 1), (1, 2), (3, 0), (1, 0)], np.array([0.25, -0.5, 0., -0.25])
    q = (0., 2.5, 15.87, 50., 84.14, 100.)
    color, n_valid = R.color_bands(Y, pairs, dzp, q)
    y_peak, index = R.peaks(Y)
    b_color, b_valid, b_peak, b_index = _brute(Y, pairs, dzp, q)
    assert np.array_equal(n_valid, b_valid) and np.all(n_valid[2, 4] == 0) and n_valid.max() < 33
    assert np.array_equal(np.isnan(color), np.isnan(b_color)) and np.all(np.isnan(color[:, 2, 4]))
    assert np.nanmax(np.abs(color - b_color)) <= 4e-16 * np.nanmax(np.abs(b_color))
    assert np.array_equal(index, b_index) and np.array_equal(y_peak, b_peak, equal_nan=True)
    assert index.dtype == np.int32 and index[7, 2] == -1 and np.isnan(y_peak[7, 2])
    assert index[9, 0] == 0 and y_peak[9, 0] == 0.
    assert np.all(index[:5, 1] == 0)
    # a colour and its reverse are mirror images (percentiles 0, 50, 100 against 100, 50, 0)
    assert np.allclose(color[[0, 3, 5], 0], -color[[5, 3, 0], 3], rtol=0., atol=1e-14, equal_nan=True)


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'lcf.h')).read()
    sigs = {name: args for name, _, args in E.SIGNATURES}
    lib = E.load_library()
    for name in NAMES:
        assert re.search(r'lcf_status\s+%s\s*\(' % name, header)
        assert len(sigs[name]) == 14 and getattr(lib, name).argtypes == sigs[name]
    assert int(re.search(r'#define LCF_ABI_VERSION (\d+)', header).group(1)) == 8 == E.LCF_ABI_VERSION == lib.lcf_abi_version()
    # argument errors come before any device call
    assert lib.lcf_predict_colors(None, None, 1, 5, 1, None, None, None, 1, 1 << 20, None, None, None, None) == 1
    assert b'null' in lib.lcf_last_error()
    for text, word in (('INTEGRATION.md', 'lcf_predict_colors'), ('DESIGN.md', 'k_cq_pass'), ('README.md', 'color_predictive')):
        assert word in open(os.path.join(ROOT, text)).read()


def test_colors_are_parsed_as_calc_colors_does():
    pairs, names, filters, index, dzp = parse_colors(('B-V', 'g-r', 'r-i'))
    f = filtdict
    assert pairs == [(f['B'], f['V']), (f['g'], f['r']), (f['r'], f['i'])] and names == ['B-V', 'g-r', 'r-i']
    assert filters == sorted({f[c] for c in 'BVgri'}) and len(filters) == 5
    assert index.dtype == np.int32 and index.shape == (3, 2)
    assert [(filters[a], filters[b]) for a, b in index] == pairs
    assert np.array_equal(dzp, [f['B'].m0 - f['V'].m0, f['g'].m0 - f['r'].m0, f['r'].m0 - f['i'].m0])
    # a pair of names, a pair of Filter objects, an alias; one filter shared by three colours
    pairs, names, filters, index, dzp = parse_colors([('B', 'V'), (f['V'], f['r']), 'V-i', 'U-B'])
    assert pairs == [(f['B'], f['V']), (f['V'], f['r']), (f['V'], f['i']), (f['U'], f['B'])]
    assert names == ['B-V', 'V-r', 'V-i', 'U-B'] and len(filters) == 5
    v = filters.index(f['V'])
    assert np.sum(index == v) == 3 and [int(k) for k in index[:, 0]] == [filters.index(a) for a, _ in pairs]
    assert dzp[1] == f['V'].m0 - f['r'].m0 and dzp[3] == f['U'].m0 - f['B'].m0
    assert parse_colors('B-V')[1] == ['B-V']
    # split at the FIRST '-': what follows it is one name
    with pytest.raises(ValueError, match="unrecognised filter 'V-r'"):
        parse_colors(['B-V-r'])


def test_every_refusal_comes_before_an_engine_is_built(monkeypatch):
    _no_engine(monkeypatch)
    m, P = M.ShockCooling(redshift=0.01), np.ones((8, 5))
    with pytest.raises(ValueError, match='unrecognised filter'):
        color_predictive(LC, m, P, colors=['B-nosuchfilter'])
    with pytest.raises(ValueError, match='unrecognised filter'):
        color_predictive(LC, m, P, colors=[('nosuchfilter', 'V')])
    with pytest.raises(ValueError, match='no zero point'):
        color_predictive(LC, m, P, colors=[(Filter('nozp', fnu=None), 'V')])
    with pytest.raises(ValueError, match='with itself'):
        color_predictive(LC, m, P, colors=['B-V', 'V-V'])
    with pytest.raises(ValueError, match='with itself'):
        color_predictive(LC, m, P, colors=[(filtdict['g'], 'g')])
    with pytest.raises(ValueError, match='must not be empty'):
        color_predictive(LC, m, P, colors=[])
    with pytest.raises(ValueError, match="form 'X-Y'"):
        color_predictive(LC, m, P, colors=['BV'])
    with pytest.raises(ValueError, match='pair'):
        color_predictive(LC, m, P, colors=[('B', 'V', 'r')])
    many = sorted({f for f in filtdict.values() if np.isfinite(f.m0)})[:18]
    assert len(many) == 18 and E.COLOR_MAX_FILTERS == 16
    with pytest.raises(ValueError, match='17 distinct filters: at most 16'):
        color_predictive(LC, m, P, colors=[(many[0], x) for x in many[1:17]])
    parse_colors([(many[0], x) for x in many[1:16]])            # 16 distinct filters are taken
    with pytest.raises(ValueError, match='columns'):
        color_predictive(LC, m, np.ones((8, 4)))
    with pytest.raises(ValueError, match='columns'):
        color_predictive(LC, m, P, use_sigma=True)
    with pytest.raises(ValueError, match='empty'):
        color_predictive(LC, m, P, percentiles=())
    with pytest.raises(ValueError, match=r'\[0, 100\]'):
        color_predictive(LC, m, P, percentiles=(50., 101.))
    with pytest.raises(ValueError, match='discard and thin'):
        color_predictive(LC, m, P, discard=2)
    with pytest.raises(ValueError, match='xscale'):
        color_predictive(LC, m, P, xscale='cubic')


def test_custom_and_central_engine_models_are_refused(monkeypatch):
    _no_engine(monkeypatch)
    src = '__device__ void lcf_user_state(double, const double*, const double*, double, double& T, double& R) { T = R = 1.; }'
    with pytest.raises(E.LcfError, match='color_predictive is compiled per built-in model.*custom_predictive') as exc:
        color_predictive(LC, M.CustomModel(src, ['a']), np.ones((4, 1)))
    assert exc.value.status == 5
    with pytest.raises(E.LcfError, match='color_predictive is compiled per photometric model.*luminosity_predictive') as exc:
        color_predictive(LC, M.Arnett(), np.ones((4, 3)))
    assert exc.value.status == 5


def test_workspace_arithmetic():
    # five colours, three percentiles: 11 bits for the 5 point histograms (40 KiB), 9 for the 15 searches' (30 KiB)
    n, nt, nc, nq = 2_048_000, 1000, 5, 3
    fixed = 64 * n + 8 * 4 * nc * nt + 4 * nc * nt + 16 * nc + 4096
    per_time = 15 * (56 + 8 * 2048) + 4 * max(5 << 11, 15 << 9)
    assert E.color_workspace(n, nt, nc, nq) == fixed + per_time
    assert E.color_workspace(n, nt, nc, nq, tile=7) == fixed + 7 * per_time
    assert E.color_workspace(n, nt, nc, nq, tile=1000) < 1 << 30        # the headline chain in one tile, by default
    # 512 searches: four bits each (32 KiB); one colour alone: eleven
    assert E.color_workspace(1, 1, 64, 8) == 64 + 8 * 9 * 64 + 4 * 64 + 16 * 64 + 4096 + 512 * (56 + 16384) + 4 * (512 << 4)
    assert E.color_workspace(10, 2, 1, 1) == 640 + 32 + 8 + 16 + 4096 + (56 + 16384) + 4 * 2048
    # the peaks are results per sample, outside the workspace
    assert E.color_peak_bytes(n, 6) == 12 * 6 * n
    with pytest.raises(ValueError, match='shape'):
        E.predict_colors(None, np.ones((2, 5)), [[0, 1, 2]], [0.], [50.])


def _result(nt=4):
    f = filtdict
    return ColorPredictive(np.array([1., 2., 4., 8.])[:nt], [(f['B'], f['V'])], ['B-V'], [f['B'], f['V']],
                           np.array([50.]), np.zeros((1, 1, nt)), np.full((1, nt), 6), 6)


def test_result_object_and_host_side_of_the_peaks():
    res = _result()
    assert 'ColorPredictive' in repr(res) and 'peaks' not in repr(res) and res.peak_index is None and res.M_peak is None
    with pytest.raises(ValueError, match='peak=True'):
        res.peak_summary()
    with pytest.raises(AttributeError):
        res.other = 1                                     # __slots__
    y_peak = np.array([[100., 1.], [0., 10.], [nan, 1e4], [1., 0.], [1e-2, nan], [1e4, 100.]])
    index = np.array([[0, 3], [0, 1], [-1, 3], [2, 0], [3, -1], [1, 2]], dtype=np.int32)
    res.set_peaks(y_peak, index, [10., 20.])
    assert 'with peaks in 2 filters' in repr(res)
    assert res.peak_index.dtype == np.int32 and res.y_peak is not None
    assert np.array_equal(res.t_peak, [[1., 8.], [1., 2.], [nan, 8.], [4., 1.], [8., nan], [2., 4.]], equal_nan=True)
    assert np.array_equal(res.M_peak, [[5., 20.], [nan, 17.5], [nan, 10.], [10., nan], [15., nan], [0., 15.]], equal_nan=True)
    assert np.array_equal(res.n_peak_first, [2, 1]) and np.array_equal(res.n_peak_last, [1, 2])
    s = res.peak_summary()
    assert s['M_peak'].shape == s['t_peak'].shape == (3, 2)
    s = res.peak_summary((0., 50., 100.))
    assert np.array_equal(s['M_peak'], [[0., 10.], [7.5, 16.25], [15., 20.]])
    assert np.array_equal(s['t_peak'], [[1., 1.], [2., 4.], [8., 8.]])
    # zero points: M0 for a 'lum' model, m0 for a 'flux' one, 90.19 apart
    assert M.ShockCooling().output_quantity == 'lum' and M.ShockCooling3().output_quantity == 'flux'
    assert filtdict['B'].M0 - filtdict['B'].m0 == pytest.approx(90.19)
    # every sample NaN in a filter: the summary is NaN, without a warning escaping
    res.set_peaks(np.full((3, 2), nan), np.full((3, 2), -1, dtype=np.int32), [0., 0.])
    assert np.all(np.isnan(res.peak_summary()['M_peak'])) and np.array_equal(res.n_peak_first, [0, 0])
