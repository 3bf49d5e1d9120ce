"""``luminosity_predictive`` without a GPU: the entry point is declared, bound and exported; what it refuses it
refuses before any engine is built; and the peak rule the device kernel ``k_lq_peak`` is held to, restated in NumPy
(``peak_rule``, which ``tests/test_gpu_luminosity.py`` imports) and checked on hand-made arrays."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from lightcurve_fitting_amd import engine as E
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.fitting import LuminosityPredictive, luminosity_predictive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LC = {'MJD': np.linspace(0., 90., 40), 'L_bol': np.ones(40), 'dL_bol': np.ones(40)}


def peak_rule(L, times, t_0, z):
    """Per row of ``L`` (n, nt) on ascending distinct ``times``: ``(index, L_peak, t_peak, t_rise)`` -- the index of
    the FIRST time at which the row's largest non-NaN value is attained, -1 and NaNs for a row that is NaN everywhere."""
    L, times = np.asarray(L, dtype=np.float64), np.asarray(times, dtype=np.float64)
    none = np.all(np.isnan(L), axis=1)
    index = np.where(none, -1, np.argmax(np.where(np.isnan(L), -np.inf, L), axis=1)).astype(np.int32)
    at = np.maximum(index, 0)
    L_peak = np.where(none, np.nan, L[np.arange(len(L)), at])
    t_peak = np.where(none, np.nan, times[at])
    return index, L_peak, t_peak, (t_peak - np.asarray(t_0, dtype=np.float64)) / (1. + z)


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'lcf.h')).read()
    assert re.search(r'lcf_status\s+lcf_predict_luminosity\s*\(', header)
    assert int(re.search(r'#define LCF_ABI_VERSION (\d+)', header).group(1)) == 8 == E.LCF_ABI_VERSION
    sig = {name: (res, args) for name, res, args in E.SIGNATURES}['lcf_predict_luminosity']
    assert sig[0] is ctypes.c_int and len(sig[1]) == 12
    lib = E.load_library()
    assert lib.lcf_predict_luminosity.argtypes == sig[1] and lib.lcf_abi_version() == 8
    # argument errors come before any device call
    assert lib.lcf_predict_luminosity(None, None, 1, 3, None, 1, 1 << 20, None, None, None, None, None) == 1
    assert b'null' in lib.lcf_last_error()


def test_other_models_are_refused_before_any_engine_is_built(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError('an engine was built')
    monkeypatch.setattr(E, 'Engine', no_engine)
    with pytest.raises(E.LcfError, match='posterior_predictive') as exc:
        luminosity_predictive(LC, M.ShockCooling(), np.ones((8, 5)))
    assert exc.value.status == 5


def test_argument_checks_need_no_device(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError('an engine was built')
    monkeypatch.setattr(E, 'Engine', no_engine)
    m = M.Arnett()
    good = np.tile([0.07, 12., -5.], (8, 1))
    with pytest.raises(ValueError, match='columns'):
        luminosity_predictive(LC, m, np.ones((8, 4)))
    with pytest.raises(ValueError, match='columns'):
        luminosity_predictive(LC, m, good, use_sigma=True)
    with pytest.raises(ValueError, match='columns'):
        luminosity_predictive(LC, M.Magnetar(gamma_leakage=True), np.ones((8, 4)))
    with pytest.raises(ValueError, match='empty'):
        luminosity_predictive(LC, m, good, percentiles=())
    for bad in ((-1., 50.), (50., 100.5), (np.nan,)):
        with pytest.raises(ValueError, match=r'\[0, 100\]'):
            luminosity_predictive(LC, m, good, percentiles=bad)
    with pytest.raises(ValueError, match='discard and thin'):
        luminosity_predictive(LC, m, good, discard=2)
    with pytest.raises(ValueError, match='discard and thin'):
        luminosity_predictive(LC, m, good, thin=3)
    with pytest.raises(ValueError, match='no samples'):
        luminosity_predictive(LC, m, np.ones((0, 3)))


def test_result_object():
    res = LuminosityPredictive(np.arange(3.), np.array([50.]), np.ones((1, 3)), np.array([4, 4, 0]), np.array([4, 1, 0]), 5)
    assert 'LuminosityPredictive' in repr(res) and res.peak_index is None and res.L_peak is None
    assert np.array_equal(res.frac_dark, [1., 0.25, np.nan], equal_nan=True)
    with pytest.raises(ValueError, match='peak=True'):
        res.peak_summary()
    with pytest.raises(AttributeError):
        res.other = 1                                     # __slots__
    res.L_peak, res.t_peak, res.t_rise = np.array([1., 3., np.nan]), np.array([5., 7., np.nan]), np.array([2., 4., np.nan])
    res.peak_index = np.array([0, 1, -1], dtype=np.int32)
    s = res.peak_summary()
    assert s['L_peak'].shape == (1,) and s['L_peak'][0] == 2. and s['t_peak'][0] == 6. and s['t_rise'][0] == 3.
    assert np.array_equal(res.peak_summary((0., 100.))['L_peak'], [1., 3.])


def test_peak_rule_on_hand_made_arrays():
    nan = np.nan
    times = np.array([1., 2., 4., 8.])
    L = np.array([[0., 3., 3., 1.],          # a tie: the first occurrence
                  [nan, 2., nan, 5.],        # NaNs are ignored
                  [nan, nan, nan, nan],      # NaN everywhere
                  [0., 0., 0., 0.],          # not exploded on the whole grid
                  [7., nan, 7., 7.],         # a tie across a NaN
                  [-0., 0., -0., 0.],        # the zeros are equal: the first of them
                  [1., 2., 3., 4.]])         # rising to the edge
    t_0 = np.array([0., 1., 0., 9., -1., 0., 0.5])
    index, L_peak, t_peak, t_rise = peak_rule(L, times, t_0, 1.)
    assert index.dtype == np.int32 and np.array_equal(index, [1, 3, -1, 0, 0, 0, 3])
    assert np.array_equal(L_peak, [3., 5., nan, 0., 7., 0., 4.], equal_nan=True)
    assert np.array_equal(t_peak, [2., 8., nan, 1., 1., 1., 8.], equal_nan=True)
    assert np.array_equal(t_rise, [1., 3.5, nan, -4., 1., 0.5, 3.75], equal_nan=True)
    # ... and it is np.nanargmax / np.nanmax where those are defined
    ok = index >= 0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        assert np.array_equal(index[ok], np.nanargmax(L[ok], axis=1))
        assert np.array_equal(L_peak, np.nanmax(L, axis=1), equal_nan=True)
