"""thermal_predictive without a GPU: the two C entry points are declared, bound and exported; argument checks come
before any device use, with posterior_predictive's rules and messages; Blackbody is rejected; the new kernels are in
the compiler's resource report without scratch or spills."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from lightcurve_fitting_amd import engine as E, fitting as F, models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lcf_predict_thermal', 'lcf_sampler_predict_thermal')
LC = {'MJD': [1., 5.], 'filter': ['g', 'r'], 'lum': [1e20, 1e20], 'dlum': [1e18, 1e18]}


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'lcf.h')).read()
    bound = {name: (res, args) for name, res, args in E.SIGNATURES}
    lib = E.load_library()
    for name in NAMES:
        assert re.search(r'lcf_status\s+%s\s*\(' % name, header), name
        assert name in bound and bound[name][0] is ctypes.c_int and len(bound[name][1]) == 12, name
        assert hasattr(lib, name)
    assert re.search(r'#define\s+LCF_ABI_VERSION\s+8\b', header)
    assert lib.lcf_abi_version() == E.LCF_ABI_VERSION == 8             # additive: the ABI version stays
    assert callable(E.predict_thermal) and 3 * (E.PREDICT_MAX_SEARCHES // E.THERMAL_SERIES) <= 512


def test_native_null_arguments_are_refused_before_device_use():
    lib = E.load_library()
    i64 = ctypes.POINTER(ctypes.c_int64)
    q, out, P = np.array([50.]), np.empty(12), np.ones((2, 5))
    nv, nc, ni = (np.empty(12, dtype=np.int64) for _ in range(3))
    pq, po, pp = q.ctypes.data_as(E._dp), out.ctypes.data_as(E._dp), P.ctypes.data_as(E._dp)
    pv, pc, pi = (a.ctypes.data_as(i64) for a in (nv, nc, ni))
    assert lib.lcf_predict_thermal(None, pp, 2, 5, pq, 1, 8.12, 1 << 30, po, pv, pc, pi) == 1
    assert b'null' in lib.lcf_last_error()
    assert lib.lcf_sampler_predict_thermal(None, None, 0, 1, pq, 1, 8.12, 1 << 30, po, pv, pc, pi) == 1
    assert b'null' in lib.lcf_last_error()


def _stub_sampler(steps, nwalkers=8, ndim=5):
    """What thermal_predictive looks at in a sampler before it reaches the device."""
    return types.SimpleNamespace(iteration=steps, nwalkers=nwalkers, ndim=ndim, _native=None, get_chain=None)


def test_argument_checks_raise_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(M.Model, '_eval_engine', no_device)
    monkeypatch.setattr(E, 'predict_thermal', no_device)
    m, P = M.ShockCooling(), np.ones((3, 5))
    for bad in ((), (-1., 50.), (50., 100.5), (np.nan,)):
        with pytest.raises(ValueError, match='percentiles'):
            F.thermal_predictive(LC, m, P, percentiles=bad)
    with pytest.raises(ValueError, match='columns'):
        F.thermal_predictive(LC, m, np.ones((3, 4)))
    with pytest.raises(ValueError, match='columns'):
        F.thermal_predictive(LC, m, P, use_sigma=True)            # five columns, six wanted
    with pytest.raises(ValueError, match='columns'):
        F.thermal_predictive(LC, m, np.ones((3, 6)))
    for kw in (dict(discard=1), dict(thin=2)):
        with pytest.raises(ValueError, match='discard and thin'):
            F.thermal_predictive(LC, m, P, **kw)
    with pytest.raises(ValueError, match='no samples'):
        F.thermal_predictive(LC, m, np.empty((0, 5)))
    with pytest.raises(ValueError, match='shape'):
        F.thermal_predictive(LC, m, np.ones(5))
    with pytest.raises(ValueError, match='xscale'):
        F.thermal_predictive(LC, m, P, xscale='symlog')
    with pytest.raises(ValueError, match='finite'):
        F.thermal_predictive(LC, m, P, t=[1., np.inf])
    # a sampler: the rules of posterior_predictive
    with pytest.raises(ValueError, match='thin'):
        F.thermal_predictive(LC, m, _stub_sampler(10), thin=0)
    with pytest.raises(ValueError, match='discard'):
        F.thermal_predictive(LC, m, _stub_sampler(10), discard=-1)
    with pytest.raises(ValueError, match='leaves no steps'):
        F.thermal_predictive(LC, m, _stub_sampler(10), discard=10)
    with pytest.raises(ValueError, match='no chain'):
        F.thermal_predictive(LC, m, _stub_sampler(0))
    with pytest.raises(ValueError, match='columns'):
        F.thermal_predictive(LC, m, _stub_sampler(10, ndim=6))
    # everything in order: the next thing is the device
    with pytest.raises(AssertionError, match='device was reached'):
        F.thermal_predictive(LC, m, P)


def test_same_messages_as_posterior_predictive(monkeypatch):
    """One set of checks serves both functions: a bad call fails with the same words in either."""
    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(M.Model, '_eval_engine', no_device)
    m = M.ShockCooling()
    for samples, kw in ((np.ones((3, 5)), dict(percentiles=(101.,))), (np.ones((3, 4)), {}), (np.ones(5), {}),
                        (np.ones((3, 5)), dict(thin=2)), (_stub_sampler(10), dict(discard=10)),
                        (_stub_sampler(0), {}), (np.ones((3, 5)), dict(use_sigma=True))):
        with pytest.raises(ValueError) as a:
            F.posterior_predictive(LC, m, samples, **kw)
        with pytest.raises(ValueError) as b:
            F.thermal_predictive(LC, m, samples, **kw)
        assert str(a.value) == str(b.value)


def test_blackbody_is_rejected(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(M.Model, '_eval_engine', no_device)
    monkeypatch.setattr(M.Blackbody, '_eval_engine', no_device)
    with pytest.raises(ValueError, match='Blackbody'):
        F.thermal_predictive(LC, M.Blackbody(), np.ones((3, 2)))


def test_result_fractions():
    r = F.ThermalPredictive(np.arange(3.), np.array([50.]), *(np.zeros((1, 3)),) * 3,
                            n_valid=np.array([[4, 2, 0]] * 3), n_cold=np.array([1, 2, 0]),
                            n_inside=np.array([0, 2, 4]), n_samples=4)
    assert np.array_equal(r.frac_cold, [0.25, 1., np.nan], equal_nan=True)
    assert np.array_equal(r.frac_inside, [0., 0.5, 1.])


def test_resource_report_lists_thermal_kernels_without_scratch():
    path = os.path.join(os.path.dirname(E.__file__), 'csrc', 'liblcf_hip.resources.txt')
    if not os.path.exists(path):
        pytest.skip('no resource report next to the library (built without the Makefile)')
    text = open(path).read()
    blocks = {}
    for m in re.finditer(r'Function Name: (\S+)(.*?)(?=Function Name:|\Z)', text, re.S):
        blocks[m.group(1)] = dict(re.findall(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)', m.group(2)))
    for name, count in (('k_th_sample', 1), ('k_th_pass', 2)):
        found = [k for k in blocks if name in k]
        assert len(found) == count, (name, sorted(blocks)[:5])
        for k in found:
            f = blocks[k]
            assert int(f['ScratchSize']) == 0 and int(f['VGPRs Spill']) == 0, (k, f)
            assert int(f['Occupancy']) >= 4, (k, f)
