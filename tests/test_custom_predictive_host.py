"""``custom_predictive`` without a GPU: the entry point is declared, bound and exported; the program a custom model's
source is compiled into holds both kernels; the offline build's resource report of the key kernel; the workspace
formula; and what the function refuses before any engine is built."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_custom_host import ARCH, SC2_CONSTS, SC2_NAMES, SC2_SOURCE, SC2_UNITS
from lightcurve_fitting_amd import engine as E
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.fitting import CustomPredictive, custom_predictive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LC = {'MJD': np.linspace(0.5, 9., 12), 'filter': ['g', 'r'] * 6, 'lum': np.ones(12), 'dlum': np.ones(12)}


def sc2_model():
    return M.CustomModel(SC2_SOURCE, SC2_NAMES, SC2_UNITS, consts=SC2_CONSTS)


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'lcf.h')).read()
    assert re.search(r'lcf_status\s+lcf_predict_custom\s*\(', header)
    assert int(re.search(r'#define LCF_ABI_VERSION (\d+)', header).group(1)) == 8 == E.LCF_ABI_VERSION
    sig = {name: (res, args) for name, res, args in E.SIGNATURES}['lcf_predict_custom']
    # grid, P, n, ld, q, n_q, T_floor, workspace_bytes, out, n_valid, n_dark, n_cold
    i64p = ctypes.POINTER(ctypes.c_int64)
    dp = ctypes.POINTER(ctypes.c_double)
    assert sig == (ctypes.c_int, [ctypes.c_void_p, dp, ctypes.c_int64, ctypes.c_int32, dp, ctypes.c_int32, ctypes.c_double,
                                  ctypes.c_int64, dp, i64p, i64p, i64p])
    declared = re.search(r'lcf_status\s+lcf_predict_custom\s*\((.*?)\);', header, re.S).group(1)
    declared = re.sub(r'/\*.*?\*/', '', declared, flags=re.S)
    assert len(declared.split(',')) == len(sig[1])
    lib = E.load_library()
    assert lib.lcf_predict_custom.argtypes == sig[1] and lib.lcf_abi_version() == 8
    # argument errors come before any device call
    assert lib.lcf_predict_custom(None, None, 1, 3, None, 1, -1., 1 << 20, None, None, None, None) == 1
    assert b'null' in lib.lcf_last_error()


def test_both_kernels_are_in_the_code_object():
    code = E.CustomProgram(SC2_SOURCE, ARCH).code
    assert b'lcf_custom_points' in code and b'lcf_custom_keys' in code


def test_the_key_kernel_in_the_resource_report():
    """The sample state function (ShockCooling2 restated) of the offline build: 78 vector registers, 6 waves per SIMD,
    no scratch.  A user's own function has its own figures; only the absence of scratch and spills is asserted."""
    path = os.path.join(os.path.dirname(E.__file__), 'csrc', 'liblcf_hip.resources.txt')
    if not os.path.exists(path):
        pytest.skip('no resource report next to the library (built without the Makefile)')
    text = open(path).read()
    blocks = [m.group(1) for m in re.finditer(r'Function Name: lcf_custom_keys\b(.*?)(?=Function Name:|\Z)', text, re.S)]
    assert len(blocks) == 1
    f = dict(re.findall(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)', blocks[0]))
    print(f'lcf_custom_keys behind the sample: {f["VGPRs"]} VGPRs, occupancy {f["Occupancy"]} waves/SIMD')
    assert int(f['ScratchSize']) == 0 and int(f['VGPRs Spill']) == 0, f


def test_custom_workspace_is_the_documented_formula():
    # 1000 samples, 7 times, 3 filters (6 series), 3 percentiles: b = 11 (3 * 2048 counters fit 48 KiB)
    fixed = 8 * 4 * 6 * 7 + 20 * 6 * 7 + 4096
    per_time = 6 * (8 * 1000 + 3 * (56 + 8 * 2048) + 4 * max(2048, 3 * 2048))
    assert fixed == 6280 and per_time == 491376
    assert E.custom_workspace(1000, 7, 3, 3) == fixed + per_time == 497656
    assert E.custom_workspace(1000, 7, 3, 3, tile=4) == fixed + 4 * per_time
    # 5 samples, 2 times, 1 filter (4 series), 512 percentiles: b = 4 (512 * 32 counters are beyond 48 KiB)
    fixed = 8 * 513 * 4 * 2 + 20 * 4 * 2 + 4096
    per_time = 4 * (8 * 5 + 512 * (56 + 8 * 2048) + 4 * 512 * 16)
    assert E.custom_workspace(5, 2, 1, 512) == fixed + per_time == 37088 + 33800352
    sizes = [E.custom_workspace(4099, 7, 3, 7, tile=k) for k in range(1, 8)]
    assert np.all(np.diff(sizes) > 0) and len(set(np.diff(sizes))) == 1


def test_argument_checks_need_no_device(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError('an engine was built')
    monkeypatch.setattr(E, 'Engine', no_engine)
    for other, cols in ((M.ShockCooling(), 5), (M.Arnett(), 3)):
        with pytest.raises(E.LcfError, match='posterior_predictive.*thermal_predictive.*luminosity_predictive') as exc:
            custom_predictive(LC, other, np.ones((8, cols)))
        assert exc.value.status == 5
    m = sc2_model()
    good = np.tile([20., 2., 10., 0.1], (8, 1))
    with pytest.raises(ValueError, match='empty'):
        custom_predictive(LC, m, good, percentiles=())
    for bad in ((-1., 50.), (50., 100.5), (np.nan,)):
        with pytest.raises(ValueError, match=r'\[0, 100\]'):
            custom_predictive(LC, m, good, percentiles=bad)
    with pytest.raises(ValueError, match='columns'):
        custom_predictive(LC, m, np.ones((8, 5)))
    with pytest.raises(ValueError, match='columns'):
        custom_predictive(LC, m, good, use_sigma=True)
    with pytest.raises(ValueError, match='columns'):
        custom_predictive(LC, m, np.ones((8, 6)), use_sigma=True)
    with pytest.raises(ValueError, match='discard and thin'):
        custom_predictive(LC, m, good, discard=2)
    with pytest.raises(ValueError, match='discard and thin'):
        custom_predictive(LC, m, good, thin=3)
    with pytest.raises(ValueError, match='no samples'):
        custom_predictive(LC, m, np.ones((0, 4)))

    class Source:                                        # anything with get_chain, as a TemperedSampler has it
        def get_chain(self, discard=0, thin=1, flat=False):
            return np.tile(good, (5, 1))[discard * 8::thin]
    with pytest.raises(ValueError, match='thin >= 1'):
        custom_predictive(LC, m, Source(), thin=0)
    with pytest.raises(ValueError, match='discard >= 0'):
        custom_predictive(LC, m, Source(), discard=-1)
    with pytest.raises(ValueError, match='leaves no steps'):
        custom_predictive(LC, m, Source(), discard=5)


def test_result_object():
    nan = np.nan
    res = CustomPredictive(np.arange(3.), ['g', 'r'], np.array([50.]), 5, np.ones((1, 2, 3)), np.full((2, 3), 4),
                           np.zeros((2, 3), dtype=int), np.ones((1, 3)), np.ones((1, 3)), np.ones((1, 3)),
                           np.array([[4, 4, 0]] * 3))
    assert 'CustomPredictive' in repr(res) and '2 filters' in repr(res) and res.n_cold is None and res.frac_cold is None
    with pytest.raises(AttributeError):
        res.other = 1                                     # __slots__
    res.n_cold = np.array([4, 1, 0])
    assert np.array_equal(res.frac_cold, [1., 0.25, nan], equal_nan=True)
