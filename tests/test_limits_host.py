"""Censored non-detections, the parts that need no GPU: the C ABI's two additions and their binding, the row split of
``nondet='censored'``, the errors raised before any engine exists, and the reference's own ``ln Phi``."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.special import log_ndtr

import limits_reference as L
from conftest import ROOT, relerr
from lightcurve_fitting_amd import engine as E
from lightcurve_fitting_amd import fitting as F
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.lightcurve import LC

_dp = ctypes.POINTER(ctypes.c_double)


def test_header_declares_the_two_functions_and_the_version_stays():
    text = open(os.path.join(ROOT, 'include', 'lcf.h')).read()
    assert re.search(r'#define\s+LCF_ABI_VERSION\s+8\b', text) and E.LCF_ABI_VERSION == 8
    assert re.search(r'lcf_status\s+lcf_engine_set_limits\(lcf_engine\*\s*e,\s*lcf_engine\*\s*at,\s*int64_t\s+n_lim,\s*'
                     r'const\s+double\*\s*L_lim,\s*const\s+double\*\s*dy\);', text)
    assert re.search(r'lcf_status\s+lcf_limit_terms\(lcf_engine\*\s*e,\s*int64_t\s+n,\s*const\s+double\*\s*P,\s*'
                     r'double\*\s*out\);', text)


def test_engine_binds_them_with_the_right_argument_types():
    sig = {name: (res, args) for name, res, args in E.SIGNATURES}
    assert sig['lcf_engine_set_limits'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _dp, _dp])
    assert sig['lcf_limit_terms'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, _dp, _dp])


def test_null_arguments_are_invalid():
    lib = E.load_library()
    assert lib.lcf_abi_version() == 8
    x = np.zeros(3)
    assert lib.lcf_engine_set_limits(None, None, 3, E._ptr(x), E._ptr(x)) == 1
    assert lib.lcf_engine_set_limits(None, None, 0, None, None) == 1
    assert lib.lcf_limit_terms(None, 1, E._ptr(x), E._ptr(x)) == 1
    assert b'null' in lib.lcf_last_error()


def test_the_row_split():
    c = L.case('ShockCooling2', 13)
    s = M.LimitSplit(c['lc'], 'lum')
    assert np.array_equal(s.lim, c['nondet']) and np.array_equal(s.det, ~c['nondet'])
    assert s.lim.sum() == 13 and s.det.sum() == 60 and 0 < np.nonzero(s.lim)[0].min() < 60      # among the detections
    assert s.nondet_sigmas == 3. and np.array_equal(s.dy, c['dy'][c['nondet']])
    assert np.array_equal(s.L_lim, 3. * c['dy'][c['nondet']])
    assert s.sigma_unit_abs == np.median(c['dy'][~c['nondet']]) != np.median(c['dy'])
    # an LC carries its own nondetSigmas; the column may be anything that reads as booleans
    lc = LC({'MJD': c['t'], 'filter': c['lc']['filter'], 'lum': c['y'], 'dlum': c['dy'],
             'nondet': c['nondet'].astype(int)})
    lc.nondetSigmas = 5.
    s5 = M.LimitSplit(lc, 'lum')
    assert np.array_equal(s5.lim, c['nondet']) and np.array_equal(s5.L_lim, 5. * c['dy'][c['nondet']])
    # no column, or no true row: nothing to split
    assert M._nondet_mask(L.without_limits(c)) is None
    assert M._nondet_mask(dict(c['lc'], nondet=np.zeros(73, dtype=bool))) is None


def test_errors_raised_before_any_engine():
    c = L.case('ShockCooling2', 13)
    m = M.ShockCooling2(redshift=L.Z)
    p = c['truth']
    for call in (lambda: m.log_likelihood(c['lc'], p, nondet='upper'),
                 lambda: m.engine_for(c['lc'], nondet='Censored'),
                 lambda: F.make_log_posterior(c['lc'], m, nondet=None),
                 lambda: M.Arnett().engine_for({'MJD': c['t'], 'L_bol': c['y'], 'dL_bol': c['dy']}, nondet='tobit')):
        with pytest.raises(ValueError, match="'gaussian'.*'censored'"):
            call()
    nothing_seen = dict(c['lc'], nondet=np.ones(73, dtype=bool))
    for call in (lambda: m.log_likelihood(nothing_seen, p, nondet='censored'),
                 lambda: m.limit_terms(nothing_seen, p),
                 lambda: F.lightcurve_mcmc(nothing_seen, m, p_lo=p * 0.9, p_up=p * 1.1, nondet='censored')):
        with pytest.raises(ValueError, match='at least one detection'):
            call()


def test_the_references_own_log_ndtr():
    z = np.concatenate([L.z_sweep(), np.linspace(-50., 37., 200)])
    exact = L.log_ndtr_exact(z)
    assert exact[z == 0.][0] == np.log(0.5) and np.all(np.diff(exact[np.argsort(z)]) >= 0.) and np.all(exact < 0.)
    assert np.isclose(exact[z == 37.][0], -5.725571e-300, rtol=1e-6)         # (Phi(-37), tabulated)
    err = relerr(log_ndtr(z), exact)
    print(f'scipy.special.log_ndtr against 60 digits over [-1e4, 37]: {err:.2e}')
    assert err < 1e-12
    # ... and the test can see a bad ln Phi: the naive form fails the same bound in each of its three ways
    naive = L.log_ndtr_naive(z)
    assert np.all(naive[z < -38.6] == -np.inf) and np.all(naive[z > 8.3] == 0.)
    mid = (z > 5.) & (z < 8.)
    worst = np.max(np.abs(naive[mid] / exact[mid] - 1.))
    print(f'naive log(erfc / 2) for 5 < z < 8: {worst:.2e}')
    assert mid.sum() > 5 and worst > 1e-9
    ok = (z > -30.) & (z < 2.)
    assert relerr(naive[ok], exact[ok]) < 1e-12                               # (where it is fine, it is fine)
