"""Central-engine models (``Arnett``, ``Magnetar``) where there is no device: the quadrature rule of their definition
against ``scipy.integrate.quad`` over the box it is specified for, the restatement's special values, the model classes'
metadata and checks, the ejecta helpers, and the ABI (the two ids; engine calls failing with a status)."""
import itertools
import os
import re

import numpy as np
import pytest

import central_reference as C
from lightcurve_fitting_amd import engine as E, models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE_BOUND = 1e-6      # the rule against the exact integral, over C.BOX
N_DRAWS = 1000


def box_points(seed):
    """(t, tau_m, t_p): N_DRAWS draws, log-uniform in each, and the box's eight corners."""
    rng = np.random.default_rng(seed)
    cols = [C.log_uniform(rng, *C.BOX[k], N_DRAWS) for k in ('t', 'tau_m', 't_p')]
    corners = np.array(list(itertools.product(C.BOX['t'], C.BOX['tau_m'], C.BOX['t_p'])))
    return [np.concatenate([c, corners[:, k]]) for k, c in enumerate(cols)]


@pytest.mark.parametrize('kind', ['arnett', 'magnetar'])
def test_rule_accuracy_over_the_box(kind):
    t, tau_m, t_p = box_points(20261018)
    src = [np.full(len(t), 0.07)] if kind == 'arnett' else [np.ones(len(t)), t_p]
    got = C.rule(kind, t, src, tau_m)
    want = np.array([C.truth(kind, t[i], [v[i] for v in src], tau_m[i]) for i in range(len(t))])
    err = np.abs(got - want) / np.abs(want)
    i = int(np.argmax(err))
    print(f'{kind}: worst {err.max():.3g} at t = {t[i]:.4g}, tau_m = {tau_m[i]:.4g}, t_p = {t_p[i]:.4g}; '
          f'corners {err[-8:].max():.3g}')
    assert np.all(want > 0.) and len(err) == N_DRAWS + 8
    assert err.max() <= RULE_BOUND


def test_the_rule_is_fixed_by_t_and_tau_m_alone():
    s_lo, s_mid = C.pieces(np.array([0.01, 10., 400.]), np.array([60., 12., 2.]))
    assert s_lo[0] == 0. and s_lo[1] == 0. and s_lo[2] == np.sqrt(400. ** 2 - 40. * 4.)
    assert np.array_equal(s_mid, s_lo + (np.array([0.01, 10., 400.]) - s_lo) / 8.)
    # a row's value is the same alone and in a block (nothing adapts to the batch)
    P = np.array([[0.07, 12., -5.], [0.2, 30., 1.], [0.01, 2., -300.]])
    mjd = np.array([-4., 0., 1., 7.5, 60., 100.])
    block = C.luminosity('arnett', mjd, P)
    for k in range(3):
        assert np.array_equal(C.luminosity('arnett', mjd, P[k:k + 1])[0], block[k])


def test_nodes_and_weights_of_the_kernel_are_leggauss_32():
    text = open(os.path.join(ROOT, 'lightcurve_fitting_amd', 'csrc', 'lcf_central.hip')).read()
    table = re.search(r'kGaussLegendre\[[^\]]*\]\s*=\s*\{([^}]*)\}', text).group(1)
    values = np.array([float(v) for v in table.replace('\n', ' ').split(',') if v.strip()])
    assert values.shape == (64,)
    assert np.max(np.abs(values[:32] - C.GL_X)) < 1e-16 and np.max(np.abs(values[32:] - C.GL_W)) < 1e-17


def test_exactly_zero_at_and_before_the_explosion():
    mjd = np.array([-10., 4.999, 5., 5. + 1e-9, 6.])
    for kind, p in (('arnett', [0.07, 12., 5.]), ('magnetar', [1., 5., 20., 5.])):
        L = C.luminosity(kind, mjd, [p])[0]
        assert np.all(L[:3] == 0.) and not np.any(np.signbit(L[:3])) and np.all(L[3:] > 0.)
        assert C.truth(kind, 0., p[:-2], p[-2]) == 0. and C.truth(kind, -1., p[:-2], p[-2]) == 0.
        Lz = C.luminosity(kind, mjd, [p], z=0.5)[0]          # the clock runs slower: the same zeros, another curve
        assert np.all(Lz[:3] == 0.) and np.all(Lz[3:] > 0.) and not np.array_equal(Lz[3:], L[3:])
        assert np.isclose(Lz[4], C.luminosity(kind, [5. + 1. / 1.5], [p])[0, 0], rtol=1e-12, atol=0.)


def test_nan_rows():
    mjd = np.array([-1., 3., 30.])
    for bad in ([np.nan, 12., 0.], [0.07, 0., 0.], [0.07, -3., 0.], [0.07, np.inf, 0.], [0.07, 12., np.nan]):
        assert np.all(np.isnan(C.luminosity('arnett', mjd, [bad])))
    for bad in ([1., 0., 20., 0.], [1., -1., 20., 0.], [np.inf, 5., 20., 0.]):
        assert np.all(np.isnan(C.luminosity('magnetar', mjd, [bad])))
    assert np.all(np.isnan(C.luminosity('arnett', mjd, [[0.07, 12., 0., 0.]], leak=True)))
    assert np.all(np.isnan(C.log_likelihood('arnett', mjd, np.ones(3), np.ones(3), [[np.nan, 12., 0.]])))


def test_leakage_factor():
    t = np.array([0.5, 10., 50., 400.])
    for t_gamma in (3., 40., 500.):
        want = 1. - np.exp(-(t_gamma / t) ** 2)
        got = C.leak_factor(t, t_gamma)
        # (1 - exp(-x) loses ~1e-16 / x to cancellation: the bound follows the formula's own rounding)
        assert np.all(np.abs(got - want) <= 4e-16 / np.minimum(1., (t_gamma / t) ** 2) * want)
        mjd, p = t + 2., [0.07, 12., 2.]
        plain = C.luminosity('arnett', mjd, [p])[0]
        leaky = C.luminosity('arnett', mjd, [[0.07, 12., t_gamma, 2.]], leak=True)[0]
        assert np.allclose(leaky, plain * got, rtol=1e-15, atol=0.)
        assert np.isclose(C.truth('arnett', 10., [0.07], 12., t_gamma), C.truth('arnett', 10., [0.07], 12.) * got[1], rtol=1e-15, atol=0.)
    assert np.all(C.leak_factor(t, 1e-3) < 1e-5) and np.all(C.leak_factor(t[:2], 1e3) == 1.)


def test_gaussian_log_likelihood_modes():
    rng = np.random.default_rng(1)
    L, y, dy = rng.uniform(1., 2., (3, 5)), rng.uniform(1., 2., 5), rng.uniform(0.05, 0.2, 5)
    sigma = np.array([0.5, 1., 2.])
    plain = C.gaussian_log_likelihood(L, y, dy)
    assert np.allclose(plain[0], -0.5 * sum(np.log(2 * np.pi * dy[i] ** 2) + ((y[i] - L[0, i]) / dy[i]) ** 2 for i in range(5)))
    rel = C.gaussian_log_likelihood(L, y, dy, sigma, 'relative')
    assert np.allclose(rel[1], C.gaussian_log_likelihood(L[1:2], y, dy * np.sqrt(2.))[0])
    ab = C.gaussian_log_likelihood(L, y, dy, sigma, 'absolute')
    assert np.allclose(ab[2], C.gaussian_log_likelihood(L[2:3], y, np.sqrt(dy ** 2 + (2. * np.median(dy)) ** 2))[0])


def test_model_classes():
    a = M.Arnett()
    assert isinstance(a, M.BaseCentralEngine) and isinstance(a, M.Model)
    assert a.input_names == ['M_\\mathrm{Ni}', '\\tau_m', 't_0'] and a.units == ['Msun', 'd', 'd']
    assert a.nparams == a.n_model_params == 3 and a.output_quantity == 'L_bol' and a.dycol == 'dL_bol'
    assert a.model_id == E.MODEL_ARNETT and a._consts() == [0., 0.] and not a.gamma_leakage
    al = M.Arnett(redshift=0.02, gamma_leakage=True, ycol='L_mcmc', dycol='err')
    assert al.input_names == ['M_\\mathrm{Ni}', '\\tau_m', 't_\\gamma', 't_0'] and al.units == ['Msun', 'd', 'd', 'd']
    assert al.nparams == al.n_model_params == 4 and al._consts() == [0.02, 1.] and al.z == 0.02
    assert al.output_quantity == 'L_mcmc' and al.dycol == 'err'
    m = M.Magnetar()
    assert m.input_names == ['E_p', 't_p', '\\tau_m', 't_0'] and m.units == ['10^51 erg', 'd', 'd', 'd']
    assert m.nparams == m.n_model_params == 4 and m.model_id == E.MODEL_MAGNETAR
    ml = M.Magnetar(gamma_leakage=True)
    assert ml.input_names == ['E_p', 't_p', '\\tau_m', 't_\\gamma', 't_0'] and ml.n_model_params == 5
    ml.input_names.append('\\sigma')                       # what lightcurve_mcmc(use_sigma=True) does
    ml.units.append('')
    assert ml.nparams == 6 and ml.n_model_params == 5 and ml.axis_labels[-1] == '$\\sigma$'
    assert ml.axis_labels[0] == '$E_p$ (10^51 erg)' and M.Arnett().input_names == a.input_names   # per instance
    assert 'gamma_leakage=True' in repr(ml)
    class WithMeta(dict):
        meta = {'redshift': 0.3}
    assert M.Arnett(WithMeta()).z == 0.3


def test_bad_uncertainties_are_named_before_anything_is_built():
    lc = {'MJD': np.arange(5.), 'L_bol': np.full(5, 1e35), 'dL_bol': np.array([1e33, np.nan, 1e33, 0., -1e33])}
    with pytest.raises(ValueError, match=r'rows \[1, 3, 4\].*dL_bol'):
        M.Arnett().log_likelihood(lc, [0.07, 12., -5.])
    with pytest.raises(ValueError, match=r'rows \[0\]'):
        M.Magnetar(dycol='e').engine_for({'MJD': [1.], 'L_bol': [1e35], 'e': [np.inf]})
    with pytest.raises(Exception, match='sigma_type'):
        M.Arnett().engine_for(lc, sigma_type='weird')
    with pytest.raises(TypeError, match='takes 3 parameters'):
        M.Arnett()(np.arange(3.), 0.07, 12.)
    with pytest.raises(E.LcfError, match='tempered') as exc:     # (refused before a device is asked for)
        M.Arnett().temperature_radius(np.arange(3.), 0.07, 12., 0.)
    assert exc.value.status == 5


def test_ejecta_helpers():
    # tau_m = 10 d, v = 10 000 km/s, kappa = 0.07: (864000 s)^2 x 13.8 x c x 1e9 cm/s / 0.14 = 2.2060e45 g = 1.1094 Msun
    mej = M.BaseCentralEngine.ejecta_mass(10., 10.)
    assert abs(mej - (864000. ** 2 * 13.8 * 2.99792458e10 * 1e9 / 0.14) / 1.988409870698051e33) < 1e-12 and abs(mej - 1.1094) < 1e-3
    assert np.isclose(M.Arnett.ejecta_mass(10., 10., kappa=0.14), mej / 2.) and np.isclose(M.Magnetar.ejecta_mass(20., 10.), 4. * mej)
    # 1 Msun at 10 000 km/s: 0.3 x 1.988e33 g x 1e18 cm^2/s^2 = 5.965e50 erg
    assert np.isclose(M.BaseCentralEngine.kinetic_energy(1., 10.), 0.5965229612094153, rtol=1e-14)
    tau, v = np.array([8., 10., 12.]), np.array([8., 10., 12.])
    masses = M.BaseCentralEngine.ejecta_mass(tau, v)
    assert masses.shape == (3,) and masses[1] == mej and np.all(np.diff(masses) > 0.)
    assert M.BaseCentralEngine.kinetic_energy(masses, v).shape == (3,)


def test_abi_ids():
    header = open(os.path.join(ROOT, 'include', 'lcf.h')).read()
    ids = dict(re.findall(r'(LCF_MODEL_\w+) = (\d+)', header))
    assert int(ids['LCF_MODEL_ARNETT']) == E.MODEL_ARNETT == 10 and int(ids['LCF_MODEL_MAGNETAR']) == E.MODEL_MAGNETAR == 11
    assert int(ids['LCF_MODEL_CUSTOM']) == E.MODEL_CUSTOM == 9 and len(ids) == 11
    assert re.search(r'#define LCF_ABI_VERSION (\d+)', header).group(1) == '8' == str(E.LCF_ABI_VERSION)
    # what the library checks before it looks for a device: n_par against the leakage flag, and no filters
    with pytest.raises(E.LcfError, match='LCF_ERR_INVALID_ARGUMENT.*n_par'):
        E.Engine(E.MODEL_ARNETT, 3, [0., 1.], [1.], [1.], [1.], None, None, None, None)
    with pytest.raises(E.LcfError, match='LCF_ERR_INVALID_ARGUMENT.*n_filters'):
        E.Engine(E.MODEL_MAGNETAR, 4, [0., 0.], [1.], [1.], [1.], [0], [0, 1], [1.], [1.])


def test_engine_calls_without_a_device_fail_with_a_status():
    lib = E.load_library()
    if lib.lcf_device_count() > 0:
        pytest.skip('a GPU is visible')
    lc = {'MJD': [1., 2.], 'L_bol': [1e35, 1e35], 'dL_bol': [1e33, 1e33]}      # no 'filter' column
    for call in (lambda: M.Arnett().log_likelihood(lc, np.array([0.07, 12., 0.])),
                 lambda: M.Magnetar(gamma_leakage=True).log_likelihood(lc, np.array([1., 5., 20., 30., 0., 0.5]),
                                                                      use_sigma=True, sigma_type='absolute'),
                 lambda: M.Arnett()(np.array([1., 2.]), 0.07, 12., 0.)):
        with pytest.raises(E.LcfError, match='LCF_ERR_NO_DEVICE'):
            call()
