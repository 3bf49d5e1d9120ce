"""``models.WithTemplate`` on the host: parameter names, units and order, every validation error, and the NumPy helper
(``template_reference``) pinned against the oracle's companion-shocking models, whose columns it reproduces with a Kasen
base and the SiFTO template."""
import itertools

import numpy as np
import pytest

import limits_reference as L
import template_reference as T
from conftest import relerr
from oracle import lcf_oracle as O
from lightcurve_fitting_amd import models as M

Z = T.Z


def sc2_lc():
    return T.case('ShockCooling2', 'sifto')['lc']


@pytest.mark.parametrize('factors,offsets', list(itertools.product(
    [(), ('r',), ('r', 'i'), ('U', 'B', 'V', 'g', 'r', 'i')], [(), ('U',), ('U', 'i')])))
@pytest.mark.parametrize('kind', ['ShockCooling', 'ShockCooling2', 'ShockCooling3', 'ShockCooling4'])
def test_names_units_and_order(kind, factors, offsets):
    base = getattr(M, kind)(redshift=Z)
    c = T.case(kind, 'sifto')
    if base.n_model_params + 2 + len(factors) + len(offsets) > 15:     # (a row has at most 16 columns, sigma included)
        with pytest.raises(ValueError, match='16 columns'):
            M.WithTemplate(base, M.sifto_template(), c['lc'], factors=factors, offsets=offsets)
        return
    model = M.WithTemplate(base, M.sifto_template(), c['lc'], factors=factors, offsets=offsets)
    extra = ['t_\\mathrm{max}', 's'] + ['r_' + x for x in factors] + ['\\Delta t_' + x for x in offsets]
    assert model.input_names == type(base).input_names + extra
    assert model.units == type(base).units + ['d', ''] + [''] * len(factors) + ['d'] * len(offsets)
    assert model.nparams == model.n_model_params == base.n_model_params + 2 + len(factors) + len(offsets)
    assert len(model.axis_labels) == model.nparams and model.axis_labels[base.n_model_params] == '$t_\\mathrm{max}$ (d)'
    assert model.z == base.z and model.output_quantity == base.output_quantity
    model.input_names.append('\\sigma')          # what lightcurve_mcmc(use_sigma=True) does: instance-level names
    model.units.append('')
    assert model.nparams == model.n_model_params + 1 and type(model).input_names == []
    assert base.input_names == type(base).input_names                      # the base instance is left as it was


def test_the_columns_of_the_companion_models():
    """The parameter order is chosen so that a Kasen base and SiFTO reproduce the reference's columns."""
    lc = sc2_lc()
    kasen = M.CustomModel('__device__ void lcf_user_state(double, const double*, const double*, double, double&, double&);',
                          T.KASEN_NAMES, ['d', '10^13 cm', 'M_Ch (10^9 cm/s)^7'], redshift=Z)
    two = M.WithTemplate(kasen, M.sifto_template(), lc, offsets=('U', 'i'))
    assert two.input_names == M.CompanionShocking2.input_names and two.units == M.CompanionShocking2.units
    one = M.WithTemplate(kasen, M.sifto_template(), lc, factors=('r', 'i'))
    assert one.input_names == M.CompanionShocking.input_names[:-1] and one.units == M.CompanionShocking.units[:-1]


def test_validation_errors():
    lc = sc2_lc()
    base = M.ShockCooling2(redshift=Z)
    sifto = M.sifto_template()
    for bad in (M.CompanionShocking(lc, redshift=Z), M.CompanionShocking2(lc, redshift=Z), M.Arnett(), M.Magnetar(),
                M.Blackbody(), M.ShockCooling2):
        with pytest.raises(TypeError, match='base of WithTemplate'):
            M.WithTemplate(bad, sifto, lc)
    ok = {c: np.ones(5) for c in T.FILTERS}
    for epochs in ([0., 1., 2.], [0., 1., 1., 2., 3.], [0., 2., 1., 3., 4.], [0., 1., np.nan, 3., 4.], [0., 1., 2., 3., np.inf]):
        with pytest.raises(ValueError, match='epochs'):
            M.WithTemplate(base, (epochs, {c: np.ones(len(epochs)) for c in T.FILTERS}), lc)
    with pytest.raises(ValueError, match='column'):
        M.WithTemplate(base, ([0., 1., 2., 3., 4.], dict(ok, U=np.ones(4))), lc)
    with pytest.raises(ValueError, match='column'):
        M.WithTemplate(base, ([0., 1., 2., 3., 4.], dict(ok, U=[1., 1., np.nan, 1., 1.])), lc)
    with pytest.raises(ValueError, match='2-D array'):
        M.WithTemplate(base, np.ones((10, 3)), lc)
    # a filter of the light curve without a column: the reference's exception
    with pytest.raises(Exception, match='No template for filter U'):
        M.WithTemplate(base, ([0., 1., 2., 3.], {c: np.ones(4) for c in 'BVgri'}), lc)
    with pytest.raises(Exception, match='No template for filter r'):
        M.WithTemplate(base, sifto, lc, columns={'r': 'z'})
    M.WithTemplate(base, ([0., 1., 2., 3.], {c: np.ones(4) for c in 'BVgri'}), lc, columns={'U': 'B'})   # (mapped: fine)
    with pytest.raises(ValueError, match='scale'):
        M.WithTemplate(base, sifto, lc, scale='area')
    with pytest.raises(ValueError, match='peak value for filter'):
        M.WithTemplate(base, sifto, lc, scale={'U': 1.})
    with pytest.raises(ValueError, match='distinct'):
        M.WithTemplate(base, sifto, lc, factors=('r', 'r'))
    with pytest.raises(ValueError, match='16 columns'):
        M.WithTemplate(M.ShockCooling3(redshift=Z), sifto, T.case('ShockCooling3', 'sifto')['lc'], factors=tuple('UBVgri'),
                       offsets=('U',))
    model = M.WithTemplate(base, sifto, lc)
    with pytest.raises(ValueError, match='out of scope'):
        model.engine_for(lc, nondet='censored')
    with pytest.raises(ValueError, match='out of scope'):
        model.log_likelihood(lc, np.ones(6), nondet='censored')
    with pytest.raises(ValueError, match='nondet must be'):
        model.engine_for(lc, nondet='tobit')
    with pytest.raises(TypeError, match='takes 6 parameters'):
        model(lc['MJD'], lc['filter'], 1., 2., 3.)


def test_scaling_and_splines_are_the_references():
    """``scale='peak'`` and the explicit form against the helper; the coefficients against SciPy's CubicSpline."""
    from scipy.interpolate import CubicSpline
    c = T.case('ShockCooling2', 'bump')
    base = M.ShockCooling2(redshift=Z)
    for scale, want in (('peak', c['scaled']),
                        ({n: 3. + k for k, n in enumerate(T.FILTERS)},
                         T.scaled_columns(c['template'], T.FILTERS, scale={n: 3. + k for k, n in enumerate(T.FILTERS)}))):
        model = M.WithTemplate(base, c['template'], c['lc'], scale=scale)
        assert len(model.template) == 6
        for filt, coef in model.template.items():
            spline = CubicSpline(c['epochs'], want[filt.name])
            assert coef.shape == (11, 4) and relerr(coef, spline.c.T) < 1e-9
            assert np.array_equal(coef[:, 3], want[filt.name][:-1])
    # a 2-D array with SiFTO's columns is the tuple form
    a = M.WithTemplate(base, M.sifto_template(), c['lc'])
    b = M.WithTemplate(base, T.templates('sifto'), c['lc'])
    assert all(np.array_equal(a.template[f], b.template[f]) for f in a.template)


# ---- the helper pinned against the oracle's companion-shocking models -------------------------------------------------
def companion_case():
    c = L.case('CompanionShocking')
    rng = np.random.default_rng(7)
    truth = c['truth']
    P = truth + rng.uniform(-1., 1., (12, 8)) * [2., 0.1, 0.3, 1., 0.03, 0.05, 0.05, 0.1]
    P[0] = truth
    return c, P


@pytest.mark.parametrize('variant', [1, 2])
def test_the_helper_is_the_oracles_companion_model(variant):
    c, P = companion_case()
    orc = O.CompanionShockingOracle(c['bands'], c['y'], Z, variant)
    scaled = T.scaled_columns(T.templates('sifto'), c['names'], c['y'])
    epochs = T.templates('sifto')[0]
    if variant == 2:    # t_0, a, M v^7, t_max, s, dt_U, dt_i
        rows = np.column_stack([P[:, :5], P[:, 5] * 10. - 9., P[:, 6] * 10. - 9.5])
        kw = dict(factors=(), offsets=('U', 'i'))
        want = np.column_stack([orc.evaluate(c['t'], c['bands'], *p) for p in rows])
    else:               # t_0, a, M v^7, t_max, s, r_r, r_i and r_U = 1
        rows = P[:, :7]
        kw = dict(factors=('r', 'i'), offsets=())
        want = np.column_stack([orc.evaluate(c['t'], c['bands'], *p, 1.) for p in rows])
    got = T.model_values(('custom', T.kasen_state, Z), epochs, scaled, c['t'], c['bands'], c['names'], rows, 3, **kw)
    tau = T.template_values(epochs, scaled, c['t'], c['names'], rows, 3, **kw)
    err = relerr(got, want)
    print(f'variant {variant}: helper vs CompanionShockingOracle.evaluate {err:.2e}; the template is '
          f'{np.min(tau[tau > 0] / got[tau > 0]):.1e} ... {np.max(tau[tau > 0] / got[tau > 0]):.3f} of the model, zero at {np.mean(tau == 0.):.2f}')
    assert np.all(np.isfinite(want)) and np.any(tau == 0.) and np.any(tau > 0.1 * got)
    assert err < 1e-14
