"""The extended-precision reference of the per-epoch SED likelihood (helpers.sed_reference) and the input families of
tests/test_gpu_sed_edges.py, checked on the host before any GPU sees them: the reference reproduces the golden
numbers, the float64 oracle agrees with it on every family (how closely is printed per regime), and every family is
built so that a model error of 1e-9 moves the log-likelihood by more than the tolerance the device is held to."""
import numpy as np
import pytest

import helpers as H
from conftest import golden, relerr

pytestmark = pytest.mark.skipif(not H.LD_OK, reason='np.longdouble is no wider than float64 here: eps = %.1e, the '
                                'reference needs eps < 1e-18' % np.finfo(np.longdouble).eps)

FAMILIES = [('listed',), ('state', 0), ('state', 1), ('state', 2), ('validity',), ('stride',), ('shapes', 1),
            ('shapes', 63), ('shapes', 64), ('shapes', 65), ('shapes', 129), ('zero',), ('many',)] + \
    [('fuzz', s) for s in range(8)]


def _family(name, *args):
    if name == 'state':
        return H.sed_case('state')[args[0]]
    return H.sed_case(name, *args)


def _forms(case):
    return (case.form,) if hasattr(case, 'form') else H.SED_FORMS


def test_reference_reproduces_the_golden_numbers():
    g = golden('sed')
    off = g['sed/ep_off']
    cut = [slice(off[e], off[e + 1]) for e in range(len(off) - 1)]
    case = H.SedCase([[str(n) for n in g['sed/names'][s]] for s in cut], [g['sed/y'][s] for s in cut],
                     [g['sed/dy'][s] for s in cut], g['sed/cand'], float(g['sed/z']))
    for form, key in zip(H.SED_FORMS, ('sed/ll', 'sed/ll_rel', 'sed/ll_abs')):
        assert relerr(case.reference(form), g[key]) < 1e-12
        assert relerr(case.oracle(form), g[key]) < 1e-12     # (the helper's route to the oracle is the golden one)


def test_zero_model_of_the_reference_is_the_oracles():
    """T <= 0, T = inf, T = NaN and R = 0 give the zero model: -1/2 sum [ln(2 pi sigma^2) + (y / sigma)^2]."""
    case = _family('zero')
    zero = case.zero_model()
    assert zero.sum() == 4 * 18     # per epoch 16 such temperatures and two radii of 0 beside them
    for form in H.SED_FORMS:
        ref, orc = case.reference(form), case.oracle(form)
        assert not np.isnan(np.asarray(ref, dtype=np.float64)).any() and not np.isnan(orc).any()
        for e, (_, y, dy) in enumerate(case.epochs):
            s = case.cand[e, :, 2] if form else np.zeros(case.cand.shape[1])
            units = dy[:, None] if form != 'absolute' else np.median(dy)
            var = dy[:, None] ** 2 + (units * s[None, :]) ** 2
            want = -0.5 * np.sum(np.log(2 * np.pi * var) + y[:, None] ** 2 / var, axis=0)
            assert relerr(np.asarray(ref[e], dtype=np.float64)[zero[e]], want[zero[e]]) < 1e-14
            assert relerr(orc[e][zero[e]], want[zero[e]]) < 1e-14


@pytest.mark.parametrize('family', FAMILIES, ids=lambda f: '-'.join(str(x) for x in f))
def test_oracle_agrees_and_family_is_sensitive(family):
    """Per family and form: (a) the float64 oracle against the reference, per temperature regime -- outside the cold
    regime it must be within 1e-12, which is what entitles the GPU tests to the project's 1e-11 there; in the cold
    regime the figure ``d_cold`` is printed and becomes the GPU tests' tolerance (helpers.sed_tolerances);
    (b) sensitivity: with the reference's model multiplied by 1 + 1e-9, the log-likelihood of at least 95 % of the
    candidates (those with a zero model aside) moves by more than the tolerance the device is held to."""
    case = _family(*family)
    T = case.cand[..., 0]
    live = case.live()
    edge = H.sed_cold_edge(case.z)
    regimes = {'cold (< %.3f kK)' % edge: live & (T < edge), '< 2 kK': live & (T >= edge) & (T < 2.),
               '2-256 kK': live & (T >= 2.) & (T < 256.), '>= 256 kK': live & (T >= 256.)}
    for form in _forms(case):
        ref = np.asarray(case.reference(form), dtype=np.float64)
        assert np.all(np.isfinite(ref[live]))
        # (the 4200 epochs of 'stride' go through the oracle once; its other forms on the epochs with cold candidates
        # and every 16th)
        some = None if family != ('stride',) or form is None else \
            np.union1d(np.arange(0, len(T), 16), np.nonzero((T < edge).any(axis=1))[0])
        with np.errstate(invalid='ignore'):   # (0 / 0 in an empty epoch: not live; NaN where the oracle was not run)
            dev = np.abs(case.oracle(form, some) - ref) / np.abs(ref)
        tol, d_cold = H.sed_tolerances(case, form)
        for k, (label, sel) in enumerate(regimes.items()):
            sel = sel & ~np.isnan(dev)
            if sel.any():
                print(f'{family} {form}: oracle vs reference, {label}: {dev[sel].max():.2e} ({sel.sum()} candidates)')
                assert k == 0 or dev[sel].max() < 1e-12
        if regimes['cold (< %.3f kK)' % edge].any():
            assert d_cold == dev[regimes['cold (< %.3f kK)' % edge]].max()
            assert d_cold < 1e-10     # (the cold tolerance follows the measurement, but not anywhere)
        if not live.any():
            continue
        with np.errstate(invalid='ignore'):
            shift = np.abs(np.asarray(case.reference(form, 1 + 1e-9), dtype=np.float64) - ref) / np.abs(ref)
        share = float(np.mean(shift[live] > tol[live]))
        print(f'{family} {form}: a model error of 1e-9 moves lnL by min {shift[live].min():.1e}, median '
              f'{np.median(shift[live]):.1e}; above the tolerance ({tol.max():.1e} at the most): {100 * share:.1f} %')
        assert share >= 0.95
