#!/usr/bin/env python3
"""Cost of ``template_predictive()`` after a fit, on the GPU, next to ``posterior_predictive`` and the host route.

After the fit of ``tools/template_timing.py`` (``WithTemplate(ShockCooling4, sifto_template(), factors=('r',),
offsets=('U',))``, 1024 walkers, 2000 stored steps, the 3000-point light curve of configs[1], through
``lightcurve_mcmc``), on the grid of its 6 filters x 1000 times:

1. the whole chain (2 048 000 samples, a host array: both functions upload it) and ``thin=100`` (20 480 samples), the
   three components, with and without ``features``;
2. in the same session ``posterior_predictive`` of the bare base model on the base's columns of the same samples and the
   same grid -- a third of the series;
3. at ``thin=100`` the host route -- ``model(t, filters, *flat.T)`` and ``model.components(...)`` (every value over PCIe),
   ``np.nanpercentile`` of the three, and the features' definitions in NumPy -- and the largest disagreement.

The calls of one sample count alternate, ``--reps`` rounds after one warm-up round; medians are reported and every
series is kept.  Every number is a host clock around a call that returns host arrays (the device work is complete when
it returns).  Kernel shares come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.  There is no
gate on any of it.

Usage:  python tools/template_predictive_timing.py [--reps 5] [--json profiles/template_predictive_timing.json]"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.fitting import lightcurve_mcmc, posterior_predictive, template_predictive  # noqa: E402
from tools.template_timing import BASE_HI, BASE_LO, BASE_PRIORS, light_curve  # noqa: E402

PERCENTILES = (15.87, 50., 84.14)


def clock_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms)),
            'all_ms': [float(v) for v in ms]}


def first_extreme(V, largest):
    """Per (filter, sample) of ``V`` (nf, nt, n): the largest (smallest) non-NaN value along the times and the first
    index it is attained at; NaN and -1 where there is none."""
    ok = ~np.isnan(V)
    filled = np.where(ok, V, -np.inf if largest else np.inf)
    at = np.argmax(filled, axis=1) if largest else np.argmin(filled, axis=1)
    at = np.where(ok.any(axis=1), at, -1)
    value = np.take_along_axis(V, np.maximum(at, 0)[:, None, :], axis=1)[:, 0]
    return np.where(at < 0, np.nan, value), at.astype(np.int32)


def host_route(model, t, filters, percentiles, flat):
    """model(...), model.components(...), nanpercentile and the features: what there was before template_predictive."""
    Y = model(t, filters, *flat.T)                                  # (nf, nt, S) float64 across PCIe, three times
    B, Tm = model.components(t, filters, *flat.T)
    bands = {name: np.nanpercentile(V, percentiles, axis=-1) for name, V in (('total', Y), ('base', B), ('template', Tm))}
    y_b, i_b = first_extreme(B, True)
    y_t, i_t = first_extreme(Tm, True)
    above = Tm > B
    i_x = np.where(above.any(axis=1), np.argmax(above, axis=1), -1).astype(np.int32)
    steps = np.arange(len(t))[None, :, None]
    between = (i_b >= 0)[:, None, :] & (i_b < i_t)[:, None, :] & (steps >= i_b[:, None, :]) & (steps <= i_t[:, None, :])
    y_d, i_d = first_extreme(np.where(between, B + Tm, np.nan), False)
    return bands, {'y_peak_base': y_b, 'y_peak_template': y_t, 'y_dip': y_d}, \
        {'i_peak_base': i_b, 'i_peak_template': i_t, 'i_cross': i_x, 'i_dip': i_d}


def run(reps, walkers, steps, burnin, num, thin):
    lc = light_curve()
    t_mid = float(np.median(lc['MJD']))
    base = M.ShockCooling4(redshift=0.)
    model = M.WithTemplate(base, M.sifto_template(), lc, factors=('r',), offsets=('U',))
    lo = np.concatenate([BASE_LO, [t_mid - 0.5, 0.03, 0.8, -0.2]])
    hi = np.concatenate([BASE_HI, [t_mid + 0.5, 0.06, 1.2, 0.2]])
    priors = BASE_PRIORS + [M.UniformPrior(t_mid - 5., t_mid + 5.), M.UniformPrior(0.01, 1.), M.UniformPrior(0., 5.),
                            M.UniformPrior(-2., 2.)]
    sampler = lightcurve_mcmc(lc, model, priors=priors, p_lo=lo, p_up=hi, nwalkers=walkers, nsteps=steps,
                              nsteps_burnin=burnin, seed=1)
    res = {'model': 'WithTemplate(ShockCooling4, sifto_template(), factors r, offsets U)', 'walkers': walkers, 'steps': steps,
           'filters': 6, 'times': num, 'percentiles': list(PERCENTILES), 'reps': reps,
           'note': 'host clocks around calls that take host samples and return host arrays; the calls of one sample '
                   'count alternate'}
    for label, every in (('whole_chain', 1), ('thinned', thin)):
        flat = np.ascontiguousarray(sampler.get_chain(thin=every, flat=True))
        flat_base = np.ascontiguousarray(flat[:, :base.n_model_params])
        calls = {'template_with_features': lambda: template_predictive(lc, model, flat, PERCENTILES, num=num),
                 'template_without_features': lambda: template_predictive(lc, model, flat, PERCENTILES, num=num, features=False),
                 'template_total_only': lambda: template_predictive(lc, model, flat, PERCENTILES, num=num, features=False,
                                                                    components='total'),
                 'posterior_predictive_base': None}
        full = calls['template_with_features']()                    # (warm-up: builds the grid engine)
        calls['posterior_predictive_base'] = lambda: posterior_predictive(lc, base, flat_base, PERCENTILES, num=num,
                                                                          filters_to_model=full.filters)
        ms = {name: [] for name in calls}
        for r in range(reps + 1):
            for name, fn in calls.items():
                t, _ = clock_ms(fn)
                if r:
                    ms[name].append(t)
        part = {'samples': full.n_samples, **{name: summary(v) for name, v in ms.items()}}
        med = {name: part[name]['median_ms'] for name in calls}
        part['ratio_template_over_posterior_predictive'] = med['template_without_features'] / med['posterior_predictive_base']
        part['ratio_total_only_over_posterior_predictive'] = med['template_total_only'] / med['posterior_predictive_base']
        part['features_cost_ms'] = med['template_with_features'] - med['template_without_features']
        part['n_cross_none'] = [int(v) for v in full.n_cross_none]
        part['n_dip_none'] = [int(v) for v in full.n_dip_none]
        part['n_dark_max'] = int(full.n_dark.max())
        res[label] = part
        print(f'{label}: {json.dumps(med)}', file=sys.stderr, flush=True)
        if every == 1:
            continue
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            old = [clock_ms(lambda: host_route(model, full.t, full.filters, full.percentiles, flat))
                   for _ in range(max(2, min(reps, 3)))]
        bands, values, indices = old[0][1]
        part['host_route'] = summary([t for t, _ in old[1:]])
        part['ratio_host_over_new'] = part['host_route']['median_ms'] / med['template_with_features']
        with np.errstate(all='ignore'):
            part['max_rel_diff_bands'] = {name: float(np.nanmax(np.abs(full.quantiles[name] - bands[name]) /
                                                                 np.maximum(np.abs(bands[name]), 1e-300))) for name in bands}
            part['bands_bitwise'] = {name: bool(np.array_equal(full.quantiles[name], bands[name], equal_nan=True)) for name in bands}
            part['max_rel_diff_values'] = {name: float(np.nanmax(np.abs(getattr(full, name) - v) / np.abs(v)))
                                           for name, v in values.items()}
        part['indices_equal_fraction'] = {name: float(np.mean(getattr(full, name) == v)) for name, v in indices.items()}
        part['values_the_host_route_moves_MB'] = 3 * full.n_samples * 6 * num * 8 / 1e6
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--small', action='store_true', help='tiny shapes (a quick check of the script itself)')
    a = ap.parse_args()
    res = run(a.reps, 64, 200, 50, 50, 10) if a.small else run(a.reps, 1024, 2000, 200, 1000, 100)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
